"""GAT attention aggregation, host side (no GPU): the backward formulas of tests/gat_ref.py are those of torch's autograd through the
plain composition, the bound is neither too tight (an fp32 emulation of the online softmax in its worst order passes on every case) nor
too loose (six planted faults each miss it), the Python mirror of the domain rule agrees with the header's, and the plug-in and the
ctypes wrappers refuse bad operands before any library call.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import gat_cases as cases
from tests import gat_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
OUTPUTS = ("z", "lse", "D", "dadst", "dasrc", "dy")


def fractions(case, got, names=OUTPUTS):
    """error / bound per output; lse over the rows that have entries (an empty row's -inf is compared for equality)."""
    live = case.live
    out = {}
    for name in names:
        if name == "lse":
            assert np.all(np.isneginf(np.asarray(got["lse"])[~live]))
            out[name] = ref.worst(np.asarray(got["lse"])[live], case.ref["lse"][live], case.bound["lse"][live])
        else:
            out[name] = ref.worst(got[name], case.ref[name], case.bound[name])
    return out


def test_every_case_is_inside_the_first_order_range():
    """The bound is first order in rho: rho <= 1e-3 on every row and head of every case (each Case asserts it when it is built)."""
    for case in cases.all_cases():
        assert float(case.bound["rho"].max()) <= ref.RHO_MAX, case.name
    assert [(c.heads, c.k // c.heads) for c in cases.config_cases()] == list(cases.CONFIGS)
    assert {c.ns for c in cases.all_cases()} == set(cases.SLOPES)
    large = cases.large_case()
    spread = np.zeros(large.m)
    np.maximum.at(spread, large.ref["row"], np.abs(large.ref["u"]).max(1))
    assert (spread > 100).sum() > large.m // 4                          # in real rows, not in one


@pytest.mark.parametrize("heads,d,ns", ((1, 7, 0.2), (8, 8, 0.0), (3, 128, 1.0)))
def test_reference_equals_torch_autograd_of_the_composition(heads, d, ns):
    """index, add, leaky_relu, a segment softmax written with index_add_, a weighted sum -- in fp64 on the CPU, under autograd."""
    case = cases.config_case(heads, d, ns)
    row, col = torch.from_numpy(case.ref["row"]), torch.from_numpy(np.array(case.col))
    y = torch.from_numpy(np.array(case.y)).double().requires_grad_(True)
    a_dst = torch.from_numpy(np.array(case.a_dst)).double().requires_grad_(True)
    a_src = torch.from_numpy(np.array(case.a_src)).double().requires_grad_(True)
    s = torch.nn.functional.leaky_relu(a_dst[row] + a_src[col], ns)                      # [nnz, H]
    top = np.full((case.m, heads), -np.inf)
    np.maximum.at(top, row.numpy(), s.detach().numpy())                                  # the shift is a constant of the softmax
    top = torch.from_numpy(top)
    w = torch.exp(s - top[row])
    den = torch.zeros(case.m, heads, dtype=torch.float64).index_add_(0, row, w)
    a = w / den[row]
    z = torch.zeros(case.m, heads, d, dtype=torch.float64).index_add_(0, row, a[:, :, None] * y.view(case.n, heads, d)[col]).view(case.m, heads * d)
    z.backward(torch.from_numpy(np.array(case.g)).double())
    lse = (top + torch.log(den)).detach().numpy()
    for name, got in (("z", z.detach().numpy()), ("dy", y.grad.numpy()), ("dadst", a_dst.grad.numpy()), ("dasrc", a_src.grad.numpy())):
        # relative to the size of the terms summed: with ns = 1 the sum d a_dst[i,h] = sum_e a_e (t_e - D) is 0 in exact arithmetic
        scale = max(np.abs(case.ref[name]).max(), np.abs(case.ref["du"]).max() if name in ("dadst", "dasrc") else 0.0)
        assert np.abs(got - case.ref[name]).max() <= 1e-12 * scale, name
    live = case.live
    assert np.abs(lse[live] - case.ref["lse"][live]).max() <= 1e-12 * np.abs(case.ref["lse"][live]).max()


def emulate_online(case):
    """The online form in fp32 NumPy with ONE slot that takes a row's edges in ascending score order per head, so that every edge raises
    the running maximum and rescales (l, acc); the backward recomputes a_e from the fp32 lse and takes D from the fp32 z, as the
    kernels do."""
    rowptr, col, H, ns = case.rowptr, case.col, case.heads, F32(case.ns)
    m, n, K = case.m, case.n, case.k
    d = K // H
    y3, g3 = ref.per_head(case.y, H), ref.per_head(case.g, H)
    row = ref.edge_rows(rowptr)
    u = (case.a_dst[row] + case.a_src[col]).astype(F32)
    s = np.where(u > 0, u, (ns * u).astype(F32)).astype(F32)
    z, lse = np.zeros((m, H, d), F32), np.full((m, H), -np.inf, F32)
    lanes = np.arange(H)
    with np.errstate(over="ignore", under="ignore"):
        for i in range(m):
            b, e = rowptr[i], rowptr[i + 1]
            if e == b:
                continue
            mrun, l, acc = np.full(H, -np.finfo(F32).max, F32), np.zeros(H, F32), np.zeros((H, d), F32)
            order = b + np.argsort(s[b:e], axis=0, kind="stable")                       # [deg, H]: each head in its own ascending order
            for q in order:
                sq = s[q, lanes]
                mnew = np.maximum(mrun, sq)
                r, w = np.exp((mrun - mnew).astype(F32)), np.exp((sq - mnew).astype(F32))
                l = (l * r + w).astype(F32)
                acc = (acc * r[:, None] + w[:, None] * y3[col[q], lanes]).astype(F32)
                mrun = mnew
            z[i], lse[i] = acc / l[:, None], (mrun + np.log(l)).astype(F32)
        a = np.exp(s - np.where(np.isfinite(lse), lse, F32(0))[row]).astype(F32)
    D = (g3 * z).sum(2, dtype=F32)
    t = (g3[row] * y3[col]).sum(2, dtype=F32)
    du = (a * (t - D[row]) * np.where(u > 0, F32(1), ns)).astype(F32)
    dadst, dasrc, dy = np.zeros((m, H), F32), np.zeros((n, H), F32), np.zeros((n, H, d), F32)
    for i in range(m):
        dadst[i] = du[rowptr[i]:rowptr[i + 1]].sum(0, dtype=F32)
    contrib = (a[:, :, None] * g3[row]).astype(F32)
    order = np.argsort(col, kind="stable")
    cuts = np.searchsorted(col[order], np.arange(n + 1))
    for j in range(n):
        dy[j] = contrib[order[cuts[j]:cuts[j + 1]]].sum(0, dtype=F32)
        dasrc[j] = du[order[cuts[j]:cuts[j + 1]]].sum(0, dtype=F32)
    return dict(z=z.reshape(m, K), lse=lse, D=D, dadst=dadst, dasrc=dasrc, dy=dy.reshape(n, K))


@pytest.mark.parametrize("case", cases.all_cases(), ids=lambda c: c.name)
def test_bound_is_not_too_tight(case):
    frac = fractions(case, emulate_online(case))
    print(case.name, {k: round(v, 4) for k, v in frac.items()})
    assert all(v <= 1.0 for v in frac.values()), frac


def _from_edges(case, s, a, keep_d=True, keep_slope=True):
    """The outputs from per-edge scores and weights in fp64, with switches for the planted faults."""
    H, ns = case.heads, case.ns
    row, col, m, n, K = case.ref["row"], case.col, case.m, case.n, case.k
    y3, g3 = ref.per_head(case.y.astype(np.float64), H), ref.per_head(case.g.astype(np.float64), H)
    z = ref.segment_sum(a[:, :, None] * y3[col], row, m)
    D = (g3 * z).sum(2)
    ds = a * ((g3[row] * y3[col]).sum(2) - (D[row] if keep_d else 0.0))
    du = ds * (np.where(case.ref["u"] > 0, 1.0, ns) if keep_slope else 1.0)
    with np.errstate(divide="ignore"):
        top = s.max()
        lse = np.where(case.live[:, None], np.log(ref.segment_sum(np.exp(s - top), row, m)) + top, -np.inf)
    return dict(z=z.reshape(m, K), lse=lse, D=D, dadst=ref.segment_sum(du, row, m), dasrc=ref.segment_sum(du, col, n),
                dy=ref.segment_sum(a[:, :, None] * g3[row], col, n).reshape(n, K))


def _softmax(case, s):
    row, m = case.ref["row"], case.m
    top = np.full((m, case.heads), -np.inf)
    np.maximum.at(top, row, s)
    w = np.exp(s - top[row])
    return w / ref.segment_sum(w, row, m)[row]


def fault_slope_dropped_from_du(case):
    return _from_edges(case, case.ref["s"], case.ref["a"], keep_slope=False)


def fault_no_d_term(case):
    return _from_edges(case, case.ref["s"], case.ref["a"], keep_d=False)


def fault_dropped_edge(case):
    keep = np.ones(case.col.size, bool)
    keep[case.rowptr[np.argmax(np.diff(case.rowptr) == 3)]] = False        # the first entry of a three-entry row
    s = np.where(keep[:, None], case.ref["s"], -np.inf)
    return _from_edges(case, np.where(keep[:, None], case.ref["s"], case.ref["s"].min()), _softmax(case, s))


def fault_no_max_shift(case):
    s = case.ref["s"].astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp(s)                                                       # fp32: overflows from 88.7 on
        a = (w / ref.segment_sum(w.astype(np.float64), case.ref["row"], case.m)[case.ref["row"]].astype(F32)).astype(np.float64)
        return _from_edges(case, case.ref["s"], a)


def fault_a_src_of_the_wrong_head(case):
    if case.heads == 1:
        return {name: case.ref[name] for name in OUTPUTS}                   # one head: no wrong head to take
    u = case.a_dst.astype(np.float64)[case.ref["row"]] + np.roll(case.a_src.astype(np.float64), 1, axis=1)[case.col]
    s = np.where(u > 0, u, case.ns * u)
    return _from_edges(case, s, _softmax(case, s))


def fault_bf16_scores(case):
    s = torch.from_numpy(case.ref["s"]).to(torch.bfloat16).to(torch.float64).numpy()
    return _from_edges(case, s, _softmax(case, s))


FAULTS = (fault_slope_dropped_from_du, fault_no_d_term, fault_dropped_edge, fault_no_max_shift, fault_a_src_of_the_wrong_head, fault_bf16_scores)


def test_the_unfaulted_restatement_passes():
    case = cases.config_case(8, 8)
    frac = fractions(case, _from_edges(case, case.ref["s"], case.ref["a"]))
    assert all(v <= 1e-3 for v in frac.values()), frac


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f.__name__)
def test_bound_is_not_too_loose(fault):
    picked = [cases.config_case(1, 47), cases.config_case(8, 8), cases.config_case(3, 128), cases.large_case()]
    missed = [c.name for c in picked if max(fractions(c, fault(c)).values()) > 1.0]
    assert missed, fault.__name__
    if fault is fault_no_max_shift:
        got = fault(cases.large_case())
        assert "large" in missed and not np.all(np.isfinite(got["z"]))      # it overflows where the scores are large
    if fault is fault_slope_dropped_from_du:
        frac = fractions(cases.config_case(8, 8), fault(cases.config_case(8, 8)))
        assert frac["dadst"] > 1.0 and frac["dasrc"] > 1.0 and frac["z"] <= 1.0 and frac["dy"] <= 1.0


DOMAIN_TABLE = (
    # rows, heads, d, ld
    (10, 1, 1, 1), (10, 1, 7, 7), (10, 1, 41, 41), (10, 1, 47, 64), (10, 1, 512, 512), (10, 1, 513, 513), (10, 1, 0, 4), (10, 0, 4, 4),
    (10, -1, 4, 4), (10, 2, 4, 8), (10, 2, 3, 6), (10, 2, 2, 4), (10, 2, 6, 12), (10, 8, 8, 64), (10, 8, 8, 63), (10, 33, 4, 132),
    (10, 128, 4, 512), (10, 129, 4, 516), (10, 2, 256, 512), (10, 2, 512, 1024), (10, 3, 128, 384), (10, 5, 8, 40), (10, 5, 12, 60),
    (10, 512, 1, 512), (10, 2, 1, 2), (2 ** 31 - 1, 1, 1, 1), (2 ** 31, 1, 1, 1), (0, 2, 4, 8), (-1, 2, 4, 8),
    (2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40),
)


def test_python_mirror_of_the_domain_rule():
    from isplib_amd import cabi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+ISPLIB_GAT_K_MAX\s+(\d+)", header).group(1)) == cabi.GAT_K_MAX == 512
    L = cabi.lib()
    top = cabi.DENSE_BYTES_MAX // 4
    table = DOMAIN_TABLE + ((top // 64, 8, 8, 64), (top // 64 + 1, 8, 8, 64), (top // 64, 4, 8, 64), (1000, 4, 4, top // 1000),
                            (1000, 4, 4, top // 1000 + 1))
    for rows, heads, d, ld in table:
        assert bool(L.isplib_gat_domain(rows, heads, d, ld)) == cabi.gat_serves(rows, heads, d, ld), (rows, heads, d, ld)
    inside = ((10, 1, 7, 7), (10, 1, 41, 41), (10, 1, 47, 64), (10, 1, 512, 512), (10, 2, 4, 8), (10, 33, 4, 132), (10, 128, 4, 512),
              (10, 2, 256, 512), (10, 3, 128, 384), (top // 64, 8, 8, 64))
    outside = ((10, 1, 513, 513), (10, 1, 0, 4), (10, 0, 4, 4), (10, 2, 3, 6), (10, 2, 2, 4), (10, 2, 6, 12), (10, 8, 8, 63), (10, 129, 4, 516),
               (10, 2, 512, 1024), (10, 5, 12, 60), (10, 512, 1, 512), (2 ** 31, 1, 1, 1), (top // 64 + 1, 8, 8, 64))
    assert all(cabi.gat_serves(*t) for t in inside) and not any(cabi.gat_serves(*t) for t in outside)
    for name in ("isplib_gat_csr_hip", "isplib_gat_bw_rows_hip", "isplib_gat_bw_cols_hip", "isplib_gat_domain"):
        assert name in cabi.EXPORTS and name in header
    assert "isplib_gat_serves" in header


def _adj(m, n):
    import isplib_amd
    rowptr = torch.arange(0, m + 1, dtype=torch.int64)
    col = torch.arange(m, dtype=torch.int64) % n
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n))


def test_plugin_refuses_bad_operands_before_any_library_call():
    import isplib_amd
    adj = _adj(6, 4)
    y, a_dst, a_src = torch.zeros(4, 16), torch.zeros(6, 2), torch.zeros(4, 2)
    with pytest.raises(TypeError, match="GPU tensor"):
        isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2)                 # CPU tensors: there is no CPU path
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gat_matmul(y, a_dst[:, 0], a_src[:, 0])                         # 1-D scores with one head are well-formed
    with pytest.raises(ValueError, match="2-D"):
        isplib_amd.gat_matmul(adj, y[0], a_dst, a_src, heads=2)
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            isplib_amd.gat_matmul(adj, y.to(dt), a_dst.to(dt), a_src.to(dt), heads=2)
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.gat_matmul(adj, y, a_dst.to(torch.bfloat16), a_src, heads=2)
    with pytest.raises(TypeError, match="tensor"):
        isplib_amd.gat_matmul(adj, y.numpy(), a_dst, a_src, heads=2)
    with pytest.raises(ValueError, match="one row per column"):
        isplib_amd.gat_matmul(adj, torch.zeros(6, 16), a_dst, a_src, heads=2)
    with pytest.raises(ValueError, match=r"`a_dst` must be \[6, 2\]"):
        isplib_amd.gat_matmul(adj, y, torch.zeros(4, 2), a_src, heads=2)
    with pytest.raises(ValueError, match=r"`a_src` must be \[4, 2\]"):
        isplib_amd.gat_matmul(adj, y, a_dst, torch.zeros(4, 1), heads=2)
    with pytest.raises(ValueError, match=r"`a_dst` must be \[6, 2\]"):
        isplib_amd.gat_matmul(adj, y, a_dst[:, 0], a_src, heads=2)           # 1-D scores need heads == 1
    with pytest.raises(ValueError, match="heads \\* d"):
        isplib_amd.gat_matmul(adj, y, torch.zeros(6, 3), torch.zeros(4, 3), heads=3)
    with pytest.raises(ValueError, match="positive int"):
        isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=0)
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.gat_matmul(adj, torch.zeros(4, 12), a_dst, a_src, heads=2)  # d = 6
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.gat_matmul(adj, torch.zeros(4, 4), a_dst, a_src, heads=2)   # d = 2
    with pytest.raises(ValueError, match="512"):
        adj.gat_matmul(torch.zeros(4, 513), a_dst[:, :1], a_src[:, :1])
    with pytest.raises(ValueError, match="512"):
        adj.gat_matmul(torch.zeros(4, 1024), a_dst, a_src, heads=2)
    assert isplib_amd.gat_matmul is isplib_amd.plugin.gat_matmul and "gat_matmul" in isplib_amd.__all__


def test_ctypes_wrappers_refuse_bad_operands_before_the_call():
    from isplib_amd import cabi
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    y, a_dst, a_src, g = torch.zeros(4, 16), torch.zeros(6, 2), torch.zeros(4, 2), torch.zeros(6, 16)
    with pytest.raises(TypeError, match="float32"):
        cabi.gat(rowptr, col, y.to(torch.bfloat16), a_dst, a_src, 2)
    with pytest.raises(TypeError, match="float32"):
        cabi.gat(rowptr, col, y, a_dst, a_src.to(torch.float16), 2)
    with pytest.raises(TypeError, match="int64"):
        cabi.gat(rowptr.to(torch.int32), col, y, a_dst, a_src, 2)
    with pytest.raises(ValueError, match=r"`a_dst` must be \[6, 2\]"):
        cabi.gat(rowptr, col, y, torch.zeros(5, 2), a_src, 2)
    with pytest.raises(ValueError, match=r"`a_src` must be \[4, 2\]"):
        cabi.gat(rowptr, col, y, a_dst, torch.zeros(4, 3), 2)
    with pytest.raises(ValueError, match="contiguous"):
        cabi.gat(rowptr, col, y, torch.zeros(6, 4)[:, :2], a_src, 2)
    with pytest.raises(ValueError, match="unit inner stride"):
        cabi.gat(rowptr, col, torch.zeros(16, 4).t(), a_dst, a_src, 2)
    with pytest.raises(ValueError, match="heads \\* d"):
        cabi.gat(rowptr, col, y, torch.zeros(6, 3), torch.zeros(4, 3), 3)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.gat(rowptr, col, y, a_dst, a_src, 2)                            # well-formed, but on the CPU
    with pytest.raises(ValueError, match="isplib_gat_serves"):
        cabi.gat(rowptr, col, torch.zeros(4, 12), a_dst, a_src, 2)           # d = 6
    with pytest.raises(ValueError, match="isplib_gat_serves"):
        cabi.gat(rowptr, col, torch.zeros(4, 513), torch.zeros(6, 1), torch.zeros(4, 1), 1)
    with pytest.raises(ValueError, match=r"`lse` must be \[6, 2\]"):
        cabi.gat_bw_rows(rowptr, col, y, a_dst, a_src, g, g, torch.zeros(5, 2), 2)
    with pytest.raises(ValueError, match=r"\[6, 16\]"):
        cabi.gat_bw_rows(rowptr, col, y, a_dst, a_src, torch.zeros(6, 15), g, a_dst, 2)
    with pytest.raises(ValueError, match=r"`dsum` must be \[6, 2\]"):
        cabi.gat_bw_cols(torch.arange(0, 5, dtype=torch.int64), col, y, a_dst, a_src, g, a_dst, torch.zeros(6, 1), 2)
