"""GATv2 attention aggregation, host side (no GPU): the formulas of tests/gatv2_ref.py are those of torch's autograd through the plain
composition, the bound is neither too tight (an fp32 emulation of the online softmax in its worst order passes on every case) nor too
loose (six planted faults each miss it -- the first of them is GAT v1's score, which says "this is not gat_matmul"), the Python mirror
of the domain rule agrees with the header's, the header, EXPORTS and the workspace query are consistent, and the plug-in and the ctypes
wrappers refuse bad operands before any library call.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import gatv2_cases as cases
from tests import gatv2_ref as ref
from tests.test_gat_host import DOMAIN_TABLE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
OUTPUTS = ("z", "lse", "D", "dx", "dy", "datt")
PICKED = cases.SLOPE_CONFIGS


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
    """The bound is first order in rho: rho <= 1e-3 on every row and head of every case but the large one, which is held to 4e-3 as
    the attention large case is (each Case asserts its cap when it is built)."""
    for case in cases.all_cases():
        cap = cases.LARGE_RHO_MAX if case.kind == "large" else ref.RHO_MAX
        assert case.rho_max == cap and float(case.bound["rho"].max()) <= cap, case.name
    assert [(c.heads, c.k // c.heads) for c in cases.config_cases()] == list(cases.CONFIGS) and len(cases.CONFIGS) == 19
    assert {c.ns for c in cases.all_cases()} == set(cases.SLOPES)
    large = cases.large_case()
    spread = np.zeros(large.m)
    np.maximum.at(spread, large.ref["row"], np.abs(large.ref["s"]).max(1))
    assert (spread > 100).sum() > large.m // 4 and np.abs(large.ref["s"]).max() > 150


@pytest.mark.parametrize("heads,d,ns", ((1, 7, 0.2), (8, 8, 0.0), (3, 128, 1.0)))
def test_reference_equals_torch_autograd_of_the_composition(heads, d, ns):
    """index, add, leaky_relu into [nnz, H, d], the att contraction, a segment softmax written with index_add_, a weighted sum -- in
    fp64 on the CPU, under autograd."""
    case = cases.config_case(heads, d, ns)
    row, col = torch.from_numpy(case.ref["row"]), torch.from_numpy(np.array(case.col))
    x = torch.from_numpy(np.array(case.x)).double().requires_grad_(True)
    y = torch.from_numpy(np.array(case.y)).double().requires_grad_(True)
    att = torch.from_numpy(np.array(case.att)).double().requires_grad_(True)
    v = torch.nn.functional.leaky_relu(x.view(case.m, heads, d)[row] + y.view(case.n, heads, d)[col], ns)      # [nnz, H, d]
    s = (v * att[None]).sum(2)
    top = np.full((case.m, heads), -np.inf)
    np.maximum.at(top, row.numpy(), s.detach().numpy())                                  # the shift is a constant of the softmax
    top = torch.from_numpy(top)
    w = torch.exp(s - top[row])
    den = torch.zeros(case.m, heads, dtype=torch.float64).index_add_(0, row, w)
    a = w / den[row]
    z = torch.zeros(case.m, heads, d, dtype=torch.float64).index_add_(0, row, a[:, :, None] * y.view(case.n, heads, d)[col]).view(case.m, heads * d)
    z.backward(torch.from_numpy(np.array(case.g)).double())
    r = case.ref
    q = np.abs(r["ds"][:, :, None] * case.att.astype(np.float64)[None] * r["sl"]).max()
    terms = dict(z=0.0, dx=q, dy=max(q, np.abs(r["a"]).max() * np.abs(case.g).max()), datt=np.abs(r["ds"][:, :, None] * r["v"]).max())
    for name, got in (("z", z.detach().numpy()), ("dx", x.grad.numpy()), ("dy", y.grad.numpy()), ("datt", att.grad.numpy())):
        # relative to the size of the terms summed: with ns = 1 the sum dx_ic = att_c sum_e ds_e is 0 in exact arithmetic
        scale = max(np.abs(r[name]).max(), terms[name])
        assert np.abs(got - r[name]).max() <= 1e-12 * scale, name
    live = case.live
    lse = (top + torch.log(den)).detach().numpy()
    assert np.abs(lse[live] - r["lse"][live]).max() <= 1e-12 * np.abs(r["lse"][live]).max()


def _dot_sequential(a3, b3):
    """sum_c a[..., c] b[..., c] in fp32, one product and one add at a time."""
    out = np.zeros(np.broadcast_shapes(a3.shape, b3.shape)[:-1], F32)
    for c in range(b3.shape[-1]):
        out = (out + (a3[..., c] * b3[..., c]).astype(F32)).astype(F32)
    return out


def emulate_online(case):
    """The operator in fp32 NumPy: sequential dot products, the online softmax with ONE slot that takes a row's edges in ascending
    score order per head, so that every edge raises the running maximum and rescales (l, acc); the backward recomputes a_e from the
    fp32 lse and takes D from the fp32 z, as the kernels do; per-row sums; datt summed per row and then sequentially over the rows."""
    rowptr, col, H, ns = case.rowptr, case.col, case.heads, F32(case.ns)
    m, n, K = case.m, case.n, case.k
    d = K // H
    x3, y3, g3, att = ref.per_head(case.x, H), ref.per_head(case.y, H), ref.per_head(case.g, H), np.asarray(case.att, F32)
    row = ref.edge_rows(rowptr)
    u = (x3[row] + y3[col]).astype(F32)                                                 # ONE fp32 add
    sl = np.where(u > 0, F32(1), ns).astype(F32)
    v = np.where(u > 0, u, (ns * u).astype(F32)).astype(F32)
    s = _dot_sequential(att[None], v)
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
    D = _dot_sequential(g3, z)
    t = _dot_sequential(g3[row], y3[col])
    ds = (a * (t - D[row])).astype(F32)
    q = ((ds[:, :, None] * att[None]).astype(F32) * sl).astype(F32)
    into_y = ((a[:, :, None] * g3[row]).astype(F32) + q).astype(F32)
    pa = (ds[:, :, None] * v).astype(F32)
    dx, dy, datt = np.zeros((m, H, d), F32), np.zeros((n, H, d), F32), np.zeros((H, d), F32)
    for i in range(m):
        dx[i] = q[rowptr[i]:rowptr[i + 1]].sum(0, dtype=F32)
        datt = (datt + pa[rowptr[i]:rowptr[i + 1]].sum(0, dtype=F32)).astype(F32)
    order = np.argsort(col, kind="stable")
    cuts = np.searchsorted(col[order], np.arange(n + 1))
    for j in range(n):
        dy[j] = into_y[order[cuts[j]:cuts[j + 1]]].sum(0, dtype=F32)
    return dict(z=z.reshape(m, K), lse=lse, D=D, dx=dx.reshape(m, K), dy=dy.reshape(n, K), datt=datt)


@pytest.mark.parametrize("case", cases.all_cases(), ids=lambda c: c.name)
def test_bound_is_not_too_tight(case):
    frac = fractions(case, emulate_online(case))
    print(case.name, {k: round(v, 4) for k, v in frac.items()})
    assert all(v <= 1.0 for v in frac.values()), frac


def _softmax(case, s):
    row, m = case.ref["row"], case.m
    top = np.full((m, case.heads), -np.inf)
    np.maximum.at(top, row, s)
    w = np.exp(s - top[row])
    return w / ref.segment_sum(w, row, m)[row]


def _from_edges(case, s, a, keep_d=True, keep_sl=True, datt_from_u=False, q_in_dy=True):
    """The outputs from per-edge scores and weights in fp64, with switches for the planted faults."""
    H = case.heads
    r = case.ref
    row, col, m, n, K = r["row"], case.col, case.m, case.n, case.k
    y3, g3 = ref.per_head(case.y.astype(np.float64), H), ref.per_head(case.g.astype(np.float64), H)
    att3 = case.att.astype(np.float64)[None]
    z = ref.segment_sum(a[:, :, None] * y3[col], row, m)
    D = (g3 * z).sum(2)
    ds = a * ((g3[row] * y3[col]).sum(2) - (D[row] if keep_d else 0.0))
    q = ds[:, :, None] * att3 * (r["sl"] if keep_sl else 1.0)
    with np.errstate(divide="ignore"):
        top = s.max()
        lse = np.where(case.live[:, None], np.log(ref.segment_sum(np.exp(s - top), row, m)) + top, -np.inf)
    return dict(z=z.reshape(m, K), lse=lse, D=D, dx=ref.segment_sum(q, row, m).reshape(m, K),
                dy=ref.segment_sum(a[:, :, None] * g3[row] + (q if q_in_dy else 0.0), col, n).reshape(n, K),
                datt=(ds[:, :, None] * (r["u"] if datt_from_u else r["v"])).sum(0))


def fault_leaky_relu_outside_the_dot_product(case):
    """GAT v1's score: the nonlinearity applied to the sum instead of inside it."""
    t = (case.att.astype(np.float64)[None] * case.ref["u"]).sum(2)
    s = np.where(t > 0, t, case.ns * t)
    return _from_edges(case, s, _softmax(case, s))


def fault_bf16_scores(case):
    s = torch.from_numpy(case.ref["s"]).to(torch.bfloat16).to(torch.float64).numpy()
    return _from_edges(case, s, _softmax(case, s))


def fault_no_d_term(case):
    return _from_edges(case, case.ref["s"], case.ref["a"], keep_d=False)


def fault_sl_dropped_from_q(case):
    return _from_edges(case, case.ref["s"], case.ref["a"], keep_sl=False)


def fault_datt_from_u(case):
    return _from_edges(case, case.ref["s"], case.ref["a"], datt_from_u=True)


def fault_q_dropped_from_dy(case):
    return _from_edges(case, case.ref["s"], case.ref["a"], q_in_dy=False)


# fault -> the outputs that must miss the bound on at least one picked case (ns = 0.2; with ns = 1 `sl` and `u` / `v` coincide)
FAULTS = ((fault_leaky_relu_outside_the_dot_product, OUTPUTS), (fault_bf16_scores, ("z", "lse", "dx", "dy")),
          (fault_no_d_term, ("dx", "dy", "datt")), (fault_sl_dropped_from_q, ("dx", "dy")), (fault_datt_from_u, ("datt",)),
          (fault_q_dropped_from_dy, ("dy",)))


def test_the_unfaulted_restatement_passes():
    for heads, d in PICKED:
        case = cases.config_case(heads, d)
        frac = fractions(case, _from_edges(case, case.ref["s"], case.ref["a"]))
        assert all(v <= 1e-3 for v in frac.values()), (case.name, frac)


@pytest.mark.parametrize("fault,outputs", FAULTS, ids=lambda f: getattr(f, "__name__", ""))
def test_bound_is_not_too_loose(fault, outputs):
    picked = [cases.config_case(h, d) for h, d in PICKED]
    fracs = [fractions(c, fault(c)) for c in picked]
    print(fault.__name__, [{k: round(v, 2) for k, v in f.items()} for f in fracs])
    assert any(max(f.values()) > 1.0 for f in fracs), fault.__name__
    for name in outputs:
        assert any(f[name] > 1.0 for f in fracs), (fault.__name__, name)
    if fault not in (fault_leaky_relu_outside_the_dot_product, fault_bf16_scores):
        for name in set(OUTPUTS) - set(outputs):                           # and only there: a switch changes nothing else
            assert all(f[name] <= 1e-3 for f in fracs), (fault.__name__, name)
    if fault is fault_leaky_relu_outside_the_dot_product:                  # "this is not GAT v1": every output, on every picked case
        assert all(f[name] > 1.0 for f in fracs for name in OUTPUTS)


def test_python_mirror_of_the_domain_rule():
    from isplib_amd import cabi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    L = cabi.lib()
    top = cabi.DENSE_BYTES_MAX // 4
    table = DOMAIN_TABLE + ((top // 64, 8, 8, 64), (top // 64 + 1, 8, 8, 64), (top // 64, 4, 8, 64), (1000, 4, 4, top // 1000),
                            (1000, 4, 4, top // 1000 + 1))
    for rows, heads, d, ld in table:
        want = bool(L.isplib_gatv2_domain(rows, heads, d, ld))
        assert want == cabi.gatv2_serves(rows, heads, d, ld) == cabi.gat_serves(rows, heads, d, ld) == bool(L.isplib_gat_domain(rows, heads, d, ld)), \
            (rows, heads, d, ld)
    assert any(cabi.gatv2_serves(*t) for t in table) and not all(cabi.gatv2_serves(*t) for t in table)
    # stated once: the header's inline returns isplib_gat_serves(...)
    assert re.search(r"static inline int isplib_gatv2_serves\([^)]*\)\s*\{\s*return isplib_gat_serves\(rows_gathered, heads, d, ld\);\s*\}", header)


def test_header_exports_and_workspace_query_are_consistent():
    from isplib_amd import cabi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    names = ("isplib_gatv2_csr_hip", "isplib_gatv2_bw_rows_hip", "isplib_gatv2_bw_rows_workspace_bytes", "isplib_gatv2_bw_cols_hip",
             "isplib_gatv2_domain")
    L = cabi.lib()
    for name in names:
        assert name in cabi.EXPORTS and re.search(r"\b%s\s*\(" % name, header), name
        getattr(L, name)
    assert [n for n in cabi.EXPORTS if "gatv2" in n] == list(names)
    # one partial row of k floats per block of the rows kernel, whole 256-byte units, never 0; more rows or columns never need less
    assert cabi.gatv2_bw_rows_workspace_bytes(0, 64) == cabi.gatv2_bw_rows_workspace_bytes(64, 0) == 256
    prev = 0
    for m in (1, 3, 4, 5, 8, 9, 16, 17, 200, 1000, 232965):
        for k in (1, 47, 64, 512):
            ws = cabi.gatv2_bw_rows_workspace_bytes(m, k)
            assert ws % 256 == 0 and ws >= 256
            assert ws <= ((m * k * 4 + 255) // 256) * 256                    # at most one partial row per row: WAVES >= 1
            assert ws >= -(-m // 16) * k * 4                                 # and WAVES <= 16
        assert cabi.gatv2_bw_rows_workspace_bytes(m, 512) >= prev
        prev = cabi.gatv2_bw_rows_workspace_bytes(m, 512)
    assert cabi.last_error() == ""


def _adj(m, n):
    import isplib_amd
    rowptr = torch.arange(0, m + 1, dtype=torch.int64)
    col = torch.arange(m, dtype=torch.int64) % n
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n))


def test_plugin_refuses_bad_operands_before_any_library_call():
    import isplib_amd
    adj, sq = _adj(6, 4), _adj(4, 4)
    x, y, att = torch.zeros(6, 16), torch.zeros(4, 16), torch.zeros(2, 8)
    with pytest.raises(TypeError, match="GPU tensor"):
        isplib_amd.gatv2_matmul(adj, x, att, y, heads=2)                     # CPU tensors: there is no CPU path
    with pytest.raises(TypeError, match="GPU tensor"):
        sq.gatv2_matmul(y, torch.zeros(16))                                 # y=None on a square graph, 1-D att with one head: well-formed
    with pytest.raises(TypeError, match="GPU tensor"):
        sq.gatv2_matmul(y, torch.zeros(1, 16), heads=1)
    with pytest.raises(ValueError, match="square"):
        isplib_amd.gatv2_matmul(adj, x, att, heads=2)                        # y=None needs a square graph
    with pytest.raises(ValueError, match="2-D"):
        isplib_amd.gatv2_matmul(adj, x[0], att, y, heads=2)
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            isplib_amd.gatv2_matmul(adj, x.to(dt), att.to(dt), y.to(dt), heads=2)
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.gatv2_matmul(adj, x, att.to(torch.bfloat16), y, heads=2)
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.gatv2_matmul(adj, x, att, y.to(torch.float16), heads=2)
    with pytest.raises(TypeError, match="tensor"):
        isplib_amd.gatv2_matmul(adj, x.numpy(), att, y, heads=2)
    with pytest.raises(TypeError, match="tensor"):
        isplib_amd.gatv2_matmul(adj, x, [0.0] * 16, y, heads=2)
    with pytest.raises(ValueError, match="one row per column"):
        isplib_amd.gatv2_matmul(adj, x, att, torch.zeros(6, 16), heads=2)
    with pytest.raises(ValueError, match="one row per row"):
        isplib_amd.gatv2_matmul(adj, torch.zeros(4, 16), att, y, heads=2)
    with pytest.raises(ValueError, match="same width"):
        isplib_amd.gatv2_matmul(adj, torch.zeros(6, 8), att, y, heads=2)
    with pytest.raises(ValueError, match=r"`att` must be \[2, 8\]"):
        isplib_amd.gatv2_matmul(adj, x, torch.zeros(2, 4), y, heads=2)
    with pytest.raises(ValueError, match=r"`att` must be \[2, 8\]"):
        isplib_amd.gatv2_matmul(adj, x, torch.zeros(16), y, heads=2)         # a 1-D att needs heads == 1
    with pytest.raises(ValueError, match="heads \\* d"):
        isplib_amd.gatv2_matmul(adj, x, torch.zeros(3, 5), y, heads=3)
    with pytest.raises(ValueError, match="positive int"):
        isplib_amd.gatv2_matmul(adj, x, att, y, heads=0)
    with pytest.raises(ValueError, match="positive int"):
        isplib_amd.gatv2_matmul(adj, x, att, y, heads=True)
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.gatv2_matmul(adj, torch.zeros(6, 12), torch.zeros(2, 6), torch.zeros(4, 12), heads=2)      # d = 6
    with pytest.raises(ValueError, match="power of two"):
        isplib_amd.gatv2_matmul(adj, torch.zeros(6, 4), torch.zeros(2, 2), torch.zeros(4, 4), heads=2)        # d = 2
    with pytest.raises(ValueError, match="512"):
        adj.gatv2_matmul(torch.zeros(6, 513), torch.zeros(513), torch.zeros(4, 513))
    with pytest.raises(ValueError, match="512"):
        adj.gatv2_matmul(torch.zeros(6, 1024), torch.zeros(2, 512), torch.zeros(4, 1024), heads=2)
    assert isplib_amd.gatv2_matmul is isplib_amd.plugin.gatv2_matmul and "gatv2_matmul" in isplib_amd.__all__
    assert "ISPLIB_HALF" not in (isplib_amd.plugin.gatv2_matmul.__doc__ or "")


def test_ctypes_wrappers_refuse_bad_operands_before_the_call():
    from isplib_amd import cabi
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    colptr = torch.arange(0, 5, dtype=torch.int64)
    x, y, att, g = torch.zeros(6, 16), torch.zeros(4, 16), torch.zeros(2, 8), torch.zeros(6, 16)
    lse = torch.zeros(6, 2)
    with pytest.raises(TypeError, match="float32"):
        cabi.gatv2(rowptr, col, x, y.to(torch.bfloat16), att, 2)
    with pytest.raises(TypeError, match="float32"):
        cabi.gatv2(rowptr, col, x.to(torch.float16), y, att, 2)
    with pytest.raises(TypeError, match="float32"):
        cabi.gatv2(rowptr, col, x, y, att.to(torch.float16), 2)
    with pytest.raises(TypeError, match="int64"):
        cabi.gatv2(rowptr.to(torch.int32), col, x, y, att, 2)
    with pytest.raises(ValueError, match=r"`att` must be \[2, 8\]"):
        cabi.gatv2(rowptr, col, x, y, torch.zeros(2, 4), 2)
    with pytest.raises(ValueError, match=r"`att` must be a 2-D"):
        cabi.gatv2(rowptr, col, x, y, torch.zeros(16), 2)
    with pytest.raises(ValueError, match="contiguous"):
        cabi.gatv2(rowptr, col, x, y, torch.zeros(2, 16)[:, :8], 2)
    with pytest.raises(ValueError, match="unit inner stride"):
        cabi.gatv2(rowptr, col, x, torch.zeros(16, 4).t(), att, 2)
    with pytest.raises(ValueError, match=r"`y` must be \[4, 16\]"):
        cabi.gatv2(rowptr, col, x, torch.zeros(4, 8), att, 2)
    with pytest.raises(ValueError, match="heads \\* d"):
        cabi.gatv2(rowptr, col, x, y, torch.zeros(3, 5), 3)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.gatv2(rowptr, col, x, y, att, 2)                                # well-formed, but on the CPU
    with pytest.raises(ValueError, match="isplib_gat_serves"):
        cabi.gatv2(rowptr, col, torch.zeros(6, 12), torch.zeros(4, 12), torch.zeros(2, 6), 2)      # d = 6
    with pytest.raises(ValueError, match="isplib_gat_serves"):
        cabi.gatv2(rowptr, col, torch.zeros(6, 513), torch.zeros(4, 513), torch.zeros(1, 513), 1)
    with pytest.raises(ValueError, match=r"`lse` must be \[6, 2\]"):
        cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, g, torch.zeros(5, 2), 2)
    with pytest.raises(ValueError, match=r"\[6, 16\]"):
        cabi.gatv2_bw_rows(rowptr, col, x, y, att, torch.zeros(6, 15), g, lse, 2)
    with pytest.raises(ValueError, match="exactly when"):
        cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, g, lse, 2, want_datt=False, out=(torch.zeros(6, 16), torch.zeros(6, 2), torch.zeros(2, 8)))
    with pytest.raises(ValueError, match="uint8"):
        cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, g, lse, 2, workspace=torch.zeros(1024))
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, g, lse, 2)
    with pytest.raises(ValueError, match=r"`dsum` must be \[6, 2\]"):
        cabi.gatv2_bw_cols(colptr, col, x, y, att, g, lse, torch.zeros(6, 1), 2)
    with pytest.raises(ValueError, match=r"`x` must be \[6, 16\]"):
        cabi.gatv2_bw_cols(colptr, col, torch.zeros(6, 8), y, att, g, lse, lse, 2)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.gatv2_bw_cols(colptr, col, x, y, att, g, lse, lse, 2)
