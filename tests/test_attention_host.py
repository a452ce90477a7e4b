"""Row-softmax attention, host side (no GPU): the bound of tests/attention_ref.py is neither too tight (an fp32 emulation of the
online softmax in its worst order passes on every case) nor too loose (six planted faults each miss it), the Python mirror of the
domain rule agrees with the header's, and the plug-in and the ctypes wrappers refuse bad operands before any library call.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import attention_cases as cases
from tests import attention_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
OUTPUTS = ("z", "lse", "dx", "dy")


def fractions(case, got):
    """error / bound per output; lse over the rows that have entries (an empty row's -inf is compared for equality)."""
    live = case.live
    out = {}
    for name in OUTPUTS:
        if name == "lse":
            assert np.all(np.isneginf(np.asarray(got["lse"])[~live]))
            out[name] = ref.worst(np.asarray(got["lse"])[live], case.ref["lse"][live], case.bound["lse"][live])
        else:
            out[name] = ref.worst(got[name], case.ref[name], case.bound[name])
    return out


def emulate_online(case):
    """The online form in fp32 NumPy with ONE slot that takes a row's edges in ascending score order, so that every edge raises the
    running maximum and rescales (l, acc); the backward recomputes a_e from the fp32 lse as the kernels do."""
    rowptr, col, p = case.rowptr, case.col, F32(case.p)
    x, y, g = case.x, case.y, case.g
    m, n, k = case.m, y.shape[0], case.k
    row = ref.edge_rows(rowptr)
    s = (p * (x[row] * y[col]).sum(1, dtype=F32)).astype(F32)
    z, lse = np.zeros((m, k), F32), np.full(m, -np.inf, F32)
    with np.errstate(over="ignore", under="ignore"):
        for i in range(m):
            b, e = rowptr[i], rowptr[i + 1]
            if e == b:
                continue
            mrun, l, acc = F32(-np.finfo(F32).max), F32(0), np.zeros(k, F32)
            for q in b + np.argsort(s[b:e], kind="stable"):
                mnew = max(mrun, s[q])
                r, w = np.exp(F32(mrun - mnew)), np.exp(F32(s[q] - mnew))
                l, acc, mrun = F32(l * r + w), (acc * r + w * y[col[q]]).astype(F32), mnew
            z[i], lse[i] = acc / l, F32(mrun + np.log(l))
        a = np.exp(s - np.where(np.isfinite(lse), lse, F32(0))[row]).astype(F32)
    D = (g * z).sum(1, dtype=F32)
    ds = (a * ((g[row] * y[col]).sum(1, dtype=F32) - D[row])).astype(F32)
    dx, dy = np.zeros((m, k), F32), np.zeros((n, k), F32)
    for i in range(m):
        b, e = rowptr[i], rowptr[i + 1]
        dx[i] = p * (ds[b:e, None] * y[col[b:e]]).sum(0, dtype=F32)
    contrib = (a[:, None] * g[row] + (p * ds)[:, None] * x[row]).astype(F32)
    order = np.argsort(col, kind="stable")
    cuts = np.searchsorted(col[order], np.arange(n + 1))
    for j in range(n):
        dy[j] = contrib[order[cuts[j]:cuts[j + 1]]].sum(0, dtype=F32)
    return dict(z=z, lse=lse, dx=dx, dy=dy)


def test_every_case_is_inside_the_first_order_range():
    """The bound is first order in rho: rho_i <= 1e-3 on every row of every case.  The exception is arithmetic: delta s_e >=
    1e-5 |s_e|, so the case the issue asks for with scores spread over +-200 cannot go below 2e-3.  It is held to LARGE_RHO_MAX = 4e-3
    instead: the neglected term of exp(rho) - 1 is rho^2 / 2 <= 8e-6, 0.2 % of rho, and the bound carries 2 rho where the first-order
    analysis needs rho for the numerator and rho for the denominator.  The one-entry case is compared bit for bit, not by the bound."""
    for case in cases.all_cases():
        top = float(case.bound["rho"].max())
        if case.kind == "bounded":
            assert top <= ref.RHO_MAX, (case.name, top)
        elif case.kind == "large":
            assert ref.RHO_MAX < top <= cases.LARGE_RHO_MAX, (case.name, top)
            assert case.ref["s"].max() > 150 and case.ref["s"].min() < -150
            spread = np.zeros(case.m)
            np.maximum.at(spread, case.ref["row"], np.abs(case.ref["s"]))
            assert (spread > 100).sum() > case.m // 4                      # in real rows, not in one
    assert sorted({c.k for c in cases.bounded_cases()}) == sorted(cases.WIDTHS)


def test_the_graph_meets_every_loop_edge():
    rowptr, col = cases.graph()
    deg, indeg = np.diff(rowptr), np.bincount(col, minlength=cases.N)
    for k in cases.WIDTHS:
        g = cases.slots(k)
        want = {0, 1, g - 1, g, g + 1, 63, 64, 65, 129, cases.HUB}
        assert want <= set(deg.tolist()) and want <= set(indeg.tolist()), k
    assert 150 <= cases.N <= 250


@pytest.mark.parametrize("case", cases.all_cases(), ids=lambda c: c.name)
def test_bound_is_not_too_tight(case):
    frac = fractions(case, emulate_online(case))
    print(case.name, {k: round(v, 4) for k, v in frac.items()})
    assert all(v <= 1.0 for v in frac.values()), frac


def _from_edges(case, s, a, keep_d=True, keep_dsx=True, p=None):
    """The outputs from per-edge scores and weights in fp64, with switches for the planted faults."""
    p = case.p if p is None else p
    row, col, m, n = case.ref["row"], case.col, case.m, case.y.shape[0]
    ye, xe, ge = case.y[col].astype(np.float64), case.x[row].astype(np.float64), case.g[row].astype(np.float64)
    z = ref.segment_sum(a[:, None] * ye, row, m)
    D = (case.g.astype(np.float64) * z).sum(1)
    ds = a * ((ge * ye).sum(1) - (D[row] if keep_d else 0.0))
    dy = ref.segment_sum(a[:, None] * ge + ((p * ds)[:, None] * xe if keep_dsx else 0.0), col, n)
    with np.errstate(divide="ignore"):
        lse = np.where(case.live, np.log(ref.segment_sum(np.exp(s - s.max()), row, m)) + s.max(), -np.inf)
    return dict(z=z, lse=lse, dx=p * ref.segment_sum(ds[:, None] * ye, row, m), dy=dy)


def _softmax(case, s):
    row, m = case.ref["row"], case.m
    top = np.full(m, -np.inf)
    np.maximum.at(top, row, s)
    w = np.exp(s - top[row])
    return w / ref.segment_sum(w, row, m)[row]


def fault_bf16_scores(case):
    s = torch.from_numpy(case.ref["s"]).to(torch.bfloat16).to(torch.float64).numpy()
    return _from_edges(case, s, _softmax(case, s))


def fault_dropped_edge(case):
    keep = np.ones(case.col.size, bool)
    keep[case.rowptr[np.argmax(np.diff(case.rowptr) == 3)]] = False        # the first entry of a three-entry row
    s = np.where(keep, case.ref["s"], -np.inf)
    return _from_edges(case, np.where(keep, case.ref["s"], case.ref["s"].min()), _softmax(case, s))


def fault_scale_omitted(case):
    s = case.ref["s"] / case.p
    return _from_edges(case, s, _softmax(case, s), p=1.0)


def fault_no_d_term(case):
    return _from_edges(case, case.ref["s"], case.ref["a"], keep_d=False)


def fault_no_max_shift(case):
    s = case.ref["s"].astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp(s)                                                       # fp32: overflows from 88.7 on
        a = (w / ref.segment_sum(w.astype(np.float64), case.ref["row"], case.m)[case.ref["row"]].astype(F32)).astype(np.float64)
        return _from_edges(case, case.ref["s"], a)


def fault_no_ds_x_term(case):
    return _from_edges(case, case.ref["s"], case.ref["a"], keep_dsx=False)


FAULTS = (fault_bf16_scores, fault_dropped_edge, fault_scale_omitted, fault_no_d_term, fault_no_max_shift, fault_no_ds_x_term)


def test_the_unfaulted_restatement_passes():
    case = cases.width_case(33)
    frac = fractions(case, _from_edges(case, case.ref["s"], case.ref["a"]))
    assert all(v <= 1e-3 for v in frac.values()), frac


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f.__name__)
def test_bound_is_not_too_loose(fault):
    picked = [cases.width_case(k) for k in (3, 33, 129)] + [cases.large_case()]
    missed = [c.name for c in picked if max(fractions(c, fault(c)).values()) > 1.0]
    assert missed, fault.__name__
    if fault is fault_no_max_shift:
        got = fault(cases.large_case())
        assert "large" in missed and not np.all(np.isfinite(got["z"]))      # it overflows where the scores are large


def test_python_mirror_of_the_domain_rule():
    from isplib_amd import cabi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+ISPLIB_ATTENTION_K_MAX\s+(\d+)", header).group(1)) == cabi.ATTENTION_K_MAX == 512
    L = cabi.lib()
    top = cabi.DENSE_BYTES_MAX // 4
    for rows, k, ld in ((10, 0, 8), (10, 1, 1), (10, 512, 512), (10, 513, 513), (10, 8, 7), (10, 8, 8), (2 ** 31 - 1, 1, 1), (2 ** 31, 1, 1),
                        (0, 4, 4), (-1, 4, 4), (top // 64, 64, 64), (top // 64 + 1, 64, 64), (top // 64, 32, 64), (1000, 16, top // 1000),
                        (1000, 16, top // 1000 + 1)):
        assert bool(L.isplib_attention_domain(rows, k, ld)) == cabi.attention_serves(rows, k, ld), (rows, k, ld)
    assert cabi.attention_serves(10, 512, 512) and not cabi.attention_serves(10, 513, 513) and not cabi.attention_serves(10, 0, 8)
    assert not cabi.attention_serves(10, 8, 7) and not cabi.attention_serves(2 ** 31, 1, 1)
    assert cabi.attention_serves(top // 64, 64, 64) and not cabi.attention_serves(top // 64 + 1, 64, 64)
    for name in ("isplib_attention_csr_hip", "isplib_attention_bw_rows_hip", "isplib_attention_bw_cols_hip", "isplib_attention_domain"):
        assert name in cabi.EXPORTS and name in header
    assert "isplib_attention_serves" in header


def _adj(m, n):
    import isplib_amd
    rowptr = torch.arange(0, m + 1, dtype=torch.int64)
    col = torch.arange(m, dtype=torch.int64) % n
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n))


def test_plugin_refuses_bad_operands_before_any_library_call():
    import isplib_amd
    adj = _adj(6, 4)
    x, y = torch.zeros(6, 8), torch.zeros(4, 8)
    with pytest.raises(TypeError, match="GPU tensor"):
        isplib_amd.attention_matmul(adj, x, y)                               # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="2-D"):
        isplib_amd.attention_matmul(adj, x[0], y)
    with pytest.raises(ValueError, match="2-D"):
        isplib_amd.attention_matmul(adj, x, y[None])
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            isplib_amd.attention_matmul(adj, x.to(dt), y.to(dt))
    with pytest.raises(TypeError, match="tensor"):
        isplib_amd.attention_matmul(adj, x.numpy(), y)
    with pytest.raises(ValueError, match="one row per row"):
        isplib_amd.attention_matmul(adj, torch.zeros(5, 8), y)
    with pytest.raises(ValueError, match="one row per column"):
        isplib_amd.attention_matmul(adj, x, torch.zeros(6, 8))
    with pytest.raises(ValueError, match="one width"):
        isplib_amd.attention_matmul(adj, x, torch.zeros(4, 9))
    with pytest.raises(ValueError, match="square"):
        isplib_amd.attention_matmul(adj, x)                                  # y=None on a 6 x 4 matrix
    with pytest.raises(ValueError, match="512"):
        adj.attention_matmul(torch.zeros(6, 513), torch.zeros(4, 513))
    with pytest.raises(ValueError, match="512"):
        adj.attention_matmul(torch.zeros(6, 0), torch.zeros(4, 0))
    assert isplib_amd.attention_matmul is isplib_amd.plugin.attention_matmul and "attention_matmul" in isplib_amd.__all__


def test_ctypes_wrappers_refuse_bad_operands_before_the_call():
    from isplib_amd import cabi
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    x, y = torch.zeros(6, 8), torch.zeros(4, 8)
    with pytest.raises(TypeError, match="float32"):
        cabi.attention(rowptr, col, x.to(torch.bfloat16), y)
    with pytest.raises(TypeError, match="int64"):
        cabi.attention(rowptr.to(torch.int32), col, x, y)
    with pytest.raises(ValueError, match=r"\[6, k\]"):
        cabi.attention(rowptr, col, torch.zeros(5, 8), y)
    with pytest.raises(ValueError, match="x's width"):
        cabi.attention(rowptr, col, x, torch.zeros(4, 9))
    with pytest.raises(ValueError, match="unit inner stride"):
        cabi.attention(rowptr, col, torch.zeros(8, 6).t(), y)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.attention(rowptr, col, x, y)                                    # well-formed, but on the CPU
    with pytest.raises(ValueError, match="isplib_attention_serves"):
        cabi.attention(rowptr, col, torch.zeros(6, 513), torch.zeros(4, 513))
    with pytest.raises(ValueError, match="contiguous float32 tensor of 6"):
        cabi.attention_bw_rows(rowptr, col, x, y, x, x, torch.zeros(5))
    with pytest.raises(ValueError, match=r"\[6, 8\]"):
        cabi.attention_bw_cols(torch.arange(0, 5, dtype=torch.int64), col, x, y, torch.zeros(6, 7), torch.zeros(6), torch.zeros(6))
