"""The 16-bit attention operator, host side (no GPU): the bound of tests/attention16_ref.py is neither too tight (an fp32 NumPy
emulation of the kernels' one-pass form, rounded once, passes on every case and dtype) nor too loose (six planted faults each miss
it), the cases stay inside the range the bound is first order in, attention16_route is a pure and total function, and the header's
rules agree with their cabi twins.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import attention16_cases as c16
from tests import attention_cases as cases
from tests import attention_ref as ref
from tests import half_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BF, FP = torch.bfloat16, torch.float16
OUT16 = ("z", "dx", "dy")


def seg32(values, ids, count):
    """A segment sum accumulated in fp32, one term after the other."""
    out = np.zeros((count,) + values.shape[1:], F32)
    np.add.at(out, ids, values.astype(F32))
    return out


def emulate32(case, d_from_z16=False):
    """The kernels' arithmetic in fp32 NumPy, before the one rounding: the softmax relative to the row maximum, the backward's
    a_e = exp(s_e - lse_i) from the fp32 lse, and the one-pass form l, Dacc, Z, A1 -> D = Dacc / l, dx = p (A1 - D Z).
    `d_from_z16`: the planted fault D_i = <g_i, z16_i>."""
    rowptr, col, p = case.rowptr, case.col, F32(case.p)
    x, y, g = case.x, case.y, case.g
    m, n = case.m, y.shape[0]
    row = ref.edge_rows(rowptr)
    live = case.live
    s = (p * (x[row] * y[col]).sum(1, dtype=F32)).astype(F32)
    top = np.full(m, -np.finfo(F32).max, F32)
    np.maximum.at(top, row, s)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        w = np.exp(s - top[row]).astype(F32)
        l = seg32(w, row, m)
        z = np.where(live[:, None], seg32(w[:, None] * y[col], row, m) / np.where(live, l, F32(1))[:, None], F32(0)).astype(F32)
        lse = np.where(live, top + np.log(np.where(live, l, F32(1))), -np.inf).astype(F32)
        a = np.exp(s - np.where(live, lse, F32(0))[row]).astype(F32)
        t = (g[row] * y[col]).sum(1, dtype=F32)
        at = (a * t).astype(F32)
        lb, dacc = seg32(a, row, m), seg32(at, row, m)
        zb, a1 = seg32(a[:, None] * y[col], row, m), seg32(at[:, None] * y[col], row, m)
        D = np.where(live, dacc / np.where(live, lb, F32(1)), F32(0)).astype(F32)
        if d_from_z16:
            D = (g * half_ref.widen(half_ref.round16(z, case.dtype))).sum(1, dtype=F32)
        dx = np.where(live[:, None], p * (a1 - D[:, None] * zb), F32(0)).astype(F32)
        pds = (p * (a * (t - D[row]))).astype(F32)
        dy = seg32(pds[:, None] * x[row] + a[:, None] * g[row], col, n)
    return dict(z=z, lse=lse, dx=dx, dy=dy, D=D)


def rounded(case, got, how=half_ref.round16):
    """z, dx and dy rounded once to the case's dtype (and widened again for the comparison); lse and D stay fp32."""
    out = dict(got)
    for name in OUT16:
        out[name] = half_ref.widen(how(got[name], case.dtype))
    return out


def truncate16(a, dtype):
    """The planted fault: an fp32 array cut to `dtype` towards zero instead of rounded to nearest."""
    a = np.ascontiguousarray(a, F32)
    if dtype == BF:
        return torch.from_numpy((a.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)).to(BF)
    r = a.astype(np.float16)
    over = np.abs(r.astype(F32)) > np.abs(a)
    return torch.from_numpy(np.where(over, np.nextafter(r, np.float16(0)), r))


def test_every_case_is_inside_the_first_order_range():
    """rho_i <= 1e-3 on every row of every width case of both graphs and dtypes; the large-score case is held to LARGE_RHO_MAX as in
    tests/test_attention_host.py, which says why that keeps the bound first order."""
    tops = [float(case.bound["rho"].max()) for case in c16.bounded_cases()]
    print("largest rho over the width cases:", max(tops))
    assert max(tops) <= ref.RHO_MAX
    assert sorted({c.k for c in c16.bounded_cases()}) == sorted(c16.WIDTHS)
    for dtype in c16.DTYPES:
        case = c16.large_case(dtype)
        top = float(case.bound["rho"].max())
        assert ref.RHO_MAX < top <= cases.LARGE_RHO_MAX, (case.name, top)
        assert case.ref["s"].max() > 150 and case.ref["s"].min() < -150


def test_the_graphs_meet_every_loop_edge():
    degs = [(np.diff(rowptr), np.bincount(col, minlength=c16.N)) for rowptr, col in c16.graphs().values()]
    seen_rows = set().union(*(set(d.tolist()) for d, _ in degs))
    seen_cols = set().union(*(set(i.tolist()) for _, i in degs))
    for k in c16.WIDTHS:
        g = c16.slots(k)
        want = {0, 1, g - 1, g, g + 1, 31, 32, 33, 63, 64, 65, 129} - {-1}
        assert want <= seen_rows and want <= seen_cols, (k, want - seen_rows, want - seen_cols)
    assert {c16.slots(k) for k in c16.WIDTHS} == {16, 8, 4, 2, 1}
    rowptr, col = c16.graph2()
    assert any(np.unique(col[rowptr[i]:rowptr[i + 1]]).size < rowptr[i + 1] - rowptr[i] for i in range(c16.N))       # duplicates
    assert any(np.any(np.diff(col[rowptr[i]:rowptr[i + 1]]) < 0) for i in range(c16.N))                             # unsorted rows


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
@pytest.mark.parametrize("k", c16.WIDTHS)
def test_bound_is_not_too_tight(k, dtype):
    for graph in ("g1", "g2"):
        case = c16.width_case(k, dtype, graph)
        frac = c16.fractions(case, rounded(case, emulate32(case)))
        print(case.name, {n: round(v, 4) for n, v in frac.items()})
        assert all(v <= 1.0 for v in frac.values()), (case.name, frac)


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
def test_bound_is_not_too_tight_on_the_special_cases(dtype):
    for case in (c16.large_case(dtype), c16.single_case(dtype)):
        frac = c16.fractions(case, rounded(case, emulate32(case)))
        print(case.name, {n: round(v, 4) for n, v in frac.items()})
        assert all(v <= 1.0 for v in frac.values()), (case.name, frac)


# ---- planted faults: each must MISS the bound ---------------------------------------------------------------------------------------

def from_edges(case, s, a):
    """The outputs in fp64 from per-edge scores and weights (D_i = sum_e a_e t_e), then rounded once."""
    row, col, m, n, p = case.ref["row"], case.col, case.m, case.y.shape[0], case.p
    ye, xe, ge = case.y[col].astype(np.float64), case.x[row].astype(np.float64), case.g[row].astype(np.float64)
    t = (ge * ye).sum(1)
    D = ref.segment_sum(a * t, row, m)
    ds = a * (t - D[row])
    top = np.full(m, -np.inf)
    np.maximum.at(top, row, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = np.where(case.live, np.log(ref.segment_sum(np.exp(s - np.where(case.live, top, 0.0)[row]), row, m)) + top, -np.inf)
    got = dict(z=ref.segment_sum(a[:, None] * ye, row, m), lse=lse, D=D, dx=p * ref.segment_sum(ds[:, None] * ye, row, m),
               dy=ref.segment_sum(a[:, None] * ge + (p * ds)[:, None] * xe, col, n))
    return rounded(case, got)


def softmax(case, s):
    row, m = case.ref["row"], case.m
    top = np.full(m, -np.inf)
    np.maximum.at(top, row, s)
    w = np.exp(s - top[row])
    return w / ref.segment_sum(w, row, m)[row]


def worst_of(case, got):
    return max(c16.fractions(case, got).values())


def test_the_unfaulted_restatement_passes():
    for dtype in c16.DTYPES:
        case = c16.width_case(30, dtype)
        assert worst_of(case, from_edges(case, case.ref["s"], case.ref["a"])) <= 1.0


def test_fault_outputs_truncated_instead_of_rounded():
    """Asserted case by case: every bf16 width, and fp16 up to K = 64 (at K = 512 fp16 the fp32 part of the bound exceeds an ulp)."""
    picked = [c16.width_case(k, BF) for k in c16.WIDTHS] + [c16.width_case(k, FP) for k in c16.WIDTHS if k <= 64]
    for case in picked:
        assert worst_of(case, rounded(case, emulate32(case), truncate16)) > 1.0, case.name


def test_fault_z_accumulated_in_16_bits():
    for dtype in c16.DTYPES:
        case = c16.width_case(64, dtype)
        got = emulate32(case)
        row, col = case.ref["row"], case.col
        a = np.exp(case.ref["s"] - np.where(case.live, case.ref["lse"], 0.0)[row]).astype(F32)
        z = torch.zeros((case.m, case.k), dtype=dtype)
        for e in range(col.size):                                            # the running sum rounded after every edge
            z[row[e]] = (z[row[e]].float() + torch.from_numpy(a[e] * case.y[col[e]])).to(dtype)
        got["z"] = half_ref.widen(z)
        assert c16.fractions(case, rounded(case, got), ("z",))["z"] > 1.0, case.name


def test_fault_scores_rounded_to_16_bits():
    for dtype in c16.DTYPES:
        missed = []
        for k in (8, 30, 64, 512):
            case = c16.width_case(k, dtype)
            s = half_ref.widen(half_ref.round16(case.ref["s"], dtype)).astype(np.float64)
            missed.append(worst_of(case, from_edges(case, s, softmax(case, s))) > 1.0)
        assert any(missed), dtype


def test_fault_d_taken_from_the_rounded_z():
    """Why the kernel does not read z: with g aligned to z at K = 512 in bf16, D = <g, z16> carries u sum |g z| into every ds_e."""
    base = c16.width_case(512, BF)
    aligned = c16.Case16("k512-aligned-g", base.rowptr, base.col, np.array(base.x), np.array(base.y),
                         (base.ref["z"] * 8.0).astype(F32), base.p, BF)
    assert worst_of(aligned, rounded(aligned, emulate32(aligned))) <= 1.0    # the one-pass form passes on the same case
    frac = c16.fractions(aligned, rounded(aligned, emulate32(aligned, d_from_z16=True)))
    print(aligned.name, {n: round(v, 3) for n, v in frac.items()})
    assert frac["D"] > 1.0 and max(frac["dx"], frac["dy"]) > 1.0


def test_fault_dropped_edge():
    for dtype in c16.DTYPES:
        case = c16.width_case(30, dtype)
        keep = np.ones(case.col.size, bool)
        keep[case.rowptr[np.argmax(np.diff(case.rowptr) == 3)]] = False      # the first entry of a three-entry row
        a = softmax(case, np.where(keep, case.ref["s"], -np.inf))
        assert worst_of(case, from_edges(case, np.where(keep, case.ref["s"], case.ref["s"].min()), a)) > 1.0


def test_fault_ragged_tail_counted_twice():
    """K % 8 != 0 with the last vector shifted back: its first components are columns the neighbouring lane multiplies too."""
    for dtype in c16.DTYPES:
        for k in (10, 30, 510):
            case = c16.width_case(k, dtype)
            dup = slice(k - 8, 8 * (k // 8))
            row, col = case.ref["row"], case.col
            s = case.ref["s"] + case.p * (case.x[row][:, dup].astype(np.float64) * case.y[col][:, dup]).sum(1)
            assert worst_of(case, from_edges(case, s, softmax(case, s))) > 1.0, case.name


# ---- the route and the rules -----------------------------------------------------------------------------------------------------------

def test_attention16_route_is_pure_and_total(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import attention16_route as route
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_ATTENTION", raising=False)
    for dtype in (BF, FP):
        for mode in ("convert", "native", "auto", "nonsense"):
            for k in (7, 63, 6, 8, 512, 514):
                for pitch in (k + 1, k + 2, k):
                    for n in (2000, 2 ** 31):
                        got = route(dtype, k, pitch, n, mode)
                        inside = k % 2 == 0 and 8 <= k <= 512 and n < 2 ** 31          # an odd pitch is packed
                        if mode == "native":
                            want = "attention16" if inside else "convert"
                        elif mode == "auto":
                            ld = pitch if pitch % 2 == 0 else k
                            want = "attention16" if inside and cabi.attention16_native_pays(n, ld) else "convert"
                        else:
                            want = "convert"
                        assert got == want, (dtype, mode, k, pitch, n)
        assert route(dtype, 64, 64, 0xE0000000 // 128, "native") == "attention16"       # the operand at the descriptor's limit
        assert route(dtype, 64, 64, 0xE0000000 // 128 + 1, "native") == "convert"
        assert route(dtype, 64, 0xE0000000 // 2 // 1000 + 2, 1000, "native") == "attention16"   # too wide a pitch is packed
    for mode in ("convert", "native", "auto"):
        assert route(torch.float32, 64, 64, 2000, mode) == "convert" and route(torch.float64, 64, 64, 2000, mode) == "convert"
    # the mode comes from ISPLIB_HALF_ATTENTION when it is not given; unset counts as convert, and ISPLIB_HALF=convert wins
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_ATTENTION", "native")
    assert route(BF, 64, 64, 2000) == "attention16" and route(BF, 63, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "auto")
    assert route(BF, 64, 64, 2000) == "attention16"
    monkeypatch.setenv("ISPLIB_HALF_ATTENTION", "auto")
    assert route(BF, 64, 64, 2000) == route(BF, 64, 64, 2000, "auto")
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "native")
    monkeypatch.setenv("ISPLIB_HALF_ATTENTION", "nonsense")
    assert route(BF, 64, 64, 2000) == "convert"


def _library():
    try:
        from isplib_amd import cabi
        return cabi, cabi.lib()
    except (ImportError, OSError) as exc:
        pytest.skip(f"the built library is absent: {exc}")


def test_header_rules_match_their_cabi_twins():
    cabi, L = _library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+ISPLIB_ATTENTION16_K_MIN\s+(\d+)", header).group(1)) == cabi.ATTENTION16_K_MIN == 8
    assert int(re.search(r"#define\s+ISPLIB_ATTENTION16_K_MAX\s+(\d+)", header).group(1)) == cabi.ATTENTION16_K_MAX == 512
    top = cabi.DENSE_BYTES_MAX // 2
    for rows, k, ld in ((10, 0, 8), (10, 6, 6), (10, 8, 8), (10, 9, 10), (10, 10, 11), (10, 10, 12), (10, 512, 512), (10, 514, 514),
                        (10, 16, 14), (2 ** 31 - 1, 8, 8), (2 ** 31, 8, 8), (0, 8, 8), (-1, 8, 8), (top // 64, 64, 64),
                        (top // 64 + 1, 64, 64), (top // 64, 32, 64), (1000, 16, top // 1000), (1000, 16, top // 1000 + 2)):
        assert bool(L.isplib_attention16_domain(rows, k, ld)) == cabi.attention16_serves(rows, k, ld), (rows, k, ld)
    assert cabi.attention16_serves(10, 8, 8) and cabi.attention16_serves(10, 512, 512) and not cabi.attention16_serves(10, 514, 514)
    assert not cabi.attention16_serves(10, 6, 6) and not cabi.attention16_serves(10, 9, 10) and not cabi.attention16_serves(10, 10, 11)
    assert cabi.attention16_serves(top // 64, 64, 64) and not cabi.attention16_serves(top // 64 + 1, 64, 64)
    for rows, ld in ((0, 64), (1000, 64), (232_965, 64), (232_965, 128), (2 ** 20, 128), (2 ** 20 + 1, 128), (2_449_029, 128), (2_449_029, 512)):
        assert bool(L.isplib_attention16_auto(rows, ld)) == cabi.attention16_native_pays(rows, ld), (rows, ld)
    declared = set(re.findall(r"^(?:int|size_t|void|const char \*|float)\s+\*?(\w+)\(", header, re.M))
    names = {"isplib_attention16_csr_hip", "isplib_attention16_bw_rows_hip", "isplib_attention16_bw_cols_hip", "isplib_attention16_domain",
             "isplib_attention16_auto"}
    assert names <= declared & set(cabi.EXPORTS)
    assert "static inline int isplib_attention16_serves(int64_t rows_gathered, int64_t k, int64_t ld)" in header
    assert "static inline int isplib_attention16_native_pays(int64_t rows_gathered, int64_t ld)" in header
    for name in names:
        getattr(L, name)


def test_plugin_and_wrappers_refuse_before_any_library_call(monkeypatch):
    import isplib_amd
    cabi, _ = _library()
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (6, 4))
    x, y = torch.zeros(6, 8, dtype=BF), torch.zeros(4, 8, dtype=BF)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_ATTENTION", raising=False)
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.attention_matmul(adj, x, y)                               # unset: as it always was
    monkeypatch.setenv("ISPLIB_HALF_ATTENTION", "native")
    with pytest.raises(TypeError, match="one dtype"):
        isplib_amd.attention_matmul(adj, x, y.to(FP))
    with pytest.raises(TypeError, match="one dtype"):
        isplib_amd.attention_matmul(adj, x, y.float())
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.attention_matmul(adj, x.float(), y)
    with pytest.raises(TypeError, match="GPU tensor"):
        isplib_amd.attention_matmul(adj, x, y)                               # CPU tensors: what the conversion route raises
    with pytest.raises(ValueError, match="one width"):
        isplib_amd.attention_matmul(adj, x, torch.zeros(4, 10, dtype=BF))
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        cabi.attention16(rowptr, col, x.float(), y)
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.attention16(rowptr, col, x, y.to(FP))
    with pytest.raises(ValueError, match="even pitch"):
        cabi.attention16(rowptr, col, torch.zeros(6, 9, dtype=BF)[:, :8], y)
    with pytest.raises(ValueError, match="isplib_attention16_serves"):
        cabi.attention16(rowptr, col, torch.zeros(6, 6, dtype=BF), torch.zeros(4, 6, dtype=BF))
    with pytest.raises(ValueError, match="contiguous float32 tensor of 6"):
        cabi.attention16_bw_rows(rowptr, col, x, y, x, torch.zeros(5))
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.attention16(rowptr, col, x, y)                                  # well-formed, but on the CPU
