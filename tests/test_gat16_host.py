"""The 16-bit GAT operator, host side (no GPU): the bound of tests/gat16_ref.py is neither too tight (an fp32 NumPy emulation of the
kernels' form -- the online forward with a rescale on every edge, the one-pass rows backward P - D Q, one rounding -- passes on every
case) nor too loose (six planted faults each miss it), gat16_route is a pure and total function, and the header's rules agree with
their cabi twins (the static inline functions compiled here into a scrap library).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import gat16_cases as c16
from tests import gat_ref as ref
from tests import half_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BF, FP = torch.bfloat16, torch.float16
OUT16 = ("z", "dy")


def seg32(values, ids, count):
    """A segment sum accumulated in fp32, one term after the other."""
    out = np.zeros((count,) + values.shape[1:], F32)
    np.add.at(out, ids, values.astype(F32))
    return out


def emulate32(case, d_from_z16=False):
    """The kernels' arithmetic in fp32 NumPy, before the one rounding.  Forward: the online form with ONE slot that takes a row's edges
    in ascending score order per head, so that every edge raises the running maximum and rescales (l, acc).  Backward: a_e = exp(s_e -
    lse) from the fp32 lse and the one-pass form l, Dacc, P, Q -> D = Dacc / l, d a_dst = P - D Q.  `d_from_z16`: the planted fault
    D[i,h] = <g_i, z16_i>_h."""
    rowptr, col, H, ns = case.rowptr, case.col, case.heads, F32(case.ns)
    m, n, K = case.m, case.n, case.k
    d = K // H
    y3, g3 = ref.per_head(case.y, H), ref.per_head(case.g, H)
    row = ref.edge_rows(rowptr)
    u = (case.a_dst[row] + case.a_src[col]).astype(F32)
    s = np.where(u > 0, u, (ns * u).astype(F32)).astype(F32)
    sl = np.where(u > 0, F32(1), ns).astype(F32)
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
    live = case.live[:, None]
    t = (g3[row] * y3[col]).sum(2, dtype=F32)
    asl = (a * sl).astype(F32)
    l1 = np.where(live, seg32(a, row, m), F32(1))
    D = np.where(live, seg32(a * t, row, m) / l1, F32(0)).astype(F32)
    if d_from_z16:
        D = (g3 * ref.per_head(half_ref.widen(half_ref.round16(z.reshape(m, K), case.dtype)), H)).sum(2, dtype=F32)
    dadst = np.where(live, seg32(asl * t, row, m) - D * seg32(asl, row, m), F32(0)).astype(F32)
    du = (a * (t - D[row]) * sl).astype(F32)
    return dict(z=z.reshape(m, K), lse=lse, D=D, dadst=dadst, dasrc=seg32(du, col, n),
                dy=seg32((a[:, :, None] * g3[row]).astype(F32), col, n).reshape(n, K))


def rounded(case, got, how=half_ref.round16):
    """z and dy rounded once to the case's dtype (and widened again for the comparison); everything else stays fp32."""
    out = dict(got)
    for name in OUT16:
        out[name] = half_ref.widen(how(got[name], case.dtype))
    return out


def worst_of(case, got):
    return max(c16.fractions(case, got).values())


def test_the_cases_cover_every_instantiation_and_head_form():
    """Every LPR by its first, last and a ragged width; heads of one lane up to half a slot; head counts that are no power of two; one
    fp16 configuration per LPR; every case inside the first-order range (each Case16 asserts rho <= RHO_MAX when it is built)."""
    one = sorted(d for h, d in c16.CONFIGS if h == 1)
    assert one == [8, 10, 30, 32, 34, 46, 64, 66, 130, 258, 510, 512]
    assert {c16.lanes_per_row(d) for d in one} == {4, 8, 16, 32, 64}
    multi = [(h, d) for h, d in c16.CONFIGS if h > 1]
    assert {d // 8 for _, d in multi} == {1, 2, 4, 8, 16, 32} and any(h & (h - 1) for h, _ in multi)
    assert all(d >= 8 and d & (d - 1) == 0 and h * d <= 512 for h, d in multi)
    assert sorted(c16.lanes_per_row(h * d) for h, d in c16.FP16_CONFIGS) == [4, 8, 16, 32, 64]
    assert len(c16.config_cases()) == len(c16.CONFIGS) + len(c16.FP16_CONFIGS) + len(c16.GRAPH2_CONFIGS)
    for case in c16.special_cases():
        assert float(case.bound["rho"].max()) <= ref.RHO_MAX, case.name
    assert {c.ns for c in c16.slope_cases()} == {0.0, 1.0} and len(c16.slope_cases()) == 6


@pytest.mark.parametrize("spec", c16.config_cases(), ids=c16.case_id)
def test_bound_is_not_too_tight(spec):
    case = c16.config_case(spec[0], spec[1], spec[2], graph=spec[3])
    frac = c16.fractions(case, rounded(case, emulate32(case)))
    print(case.name, {n: round(v, 4) for n, v in frac.items()})
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)


@pytest.mark.parametrize("case", c16.special_cases(), ids=lambda c: c.name)
def test_bound_is_not_too_tight_on_the_special_cases(case):
    frac = c16.fractions(case, rounded(case, emulate32(case)))
    print(case.name, {n: round(v, 4) for n, v in frac.items()})
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)


# ---- planted faults: each must MISS the bound ---------------------------------------------------------------------------------------

def from_edges(case, s, a, keep_slope=True):
    """The outputs in fp64 from per-edge scores and weights (D = sum_e a_e t_e), then rounded once."""
    H, ns = case.heads, case.ns
    row, col, m, n, K = case.ref["row"], case.col, case.m, case.n, case.k
    y3, g3 = ref.per_head(case.y.astype(np.float64), H), ref.per_head(case.g.astype(np.float64), H)
    t = (g3[row] * y3[col]).sum(2)
    D = ref.segment_sum(a * t, row, m)
    du = a * (t - D[row]) * (np.where(case.ref["u"] > 0, 1.0, ns) if keep_slope else 1.0)
    top = np.full((m, H), -np.inf)
    np.maximum.at(top, row, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        shift = np.where(case.live[:, None], top, 0.0)
        lse = np.where(case.live[:, None], np.log(ref.segment_sum(np.exp(s - shift[row]), row, m)) + shift, -np.inf)
    got = dict(z=ref.segment_sum(a[:, :, None] * y3[col], row, m).reshape(m, K), lse=lse, D=D, dadst=ref.segment_sum(du, row, m),
               dasrc=ref.segment_sum(du, col, n), dy=ref.segment_sum(a[:, :, None] * g3[row], col, n).reshape(n, K))
    return rounded(case, got)


def softmax(case, s):
    row, m = case.ref["row"], case.m
    top = np.full((m, case.heads), -np.inf)
    np.maximum.at(top, row, s)
    w = np.exp(s - top[row])
    return w / ref.segment_sum(w, row, m)[row]


def picked():
    return [c16.config_case(1, 46), c16.config_case(8, 8), c16.config_case(3, 128), c16.large_case()]


def test_the_unfaulted_restatement_passes():
    for case in picked():
        assert worst_of(case, from_edges(case, case.ref["s"], case.ref["a"])) <= 1.0, case.name


def test_fault_slope_dropped_from_du():
    case = c16.config_case(8, 8)
    frac = c16.fractions(case, from_edges(case, case.ref["s"], case.ref["a"], keep_slope=False))
    assert frac["dadst"] > 1.0 and frac["dasrc"] > 1.0 and frac["z"] <= 1.0 and frac["dy"] <= 1.0 and frac["D"] <= 1.0


def test_fault_d_taken_from_the_rounded_z():
    """Why the rows kernel does not read z: with g aligned to z at K = 512 in bf16, D = <g, z16> carries u sum |g z| into every du_e."""
    base = c16.config_case(1, 512)
    aligned = c16.Case16("h1d512-aligned-g", base.rowptr, base.col, np.array(base.y), base.a_dst, base.a_src,
                         (base.ref["z"] * 8.0).astype(F32), 1, base.ns, BF)
    assert worst_of(aligned, rounded(aligned, emulate32(aligned))) <= 1.0    # the one-pass form passes on the same case
    frac = c16.fractions(aligned, rounded(aligned, emulate32(aligned, d_from_z16=True)))
    print(aligned.name, {n: round(v, 3) for n, v in frac.items()})
    assert frac["D"] > 1.0 and max(frac["dadst"], frac["dasrc"]) > 1.0


def test_fault_dropped_edge():
    for case in picked()[:3]:
        keep = np.ones(case.col.size, bool)
        keep[case.rowptr[np.argmax(np.diff(case.rowptr) == 3)]] = False      # the first entry of a three-entry row
        a = softmax(case, np.where(keep[:, None], case.ref["s"], -np.inf))
        assert worst_of(case, from_edges(case, np.where(keep[:, None], case.ref["s"], case.ref["s"].min()), a)) > 1.0, case.name


def test_fault_a_e_without_the_maximum_shift():
    case = c16.large_case()
    s = case.ref["s"].astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp(s)                                                       # fp32: overflows from 88.7 on
        a = (w / ref.segment_sum(w.astype(np.float64), case.ref["row"], case.m)[case.ref["row"]].astype(F32)).astype(np.float64)
        got = from_edges(case, case.ref["s"], a)
    assert not np.all(np.isfinite(got["z"])) and worst_of(case, got) > 1.0


def test_fault_a_src_of_the_wrong_head():
    for case in (c16.config_case(8, 8), c16.config_case(3, 128)):
        u = case.a_dst.astype(np.float64)[case.ref["row"]] + np.roll(case.a_src.astype(np.float64), 1, axis=1)[case.col]
        s = np.where(u > 0, u, case.ns * u)
        assert worst_of(case, from_edges(case, s, softmax(case, s))) > 1.0, case.name


def truncate16(a, dtype):
    """An fp32 array cut to bf16 towards zero instead of rounded to nearest."""
    assert dtype == BF
    a = np.ascontiguousarray(a, F32)
    return torch.from_numpy((a.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)).to(BF)


def through_fp16(a, dtype):
    """An fp32 array rounded to fp16 and then to bf16: two roundings."""
    assert dtype == BF
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(FP).to(BF)


@pytest.mark.parametrize("how", (truncate16, through_fp16), ids=lambda f: f.__name__)
def test_fault_z_rounded_twice_or_truncated(how):
    for case in picked()[:3]:
        got = rounded(case, emulate32(case))
        got["z"] = half_ref.widen(how(emulate32(case)["z"], case.dtype))
        assert c16.fractions(case, got, ("z",))["z"] > 1.0, case.name


# ---- the route and the rules -----------------------------------------------------------------------------------------------------------

def test_gat16_route_is_pure_and_total(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import gat16_route as route
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_GAT", raising=False)
    for dtype in (BF, FP):
        for mode in ("convert", "native", "auto", "nonsense"):
            for heads, d in ((1, 7), (1, 63), (1, 6), (1, 8), (1, 512), (1, 514), (8, 4), (8, 8), (2, 12), (64, 8), (65, 8), (3, 128), (2, 2)):
                k = heads * d
                for pitch in (k + 1, k + 2, k):
                    for n in (2000, 2 ** 31):
                        got = route(dtype, heads, d, pitch, n, mode)
                        shape = (d % 2 == 0) if heads == 1 else (d >= 8 and d & (d - 1) == 0)
                        inside = shape and 8 <= k <= 512 and n < 2 ** 31             # an odd pitch is packed
                        if mode == "native":
                            want = "gat16" if inside else "convert"
                        elif mode == "auto":
                            ld = pitch if pitch % 2 == 0 else k
                            want = "gat16" if inside and cabi.gat16_native_pays(n, ld) else "convert"
                        else:
                            want = "convert"
                        assert got == want, (dtype, mode, heads, d, pitch, n)
        assert route(dtype, 8, 8, 64, 0xE0000000 // 128, "native") == "gat16"            # the operand at the descriptor's limit
        assert route(dtype, 8, 8, 64, 0xE0000000 // 128 + 1, "native") == "convert"
        assert route(dtype, 8, 8, 0xE0000000 // 2 // 1000 + 2, 1000, "native") == "gat16"    # too wide a pitch is packed
    for mode in ("convert", "native", "auto"):
        assert route(torch.float32, 8, 8, 64, 2000, mode) == "convert" and route(torch.float64, 8, 8, 64, 2000, mode) == "convert"
    # the mode comes from ISPLIB_HALF_GAT when it is not given; unset counts as convert, and ISPLIB_HALF=convert wins
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_GAT", "native")
    assert route(BF, 8, 8, 64, 2000) == "gat16" and route(BF, 1, 63, 64, 2000) == "convert" and route(BF, 8, 4, 32, 2000) == "convert"
    assert route(BF, 8, 8, 65, 2000) == "gat16"                                          # an odd pitch: packed
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "auto")
    assert route(BF, 8, 8, 64, 2000) == "gat16"
    monkeypatch.setenv("ISPLIB_HALF_GAT", "auto")
    assert route(BF, 8, 8, 64, 2000) == route(BF, 8, 8, 64, 2000, "auto")
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "native")
    monkeypatch.setenv("ISPLIB_HALF_GAT", "nonsense")
    assert route(BF, 8, 8, 64, 2000) == "convert"


_RULES_SRC = r"""
#include "isplib_hip.h"
extern "C" int gat16_serves(long long rows, long long heads, long long d, long long ld) { return isplib_gat16_serves(rows, heads, d, ld); }
extern "C" int gat16_pays(long long rows, long long ld) { return isplib_gat16_native_pays(rows, ld); }
"""

SERVES_TABLE = (
    # rows, heads, d, ld
    (10, 1, 8, 8), (10, 1, 6, 6), (10, 1, 7, 8), (10, 1, 9, 10), (10, 1, 10, 10), (10, 1, 10, 11), (10, 1, 10, 12), (10, 1, 512, 512),
    (10, 1, 514, 514), (10, 1, 0, 8), (10, 0, 8, 8), (10, -1, 8, 8), (10, 2, 4, 8), (10, 2, 8, 16), (10, 2, 8, 14), (10, 2, 8, 17),
    (10, 2, 12, 24), (10, 2, 6, 12), (10, 8, 8, 64), (10, 8, 8, 66), (10, 64, 8, 512), (10, 65, 8, 520), (10, 33, 8, 264), (10, 5, 8, 40),
    (10, 3, 16, 48), (10, 3, 128, 384), (10, 2, 256, 512), (10, 2, 512, 1024), (10, 4, 2, 8), (10, 8, 1, 8), (10, 512, 1, 512),
    (2 ** 31 - 1, 1, 8, 8), (2 ** 31, 1, 8, 8), (0, 2, 8, 16), (-1, 2, 8, 16), (2 ** 40, 2 ** 40, 2 ** 40, 2 ** 40),
)


def test_header_rules_match_their_cabi_twins(tmp_path):
    from isplib_amd import cabi
    src, so = tmp_path / "rules.cpp", tmp_path / "rules.so"
    src.write_text(_RULES_SRC)
    subprocess.run(["g++", "-shared", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True, timeout=120)
    H = ctypes.CDLL(str(so))
    H.gat16_serves.argtypes = [ctypes.c_longlong] * 4
    H.gat16_pays.argtypes = [ctypes.c_longlong] * 2
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+ISPLIB_GAT16_K_MIN\s+(\d+)", header).group(1)) == cabi.GAT16_K_MIN == 8
    assert int(re.search(r"#define\s+ISPLIB_GAT16_K_MAX\s+(\d+)", header).group(1)) == cabi.GAT16_K_MAX == 512
    top = cabi.DENSE_BYTES_MAX // 2
    table = SERVES_TABLE + ((top // 64, 8, 8, 64), (top // 64 + 1, 8, 8, 64), (top // 64, 4, 8, 64), (1000, 2, 8, top // 1000),
                            (1000, 2, 8, top // 1000 + 2))
    for rows, heads, d, ld in table:
        assert bool(H.gat16_serves(rows, heads, d, ld)) == cabi.gat16_serves(rows, heads, d, ld), (rows, heads, d, ld)
    inside = ((10, 1, 8, 8), (10, 1, 10, 10), (10, 1, 10, 12), (10, 1, 512, 512), (10, 2, 8, 16), (10, 8, 8, 66), (10, 64, 8, 512),
              (10, 33, 8, 264), (10, 3, 128, 384), (10, 2, 256, 512), (top // 64, 8, 8, 64))
    outside = ((10, 1, 6, 6), (10, 1, 7, 8), (10, 1, 9, 10), (10, 1, 10, 11), (10, 1, 514, 514), (10, 0, 8, 8), (10, 2, 4, 8), (10, 2, 8, 14),
               (10, 2, 8, 17), (10, 2, 12, 24), (10, 65, 8, 520), (10, 2, 512, 1024), (10, 8, 1, 8), (2 ** 31 - 1, 1, 8, 8), (2 ** 31, 1, 8, 8),
               (top // 64 + 1, 8, 8, 64), (1000, 2, 8, top // 1000 + 2))
    assert all(cabi.gat16_serves(*t) for t in inside) and not any(cabi.gat16_serves(*t) for t in outside)
    for rows, ld in ((0, 64), (1000, 64), (232_965, 64), (232_965, 128), (2 ** 20, 128), (2 ** 20 + 1, 128), (2_449_029, 128), (2_449_029, 512)):
        assert bool(H.gat16_pays(rows, ld)) == cabi.gat16_native_pays(rows, ld), (rows, ld)
    declared = set(re.findall(r"^(?:int|size_t|void|const char \*|float)\s+\*?(\w+)\(", header, re.M))
    names = {"isplib_gat16_csr_hip", "isplib_gat16_bw_rows_hip", "isplib_gat16_bw_cols_hip", "isplib_gat16_domain", "isplib_gat16_auto"}
    assert names <= declared & set(cabi.EXPORTS)
    assert "static inline int isplib_gat16_serves(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld)" in header
    assert "static inline int isplib_gat16_native_pays(int64_t rows_gathered, int64_t ld)" in header
    L = cabi.lib()                                                           # the symbols restate the inline rules
    for rows, heads, d, ld in table:
        assert bool(L.isplib_gat16_domain(rows, heads, d, ld)) == cabi.gat16_serves(rows, heads, d, ld), (rows, heads, d, ld)
    assert bool(L.isplib_gat16_auto(2_449_029, 128)) == cabi.gat16_native_pays(2_449_029, 128)
    assert bool(L.isplib_gat16_auto(232_965, 64)) == cabi.gat16_native_pays(232_965, 64)


def test_plugin_and_wrappers_refuse_before_any_library_call(monkeypatch):
    import isplib_amd
    from isplib_amd import cabi
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (6, 4))
    y, a_dst, a_src = torch.zeros(4, 16, dtype=BF), torch.zeros(6, 2), torch.zeros(4, 2)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_GAT", raising=False)
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2)                 # unset: as it always was
    for mode in ("convert", "native", "auto"):
        monkeypatch.setenv("ISPLIB_HALF_GAT", mode)
        with pytest.raises(TypeError, match="`y`'s dtype"):
            isplib_amd.gat_matmul(adj, y, a_dst.to(FP), a_src, heads=2)
        with pytest.raises(TypeError, match="`y`'s dtype"):
            isplib_amd.gat_matmul(adj, y, a_dst, a_src.double(), heads=2)
        with pytest.raises(TypeError, match="float32"):
            isplib_amd.gat_matmul(adj, y.float(), a_dst.to(BF), a_src, heads=2)   # an fp32 call does not read the variable
        with pytest.raises(TypeError, match="GPU tensor"):
            isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=2)             # CPU tensors: what the conversion route raises
        with pytest.raises(TypeError, match="GPU tensor"):
            isplib_amd.gat_matmul(adj, y, a_dst.to(BF), a_src.to(BF), heads=2)
        with pytest.raises(ValueError, match="power of two"):
            isplib_amd.gat_matmul(adj, torch.zeros(4, 12, dtype=BF), a_dst, a_src, heads=2)   # d = 6: what the fp32 call raises
        with pytest.raises(ValueError, match="positive int"):
            isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=0)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        cabi.gat16_forward(rowptr, col, y.float(), a_dst, a_src, 2)
    with pytest.raises(TypeError, match="float32"):
        cabi.gat16_forward(rowptr, col, y, a_dst.to(BF), a_src, 2)
    with pytest.raises(ValueError, match="even pitch"):
        cabi.gat16_forward(rowptr, col, torch.zeros(4, 17, dtype=BF)[:, :16], a_dst, a_src, 2)
    with pytest.raises(ValueError, match="isplib_gat16_serves"):
        cabi.gat16_forward(rowptr, col, torch.zeros(4, 8, dtype=BF), a_dst, a_src, 2)             # d = 4
    with pytest.raises(ValueError, match="isplib_gat16_serves"):
        cabi.gat16_forward(rowptr, col, torch.zeros(4, 6, dtype=BF), torch.zeros(6, 1), torch.zeros(4, 1), 1)
    with pytest.raises(ValueError, match=r"`lse` must be \[6, 2\]"):
        cabi.gat16_backward_rows(rowptr, col, y, a_dst, a_src, torch.zeros(6, 16, dtype=BF), torch.zeros(5, 2), 2)
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.gat16_backward_rows(rowptr, col, y, a_dst, a_src, torch.zeros(6, 16, dtype=FP), a_dst, 2)
    with pytest.raises(ValueError, match=r"`dsum` must be \[6, 2\]"):
        cabi.gat16_backward_cols(torch.arange(0, 5, dtype=torch.int64), col, y, a_dst, a_src, torch.zeros(6, 16, dtype=BF), a_dst,
                                 torch.zeros(6, 1), 2)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.gat16_forward(rowptr, col, y, a_dst, a_src, 2)                  # well-formed, but on the CPU
