"""The 16-bit GATv2 operator, host side (no GPU): the bound of tests/gatv2_16_ref.py is neither too tight (an fp32 NumPy emulation in
the kernels' own form -- per-lane dot products joined by the head's butterfly, the online forward with one rescale per step of U edges
in every one of the G slots, the pairwise slot merge, the one-pass rows backward P - D Q and R - D S, the block and lane order of the
datt fold, one rounding -- passes on every case) nor too loose (the planted faults each miss it), gatv2_16_route is a pure and total
function, and the header's rules agree with their cabi twins (the static inline functions compiled here into a scrap library).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import gatv2_16_cases as c16
from tests import gatv2_ref as ref
from tests import half_ref
from tests import test_gatv2_host as v2host
from tests.gat_ref import per_head
from tests.test_gat16_host import SERVES_TABLE, through_fp16, truncate16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BF, FP = torch.bfloat16, torch.float16
OUT16 = ("z", "dx", "dy")
U = 2                                                                        # GATV2_16_FW_U: edges per slot and step of the forward
ROWS_WAVES = 8                                                               # rows per block of the rows kernel


def fma(a, b, c):
    """fl32(a * b + c) with one rounding (the product of two fp32 numbers is exact in fp64)."""
    return (a.astype(np.float64) * b + c).astype(F32)


def seq_sum(values):
    """The sum along axis 0 in fp32, one term after the other."""
    return np.cumsum(values, axis=0, dtype=F32)[-1] if len(values) else np.zeros(values.shape[1:], F32)


def tree_sum(parts):
    """parts [P, ...], P a power of two, added pairwise with partner 1 first: the slot merge (xor LPR, 2 LPR, ...) takes neighbouring
    slots first."""
    while parts.shape[0] > 1:
        parts = (parts[0::2] + parts[1::2]).astype(F32)
    return parts[0]


def head_dots(a3, b3):
    """sum_c a[..., h, c] b[..., h, c] -> [..., h] as the kernels form it: per lane of eight columns one fma after the other, then the
    pairwise sums of the head's butterfly (lanes past the width hold zeros)."""
    d = a3.shape[-1]
    lanes = 1
    while lanes * 8 < d:
        lanes *= 2
    shape = np.broadcast_shapes(a3.shape, b3.shape)
    a, b = np.zeros(shape[:-1] + (lanes * 8,), F32), np.zeros(shape[:-1] + (lanes * 8,), F32)
    a[..., :d], b[..., :d] = a3, b3
    a, b = a.reshape(shape[:-1] + (lanes, 8)), b.reshape(shape[:-1] + (lanes, 8))
    p = np.zeros(shape[:-1] + (lanes,), F32)
    for v in range(8):
        p = fma(a[..., v], b[..., v], p)
    while p.shape[-1] > 1:
        p = (p[..., 0::2] + p[..., 1::2]).astype(F32)
    return p[..., 0]


def slot_edges(b, e, G):
    """The edges [b, e) of one row as the kernels deal them: batches of 64, in a batch edge q goes to slot q % G, U per slot and step.
    -> a list of steps, each an index array [U, G] with -1 for a dead edge."""
    steps = []
    for base in range(b, e, 64):
        cnt = min(64, e - base)
        for s0 in range(0, cnt, G * U):
            q = s0 + np.arange(U)[:, None] * G + np.arange(G)[None, :]
            steps.append(np.where(q < cnt, base + q, -1))
    return steps


def per_slot_sums(b, e, G, terms):
    """Every array of `terms` ([nnz, ...]) summed over the edges [b, e): one term after the other inside each of the G slots, then
    the slots by the pairwise tree."""
    pos = np.arange(e - b)
    slot = (pos % 64) % G
    out = []
    for tm in terms:
        parts = np.stack([seq_sum(tm[b:e][slot == g]) for g in range(G)])
        out.append(tree_sum(parts))
    return out


def emulate32(case, d_from_z16=False):
    """The kernels' arithmetic in fp32 NumPy, before the one rounding of z, dx and dy.  `d_from_z16`: the planted fault
    D[i,h] = <g_i, z16_i>_h."""
    rowptr, col, H, ns = case.rowptr, case.col, case.heads, F32(case.ns)
    m, n, K = case.m, case.n, case.k
    d = K // H
    G = 64 // c16.lanes_per_row(K)
    x3, y3, g3, att = per_head(case.x, H), per_head(case.y, H), per_head(case.g, H), np.asarray(case.att, F32)
    row = ref.edge_rows(rowptr)
    u = (x3[row] + y3[col]).astype(F32)                                                  # ONE fp32 add
    pos = u > 0
    v = np.where(pos, u, (ns * u).astype(F32)).astype(F32)
    s = head_dots(att[None], v)                                                          # [nnz, H]
    t = head_dots(g3[row], y3[col])
    none = -np.finfo(F32).max
    z, lse = np.zeros((m, H, d), F32), np.full((m, H), -np.inf, F32)
    with np.errstate(over="ignore", under="ignore"):
        for i in range(m):
            b, e = int(rowptr[i]), int(rowptr[i + 1])
            if e == b:
                continue
            mrun, l, acc = np.full((G, H), none, F32), np.zeros((G, H), F32), np.zeros((G, H, d), F32)
            for idx in slot_edges(b, e, G):                                              # [U, G]
                live = idx >= 0
                sc = np.where(live[:, :, None], s[np.maximum(idx, 0)], none)             # [U, G, H]
                mnew = np.maximum(mrun, sc.max(0))
                r = np.exp((mrun - mnew).astype(F32))
                mrun, l, acc = mnew, (l * r).astype(F32), (acc * r[:, :, None]).astype(F32)
                for q in range(U):
                    w = np.where(live[q][:, None], np.exp((sc[q] - mnew).astype(F32)), F32(0)).astype(F32)
                    l = (l + w).astype(F32)
                    acc = fma(w[:, :, None], y3[col[np.maximum(idx[q], 0)]], acc)
            while mrun.shape[0] > 1:                                                     # the slots pairwise, by the rule of a step
                ma, mb = mrun[0::2], mrun[1::2]
                mnew = np.maximum(ma, mb)
                ra, rb = np.exp((ma - mnew).astype(F32)), np.exp((mb - mnew).astype(F32))
                l = ((l[0::2] * ra).astype(F32) + (l[1::2] * rb).astype(F32)).astype(F32)
                acc = ((acc[0::2] * ra[:, :, None]).astype(F32) + (acc[1::2] * rb[:, :, None]).astype(F32)).astype(F32)
                mrun = mnew
            z[i], lse[i] = acc[0] / l[0][:, None], (mrun[0] + np.log(l[0])).astype(F32)
        a = np.exp((s - np.where(np.isfinite(lse), lse, F32(0))[row]).astype(F32)).astype(F32)
    # the one-pass backward over the rows
    aet = (a * t).astype(F32)
    p_t = np.where(pos, aet[:, :, None], (ns * aet).astype(F32)[:, :, None]).astype(F32)
    q_t = np.where(pos, a[:, :, None], (ns * a).astype(F32)[:, :, None]).astype(F32)
    r_t, s_t = (aet[:, :, None] * v).astype(F32), (a[:, :, None] * v).astype(F32)
    D, dx, pa = np.zeros((m, H), F32), np.zeros((m, H, d), F32), np.zeros((m, H, d), F32)
    z16 = per_head(half_ref.widen(half_ref.round16(z.reshape(m, K), case.dtype)), H)
    for i in range(m):
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        if e == b:
            continue
        l, dacc, P, Q, R, S = per_slot_sums(b, e, G, (a, aet, p_t, q_t, r_t, s_t))
        D[i] = head_dots(g3[i], z16[i]) if d_from_z16 else (dacc / l).astype(F32)
        dx[i] = (att * (P - (D[i][:, None] * Q).astype(F32)).astype(F32)).astype(F32)
        pa[i] = (R - (D[i][:, None] * S).astype(F32)).astype(F32)
    # datt: per block of ROWS_WAVES rows one partial row (its waves in order), lane l of the fold takes the blocks l, l + 64, ..., then
    # the 64 lane sums by the butterfly
    nb = -(-m // ROWS_WAVES)
    blocks = np.stack([seq_sum(pa[bk * ROWS_WAVES:(bk + 1) * ROWS_WAVES]) for bk in range(nb)])
    datt = np.stack([seq_sum(blocks[lane::64]) for lane in range(64)])
    for o in (32, 16, 8, 4, 2, 1):                                                       # partner 32 first
        datt = (datt[:o] + datt[o:2 * o]).astype(F32)
    datt = datt[0]
    # the backward over the columns, on the transposed structure (entries of a column in row order)
    order = np.argsort(col, kind="stable")
    cuts = np.searchsorted(col[order], np.arange(n + 1))
    ds = (a * (t - D[row]).astype(F32)).astype(F32)
    dsa = (ds[:, :, None] * att[None]).astype(F32)
    into_y = fma(a[:, :, None], g3[row], np.where(pos, dsa, (ns * dsa).astype(F32)))[order]
    dy = np.zeros((n, H, d), F32)
    for j in range(n):
        if cuts[j + 1] > cuts[j]:
            dy[j] = per_slot_sums(int(cuts[j]), int(cuts[j + 1]), G, (into_y,))[0]
    return dict(z=z.reshape(m, K), lse=lse, D=D, dx=dx.reshape(m, K), dy=dy.reshape(n, K), datt=datt)


def rounded(case, got, how=half_ref.round16):
    """z, dx and dy rounded once to the case's dtype (and widened again for the comparison); everything else stays fp32."""
    out = dict(got)
    for name in OUT16:
        out[name] = half_ref.widen(how(np.asarray(got[name], F32), case.dtype))
    return out


def worst_of(case, got):
    return max(c16.fractions(case, got).values())


def test_the_cases_cover_every_instantiation_and_head_form():
    """All 24 configurations of the 16-bit GAT tests in bf16 (every LPR by its first, last and a ragged width; heads of one lane up to
    half a slot; head counts that are no power of two), one fp16 configuration per LPR, two on the second graph, the slopes 0 and 1,
    the large and the single case; every case inside the first-order range (each Case16 asserts its rho cap when it is built)."""
    assert len(c16.CONFIGS) == 24 and sorted(d for h, d in c16.CONFIGS if h == 1) == [8, 10, 30, 32, 34, 46, 64, 66, 130, 258, 510, 512]
    assert sorted(c16.lanes_per_row(h * d) for h, d in c16.FP16_CONFIGS) == [4, 8, 16, 32, 64]
    assert len(c16.config_cases()) == len(c16.CONFIGS) + len(c16.FP16_CONFIGS) + len(c16.GRAPH2_CONFIGS)
    assert {c.ns for c in c16.slope_cases()} == {0.0, 1.0} and len(c16.slope_cases()) == 6
    for case in c16.special_cases():
        cap = c16.LARGE_RHO_MAX if case.kind == "large" else c16.RHO_MAX
        assert case.rho_max == cap and float(case.bound["rho"].max()) <= cap, case.name
    assert c16.RHO_MAX == 1e-3 and c16.LARGE_RHO_MAX == 4e-3
    large = c16.large_case()
    assert large.ref["s"].max() > 150 and large.ref["s"].min() < -150


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


# ---- planted faults: each must MISS the bound on its named outputs --------------------------------------------------------------------

def picked():
    return [c16.config_case(h, d) for h, d in c16.SLOPE_CONFIGS]


def test_the_unfaulted_restatement_passes():
    """tests/test_gatv2_host.py's fp64 restatement from per-edge scores and weights, rounded once: D = <g, z> equals sum_e a_e t_e."""
    for case in picked():
        got = rounded(case, v2host._from_edges(case, case.ref["s"], case.ref["a"]))
        assert worst_of(case, got) <= 1.0, case.name


def test_fault_d_taken_from_the_rounded_z():
    """Why the rows kernel does not read z: with g aligned to z at H = 1, K = 512 in bf16, D = <g, z16> carries u sum |g z| into D
    and, through R - D S, into datt -- the fp32 outputs."""
    base = c16.config_case(1, 512)
    aligned = c16.Case16("h1d512-aligned-g", base.rowptr, base.col, np.array(base.x), np.array(base.y), base.att,
                         (base.ref["z"] * 8.0).astype(F32), 1, base.ns, BF)
    assert worst_of(aligned, rounded(aligned, emulate32(aligned))) <= 1.0    # the one-pass form passes on the same case
    frac = c16.fractions(aligned, rounded(aligned, emulate32(aligned, d_from_z16=True)))
    print(aligned.name, {n: round(v, 3) for n, v in frac.items()})
    assert frac["D"] > 1.0 or frac["datt"] > 1.0


# fault of tests/test_gatv2_host.py -> the outputs that must miss the 16-bit bound on at least one picked case
FAULTS = ((v2host.fault_leaky_relu_outside_the_dot_product, c16.OUTPUTS), (v2host.fault_sl_dropped_from_q, ("dx", "dy")),
          (v2host.fault_datt_from_u, ("datt",)), (v2host.fault_q_dropped_from_dy, ("dy",)))


@pytest.mark.parametrize("fault,outputs", FAULTS, ids=lambda f: getattr(f, "__name__", ""))
def test_bound_is_not_too_loose(fault, outputs):
    """GAT v1's score (LeakyReLU outside the dot product), sl dropped from P / Q, R - D S formed from u instead of v, q dropped from
    dy: each restated in fp64 and rounded once."""
    fracs = [c16.fractions(c, rounded(c, fault(c))) for c in picked()]
    print(fault.__name__, [{k: round(v, 2) for k, v in f.items()} for f in fracs])
    for name in outputs:
        assert any(f[name] > 1.0 for f in fracs), (fault.__name__, name)


def test_fault_dropped_edge():
    for case in picked():
        keep = np.ones(case.col.size, bool)
        keep[case.rowptr[np.argmax(np.diff(case.rowptr) == 3)]] = False      # the first entry of a three-entry row
        s = np.where(keep[:, None], case.ref["s"], -np.inf)
        got = v2host._from_edges(case, np.where(keep[:, None], case.ref["s"], case.ref["s"].min()), v2host._softmax(case, s))
        assert worst_of(case, rounded(case, got)) > 1.0, case.name


@pytest.mark.parametrize("how", (truncate16, through_fp16), ids=lambda f: f.__name__)
def test_fault_z_rounded_twice_or_truncated(how):
    for case in picked():
        raw = emulate32(case)
        got = rounded(case, raw)
        got["z"] = half_ref.widen(how(raw["z"], case.dtype))
        assert c16.fractions(case, got, ("z",))["z"] > 1.0, case.name


# ---- the route and the rules -----------------------------------------------------------------------------------------------------------

def test_gatv2_16_route_is_pure_and_total(monkeypatch):
    """Over dtype, domain edges and mode; cabi.gatv2_16_serves and gatv2_16_native_pays are plain Python, so no library is loaded.
    Under `auto` the measured rule is also replaced by both constant answers: the route follows whatever it says."""
    from isplib_amd import cabi
    from isplib_amd.plugin import gatv2_16_route as route
    for pays in (True, False):
        with monkeypatch.context() as mp:
            mp.setattr(cabi, "gatv2_16_native_pays", lambda rows, ld, pays=pays: pays)
            assert route(BF, 8, 8, 64, 2000, "auto") == ("gatv2_16" if pays else "convert")
            assert route(BF, 8, 4, 32, 2000, "auto") == "convert" and route(BF, 8, 8, 64, 2000, "native") == "gatv2_16"
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_GATV2", raising=False)
    for dtype in (BF, FP):
        for mode in ("convert", "native", "auto", "nonsense"):
            for heads, d in ((1, 7), (1, 63), (1, 6), (1, 8), (1, 512), (1, 514), (8, 4), (2, 4), (8, 8), (2, 12), (64, 8), (65, 8), (3, 128),
                             (2, 2)):
                k = heads * d
                for pitch in (k + 1, k + 2, k):
                    for n in (2000, 2 ** 31):
                        got = route(dtype, heads, d, pitch, n, mode)
                        shape = (d % 2 == 0) if heads == 1 else (d >= 8 and d & (d - 1) == 0)
                        inside = shape and 8 <= k <= 512 and n < 2 ** 31             # an odd pitch is packed
                        if mode == "native":
                            want = "gatv2_16" if inside else "convert"
                        elif mode == "auto":
                            ld = pitch if pitch % 2 == 0 else k
                            want = "gatv2_16" if inside and cabi.gatv2_16_native_pays(n, ld) else "convert"
                        else:
                            want = "convert"
                        assert got == want, (dtype, mode, heads, d, pitch, n)
        assert route(dtype, 8, 8, 64, 0xE0000000 // 128, "native") == "gatv2_16"         # the operand at the descriptor's limit
        assert route(dtype, 8, 8, 64, 0xE0000000 // 128 + 1, "native") == "convert"
        assert route(dtype, 8, 8, 0xE0000000 // 2 // 1000 + 2, 1000, "native") == "gatv2_16"    # too wide a pitch is packed
    for mode in ("convert", "native", "auto"):
        assert route(torch.float32, 8, 8, 64, 2000, mode) == "convert" and route(torch.float64, 8, 8, 64, 2000, mode) == "convert"
    # the mode comes from ISPLIB_HALF_GATV2 when it is not given; unset counts as convert, and ISPLIB_HALF=convert wins
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "native")
    assert route(BF, 8, 8, 64, 2000) == "gatv2_16" and route(BF, 1, 63, 64, 2000) == "convert" and route(BF, 8, 4, 32, 2000) == "convert"
    assert route(BF, 8, 8, 65, 2000) == "gatv2_16"                                       # an odd pitch: packed
    monkeypatch.setenv("ISPLIB_HALF_GAT", "convert")                                     # GAT v1's variable is another one
    assert route(BF, 8, 8, 64, 2000) == "gatv2_16"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "auto")
    assert route(BF, 8, 8, 64, 2000) == "gatv2_16"
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "auto")
    assert route(BF, 8, 8, 64, 2000) == route(BF, 8, 8, 64, 2000, "auto")
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "native")
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "nonsense")
    assert route(BF, 8, 8, 64, 2000) == "convert"


_RULES_SRC = r"""
#include "isplib_hip.h"
extern "C" int gatv2_16_serves(long long rows, long long heads, long long d, long long ld) { return isplib_gatv2_16_serves(rows, heads, d, ld); }
extern "C" int gat16_serves(long long rows, long long heads, long long d, long long ld) { return isplib_gat16_serves(rows, heads, d, ld); }
extern "C" int gatv2_16_pays(long long rows, long long ld) { return isplib_gatv2_16_native_pays(rows, ld); }
"""


def test_header_rules_match_their_cabi_twins(tmp_path):
    from isplib_amd import _lib, cabi
    src, so = tmp_path / "rules.cpp", tmp_path / "rules.so"
    src.write_text(_RULES_SRC)
    subprocess.run(["g++", "-shared", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True, timeout=120)
    H = ctypes.CDLL(str(so))
    H.gatv2_16_serves.argtypes = H.gat16_serves.argtypes = [ctypes.c_longlong] * 4
    H.gatv2_16_pays.argtypes = [ctypes.c_longlong] * 2
    # the 16-bit GATv2 entries have a header of their own, which isplib_hip.h includes (the scrap library above includes only the latter)
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    assert re.search(r'^#include "isplib_hip_gatv2_16.h"$', main, re.M) and "gatv2_16_" not in main.replace("isplib_hip_gatv2_16.h", "")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip_gatv2_16.h")).read(), flags=re.S)
    # stated once: the header's inline returns isplib_gat16_serves(...)
    assert re.search(r"static inline int isplib_gatv2_16_serves\([^)]*\)\s*\{\s*return isplib_gat16_serves\(rows_gathered, heads, d, ld\);\s*\}",
                     header)
    top = cabi.DENSE_BYTES_MAX // 2
    table = SERVES_TABLE + ((top // 64, 8, 8, 64), (top // 64 + 1, 8, 8, 64), (top // 64, 4, 8, 64), (1000, 2, 8, top // 1000),
                            (1000, 2, 8, top // 1000 + 2))
    L = cabi.lib()
    for rows, heads, d, ld in table:
        want = cabi.gatv2_16_serves(rows, heads, d, ld)
        assert want == cabi.gat16_serves(rows, heads, d, ld) == bool(H.gatv2_16_serves(rows, heads, d, ld)) == \
            bool(H.gat16_serves(rows, heads, d, ld)) == bool(L.isplib_gatv2_16_domain(rows, heads, d, ld)), (rows, heads, d, ld)
    assert any(cabi.gatv2_16_serves(*t) for t in table) and not all(cabi.gatv2_16_serves(*t) for t in table)
    assert not cabi.gatv2_16_serves(10, 2, 4, 8) and not cabi.gatv2_16_serves(10, 1, 6, 6) and not cabi.gatv2_16_serves(10, 1, 9, 10)
    for rows, ld in ((0, 64), (1000, 64), (232_965, 64), (232_965, 128), (2 ** 20, 128), (2 ** 20 + 1, 128), (2_449_029, 128), (2_449_029, 512)):
        assert bool(H.gatv2_16_pays(rows, ld)) == cabi.gatv2_16_native_pays(rows, ld) == bool(L.isplib_gatv2_16_auto(rows, ld)), (rows, ld)
    declared = set(re.findall(r"^(?:int|size_t|void|const char \*|float)\s+\*?(\w+)\(", header, re.M))
    names = {"isplib_gatv2_16_csr_hip", "isplib_gatv2_16_bw_rows_hip", "isplib_gatv2_16_bw_rows_workspace_bytes",
             "isplib_gatv2_16_bw_cols_hip", "isplib_gatv2_16_domain", "isplib_gatv2_16_auto"}
    # that header, its name list in cabi and the library's dynamic symbols agree; cabi.EXPORTS stays what isplib_hip.h itself declares
    assert names == declared == set(cabi.GATV2_16_EXPORTS) and not names & set(cabi.EXPORTS)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.CABI_PATH], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert names <= exported and {n for n in exported if n.startswith("isplib_gatv2_16")} == names
    for name in names:
        getattr(L, name)
    assert "static inline int isplib_gatv2_16_native_pays(int64_t rows_gathered, int64_t ld)" in header
    # the rows entry takes no z: one leading dimension less than the fp32 entry's list
    proto = re.search(r"isplib_gatv2_16_bw_rows_hip\((.*?)\);", header, re.S).group(1)
    assert "ldz" not in proto and "*z" not in proto and "datt" in proto and "workspace_bytes" in proto
    # the workspace: one partial row of k floats per block of ROWS_WAVES rows, whole 256-byte units, never 0
    assert cabi.gatv2_16_bw_rows_workspace_bytes(0, 64) == cabi.gatv2_16_bw_rows_workspace_bytes(64, 0) == 256
    for m in (1, 7, 8, 9, 200, 232_965):
        for k in (8, 46, 512):
            assert cabi.gatv2_16_bw_rows_workspace_bytes(m, k) == (-(-m // ROWS_WAVES) * k * 4 + 255) // 256 * 256


def test_plugin_and_wrappers_refuse_before_any_library_call(monkeypatch):
    import isplib_amd
    from isplib_amd import cabi
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (6, 4))
    sq = isplib_amd.SparseTensor.from_csr(torch.arange(0, 5, dtype=torch.int64), torch.arange(4, dtype=torch.int64), None, (4, 4))
    x, y, att = torch.zeros(6, 16, dtype=BF), torch.zeros(4, 16, dtype=BF), torch.zeros(2, 8)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_GATV2", raising=False)
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.gatv2_matmul(adj, x, att, y, heads=2)                     # unset: as it always was
    for mode in ("convert", "native", "auto"):
        monkeypatch.setenv("ISPLIB_HALF_GATV2", mode)
        with pytest.raises(TypeError, match="share one 16-bit dtype"):
            isplib_amd.gatv2_matmul(adj, x, att, y.to(FP), heads=2)
        with pytest.raises(TypeError, match="share one 16-bit dtype"):
            isplib_amd.gatv2_matmul(adj, x, att, y.float(), heads=2)
        with pytest.raises(TypeError, match="share one 16-bit dtype"):
            isplib_amd.gatv2_matmul(adj, x.float(), att, y, heads=2)
        with pytest.raises(TypeError, match="`x`'s dtype"):
            isplib_amd.gatv2_matmul(adj, x, att.to(FP), y, heads=2)
        with pytest.raises(TypeError, match="`x`'s dtype"):
            isplib_amd.gatv2_matmul(adj, x, att.double(), y, heads=2)
        with pytest.raises(TypeError, match="float32"):
            isplib_amd.gatv2_matmul(adj, x.float(), att.to(BF), y.float(), heads=2)   # an fp32 call does not read the variable
        with pytest.raises(TypeError, match="GPU tensor"):
            isplib_amd.gatv2_matmul(adj, x, att, y, heads=2)                 # CPU tensors: what the conversion route raises
        with pytest.raises(TypeError, match="GPU tensor"):
            isplib_amd.gatv2_matmul(adj, x, att.to(BF), y, heads=2)
        with pytest.raises(TypeError, match="GPU tensor"):
            sq.gatv2_matmul(y, att, heads=2)                                 # y=None on a square graph
        with pytest.raises(ValueError, match="square"):
            isplib_amd.gatv2_matmul(adj, x, att, heads=2)                    # y=None needs a square graph: what the fp32 call raises
        with pytest.raises(ValueError, match="power of two"):
            isplib_amd.gatv2_matmul(adj, torch.zeros(6, 12, dtype=BF), torch.zeros(2, 6), torch.zeros(4, 12, dtype=BF), heads=2)   # d = 6
        with pytest.raises(ValueError, match="positive int"):
            isplib_amd.gatv2_matmul(adj, x, att, y, heads=0)
    g, lse = torch.zeros(6, 16, dtype=BF), torch.zeros(6, 2)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        cabi.gatv2_16_forward(rowptr, col, x.float(), y, att, 2)
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.gatv2_16_forward(rowptr, col, x, y.to(FP), att, 2)
    with pytest.raises(TypeError, match="float32"):
        cabi.gatv2_16_forward(rowptr, col, x, y, att.to(BF), 2)
    with pytest.raises(ValueError, match="even pitch"):
        cabi.gatv2_16_forward(rowptr, col, x, torch.zeros(4, 17, dtype=BF)[:, :16], att, 2)
    with pytest.raises(ValueError, match="isplib_gatv2_16_serves"):
        cabi.gatv2_16_forward(rowptr, col, torch.zeros(6, 8, dtype=BF), torch.zeros(4, 8, dtype=BF), torch.zeros(2, 4), 2)      # d = 4
    with pytest.raises(ValueError, match="isplib_gatv2_16_serves"):
        cabi.gatv2_16_forward(rowptr, col, torch.zeros(6, 6, dtype=BF), torch.zeros(4, 6, dtype=BF), torch.zeros(1, 6), 1)
    with pytest.raises(ValueError, match=r"`lse` must be \[6, 2\]"):
        cabi.gatv2_16_backward_rows(rowptr, col, x, y, att, g, torch.zeros(5, 2), 2)
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.gatv2_16_backward_rows(rowptr, col, x, y, att, g.to(FP), lse, 2)
    with pytest.raises(ValueError, match="exactly when"):
        cabi.gatv2_16_backward_rows(rowptr, col, x, y, att, g, lse, 2, want_datt=False, out=(torch.zeros(6, 16, dtype=BF), lse, torch.zeros(2, 8)))
    with pytest.raises(ValueError, match="uint8"):
        cabi.gatv2_16_backward_rows(rowptr, col, x, y, att, g, lse, 2, workspace=torch.zeros(1024))
    with pytest.raises(ValueError, match=r"`dsum` must be \[6, 2\]"):
        cabi.gatv2_16_backward_cols(torch.arange(0, 5, dtype=torch.int64), col, x, y, att, g, lse, torch.zeros(6, 1), 2)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.gatv2_16_forward(rowptr, col, x, y, att, 2)                     # well-formed, but on the CPU
