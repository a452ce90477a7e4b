"""The 16-bit multi-head attention operator (q, k, v), host side (no GPU): the bound of tests/mha16_ref.py is neither too tight (an
fp32 NumPy emulation in the kernels' own form -- per-lane fma chains of eight columns joined by the head's butterfly, the online forward
with one rescale per step of U edges in every one of the G slots, the pairwise slot merge, the one-pass rows backward P - D Q, one
rounding -- passes on every case) nor too loose (the planted faults each miss it), mha16_route is a pure and total function, the
header's rules agree with their cabi twins (the static inline functions compiled here into a scrap library), the header, MHA16_EXPORTS
and the library's symbols are consistent, and the plug-in and the wrappers refuse bad operands before anything is launched.
"""
import ctypes
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import half_ref
from tests import mha16_cases as c16
from tests import mha_ref as ref
from tests import test_mha_host as mhost
from tests.gat_ref import per_head
from tests.test_gat16_host import SERVES_TABLE, through_fp16, truncate16
from tests.test_gatv2_16_host import fma, head_dots, per_slot_sums, tree_sum

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BF, FP = torch.bfloat16, torch.float16
ENTRIES = ("isplib_qkv16_csr_hip", "isplib_qkv16_bw_rows_hip", "isplib_qkv16_bw_cols_hip", "isplib_qkv16_domain", "isplib_qkv16_auto")
SCHEMA = ("mha_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor q, Tensor k, Tensor v, int heads, float scale) "
          "-> Tensor")
PICKED = ((1, 46), (8, 8), (3, 128))


def forward_step_width():
    """MHA16_FW_U of isplib_amd/csrc/mha16.hip: edges per slot and step of the forward (the only kernel whose rounding depends on it)."""
    src = open(os.path.join(ROOT, "isplib_amd", "csrc", "mha16.hip")).read()
    return int(re.search(r"#define ISPLIB_MHA16_FW_U (\d+)", src).group(1))


def slot_edges(b, e, G, U):
    """The edges [b, e) of one row as the kernels deal them: batches of 64, in a batch edge q goes to slot q % G, U per slot and step.
    -> a list of steps, each an index array [U, G] with -1 for a dead edge."""
    steps = []
    for base in range(b, e, 64):
        cnt = min(64, e - base)
        for s0 in range(0, cnt, G * U):
            q = s0 + np.arange(U)[:, None] * G + np.arange(G)[None, :]
            steps.append(np.where(q < cnt, base + q, -1))
    return steps


def per_slot_fma(b, e, G, w, x):
    """sum over the edges [b, e) of w[e] x[e] ([nnz, H] times [nnz, H, d]) as the backward kernels form it: in each of the G slots one
    fma after the other (edge `pos` of the row sits in slot pos % G: 64 is a multiple of G), then the slots by the pairwise tree."""
    cnt = e - b
    steps = -(-cnt // G)
    idx = np.arange(steps * G).reshape(steps, G)
    acc = np.zeros((G,) + x.shape[1:], F32)
    for t in range(steps):
        live = idx[t] < cnt
        at = b + np.minimum(idx[t], cnt - 1)
        acc = np.where(live[:, None, None], fma(w[at][:, :, None], x[at], acc), acc)
    return tree_sum(acc)


def emulate32(case, d_from_z16=False, U=None):
    """The kernels' arithmetic in fp32 NumPy, before the one rounding of z, dq, dk and dv.  `d_from_z16`: the planted fault
    D[i,h] = <g_i, z16_i>_h."""
    U = forward_step_width() if U is None else U
    rowptr, col, H, p = case.rowptr, case.col, case.heads, F32(case.p)
    m, n, K = case.m, case.n, case.width
    d = K // H
    G = 64 // c16.lanes_per_row(K)
    q3, k3, v3, g3 = per_head(case.q, H), per_head(case.k, H), per_head(case.v, H), per_head(case.g, H)
    row = ref.edge_rows(rowptr)
    s = (head_dots(q3[row], k3[col]) * p).astype(F32)                                    # p multiplies the finished dot product
    t = head_dots(g3[row], v3[col])
    none = -np.finfo(F32).max
    z, lse = np.zeros((m, H, d), F32), np.full((m, H), -np.inf, F32)
    with np.errstate(over="ignore", under="ignore"):
        for i in range(m):
            b, e = int(rowptr[i]), int(rowptr[i + 1])
            if e == b:
                continue
            mrun, l, acc = np.full((G, H), none, F32), np.zeros((G, H), F32), np.zeros((G, H, d), F32)
            for idx in slot_edges(b, e, G, U):                                           # [U, G]
                live = idx >= 0
                sc = np.where(live[:, :, None], s[np.maximum(idx, 0)], none)             # [U, G, H]
                mnew = np.maximum(mrun, sc.max(0))
                r = np.exp((mrun - mnew).astype(F32))
                mrun, l, acc = mnew, (l * r).astype(F32), (acc * r[:, :, None]).astype(F32)
                for u in range(U):
                    w = np.where(live[u][:, None], np.exp((sc[u] - mnew).astype(F32)), F32(0)).astype(F32)
                    l = (l + w).astype(F32)
                    acc = fma(w[:, :, None], v3[col[np.maximum(idx[u], 0)]], acc)
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
    ke, qe, ge = k3[col], q3[row], g3[row]
    D, dq = np.zeros((m, H), F32), np.zeros((m, H, d), F32)
    z16 = per_head(half_ref.widen(half_ref.round16(z.reshape(m, K), case.dtype)), H)
    for i in range(m):
        b, e = int(rowptr[i]), int(rowptr[i + 1])
        if e == b:
            continue
        l, dacc = per_slot_sums(b, e, G, (a, aet))
        P, Q = per_slot_fma(b, e, G, aet, ke), per_slot_fma(b, e, G, a, ke)
        D[i] = head_dots(g3[i], z16[i]) if d_from_z16 else (dacc / l).astype(F32)
        dq[i] = (p * fma(-D[i][:, None], Q, P)).astype(F32)
    # the backward over the columns, on the transposed structure (entries of a column in row order)
    order = np.argsort(col, kind="stable")
    cuts = np.searchsorted(col[order], np.arange(n + 1))
    ds = (a * (t - D[row]).astype(F32)).astype(F32)
    ds_t, a_t, q_t, g_t = ds[order], a[order], qe[order], ge[order]
    dk, dv = np.zeros((n, H, d), F32), np.zeros((n, H, d), F32)
    for j in range(n):
        b, e = int(cuts[j]), int(cuts[j + 1])
        if e > b:
            dk[j] = (per_slot_fma(b, e, G, ds_t, q_t) * p).astype(F32)
            dv[j] = per_slot_fma(b, e, G, a_t, g_t)
    return dict(z=z.reshape(m, K), lse=lse, D=D, dq=dq.reshape(m, K), dk=dk.reshape(n, K), dv=dv.reshape(n, K))


def rounded(case, got, how=half_ref.round16):
    """z, dq, dk and dv rounded once to the case's dtype (and widened again for the comparison); lse and D stay as they are."""
    out = dict(got)
    for name in c16.OUT16:
        out[name] = half_ref.widen(how(np.asarray(got[name], F32), case.dtype))
    return out


def worst_of(case, got):
    return max(c16.fractions(case, got).values())


def test_the_cases_cover_every_instantiation_and_head_form():
    """All 24 configurations of the 16-bit GAT tests in bf16 (every LPR by its first, last and a ragged width; heads of one lane up to
    half a slot; head counts that are no power of two), one fp16 configuration per LPR, two on the second graph, and the special
    cases; every case inside the first-order range (each Case16 asserts its rho cap when it is built)."""
    assert len(c16.CONFIGS) == 24 and sorted(d for h, d in c16.CONFIGS if h == 1) == [8, 10, 30, 32, 34, 46, 64, 66, 130, 258, 510, 512]
    assert sorted(c16.lanes_per_row(h * d) for h, d in c16.FP16_CONFIGS) == [4, 8, 16, 32, 64]
    assert len(c16.config_cases()) == len(c16.CONFIGS) + len(c16.FP16_CONFIGS) + len(c16.GRAPH2_CONFIGS)
    assert c16.RHO_MAX == 1e-3 and c16.LARGE_RHO_MAX == 4e-3
    kinds = [c.kind for c in c16.special_cases()]
    assert kinds.count("large") == 2 and kinds.count("single") == 2
    for case in c16.special_cases():
        cap = c16.LARGE_RHO_MAX if case.kind == "large" else c16.RHO_MAX
        assert case.rho_max == cap and float(case.bound["rho"].max()) <= cap, case.name
    large = c16.large_case()
    assert large.ref["s"].max() > 150 and large.ref["s"].min() < -150
    assert c16.shared_case(8, 8).v16 is c16.shared_case(8, 8).k16 and not c16.zero_q_case(8, 8).q.any()
    assert {(c.m, c.n) for c in c16.special_cases() if c.m != c.n} == {(233, 67), (67, 233)}


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


@pytest.mark.parametrize("spec", ((8, 8), (1, 46), (8, 64)), ids=lambda s: f"h{s[0]}d{s[1]}")
def test_bound_holds_for_either_step_width(spec):
    """U is chosen by measurement among {2, 4}: the bound must not depend on the choice."""
    case = c16.config_case(*spec)
    for U in (2, 4):
        assert worst_of(case, rounded(case, emulate32(case, U=U))) <= 1.0, (case.name, U)


# ---- planted faults: each must MISS the bound on its named outputs --------------------------------------------------------------------

def picked():
    return [c16.config_case(h, d) for h, d in PICKED]


def test_the_unfaulted_restatement_passes():
    """tests/test_mha_host.py's fp64 restatement, rounded once."""
    for case in picked():
        assert worst_of(case, rounded(case, mhost._restated(case))) <= 1.0, case.name


def test_fault_d_taken_from_the_rounded_z():
    """Why the rows kernel does not read z: with g aligned to z at H = 1, K = 512 in bf16, D = <g, z16> carries u sum |g z| into D
    (an fp32 output) and, through it, into dq and dk."""
    base = c16.config_case(1, 512)
    aligned = c16.Case16("h1d512-aligned-g", base.rowptr, base.col, np.array(base.q), np.array(base.k), np.array(base.v),
                         (base.ref["z"] * 8.0).astype(F32), 1, base.p, BF)
    assert worst_of(aligned, rounded(aligned, emulate32(aligned))) <= 1.0    # the one-pass form passes on the same case
    frac = c16.fractions(aligned, rounded(aligned, emulate32(aligned, d_from_z16=True)))
    print(aligned.name, {n: round(v, 3) for n, v in frac.items()})
    assert frac["D"] > 1.0
    assert frac["z"] <= 1.0 and frac["lse"] <= 1.0 and frac["dv"] <= 1.0     # what D does not touch


# fault of tests/test_mha_host.py's restatement -> the outputs that must miss the 16-bit bound on at least one picked case
FAULTS = (("key_used_as_value", lambda c: mhost._restated(c, value=c.k), ("z", "D", "dq", "dk")),
          ("scale_from_K_not_d", lambda c: mhost._restated(c, p_score=1.0 / np.sqrt(c.width)), ("z", "lse", "dq", "dk", "dv")),
          ("scale_dropped_from_dk", lambda c: mhost._restated(c, p_in_dk=False), ("dk",)),
          ("dv_from_ds", lambda c: mhost._restated(c, dv_from_ds=True), ("dv",)))


@pytest.mark.parametrize("name,fault,outputs", FAULTS, ids=[f[0] for f in FAULTS])
def test_bound_is_not_too_loose(name, fault, outputs):
    """The key used as the value, the scale taken from K instead of the head width (only where H > 1), p dropped from dk, dv formed
    from ds: each restated in fp64 and rounded once.  A switch that touches one backward output leaves the others alone."""
    cases = picked()
    fracs = [c16.fractions(c, rounded(c, fault(c))) for c in cases]
    print(name, [{k: round(v, 2) for k, v in f.items()} for f in fracs])
    for out in outputs:
        assert any(f[out] > 1.0 for f in fracs), (name, out)
    if name in ("scale_dropped_from_dk", "dv_from_ds"):
        for out in set(c16.OUTPUTS) - set(outputs):
            assert all(f[out] <= 1.0 for f in fracs), (name, out)
    if name == "scale_from_K_not_d":                                         # one head: K is d, the two scales coincide
        assert all(v <= 1.0 for v in fracs[0].values())


def test_fault_dropped_edge():
    """The first entry of a three-entry row left out of the structure the restatement walks."""
    for case in picked():
        keep = np.ones(case.col.size, bool)
        keep[case.rowptr[np.argmax(np.diff(case.rowptr) == 3)]] = False
        shadow = types.SimpleNamespace(heads=case.heads, m=case.m, n=case.n, width=case.width, p=case.p, q=case.q, k=case.k, v=case.v,
                                       g=case.g, col=case.col[keep], ref=dict(row=case.ref["row"][keep]), live=case.live)
        assert worst_of(case, rounded(case, mhost._restated(shadow))) > 1.0, case.name


@pytest.mark.parametrize("how", (truncate16, through_fp16), ids=lambda f: f.__name__)
def test_fault_z_rounded_twice_or_truncated(how):
    """z misses the bound on at least one picked configuration (a second rounding through fp16 moves few elements of a narrow z
    across a bf16 tie); the other outputs are left alone."""
    fracs = []
    for case in picked():
        raw = emulate32(case)
        got = rounded(case, raw)
        got["z"] = half_ref.widen(how(raw["z"], case.dtype))
        fracs.append(c16.fractions(case, got))
    print(how.__name__, [round(f["z"], 3) for f in fracs])
    assert any(f["z"] > 1.0 for f in fracs)
    assert all(v <= 1.0 for f in fracs for n, v in f.items() if n != "z")


# ---- the route and the rules -----------------------------------------------------------------------------------------------------------

def test_mha16_route_is_pure_and_total(monkeypatch):
    """Over dtype, domain edges and mode; cabi.mha16_serves and mha16_native_pays are plain Python, so no library is loaded.  Under
    `auto` the measured rule is also replaced by both constant answers: the route follows whatever it says."""
    from isplib_amd import cabi
    from isplib_amd.plugin import mha16_route as route
    for pays in (True, False):
        with monkeypatch.context() as mp:
            mp.setattr(cabi, "mha16_native_pays", lambda rows, ld, pays=pays: pays)
            assert route(BF, 8, 8, 64, 2000, "auto") == ("mha16" if pays else "convert")
            assert route(BF, 8, 4, 32, 2000, "auto") == "convert" and route(BF, 8, 8, 64, 2000, "native") == "mha16"
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_MHA", raising=False)
    for dtype in (BF, FP):
        for mode in ("convert", "native", "auto", "nonsense"):
            for heads, d in ((1, 7), (1, 63), (1, 6), (1, 8), (1, 512), (1, 514), (8, 4), (2, 4), (8, 8), (2, 12), (64, 8), (65, 8), (3, 128),
                             (2, 2)):
                k = heads * d
                for pitch in (k + 1, k + 2, k, 3 * k):
                    for n in (2000, 2 ** 31):
                        got = route(dtype, heads, d, pitch, n, mode)
                        shape = (d % 2 == 0) if heads == 1 else (d >= 8 and d & (d - 1) == 0)
                        inside = shape and 8 <= k <= 512 and n < 2 ** 31             # an odd pitch is packed
                        if mode == "native":
                            want = "mha16" if inside else "convert"
                        elif mode == "auto":
                            ld = pitch if pitch % 2 == 0 else k
                            want = "mha16" if inside and cabi.mha16_native_pays(n, ld) else "convert"
                        else:
                            want = "convert"
                        assert got == want, (dtype, mode, heads, d, pitch, n)
        assert route(dtype, 8, 8, 64, 0xE0000000 // 128, "native") == "mha16"            # the operand at the descriptor's limit
        assert route(dtype, 8, 8, 64, 0xE0000000 // 128 + 1, "native") == "convert"
        assert route(dtype, 8, 8, 0xE0000000 // 2 // 1000 + 2, 1000, "native") == "mha16"       # too wide a pitch is packed
    for mode in ("convert", "native", "auto"):
        assert route(torch.float32, 8, 8, 64, 2000, mode) == "convert" and route(torch.float64, 8, 8, 64, 2000, mode) == "convert"
    # the mode comes from ISPLIB_HALF_MHA when it is not given; unset counts as convert, and ISPLIB_HALF=convert wins
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_MHA", "native")
    assert route(BF, 8, 8, 64, 2000) == "mha16" and route(BF, 1, 63, 64, 2000) == "convert" and route(BF, 8, 4, 32, 2000) == "convert"
    assert route(BF, 8, 8, 65, 2000) == "mha16"                                          # an odd pitch: packed
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "convert")                                   # GATv2's variable is another one
    assert route(BF, 8, 8, 64, 2000) == "mha16"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "auto")
    assert route(BF, 8, 8, 64, 2000) == "mha16"
    monkeypatch.setenv("ISPLIB_HALF_MHA", "auto")
    assert route(BF, 8, 8, 64, 2000) == route(BF, 8, 8, 64, 2000, "auto")
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 8, 8, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "native")
    monkeypatch.setenv("ISPLIB_HALF_MHA", "nonsense")
    assert route(BF, 8, 8, 64, 2000) == "convert"


_RULES_SRC = r"""
#include "isplib_hip.h"
extern "C" int qkv16_serves(long long rows, long long heads, long long d, long long ld) { return isplib_qkv16_serves(rows, heads, d, ld); }
extern "C" int gat16_serves(long long rows, long long heads, long long d, long long ld) { return isplib_gat16_serves(rows, heads, d, ld); }
extern "C" int qkv16_pays(long long rows, long long ld) { return isplib_qkv16_native_pays(rows, ld); }
"""


def _names(proto):
    return [re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", a)).strip().split(" ")[-1].lstrip("*") for a in proto.split(",")]


def test_header_rules_exports_and_symbols_are_consistent(tmp_path):
    from isplib_amd import _lib, cabi
    src, so = tmp_path / "rules.cpp", tmp_path / "rules.so"
    src.write_text(_RULES_SRC)
    subprocess.run(["g++", "-shared", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True, timeout=120)
    H = ctypes.CDLL(str(so))
    H.qkv16_serves.argtypes = H.gat16_serves.argtypes = [ctypes.c_longlong] * 4
    H.qkv16_pays.argtypes = [ctypes.c_longlong] * 2
    # the entries have a header of their own, which isplib_hip.h includes (the scrap library above includes only the latter)
    main = open(os.path.join(ROOT, "include", "isplib_hip.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert re.search(r'^#include "isplib_hip_mha16.h"$', bare, re.M) and "qkv16_" not in bare
    assert bare.rstrip().endswith('#include "isplib_hip_mha16.h"\n\n#endif')              # at the end of isplib_hip.h
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip_mha16.h")).read(), flags=re.S)
    # stated once: the header's inline returns isplib_gat16_serves(...)
    assert re.search(r"static inline int isplib_qkv16_serves\([^)]*\)\s*\{\s*return isplib_gat16_serves\(rows_gathered, heads, d, ld\);\s*\}",
                     header)
    assert "static inline int isplib_qkv16_native_pays(int64_t rows_gathered, int64_t ld)" in header
    top = cabi.DENSE_BYTES_MAX // 2
    table = SERVES_TABLE + ((top // 64, 8, 8, 64), (top // 64 + 1, 8, 8, 64), (top // 64, 4, 8, 64), (1000, 2, 8, top // 1000),
                            (1000, 2, 8, top // 1000 + 2), (top // 192, 8, 8, 192), (top // 192 + 1, 8, 8, 192))
    L = cabi.lib()
    for rows, heads, d, ld in table:
        want = cabi.mha16_serves(rows, heads, d, ld)
        assert want == cabi.gat16_serves(rows, heads, d, ld) == bool(H.qkv16_serves(rows, heads, d, ld)) == \
            bool(H.gat16_serves(rows, heads, d, ld)) == bool(L.isplib_qkv16_domain(rows, heads, d, ld)), (rows, heads, d, ld)
    assert any(cabi.mha16_serves(*t) for t in table) and not all(cabi.mha16_serves(*t) for t in table)
    assert not cabi.mha16_serves(10, 2, 4, 8) and not cabi.mha16_serves(10, 1, 6, 6) and not cabi.mha16_serves(10, 1, 9, 10)
    for rows, ld in ((0, 64), (1000, 64), (232_965, 64), (232_965, 128), (2 ** 20, 128), (2 ** 20 + 1, 128), (2_449_029, 128), (2_449_029, 512)):
        assert bool(H.qkv16_pays(rows, ld)) == cabi.mha16_native_pays(rows, ld) == bool(L.isplib_qkv16_auto(rows, ld)), (rows, ld)
    # that header, its name list in cabi and the library's dynamic symbols agree; cabi.EXPORTS stays what isplib_hip.h itself declares
    declared = set(re.findall(r"^(?:int|size_t|void|const char \*|float)\s+\*?(\w+)\(", header, re.M))
    assert declared == set(ENTRIES) == set(cabi.MHA16_EXPORTS) and not set(ENTRIES) & set(cabi.EXPORTS)
    assert not set(ENTRIES) & set(cabi.MHA_EXPORTS) and len(cabi.MHA16_EXPORTS) == len(ENTRIES)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.CABI_PATH], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert {n for n in exported if n.startswith("isplib_qkv16")} == set(ENTRIES)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert getattr(L, name) is not None
        assert name in integration, name
    assert int(re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+(\d+)", main).group(1)) == L.isplib_hip_abi_version() == 1
    # the argument lists: the fp32 entries' behind a dtype; the rows entry takes no z
    fw = re.search(r"isplib_qkv16_csr_hip\((.*?)\);", header, re.S).group(1)
    rows = re.search(r"isplib_qkv16_bw_rows_hip\((.*?)\);", header, re.S).group(1)
    cols = re.search(r"isplib_qkv16_bw_cols_hip\((.*?)\);", header, re.S).group(1)
    assert _names(fw) == ["dtype", "m", "n", "k", "nnz", "indx", "pntrb", "pntre", "heads", "scale", "q", "ldq", "key", "ldk", "v", "ldv",
                          "z", "ldz", "lse", "stream"]
    assert _names(rows)[:16] == _names(fw)[:16] and _names(rows)[16:] == ["g", "ldg", "lse", "dq", "lddq", "dsum", "stream"]
    assert _names(cols) == ["dtype", "m", "n", "k", "nnz", "row_t", "colb", "cole", "heads", "scale", "q", "ldq", "g", "ldg", "lse", "dsum",
                            "key", "ldk", "v", "ldv", "dkey", "lddk", "dv", "lddv", "stream"]
    for fn, proto in ((L.isplib_qkv16_csr_hip, fw), (L.isplib_qkv16_bw_rows_hip, rows), (L.isplib_qkv16_bw_cols_hip, cols)):
        assert len(fn.argtypes) == len(_names(proto))
    mk = open(os.path.join(ROOT, "isplib_amd", "csrc", "Makefile")).read()
    assert re.search(r"^HIP_SRCS\s*:=.*\bmha16\.hip\b", mk, re.M)
    assert all("isplib_hip_mha16.h" in line for line in mk.splitlines() if "isplib_hip_mha.h" in line)


def test_the_operator_schema_is_registered():
    import isplib_amd  # noqa: F401
    assert str(torch.ops.isplib.mha_spmm16.default._schema) == "isplib::" + SCHEMA


# ---- refusals, with CPU tensors and fake operators: nothing is launched ------------------------------------------------------------------

def _fake_ops(monkeypatch, calls):
    from isplib_amd import plugin

    class Ops:
        @staticmethod
        def mha_spmm16(*args):
            calls.append(("mha16",) + args)
            return torch.zeros(args[4].shape, dtype=args[4].dtype)

        @staticmethod
        def mha_spmm(*args):
            calls.append(("mha",) + args)
            return torch.zeros(args[4].shape, dtype=args[4].dtype)

    class FakeTorchOps:
        isplib = Ops

    monkeypatch.setattr(plugin.torch, "ops", FakeTorchOps)
    adj = mhost._adj(6, 6)
    st = adj.storage
    st._colptr, st._csr2csc, st._row_t = torch.zeros(7, dtype=torch.int64), torch.arange(6), torch.arange(6)    # the cached transpose
    return adj, st


def test_plugin_refuses_before_any_library_call(monkeypatch):
    import isplib_amd
    adj = mhost._adj(6, 4)
    q, k, v = torch.zeros(6, 16, dtype=BF), torch.zeros(4, 16, dtype=BF), torch.zeros(4, 16, dtype=BF)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_MHA", raising=False)
    for ops in ((q, k, v), (q.float(), k, v.float()), (q.to(FP), k.to(FP), v.to(FP))):
        with pytest.raises(TypeError, match="float32"):
            isplib_amd.mha_matmul(adj, *ops, heads=2)                            # unset: as it always was
    for mode in ("convert", "native", "auto"):
        monkeypatch.setenv("ISPLIB_HALF_MHA", mode)
        for pos in range(3):
            for other in (FP, torch.float32, torch.float64):
                ops = [q, k, v]
                ops[pos] = ops[pos].to(other)
                with pytest.raises(TypeError, match="share one 16-bit dtype"):
                    isplib_amd.mha_matmul(adj, *ops, heads=2)
            ops = [q, k, v]
            ops[pos] = ops[pos].float().numpy()
            with pytest.raises(TypeError, match="tensor"):
                isplib_amd.mha_matmul(adj, *ops, heads=2)
        with pytest.raises(TypeError, match="float32"):
            isplib_amd.mha_matmul(adj, q.float(), k.float(), v.double(), heads=2)     # an fp32 call does not read the variable
        with pytest.raises(TypeError, match="GPU tensor"):
            isplib_amd.mha_matmul(adj, q, k, v, heads=2)                         # CPU tensors: what the conversion route raises
        with pytest.raises(TypeError, match="GPU tensor"):
            adj.mha_matmul(q, k, k, 2, 0.25)                                     # k is v
        with pytest.raises(TypeError, match="GPU tensor"):
            adj.mha_matmul(q.to(FP), k.to(FP), v.to(FP))
        with pytest.raises(ValueError, match="power of two"):
            isplib_amd.mha_matmul(adj, torch.zeros(6, 12, dtype=BF), torch.zeros(4, 12, dtype=BF), torch.zeros(4, 12, dtype=BF), heads=2)
        with pytest.raises(ValueError, match="positive int"):
            isplib_amd.mha_matmul(adj, q, k, v, heads=0)
        with pytest.raises(ValueError, match="same width"):
            isplib_amd.mha_matmul(adj, q, torch.zeros(4, 8, dtype=BF), v, heads=2)
        with pytest.raises(ValueError, match="`scale` must be a finite Python number"):
            isplib_amd.mha_matmul(adj, q, k, v, heads=2, scale=float("nan"))
    doc = isplib_amd.plugin.mha_matmul.__doc__
    assert "dropout" in doc and "edge features" in doc and "beta" in doc and "no fallback" in doc and "mha16_route" in doc
    assert "ISPLIB_HALF_MHA" in isplib_amd.plugin.__doc__


def test_the_plugin_passes_the_views_own_pitches_and_the_head_scale(monkeypatch):
    import isplib_amd
    calls = []
    adj, st = _fake_ops(monkeypatch, calls)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.setenv("ISPLIB_HALF_MHA", "native")
    K = 32
    fused = torch.zeros(6, 3 * K, dtype=BF).as_subclass(mhost._Flagged)
    q, k, v = fused[:, :K], fused[:, K:2 * K], fused[:, 2 * K:]
    isplib_amd.mha_matmul(adj, q, k, v, heads=4)
    adj.mha_matmul(q, k, k, 4, -0.5)
    adj.mha_matmul(q, k, v)
    assert [c[0] for c in calls] == ["mha16"] * 3
    a, b, c = (call[1:] for call in calls)
    assert len(a) == 9 and a[0] is st._rowptr and a[1] is st._col and a[2] is st._colptr and a[3] is st._row_t
    assert a[4] is q and a[5] is k and a[6] is v                             # the views themselves: no copy, no .contiguous(), no cast
    assert [t.stride(0) for t in a[4:7]] == [3 * K] * 3 and [t.storage_offset() for t in a[4:7]] == [0, K, 2 * K]
    assert a[7] == 4 and type(a[8]) is float and a[8] == 1.0 / math.sqrt(8)  # the HEAD width, not K
    assert b[5] is k and b[6] is k and b[7:] == (4, -0.5)
    assert c[7] == 1 and c[8] == 1.0 / math.sqrt(K)
    # an operand outside the route falls to the conversion route, not to an error: d = 4 is outside the 16-bit domain and inside the
    # fp32 one; `convert` and ISPLIB_HALF=convert take every call there
    del calls[:]
    q4, k4 = torch.zeros(6, 16, dtype=BF).as_subclass(mhost._Flagged), torch.zeros(6, 16, dtype=BF).as_subclass(mhost._Flagged)
    out = isplib_amd.mha_matmul(adj, q4, k4, k4, heads=4)
    assert out.dtype == BF and calls[0][0] == "mha" and all(t.dtype == torch.float32 for t in calls[0][5:8])
    assert calls[0][6] is calls[0][7] and calls[0][9] == 0.5                 # k is v survives the conversion; 1 / sqrt(4)
    monkeypatch.setenv("ISPLIB_HALF_MHA", "convert")
    assert isplib_amd.mha_matmul(adj, q, k, v, heads=4).dtype == BF and calls[-1][0] == "mha"
    monkeypatch.setenv("ISPLIB_HALF_MHA", "native")
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert isplib_amd.mha_matmul(adj, q, k, v, heads=4).dtype == BF and calls[-1][0] == "mha"
    # an odd pitch is outside the route at that pitch: the operator packs such an operand itself, so the route stays native
    monkeypatch.setenv("ISPLIB_HALF", "auto")
    odd = torch.zeros(6, K + 1, dtype=FP).as_subclass(mhost._Flagged)[:, :K]
    fp = torch.zeros(6, K, dtype=FP).as_subclass(mhost._Flagged)
    isplib_amd.mha_matmul(adj, fp, odd, fp, heads=4)
    assert calls[-1][0] == "mha16" and calls[-1][6] is odd


def test_ctypes_wrappers_refuse_bad_operands_before_the_call():
    from isplib_amd import cabi
    rowptr, col = torch.arange(0, 7, dtype=torch.int64), torch.arange(6, dtype=torch.int64) % 4
    colptr = torch.arange(0, 5, dtype=torch.int64)
    q, k, v, g = (torch.zeros(r, 16, dtype=BF) for r in (6, 4, 4, 6))
    lse = torch.zeros(6, 2)
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        cabi.mha16_forward(rowptr, col, q.float(), k, v, 2)
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.mha16_forward(rowptr, col, q, k.to(FP), v, 2)
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.mha16_forward(rowptr, col, q, k, v.float(), 2)
    with pytest.raises(TypeError, match="int64"):
        cabi.mha16_forward(rowptr.to(torch.int32), col, q, k, v, 2)
    with pytest.raises(ValueError, match="unit inner stride"):
        cabi.mha16_forward(rowptr, col, q, torch.zeros(16, 4, dtype=BF).t(), v, 2)
    with pytest.raises(ValueError, match="even pitch"):
        cabi.mha16_forward(rowptr, col, q, k, torch.zeros(4, 17, dtype=BF)[:, :16], 2)
    with pytest.raises(ValueError, match=r"`v` must be \[4, 16\]"):
        cabi.mha16_forward(rowptr, col, q, k, torch.zeros(4, 8, dtype=BF), 2)
    with pytest.raises(ValueError, match="heads \\* d"):
        cabi.mha16_forward(rowptr, col, q, k, v, 3)
    with pytest.raises(ValueError, match="`scale` must be a finite number"):
        cabi.mha16_forward(rowptr, col, q, k, v, 2, float("nan"))
    with pytest.raises(ValueError, match="isplib_qkv16_serves"):
        cabi.mha16_forward(rowptr, col, torch.zeros(6, 8, dtype=BF), torch.zeros(4, 8, dtype=BF), torch.zeros(4, 8, dtype=BF), 2)   # d = 4
    with pytest.raises(ValueError, match="isplib_qkv16_serves"):
        cabi.mha16_forward(rowptr, col, torch.zeros(6, 6, dtype=BF), torch.zeros(4, 6, dtype=BF), torch.zeros(4, 6, dtype=BF), 1)
    with pytest.raises(ValueError, match=r"`out\[1\]` must be \[6, 2\]"):
        cabi.mha16_forward(rowptr, col, q, k, v, 2, out=(torch.zeros(6, 16, dtype=BF), torch.zeros(6, 1)))
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.mha16_forward(rowptr, col, q, k, v, 2, out=(torch.zeros(6, 16), lse))
    with pytest.raises(ValueError, match=r"`lse` must be \[6, 2\]"):
        cabi.mha16_backward_rows(rowptr, col, q, k, v, g, torch.zeros(5, 2), 2)
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.mha16_backward_rows(rowptr, col, q, k, v, g.to(FP), lse, 2)
    with pytest.raises(ValueError, match=r"\(dq, D\)"):
        cabi.mha16_backward_rows(rowptr, col, q, k, v, g, lse, 2, out=(torch.zeros(6, 16, dtype=BF),))
    with pytest.raises(ValueError, match=r"`dsum` must be \[6, 2\]"):
        cabi.mha16_backward_cols(colptr, col, q, k, v, g, lse, torch.zeros(6, 1), 2)
    with pytest.raises(ValueError, match=r"\(dk, dv\)"):
        cabi.mha16_backward_cols(colptr, col, q, k, v, g, lse, lse, 2, out=(torch.zeros(4, 16, dtype=BF),))
    with pytest.raises(TypeError, match="bfloat16"):
        cabi.mha16_backward_cols(colptr, col, q.to(FP), k, v, g, lse, lse, 2)
    for call in (lambda: cabi.mha16_forward(rowptr, col, q, k, v, 2), lambda: cabi.mha16_backward_rows(rowptr, col, q, k, v, g, lse, 2),
                 lambda: cabi.mha16_backward_cols(colptr, col, q, k, v, g, lse, lse, 2)):
        with pytest.raises(ValueError, match="GPU tensor"):
            call()                                                               # well-formed, but on the CPU
    assert cabi.mha16_serves(10, 8, 8, 64) and cabi.mha16_serves is not cabi.gat16_serves
