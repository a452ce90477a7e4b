"""The 16-bit multi-head attention operator (q, k, v) with attention dropout, host side (no GPU): the bound of
tests/mha16_dropout_ref.py is neither too tight (an fp32 NumPy emulation in the kernels' own form -- tests/test_mha16_host.py's, with
the masked value accumulation beside the unmasked l, the finished row times c, the masked t_e after the butterfly in the one-pass rows
backward, the value coefficient q_e ? a_e c : 0 of the columns kernel, one rounding -- passes on every case) nor too loose (the planted
faults each miss it by a wide margin), mha16_drop_route is a pure and total function over both variables and ISPLIB_HALF, the header's
rule agrees with its cabi twin and the symbol, the header (alone, as C and as C++), MHA16_DROP_EXPORTS, the library's symbols and
INTEGRATION.md are consistent, the entries refuse in their stated order before anything is launched (CPU pointers), and the docstring
keeps its pinned phrases.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import half_ref
from tests import mha16_cases as c16
from tests import mha16_dropout_cases as cases
from tests import mha_dropout_ref as ref
from tests import test_mha16_host as host16
from tests.gat_ref import per_head
from tests.test_mha16_host import fma, head_dots, per_slot_fma, per_slot_sums, slot_edges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BF, FP = torch.bfloat16, torch.float16
ENTRIES = ("isplib_qkv_half_drop_csr_hip", "isplib_qkv_half_drop_bw_rows_hip", "isplib_qkv_half_drop_bw_cols_hip",
           "isplib_qkv_half_drop_auto")
SCHEMA = ("mha_drop_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor q, Tensor k, Tensor v, "
          "int heads, float scale, float p, int seed) -> Tensor")
WIDE = 10.0                                            # a planted fault must miss the bound by more than this factor


def emulate32(case, mask=None, mask_cols=None, c=None, mask_l=False, c_in_dv=True, d_from_z16=False, U=None):
    """The DROP kernels' arithmetic in fp32 NumPy, before the one rounding of z, dq, dk and dv.  `mask` [nnz, H]: the keep bits the
    forward and the rows kernel use (None: the case's); `mask_cols`: those of the columns kernel, per CSR position (None: `mask`);
    `c`: the keep scale (None: the case's).  The planted faults: `mask_l` (l sums the kept weights only), `c_in_dv` False (the value
    coefficient of dv without c), `d_from_z16` (D[i,h] = <g_i, z16_i>_h)."""
    U = host16.forward_step_width() if U is None else U
    rowptr, col, H, p = case.rowptr, case.col, case.heads, F32(case.ps)
    mask = case.ref["q"] if mask is None else mask
    mask_cols = mask if mask_cols is None else mask_cols
    c = F32(case.scale if c is None else c)
    m, n, K = case.m, case.n, case.width
    d = K // H
    G = 64 // c16.lanes_per_row(K)
    q3, k3, v3, g3 = per_head(case.q, H), per_head(case.k, H), per_head(case.v, H), per_head(case.g, H)
    row = ref.edge_rows(rowptr)
    s = (head_dots(q3[row], k3[col]) * p).astype(F32)                                    # p multiplies the finished dot product
    t = head_dots(g3[row], v3[col])                                                      # the butterfly's sum, before the mask
    none = -np.finfo(F32).max
    z, lse = np.zeros((m, H, d), F32), np.full((m, H), -np.inf, F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for i in range(m):
            b, e = int(rowptr[i]), int(rowptr[i + 1])
            if e == b:
                continue
            mrun, l, lk, acc = np.full((G, H), none, F32), np.zeros((G, H), F32), np.zeros((G, H), F32), np.zeros((G, H, d), F32)
            for idx in slot_edges(b, e, G, U):                                           # [U, G]
                live = idx >= 0
                at = np.maximum(idx, 0)
                sc = np.where(live[:, :, None], s[at], none)                             # [U, G, H]
                mnew = np.maximum(mrun, sc.max(0))
                r = np.exp((mrun - mnew).astype(F32))
                mrun, l, lk, acc = mnew, (l * r).astype(F32), (lk * r).astype(F32), (acc * r[:, :, None]).astype(F32)
                for u in range(U):
                    w = np.where(live[u][:, None], np.exp((sc[u] - mnew).astype(F32)), F32(0)).astype(F32)
                    wk = np.where(mask[at[u]], w, F32(0)).astype(F32)                    # the mask reaches the values only
                    l = (l + w).astype(F32)
                    lk = (lk + wk).astype(F32)
                    acc = fma(wk[:, :, None], v3[col[at[u]]], acc)
            while mrun.shape[0] > 1:                                                     # the slots pairwise, by the rule of a step
                ma, mb = mrun[0::2], mrun[1::2]
                mnew = np.maximum(ma, mb)
                ra, rb = np.exp((ma - mnew).astype(F32)), np.exp((mb - mnew).astype(F32))
                l = ((l[0::2] * ra).astype(F32) + (l[1::2] * rb).astype(F32)).astype(F32)
                lk = ((lk[0::2] * ra).astype(F32) + (lk[1::2] * rb).astype(F32)).astype(F32)
                acc = ((acc[0::2] * ra[:, :, None]).astype(F32) + (acc[1::2] * rb[:, :, None]).astype(F32)).astype(F32)
                mrun = mnew
            den = np.where(lk[0] > 0, lk[0], F32(1)) if mask_l else l[0]
            z[i] = ((acc[0] / den[:, None]).astype(F32) * c).astype(F32)                 # the finished row times c
            lse[i] = (mrun[0] + np.log(l[0])).astype(F32)
        a = np.exp((s - np.where(np.isfinite(lse), lse, F32(0))[row]).astype(F32)).astype(F32)
    # the one-pass backward over the rows: t_e takes the mask after the butterfly
    tm = (t * np.where(mask, c, F32(0)).astype(F32)).astype(F32)
    aet = (a * tm).astype(F32)
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
    # the backward over the columns, on the transposed structure (entries of a column in row order; the bit of the CSR position)
    order = np.argsort(col, kind="stable")
    cuts = np.searchsorted(col[order], np.arange(n + 1))
    tmc = (t * np.where(mask_cols, c, F32(0)).astype(F32)).astype(F32)
    ds = (a * (tmc - D[row]).astype(F32)).astype(F32)
    aev = np.where(mask_cols, (a * c).astype(F32) if c_in_dv else a, F32(0)).astype(F32)
    ds_t, a_t, q_t, g_t = ds[order], aev[order], qe[order], ge[order]
    dk, dv = np.zeros((n, H, d), F32), np.zeros((n, H, d), F32)
    for j in range(n):
        b, e = int(cuts[j]), int(cuts[j + 1])
        if e > b:
            dk[j] = (per_slot_fma(b, e, G, ds_t, q_t) * p).astype(F32)
            dv[j] = per_slot_fma(b, e, G, a_t, g_t)
    return dict(z=z.reshape(m, K), lse=lse, D=D, dq=dq.reshape(m, K), dk=dk.reshape(n, K), dv=dv.reshape(n, K))


def rounded(case, got):
    """z, dq, dk and dv rounded once to the case's dtype (and widened again for the comparison); lse and D stay as they are."""
    out = dict(got)
    for name in cases.OUT16:
        out[name] = half_ref.widen(half_ref.round16(np.asarray(got[name], F32), case.dtype))
    return out


def held(case, **how):
    frac = cases.fractions(case, rounded(case, emulate32(case, **how)))
    print(case.name, how and sorted(how), {n: round(v, 4) for n, v in frac.items()})
    return frac


# ---- the cases and the bound ------------------------------------------------------------------------------------------------------------

def test_the_cases_assert_their_conditions():
    """Every case asserts its rho cap and that its mask keeps some entries and drops some when it is built; here the rest."""
    assert cases.check_fully_dropped_rows()
    assert len(cases.config_specs()) == len(c16.CONFIGS) + len(c16.FP16_CONFIGS) + len(c16.GRAPH2_CONFIGS)
    assert len(cases.p_specs()) == 9 and {p for _, _, p in cases.p_specs()} == {0.1, 0.6, 0.9}
    kinds = [c.kind for c in cases.special_cases()]
    assert kinds.count("large") == 2 and kinds.count("single") == 2 and {"duplicates", "position", "shared", "rect"} <= set(kinds)
    assert {(c.m, c.n) for c in cases.special_cases() if c.kind == "rect"} == {(233, 67), (67, 233)}
    large = cases.large_case()
    assert large.ref["s"].max() > 150 and large.ref["s"].min() < -150 and float(large.bound["rho"].max()) <= c16.LARGE_RHO_MAX
    dup, pos = cases.duplicate_case(), cases.position_case()
    assert dup.wide.any() and (np.abs(pos.wrong["dv"] - pos.ref["dv"]) > WIDE * pos.bound["dv"]).any()
    assert all(c.m <= 233 and c.n <= 233 for c in cases.special_cases())                   # nothing larger than the existing graphs
    fused = cases.fused_case(8, 16)
    assert fused.fused.dtype == BF and fused.fused.stride(0) == 3 * fused.width


@pytest.mark.parametrize("spec", cases.config_specs(), ids=cases.case_id)
def test_bound_is_not_too_tight(spec):
    frac = held(cases.config_case(*spec))
    assert all(v <= 1.0 for v in frac.values()), frac


@pytest.mark.parametrize("spec", cases.p_specs(), ids=lambda s: f"h{s[0]}d{s[1]}-p{s[2]}")
def test_bound_is_not_too_tight_at_every_p(spec):
    h, d, p = spec
    case = cases.config_case(h, d, BF, "g1", p)
    got = rounded(case, emulate32(case))
    frac = cases.fractions(case, got)
    print(case.name, {n: round(v, 4) for n, v in frac.items()})
    assert all(v <= 1.0 for v in frac.values()), frac
    gone = case.all_dropped()                                     # a live (row, head) with every entry dropped: z = 0 exactly, lse finite
    assert np.all(per_head(got["z"], h)[gone] == 0) and np.all(np.isfinite(got["lse"][gone]))


@pytest.mark.parametrize("case", cases.special_cases(), ids=lambda c: c.name)
def test_bound_is_not_too_tight_on_the_special_cases(case):
    frac = held(case)
    assert all(v <= 1.0 for v in frac.values()), frac


def test_single_entry_rows_are_exact_in_the_emulation():
    """a_e = 1: a kept (row, head) is round16(float32(v_j c)), a dropped one 0."""
    for dt in (BF, FP):
        case = cases.single_case(dt)
        z = rounded(case, emulate32(case))["z"]
        row, H = case.ref["row"], case.heads
        want = np.zeros((case.m, H, case.d), F32)
        want[row] = np.where(case.ref["q"][:, :, None], (per_head(case.v, H)[case.col] * F32(case.scale)).astype(F32), F32(0))
        assert np.array_equal(z, half_ref.widen(half_ref.round16(want.reshape(case.m, case.width), dt)))


def test_every_bit_kept_and_c_one_is_the_emulation_without_dropout():
    """T = 0 and c = 1 give the bits of DROP = false: the same holds of the two emulations."""
    for h, d in ((8, 8), (1, 46)):
        case = cases.config_case(h, d)
        got = emulate32(case, mask=np.ones_like(case.ref["q"]), c=1.0)
        want = host16.emulate32(case.base)
        for name in cases.OUTPUTS:
            assert np.array_equal(got[name], want[name]), (case.name, name)


# ---- planted faults: each must miss the bound by a wide margin --------------------------------------------------------------------------

def test_fault_mask_keyed_by_row_and_column():
    case = cases.duplicate_case()
    frac = held(case, mask=cases.pair_mask(case))
    assert frac["z"] > WIDE and frac["lse"] <= 1.0                 # lse does not see the mask


def test_fault_mask_applied_to_l():
    """A softmax over the kept entries only."""
    for h, d in cases.FORM_CONFIGS:
        frac = held(cases.config_case(h, d), mask_l=True)
        assert frac["z"] > WIDE and frac["lse"] <= 1.0


def test_fault_c_missing_from_dv():
    for h, d in cases.FORM_CONFIGS:
        frac = held(cases.config_case(h, d), c_in_dv=False)
        assert frac["dv"] > WIDE
        assert all(v <= 1.0 for n, v in frac.items() if n != "dv")


def test_fault_transposed_position_hashed_in_the_columns_kernel():
    case = cases.position_case()
    frac = held(case, mask_cols=case.wrong_mask)
    assert frac["dv"] > WIDE and frac["dk"] > WIDE
    assert all(frac[n] <= 1.0 for n in ("z", "lse", "D", "dq"))    # the forward and the rows kernel hash base + lane


def test_fault_d_taken_from_the_rounded_z():
    """With g aligned to z at H = 1, K = 512 in bf16, D = <g, z16> carries u sum |g z| into D (an fp32 output)."""
    base = c16.config_case(1, 512)
    z = ref.mha_drop(base.rowptr, base.col, base.q, base.k, base.v, 1, base.p, cases.P, cases.SEED, fwd=base.ref)["z"]
    aligned = cases.Case(c16.Case16("h1d512-aligned-g", base.rowptr, base.col, np.array(base.q), np.array(base.k), np.array(base.v),
                                    (z * 8.0).astype(F32), 1, base.p, BF), cases.P, cases.SEED)
    assert max(held(aligned).values()) <= 1.0                       # the one-pass form passes on the same case
    frac = held(aligned, d_from_z16=True)
    assert frac["D"] > WIDE
    assert frac["z"] <= 1.0 and frac["lse"] <= 1.0 and frac["dv"] <= 1.0     # what D does not touch


# ---- the route ---------------------------------------------------------------------------------------------------------------------------

def test_mha16_drop_route_truth_table(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import mha16_drop_route as route
    for name in ("ISPLIB_HALF", "ISPLIB_HALF_MHA", "ISPLIB_HALF_MHA_DROP"):
        monkeypatch.delenv(name, raising=False)
    shape = (BF, 8, 8, 64, 2000)
    for half in (None, "auto", "native", "convert"):
        for mha in (None, "convert", "native", "auto", "nonsense"):
            for drop in (None, "convert", "native", "auto", "nonsense"):
                for pays in (True, False):
                    with monkeypatch.context() as mp:
                        for name, value in (("ISPLIB_HALF", half), ("ISPLIB_HALF_MHA", mha), ("ISPLIB_HALF_MHA_DROP", drop)):
                            if value is not None:
                                mp.setenv(name, value)
                        mp.setattr(cabi, "mha16_drop_native_pays", lambda rows, ld, pays=pays: pays)
                        admitted = half != "convert" and mha in ("native", "auto")          # mha16_native_pays: both classes pay
                        want = admitted and (drop == "native" or (drop == "auto" and pays))
                        assert route(*shape) == ("mha16drop" if want else "convert"), (half, mha, drop, pays)
                        assert route(torch.float32, 8, 8, 64, 2000) == "convert"
                        assert route(BF, 8, 4, 32, 2000) == "convert" and route(BF, 1, 9, 10, 2000) == "convert"       # the family's domain
                        assert route(BF, 8, 8, 64, 2 ** 31) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_MHA", "native")
    assert route(*shape) == "convert"                                                    # unset means convert
    assert route(*shape, mode="native") == "mha16drop" and route(*shape, mode="convert") == "convert"
    assert route(*shape, mode="auto") == ("mha16drop" if cabi.mha16_drop_native_pays(2000, 64) else "convert")
    assert route(BF, 8, 8, 65, 2000, mode="native") == "mha16drop"                        # an odd pitch: packed
    monkeypatch.setenv("ISPLIB_HALF_MHA", "convert")
    assert route(*shape, mode="native") == "convert"                                     # ISPLIB_HALF_MHA=convert wins
    monkeypatch.delenv("ISPLIB_HALF_MHA")
    assert route(*shape, mode="native") == "convert"                                     # unset: mha_matmul raises before it asks


# ---- the header, the exports, the symbols ----------------------------------------------------------------------------------------------------

def _bare(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _names(proto):
    return [re.sub(r"\s+", " ", a).strip().split(" ")[-1].lstrip("*") for a in proto.split(",")]


def _proto(header, name):
    return _names(re.search(name + r"\((.*?)\);", header, re.S).group(1))


def test_header_exports_symbols_and_integration_are_consistent():
    from isplib_amd import _lib, cabi
    main = _bare("isplib_hip.h")
    assert re.search(r'^#include "isplib_hip_mha16_drop.h"$', main, re.M)
    assert main.index('#include "isplib_hip_mha16_drop.h"') < main.index('#include "isplib_hip_mha16.h"')
    assert main.rstrip().endswith('#include "isplib_hip_mha16.h"\n\n#endif') and "qkv_half_drop" not in main
    header = _bare("isplib_hip_mha16_drop.h")
    declared = sorted(set(re.findall(r"^\s*int\s+(\w+)\s*\(", header, flags=re.M)))
    assert declared == sorted(ENTRIES) == sorted(cabi.MHA16_DROP_EXPORTS)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.CABI_PATH], text=True)
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert {n for n in exported if n.startswith("isplib_qkv_half_drop_")} == set(ENTRIES)
    assert not any(n.startswith(("isplib_mha", "isplib_qkv16", "isplib_qkv_drop")) for n in ENTRIES)      # those prefixes are pinned elsewhere
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = cabi.lib()
    for name in ENTRIES:
        assert name not in cabi.EXPORTS + cabi.MHA_EXPORTS + cabi.MHA16_EXPORTS + cabi.MHA_DROP_EXPORTS
        assert getattr(L, name) is not None and name in integration, name
    assert "ISPLIB_HALF_MHA_DROP" in integration
    assert int(re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+(\d+)", main).group(1)) == 1 and L.isplib_hip_abi_version() == 1
    # the argument lists: those of isplib_hip_mha16.h (csr2csc after cole in the columns entry), then threshold, keep_scale, seed
    plain = _bare("isplib_hip_mha16.h")
    for old, new, extra in (("isplib_qkv16_csr_hip", ENTRIES[0], 3), ("isplib_qkv16_bw_rows_hip", ENTRIES[1], 3),
                            ("isplib_qkv16_bw_cols_hip", ENTRIES[2], 4)):
        was, now = _proto(plain, old), _proto(header, new)
        assert len(now) == len(was) + extra and now[-3:] == ["threshold", "keep_scale", "seed"]
        at = was.index("cole") + 1 if extra == 4 else len(was)
        assert now[:-3] == was[:at] + ["csr2csc"] * (extra - 3) + was[at:], new
        assert len(getattr(L, new).argtypes) == len(getattr(L, old).argtypes) + extra == len(now)
        assert getattr(L, new).argtypes[-3:] == [ctypes.c_uint32, ctypes.c_float, ctypes.c_uint64]
    # one statement of the bit, no new kernel file, the header among the build's dependencies
    src = open(os.path.join(ROOT, "isplib_amd", "csrc", "mha16.hip")).read()
    assert '#include "gat_dropout.h"' in src and "fmix32" not in src.replace("one fmix32", "") and "0x9E3779B9" not in src
    assert '#include "attn_common.h"' in src and "struct AttnDrop" not in src
    mk = open(os.path.join(ROOT, "isplib_amd", "csrc", "Makefile")).read()
    assert "mha_drop.hip" not in mk and "mha16_drop.hip" not in mk
    assert all("isplib_hip_mha16_drop.h" in line for line in mk.splitlines() if "isplib_hip_mha16.h" in line)
    build = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "cabi.MHA16_DROP_EXPORTS" in build


_SCRAP = r"""
#include "isplib_hip_mha16_drop.h"
int pays(long long rows, long long ld) { return isplib_qkv_half_drop_native_pays(rows, ld); }
int (*forward)(int, int64_t, int64_t, int64_t, int64_t, const int64_t *, const int64_t *, const int64_t *, int64_t, float, const void *,
               int64_t, const void *, int64_t, const void *, int64_t, void *, int64_t, float *, void *, uint32_t, float, uint64_t)
    = isplib_qkv_half_drop_csr_hip;
int dtype_bf16(void) { return ISPLIB_DTYPE_BF16; }
"""


def test_the_header_alone_compiles_as_c_and_as_cxx_and_its_rule_is_the_librarys(tmp_path):
    from isplib_amd import _lib, cabi
    inc = os.path.join(ROOT, "include")
    for compiler, lang, src in (("gcc", "c", "scrap.c"), ("g++", "c++", "scrap.cpp")):
        (tmp_path / src).write_text(_SCRAP)
        subprocess.check_call([compiler, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(tmp_path / src)])
    # through isplib_hip.h too, in either order
    (tmp_path / "both.c").write_text('#include "isplib_hip.h"\n#include "isplib_hip_mha16_drop.h"\n'
                                     "int pays(long long r, long long l) { return isplib_qkv_half_drop_native_pays(r, l) + "
                                     "isplib_qkv16_native_pays(r, l); }\n")
    subprocess.check_call(["gcc", "-x", "c", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(tmp_path / "both.c")])
    so = tmp_path / "rule.so"
    (tmp_path / "rule.cpp").write_text('#include "isplib_hip_mha16_drop.h"\nextern "C" int pays(long long r, long long l) '
                                       "{ return isplib_qkv_half_drop_native_pays(r, l); }\n")
    subprocess.check_call(["g++", "-shared", "-fPIC", "-I", inc, str(tmp_path / "rule.cpp"), "-o", str(so)])
    H = ctypes.CDLL(str(so))
    H.pays.argtypes = [ctypes.c_longlong] * 2
    L = cabi.lib()
    for rows, ld in ((0, 64), (1000, 64), (232_965, 64), (232_965, 128), (2 ** 20, 128), (2 ** 20 + 1, 128), (2_449_029, 128), (2_449_029, 512)):
        assert bool(H.pays(rows, ld)) == cabi.mha16_drop_native_pays(rows, ld) == bool(L.isplib_qkv_half_drop_auto(rows, ld)), (rows, ld)
    assert _lib.CABI_PATH


def test_the_operator_schema_is_registered():
    import isplib_amd  # noqa: F401
    schema = str(torch.ops.isplib.mha_drop_spmm16.default._schema)
    assert schema == "isplib::" + SCHEMA, schema


def test_the_docstrings_keep_their_pinned_phrases():
    import isplib_amd
    doc = isplib_amd.plugin.mha_matmul.__doc__
    assert "kernel ARGUMENT" in doc and "no 16-bit dropout kernel" in doc and "mha16_drop_route" in doc and "ISPLIB_HALF_MHA_DROP" in doc
    gap = re.search(r"Not part of the operator:(.*?)\.", doc, re.S).group(1)
    assert "dropout" not in gap and "edge features" in gap and "root weight" in gap and "beta" in gap
    assert "ISPLIB_HALF_MHA_DROP" in isplib_amd.plugin.__doc__ and "mha16_drop_route" in isplib_amd.plugin.__doc__


# ---- the refusals, in their order, with CPU pointers: nothing is launched ----------------------------------------------------------------

def _refusal_steps(which):
    """(argument, bad value, status, message) in the order the entry refuses: every call below carries ALL the faults from its own on,
    so the message names the FIRST check that fails; `which`: 0 forward, 1 rows, 2 columns."""
    own_ld = "ldk" if which == 2 else "ldq"                  # a row-resident pitch, below k
    gathered_ld = "ldq" if which == 2 else "ldk"             # a gathered pitch, odd: outside the domain
    steps = [("dtype", 7, 1, "dtype must be"), ("n" if which == 2 else "m", -1, 1, "negative dimension"), (own_ld, 8, 1, "leading dimension"),
             ("heads", 3, 1, "multiple of heads"), ("scale", float("nan"), 1, "finite"), (gathered_ld, 17, 128, "isplib_qkv16_serves"),
             ("key" if which == 2 else "q", None, 1, "null operand"), ("v", "odd", 1, "4-byte aligned"),
             ("keep_scale", 0.0, 1, "keep_scale must be a positive finite number"), ("nnz", 2 ** 31, 1, "nnz must be below 2^31"),
             ("seed", 2 ** 63, 1, "seed must be below 2^63")]
    if which == 2:
        steps.append(("csr2csc", None, 1, "null csr2csc"))
    return steps


@pytest.mark.parametrize("which", (0, 1, 2), ids=("forward", "rows", "columns"))
def test_the_entries_refuse_in_the_stated_order_before_any_launch(which):
    from isplib_amd import cabi
    L = cabi.lib()
    fn = getattr(L, ENTRIES[which])
    names = _proto(_bare("isplib_hip_mha16_drop.h"), ENTRIES[which])
    buf = np.zeros(4096, np.uint8)                                               # CPU memory: a launch would fault, none happens
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    good = dict(dtype=cabi.DTYPE_BF16, m=4, n=4, k=16, nnz=4, heads=2, scale=0.25, stream=None, threshold=1 << 31, keep_scale=2.0, seed=5)
    for name in names:
        if name.startswith("ld"):
            good[name] = 16
        elif name not in good:
            good[name] = base                                                    # every pointer: non-null, 16-byte aligned
    steps = _refusal_steps(which)
    bad = {name: (base + 2 if value == "odd" else value) for name, value, _, _ in steps}

    def call(args):
        return fn(*[ctypes.c_void_p(args[n]) if fn.argtypes[i] is ctypes.c_void_p else args[n] for i, n in enumerate(names)])

    for at, (name, _, status, message) in enumerate(steps):
        args = dict(good)
        args.update({n: bad[n] for n, _, _, _ in steps[at:]})                    # this fault and every later one
        assert call(args) == status, (name, cabi.last_error())
        assert message in cabi.last_error() and ENTRIES[which] in cabi.last_error(), (name, cabi.last_error())
    # nothing to do succeeds without a launch, and before the dropout arguments are looked at, as in the entries without dropout
    empty = dict(good)
    empty.update({("n" if which == 2 else "m"): 0, "keep_scale": 0.0, "seed": 2 ** 63})
    assert call(empty) == 0
