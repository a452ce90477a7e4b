"""Host side of the 16-bit SDDMM row kernel (isplib_sddmm_csr_rows16_hip): the plug-in's choice as a pure function, the measured
rule's mirror, the header, the wrapper's operand checks, a census of the GPU tests' inputs, and a numpy emulation of the kernel's
summation order held to the bounds the GPU tests assert.  No device."""
import os
import re

import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests import sddmm_rows16_cases as cs

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
BIG = 2_449_029                                # the ogbn-products shape


def test_rows16_da_route_is_pure_and_total(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import rows16_da_route as route
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_DA", raising=False)
    for dtype in (BF, FP):
        assert route(dtype, 64, 64, 2000, False, "native") == "rows16"
        assert route(dtype, 64, 64, 2000, False, "convert") == "convert"
        assert route(dtype, 64, 64, 2000, False, "nonsense") == "convert"
        for n, k in ((2000, 64), (BIG, 128), (BIG, 256)):
            for ordered in (False, True):
                want = "rows16" if cabi.sddmm_rows16_native_pays(n, k, ordered) else "convert"
                assert route(dtype, k, k, n, ordered, "auto") == want
                assert route(dtype, k, k, n, ordered, "native") == "rows16"
                # a graph the handle's whole-row task plan serves keeps the fp32 task-list SDDMM, whatever the mode
                for mode in ("auto", "native", "convert"):
                    assert route(dtype, k, k, n, ordered, mode, whole_row_slices=4) == "convert"
        # the domain's edges: never an error, whatever the mode
        for mode in ("auto", "native", "convert"):
            assert route(dtype, 41, 41, 2000, False, mode) == "convert"         # odd k
            assert route(dtype, 6, 6, 2000, False, mode) == "convert"           # narrow k
            assert route(dtype, 1026, 1026, 2000, False, mode) == "convert"     # g[row, :] no longer fits the registers
            assert route(dtype, 2 ** 24, 2 ** 24, 1, False, mode) == "convert"
            assert route(dtype, 64, 64, 0xE0000000 // 128 + 1, False, mode) == "convert"
        assert route(dtype, 8, 8, 2000, False, "native") == "rows16"
        assert route(dtype, 1024, 1024, 2000, False, "native") == "rows16"     # the two-chunk form
        assert route(dtype, 64, 64, 0xE0000000 // 128, False, "native") == "rows16"   # X at the descriptor's limit (3.5 GiB)
        assert route(dtype, 64, 67, 2000, False, "native") == "rows16"         # an odd pitch is packed
        assert route(dtype, 64, 192, 2000, True, "native") == "rows16"
        assert route(dtype, 64, 64, 0, True, "native") == "rows16"
    for mode in ("auto", "native", "convert"):
        assert route(F32, 64, 64, 2000, False, mode) == "convert"               # consulted for 16-bit features only
        assert route(torch.float64, 64, 64, 2000, True, mode) == "convert"
    # the mode comes from ISPLIB_HALF_DA when it is not given; unset means convert, and ISPLIB_HALF=convert wins
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_DA", "native")
    assert route(BF, 64, 64, 2000) == "rows16"
    assert route(BF, 64, 64, 2000, whole_row_slices=2) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "native")
    assert route(BF, 64, 64, 2000) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF", "auto")
    assert route(BF, 64, 64, 2000) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF_DA", "auto")
    assert route(BF, 64, 64, 2000) == route(BF, 64, 64, 2000, False, "auto")
    assert route(BF, 128, 128, BIG, True) == route(BF, 128, 128, BIG, True, "auto")
    monkeypatch.setenv("ISPLIB_HALF_DA", "convert")
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_DA", "nonsense")
    assert route(BF, 64, 64, 2000) == "convert"


def test_domain_and_auto_rule_mirrors_match_the_library():
    """cabi.sddmm_rows16_native_pays restates isplib_sddmm_rows16_native_pays (isplib_sddmm_rows16_auto exports it), and
    cabi.sddmm_rows16_serves is the row family's domain with k <= 1024."""
    from isplib_amd import cabi
    for n, ldy in ((0, 64), (1000, 64), (50_000, 64), (612_000, 128), (BIG, 128), (BIG, 256), (2 ** 20, 128), (2 ** 20 + 1, 128)):
        for ordered in (False, True):
            assert bool(cabi.lib().isplib_sddmm_rows16_auto(n, ldy, int(ordered))) == cabi.sddmm_rows16_native_pays(n, ldy, ordered)
    for k in (6, 8, 10, 63, 64, 1022, 1024, 1026, 2048):
        for ldy, ldg in ((k, k), (k + 1, k), (k, k + 1), (k + 2, k + 4)):
            assert cabi.sddmm_rows16_serves(2000, k, ldy, ldg) == (bool(cabi.lib().isplib_rows16_domain(2000, k, ldy, ldg)) and k <= 1024)
    assert cabi.sddmm_rows16_serves(2000, 1024, 1024, 1024) and not cabi.sddmm_rows16_serves(2000, 1026, 1026, 1026)
    assert not cabi.sddmm_rows16_serves(2000, 64, 65, 64) and not cabi.sddmm_rows16_serves(2000, 64, 64, 65)


def test_header_declarations_match_the_exports():
    from isplib_amd import cabi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "isplib_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|void|const char \*|float)\s+\*?(\w+)\(", header, re.M))
    assert {"isplib_sddmm_csr_rows16_hip", "isplib_sddmm_rows16_auto"} <= declared & set(cabi.EXPORTS)
    assert "static inline int isplib_sddmm_rows16_serves(int64_t n, int64_t k, int64_t ldy, int64_t ldg)" in header
    assert "static inline int isplib_sddmm_rows16_native_pays(int64_t n, int64_t ldy, int ordered)" in header
    assert re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+1\b", header)
    for name in ("isplib_sddmm_csr_rows16_hip", "isplib_sddmm_rows16_auto"):
        getattr(cabi.lib(), name)


def test_wrapper_raises_on_mis_shaped_operands_without_a_device():
    """The shape checks come before anything touches a device: a mis-shaped g or y never reaches the entry."""
    from isplib_amd import cabi
    rowptr, col = (torch.from_numpy(a) for a in cases.random_csr(30, 20, 3.0, 1))
    y, g = torch.zeros((20, 64), dtype=BF), torch.zeros((30, 64), dtype=BF)
    for bad_y, bad_g, err in ((y, g[:-1], ValueError), (y, g[:, :62], ValueError), (y, g.reshape(-1), ValueError), (y.reshape(-1), g, ValueError),
                              (y, g.to(FP), TypeError), (y.to(F32), g.to(F32), TypeError), (y.t().contiguous().t(), g, ValueError),
                              (y, g.t().contiguous().t(), ValueError)):
        with pytest.raises(err):
            cabi.sddmm_rows16(rowptr, col, bad_y, bad_g)
    with pytest.raises(ValueError):                                            # well-shaped, but there is no CPU path
        cabi.sddmm_rows16(rowptr, col, y, g)


def test_inputs_hold_what_the_gpu_tests_are_for(oracle_mod):
    rowptr, col = cs.hub_graph()
    deg = np.diff(rowptr)
    assert rowptr.size - 1 == 300 and col.max() < cs.N
    assert all(deg[r] == 0 for r in (0, 150, 299)) and deg.max() > cs.LONG_ROW and deg[7] == deg.max() == 2500
    assert any(np.any(np.diff(col[rowptr[r]:rowptr[r + 1]]) == 0) for r in range(300)), "duplicate columns"
    # the slot widths: every LPR once whole and once ragged, and the two-chunk form
    assert [cs.slot(k) for k in cs.WIDTHS] == [(8, 1), (8, 1), (8, 1), (16, 1), (16, 1), (32, 1), (32, 1), (64, 1), (64, 1), (64, 2), (64, 2), (64, 2)]
    assert [cs.slot(k) for k in cs.LENGTH_WIDTHS] == [(8, 1), (32, 1), (64, 2)]
    # the degree list names every loop edge of this kernel: G = 64 / LPR edges per gather, U = 4 gathers per step
    lengths = set(cs.length_degrees())
    want = {0, 1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 6144}
    for g in (8, 2, 1):
        want |= {g - 1, g, g + 1, g * cs.U - 1, g * cs.U, g * cs.U + 1}
    assert cs.U == 4 and want <= lengths
    rp2, col2 = cs.length_graph()
    assert sorted(set(np.diff(rp2).tolist())) == sorted(lengths) and col2.max() < cs.N
    source = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "isplib_amd", "csrc", "sddmm_rows16.hip")).read()
    assert re.search(r"constexpr int SDDMM16_U = 4;", source) and re.search(r"a\.long_row = 2048;", source)
    # the integer cases: |x| <= 3, so |dot| <= 9 * 1024 < 2^24 -- exact in fp32 in any order
    for k in cs.WIDTHS:
        assert np.abs(cases.dense(cs.N, k, 3, "integer")).max() <= 3 and np.abs(cases.dense(300, k, 5, "integer")).max() <= 3
    assert 9 * max(cs.WIDTHS) < 2 ** 24
    # the Inf case's columns are exactly the ones the shifted vector of k = 66 gathers twice
    assert cs.duplicated_columns(66) == [58, 59, 60, 61, 62, 63] and cs.duplicated_columns(64) == [] and cs.duplicated_columns(1022) == [1014, 1015]
    y, g = cs.ragged_trap(300)
    assert sorted(set(np.nonzero(np.isinf(y))[1].tolist())) == cs.duplicated_columns(66)
    hot = np.isinf(y).any(1)
    assert hot.any() and not hot.all() and np.any(y[hot, 58] > 0) and np.any(y[hot, 58] < 0)
    assert np.all(np.isfinite(g)) and np.all(g[:, cs.duplicated_columns(66)] > 0)
    assert np.all(np.isfinite(np.delete(y, cs.duplicated_columns(66), axis=1)))
    ref = oracle_mod.sddmm(rowptr, col, y, g)
    assert np.array_equal(np.isinf(ref), hot[col]) and not np.any(np.isnan(ref)) and np.any(hot[col])
    # the non-finite case: the reference holds NaN, Inf and finite results
    rp3, col3 = cases.random_csr(64, cs.N, 6.0, 41, empty_rows=(5,), hub=(9, 300))
    for k in (64, 66):
        yn = half_ref.widen(half_ref.to16(cases.dense(cs.N, k, 3, "nonfinite"), BF))
        gn = half_ref.widen(half_ref.to16(cases.dense(64, k, 5, "nonfinite"), BF))
        with np.errstate(invalid="ignore"):
            ref = oracle_mod.sddmm(rp3, col3, yn, gn)
        assert np.any(np.isnan(ref)) and np.any(np.isinf(ref)) and np.any(np.isfinite(ref))


@pytest.mark.parametrize("dtype", (BF, FP), ids=("bf16", "fp16"))
@pytest.mark.parametrize("k", (66, 256, 1024))
def test_emulated_summation_order_meets_the_bounds(oracle_mod, k, dtype):
    """The kernel's order of additions in numpy fp32 (8 or 16 products per lane, then a pairwise tree over the slot) against
    oracle.sddmm: real-valued data within 1e-5 * mag, integer data exact and its mean within 1e-6 * mag -- the bounds are met by
    correct code before any GPU run."""
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    y = half_ref.widen(half_ref.to16(cases.dense(cs.N, k, 3, "uniform"), dtype))
    g = half_ref.widen(half_ref.to16(cases.dense(m, k, 5, "uniform"), dtype))
    for mean in (False, True):
        ref = oracle_mod.sddmm(rowptr, col, y, g, mean=mean)
        mag = oracle_mod.sddmm(rowptr, col, np.abs(y), np.abs(g), mean=mean)
        err = np.abs(cs.emulate(rowptr, col, y, g, mean).astype(np.float64) - ref)
        assert np.all(err <= 1e-5 * mag + 1e-30), (k, mean, np.max(err / (1e-5 * mag + 1e-30)))
        assert np.max(err / (mag + 1e-30)) <= 23 * 2.0 ** -24, "the derivation: at most 23 roundings of 2^-24"
    yi = half_ref.widen(half_ref.to16(cases.dense(cs.N, k, 3, "integer"), dtype))
    gi = half_ref.widen(half_ref.to16(cases.dense(m, k, 5, "integer"), dtype))
    assert np.array_equal(cs.emulate(rowptr, col, yi, gi), oracle_mod.sddmm(rowptr, col, yi, gi))
    magi = oracle_mod.sddmm(rowptr, col, np.abs(yi), np.abs(gi), mean=True)
    assert np.all(np.abs(cs.emulate(rowptr, col, yi, gi, True).astype(np.float64) - oracle_mod.sddmm(rowptr, col, yi, gi, mean=True)) <= 1e-6 * magi + 1e-30)


@pytest.mark.parametrize("k", (66, 256))
def test_emulated_subnormal_products_meet_the_bound(oracle_mod, k):
    """bf16 operands of magnitude ~1e-20: the products are fp32 subnormals, nothing is flushed, and the emulated order stays within
    1e-5 * mag + k * 2^-149 of the oracle."""
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    y, g = cs.subnormal_operands(m, k)
    y, g = half_ref.widen(half_ref.to16(y, BF)), half_ref.widen(half_ref.to16(g, BF))
    ref = oracle_mod.sddmm(rowptr, col, y, g)
    assert np.any((ref != 0) & (np.abs(ref) < np.float32(2.0 ** -126))) and np.count_nonzero(ref) > ref.size // 2
    mag = oracle_mod.sddmm(rowptr, col, np.abs(y), np.abs(g)).astype(np.float64)
    err = np.abs(cs.emulate(rowptr, col, y, g).astype(np.float64) - ref)
    assert np.all(err <= 1e-5 * mag + k * 2.0 ** -149)
