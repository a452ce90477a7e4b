"""Host side of the column-scaled 16-bit row kernel (fusedMM_csr_rows16_colscale_hip) and of the unit-weight mean backward that runs
on it: the plug-in's choice as a pure function, the measured rule's mirror, the fact about 1 / deg the bit equality with the weighted
mean backward rests on, and a census of the GPU tests' inputs.  No device."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests import rows16_colscale_cases as cs

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
BIG = 2_449_029                                # the ogbn-products shape


def test_rows16_mean_bw_route_is_pure_and_total(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import rows16_mean_bw_route as route
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_MEAN_BW", raising=False)
    for dtype in (BF, FP):
        assert route(dtype, 64, 2000, False, "native") == "rows16"
        assert route(dtype, 64, 2000, False, "convert") == "convert"
        assert route(dtype, 64, 2000, False, "nonsense") == "convert"
        for n, k in ((2000, 64), (BIG, 128), (BIG, 256)):
            for ordered in (False, True):
                want = "rows16" if cabi.rows16_colscale_native_pays(n, k, ordered) else "convert"
                assert route(dtype, k, n, ordered, "auto") == want
                assert route(dtype, k, n, ordered, "native") == "rows16"
        # the domain's edges: never an error, whatever the mode
        for mode in ("auto", "native", "convert"):
            assert route(dtype, 41, 2000, False, mode) == "convert"             # odd k
            assert route(dtype, 6, 2000, False, mode) == "convert"              # narrow k
            assert route(dtype, 2 ** 24, 1, False, mode) == "convert"
            assert route(dtype, 64, 0xE0000000 // 128 + 1, False, mode) == "convert"
        assert route(dtype, 8, 2000, False, "native") == "rows16"
        assert route(dtype, 2 ** 24 - 2, 1, False, "native") == "rows16"
        assert route(dtype, 64, 0xE0000000 // 128, False, "native") == "rows16"  # dY at the descriptor's limit
        assert route(dtype, 64, 0, True, "native") == "rows16"
    for mode in ("auto", "native", "convert"):
        assert route(F32, 64, 2000, False, mode) == "convert"                   # consulted for 16-bit features only
        assert route(torch.float64, 64, 2000, True, mode) == "convert"
    # the mode comes from ISPLIB_HALF_MEAN_BW when it is not given; unset means convert, and ISPLIB_HALF=convert wins
    assert route(BF, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_MEAN_BW", "native")
    assert route(BF, 64, 2000) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "native")
    assert route(BF, 64, 2000) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF", "auto")
    assert route(BF, 64, 2000) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF_MEAN_BW", "auto")
    assert route(BF, 64, 2000) == route(BF, 64, 2000, False, "auto")
    assert route(BF, 128, BIG, True) == route(BF, 128, BIG, True, "auto")
    monkeypatch.setenv("ISPLIB_HALF_MEAN_BW", "convert")
    assert route(BF, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_MEAN_BW", "nonsense")
    assert route(BF, 64, 2000) == "convert"


def test_auto_rule_mirror_matches_the_library():
    """cabi.rows16_colscale_native_pays restates isplib_rows16_colscale_native_pays (isplib_rows16_colscale_auto exports it)."""
    from isplib_amd import cabi
    for n, ldy in ((0, 64), (1000, 64), (50_000, 64), (612_000, 128), (BIG, 128), (BIG, 256), (2 ** 20, 128), (2 ** 20 + 1, 128)):
        for ordered in (False, True):
            assert bool(cabi.lib().isplib_rows16_colscale_auto(n, ldy, int(ordered))) == cabi.rows16_colscale_native_pays(n, ldy, ordered)


def test_header_declarations_match_the_exports():
    import os
    import re
    from isplib_amd import cabi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "isplib_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|void|const char \*|float)\s+\*?(\w+)\(", header, re.M))
    assert {"fusedMM_csr_rows16_colscale_hip", "isplib_rows16_colscale_auto"} <= declared & set(cabi.EXPORTS)
    assert "static inline int isplib_rows16_colscale_native_pays(int64_t n, int64_t ldy, int ordered)" in header
    assert re.search(r"#define\s+ISPLIB_HIP_ABI_VERSION\s+1\b", header)
    for name in ("fusedMM_csr_rows16_colscale_hip", "isplib_rows16_colscale_auto"):
        getattr(cabi.lib(), name)


def test_inv_rowcount_is_one_fp32_division_by_the_degree():
    """What the equality with the weighted mean backward rests on: that backward multiplies by 1.0f / (float)max(deg, 1) per edge (the
    library's csr2csc with mean_scale on all-ones weights), one correctly rounded fp32 division -- and so is every entry of
    SparseStorage.inv_rowcount(), for every degree up to 100,000.  Degree 0 maps to 1."""
    from isplib_amd.sparse import SparseStorage
    deg = np.arange(0, 100_001, dtype=np.int64)
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(deg)]).astype(np.int64))
    s = SparseStorage(rowptr, torch.empty(0, dtype=torch.int64), None, (deg.size, 1))    # only the degrees are read
    inv = s.inv_rowcount()
    assert inv.dtype == F32 and inv.shape == (deg.size,) and inv is s.inv_rowcount()      # cached
    want = np.float32(1.0) / np.maximum(deg, 1).astype(np.float32)                        # IEEE division, rounded once
    assert want.dtype == np.float32 and np.array_equal(inv.numpy().view(np.uint32), want.view(np.uint32))
    assert inv[0].item() == 1.0 and inv[1].item() == 1.0 and inv[2].item() == 0.5
    for d in (1, 2, 3, 7, 1000, 99_999, 100_000):
        assert (torch.ones((), dtype=F32) / d).view(torch.int32).item() == inv[d].view(torch.int32).item()
    every = torch.ones((), dtype=F32) / torch.arange(1, 100_001, dtype=F32)
    assert torch.equal(every.view(torch.int32), inv[1:].view(torch.int32))
    # and it is NOT what rounding the double quotient twice, or a reciprocal estimate, would give in general: the exact quotient
    # rounded once is the definition
    exact = (1.0 / np.maximum(deg, 1).astype(np.float64)).astype(np.float32)
    assert np.array_equal(want.view(np.uint32), exact.view(np.uint32))


def test_inputs_hold_what_the_gpu_tests_are_for(oracle_mod):
    rowptr, col = cs.hub_graph()
    deg = np.diff(rowptr)
    assert rowptr.size - 1 == 300 and col.max() < cs.N
    assert all(deg[r] == 0 for r in (0, 150, 299)) and deg.max() > cs.LONG_ROW and deg[7] == deg.max()
    assert any(np.any(np.diff(col[rowptr[r]:rowptr[r + 1]]) == 0) for r in range(300)), "duplicate columns"
    # the degree list names every loop edge: G = 64 / LPR slots (k = 64: 8, k = 256: 2), U = 6 gathers per slot and step
    lengths = set(cs.length_degrees())
    want = {0, 1, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 6144}
    for g in (8, 2):
        want |= {g - 1, g, g + 1, g * cs.U - 1, g * cs.U, g * cs.U + 1}
    assert want <= lengths
    rp2, col2 = cs.length_graph()
    assert sorted(set(np.diff(rp2).tolist())) == sorted(lengths) and col2.max() < cs.N
    # the scale table: 1 / deg-like values, negatives, zeros of both signs, one subnormal -- all of them referenced by the graphs
    s = cs.scale_table()
    assert s.dtype == np.float32 and s.size == cs.N
    sub = (s != 0) & (np.abs(s) < np.float32(2.0 ** -126))
    assert np.count_nonzero(sub) == 1 and np.any(s < 0) and np.any((s == 0) & np.signbit(s)) and np.any((s == 0) & ~np.signbit(s))
    assert np.any((s > 0) & (s <= 1))
    for c in (col, col2):
        used = s[c]
        assert np.any(used < 0) and np.any(used == 0) and np.any((used != 0) & (np.abs(used) < np.float32(2.0 ** -126)))
    # integer scales and operands: exact sums
    si = cs.integer_scale()
    assert np.all(si == np.round(si)) and np.abs(si).max() <= 5 and 6144 * 5 * 3 < 2 ** 24
    # the special-value cases: the reference holds NaN and Inf results (nonfinite) and subnormal ones (denormal)
    n, k = 97, 64
    rp3, col3 = cases.random_csr(64, n, 3.0, 41)
    for where in ("scale", "operand"):
        for kind in ("nonfinite", "denormal"):
            scale = cs.special_scale(kind, n) if where == "scale" else cs.scale_table(n)
            x = half_ref.widen(half_ref.to16(cases.dense(n, k, 3, kind if where == "operand" else "uniform"), BF))
            ref, _ = oracle_mod.spmm_fw(rp3, col3, scale[col3], x, "sum")
            if kind == "nonfinite":
                assert np.any(np.isnan(ref)) and np.any(np.isinf(ref)), (where, kind)
            else:
                assert np.any((ref != 0) & (np.abs(ref) < np.float32(2.0 ** -126))), (where, kind)
