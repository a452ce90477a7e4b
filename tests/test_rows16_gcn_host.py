"""Host side of the 16-bit row kernel with an epilogue (fusedMM_csr_rows16_epilogue_hip) and of the fused GCN layer that runs on it
(gcn_norm_matmul under ISPLIB_HALF_GCN): the plug-in's choice as a pure function, the measured rule's mirror, the numpy emulation of the
epilogue's order that gives the expected bits of the GPU tests' integer cases, and a census of those tests' inputs.  No device."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests import rows16_gcn_cases as gc

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
BIG = 2_449_029                                # the ogbn-products shape


def test_rows16_gcn_route_is_pure_and_total(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import rows16_gcn_route as route
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_GCN", raising=False)
    for dtype in (BF, FP):
        assert route(dtype, 64, 64, 2000, False, "native") == "rows16"
        assert route(dtype, 64, 64, 2000, False, "convert") == "convert"
        assert route(dtype, 64, 64, 2000, False, "nonsense") == "convert"
        for n, k in ((2000, 64), (232_965, 32), (232_965, 48), (BIG, 128), (BIG, 256)):
            for ordered in (False, True):
                want = "rows16" if cabi.rows16_gcn_native_pays(n, k, ordered) else "convert"
                assert route(dtype, k, k, n, ordered, "auto") == want
                assert route(dtype, k, k, n, ordered, "native") == "rows16"
        # the domain's edges: never an error, whatever the mode
        for mode in ("auto", "native", "convert"):
            assert route(dtype, 41, 41, 2000, False, mode) == "convert"             # odd k
            assert route(dtype, 6, 6, 2000, False, mode) == "convert"               # narrow k
            assert route(dtype, 2 ** 24, 2 ** 24, 1, False, mode) == "convert"
            assert route(dtype, 64, 64, 0xE0000000 // 128 + 1, False, mode) == "convert"
        assert route(dtype, 8, 8, 2000, False, "native") == "rows16"
        assert route(dtype, 64, 65, 2000, False, "native") == "rows16"              # an odd pitch: packed
        assert route(dtype, 64, 192, 2000, False, "native") == "rows16"             # a column view, as it lies
        assert route(dtype, 64, 64, 0xE0000000 // 128, False, "native") == "rows16"  # X at the descriptor's limit
    for mode in ("auto", "native", "convert"):
        assert route(F32, 64, 64, 2000, False, mode) == "convert"                   # consulted for 16-bit features only
        assert route(torch.float64, 64, 64, 2000, True, mode) == "convert"
    # the mode comes from ISPLIB_HALF_GCN when it is not given; unset counts as convert, and ISPLIB_HALF=convert wins
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_GCN", "native")
    assert route(BF, 64, 64, 2000) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "native")
    assert route(BF, 64, 64, 2000) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF", "auto")
    assert route(BF, 64, 64, 2000) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF_GCN", "auto")
    assert route(BF, 64, 64, 2000) == route(BF, 64, 64, 2000, False, "auto")
    assert route(BF, 128, 128, BIG, True) == route(BF, 128, 128, BIG, True, "auto")
    monkeypatch.setenv("ISPLIB_HALF_GCN", "convert")
    assert route(BF, 64, 64, 2000) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_GCN", "nonsense")
    assert route(BF, 64, 64, 2000) == "convert"


def test_auto_rule_mirror_matches_the_library():
    """cabi.rows16_gcn_native_pays restates isplib_rows16_gcn_native_pays (isplib_rows16_gcn_auto exports it)."""
    from isplib_amd import cabi
    for n, ldy in ((0, 64), (1000, 64), (50_000, 64), (232_965, 32), (232_965, 48), (612_000, 128), (BIG, 128), (BIG, 256), (2 ** 20, 128),
                   (2 ** 20 + 1, 128)):
        for ordered in (False, True):
            assert bool(cabi.lib().isplib_rows16_gcn_auto(n, ldy, int(ordered))) == cabi.rows16_gcn_native_pays(n, ldy, ordered)


def test_header_declarations_match_the_exports():
    import os
    import re
    from isplib_amd import cabi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "isplib_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|void|const char \*|float)\s+\*?(\w+)\(", header, re.M))
    names = {"fusedMM_csr_rows16_epilogue_hip", "isplib_rows16_gcn_auto", "isplib_masked_colsum16_hip", "isplib_masked_colsum16_workspace_bytes"}
    assert names <= declared & set(cabi.EXPORTS)
    assert "static inline int isplib_rows16_gcn_native_pays(int64_t n, int64_t ldy, int ordered)" in header
    assert "} isplib_epilogue16;" in header
    for name in names:
        getattr(cabi.lib(), name)
    # the struct the wrapper hands over has the header's members in the header's order
    assert [f[0] for f in cabi.Epilogue16._fields_] == re.findall(r"^\s+(?:const float \*|int\s+)(\w+);", header[header.index("typedef struct isplib_epilogue16"):header.index("} isplib_epilogue16;")], re.M)


def test_unset_variable_keeps_the_refusal():
    """gcn_norm_matmul reads ISPLIB_HALF_GCN before anything else: unset, a 16-bit operand is refused with the text it always had
    (a host tensor here: the device check comes first either way)."""
    import isplib_amd
    with pytest.raises(RuntimeError, match="needs a float32 GPU matrix"):
        isplib_amd.gcn_norm_matmul(None, torch.zeros((4, 8), dtype=BF))


@pytest.mark.parametrize("dtype", (BF, FP), ids=("bf16", "fp16"))
@pytest.mark.parametrize("act", (False, True), ids=("linear", "relu"))
def test_emulation_of_the_epilogue_order_gives_the_formula_on_integer_data(oracle_mod, act, dtype):
    """The kernel's order -- the fp32 sum, one fma with the self row, * rs_i, + bias, v > 0 ? v : 0, every step rounded to fp32 -- on
    the GPU tests' integer cases: every intermediate is an integer or a half-integer below 2^24, so the emulation IS the fp64 formula,
    and round16 of it is the expected output of tests/test_gpu_rows16_gcn.py's integer test, bit for bit."""
    for rowptr, col in (gc.hub_graph(), gc.length_graph()):
        m = rowptr.size - 1
        for k in (10, 64):
            x16 = half_ref.to16(cases.dense(m, k, 3, "integer"), dtype)
            x32 = half_ref.widen(x16)
            assert np.array_equal(x32, cases.dense(m, k, 3, "integer")), "small integers are exact in 16 bits"
            for which in gc.MEMBER_SETS:
                mem = gc.integer_members(which, m, k)
                w = np.ones(col.size, np.float32) if mem["col_scale"] is None else mem["col_scale"][col]
                agg32, _ = oracle_mod.spmm_fw(rowptr, col, w, x32, "sum")
                emu = gc.epilogue_emulation(agg32, x32, mem["self_scale"], mem["row_scale"], mem["bias"], act)
                ref, mag = gc.formula64(rowptr, col, x32, mem["col_scale"], mem["self_scale"], mem["row_scale"], mem["bias"], act)
                assert emu.dtype == np.float32 and np.array_equal(emu.astype(np.float64), ref), which
                assert mag.max() < 2 ** 24 and np.array_equal(2 * ref, np.round(2 * ref)), which
                assert np.array_equal(half_ref.bits(half_ref.round16(emu, dtype)), half_ref.bits(half_ref.round16(ref, dtype)))


def test_relu_emulation_is_the_fp32_epilogues():
    """v > 0 ? v : 0: -0.0, NaN and -Inf give +0.0, +Inf stays."""
    v = np.array([-0.0, 0.0, np.nan, -np.inf, np.inf, -1.5, 2.5], np.float32)
    r = gc.relu(v)
    assert r.dtype == np.float32 and np.array_equal(r.view(np.uint32), np.array([0, 0, 0, 0, np.inf, 0, 2.5], np.float32).view(np.uint32))


def test_inputs_hold_what_the_gpu_tests_are_for():
    rowptr, col = gc.hub_graph()
    deg = np.diff(rowptr)
    assert rowptr.size - 1 == gc.N_HUB == 300 and col.max() < gc.N_HUB, "square"
    assert all(deg[r] == 0 for r in (0, 150, 299)) and deg.max() > gc.LONG_ROW and deg[7] == deg.max() == 2500
    assert any(np.any(np.diff(col[rowptr[r]:rowptr[r + 1]]) == 0) for r in range(300)), "duplicate columns"
    # the length graph: every length of test_gpu_rows16._edge_degrees() twice, square
    from tests.test_gpu_rows16 import _edge_degrees
    lengths = _edge_degrees()
    rp2, col2 = gc.length_graph()
    assert sorted(np.diff(rp2).tolist()) == sorted(lengths + lengths) and col2.max() < rp2.size - 1
    assert {0, 1, 63, 64, 65, gc.LONG_ROW, gc.LONG_ROW + 1, 3 * gc.LONG_ROW} <= set(lengths)
    # the integer cases: exact sums (the longest row, every factor at its largest, the self term, the row scale, the bias)
    longest = max(deg.max(), max(lengths))
    assert (longest * 5 * 3 + 5 * 3) * 2 + 3 < 2 ** 24
    for m in (300, len(lengths) * 2):
        mem = gc.integer_members("all", m, 64)
        assert np.abs(mem["col_scale"]).max() <= 5 and np.abs(mem["self_scale"]).max() <= 5 and np.abs(mem["bias"]).max() <= 3
        assert set(np.abs(mem["row_scale"]).tolist()) <= {0.5, 1.0, 2.0} and np.any(mem["row_scale"] < 0)
        assert all(np.array_equal(v, np.round(v)) for key, v in mem.items() if key != "row_scale")
    for which in gc.MEMBER_SETS[1:]:
        mem = gc.integer_members(which, 300, 64)
        assert [key for key, v in mem.items() if v is None] == [which[3:]]
    # the special-value cases of the GPU test hold NaN and Inf results without ReLU, for every place the special values go
    n, k = 97, 66
    rp3, col3 = cases.random_csr(n, n, 3.0, 41, empty_rows=(5,))
    for where in ("operand", "col_scale", "self_scale", "row_scale", "bias"):
        x32 = half_ref.widen(half_ref.to16(cases.dense(n, k, 3, "nonfinite" if where == "operand" else "uniform"), BF))
        mem = {"col_scale": gc.scale_table(n), "self_scale": gc.scale_table(n, 61), "row_scale": gc.scale_table(n, 67), "bias": gc.real_bias(k)}
        if where != "operand":
            mem[where] = gc.special_scale("nonfinite", k if where == "bias" else n)
        ref, _ = gc.formula64(rp3, col3, x32, mem["col_scale"], mem["self_scale"], mem["row_scale"], mem["bias"], False)
        assert np.any(np.isnan(ref)) and np.any(np.isinf(ref)), where
