"""Host side of the 16-bit max / min row kernel (fusedMM_csr_rows16_minmax_hip): the plug-in's choice as a pure function, the measured
rule's mirror, the rounding facts the bit-equality contract leans on, and a census of the GPU tests' inputs -- the reference alone
must hold the ties, the rows in which nothing wins and the empty rows those tests are for.  No device."""
import numpy as np
import pytest
import torch

from tests import half_ref
from tests import rows16_minmax_cases as mm

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32
BIG = 2_449_029                                # the ogbn-products shape


def test_rows16_minmax_route_is_pure_and_total(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import rows16_minmax_route as route
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_MINMAX", raising=False)
    for dtype in (BF, FP):
        for red in ("max", "min"):
            assert route(dtype, red, 64, 64, "native") == "rows16"
            assert route(dtype, red, 64, 64, "convert") == "convert"
            assert route(dtype, red, 64, 64, "nonsense") == "convert"
            for n, k in ((2000, 64), (BIG, 128), (BIG, 256)):
                for ordered in (False, True):
                    for weighted in (False, True):
                        for want_arg in (False, True):
                            want = "rows16" if cabi.rows16_minmax_native_pays(n, k, ordered, weighted, want_arg) else "convert"
                            assert route(dtype, red, k, k, "auto", n, ordered, weighted, want_arg) == want
                            assert route(dtype, red, k, k, "native", n, ordered, weighted, want_arg) == "rows16"
            # the domain's edges: never an error, whatever the mode
            for mode in ("auto", "native", "convert"):
                assert route(dtype, red, 41, 41, mode) == "convert"             # odd k
                assert route(dtype, red, 6, 6, mode) == "convert"               # narrow k
                assert route(dtype, red, 2 ** 24, 2 ** 24, mode) == "convert"
            assert route(dtype, red, 8, 8, "native") == "rows16"
            assert route(dtype, red, 2 ** 24 - 2, 2 ** 24 - 2, "native") == "rows16"
            assert route(dtype, red, 64, 65, "native") == "rows16"              # an odd pitch: served only packed
            assert route(dtype, red, 64, 192, "native") == "rows16"             # a column view keeps its pitch
            assert route(dtype, red, 64, 64, "native", n=0xE0000000 // 128) == "rows16"
            assert route(dtype, red, 64, 64, "native", n=0xE0000000 // 128 + 1) == "convert"
            assert route(dtype, red, 64, 192, "native", n=0xE0000000 // 128) == "rows16"   # too wide a pitch, the packed operand fits
        for red in ("sum", "add", "mean", "prod"):
            assert route(dtype, red, 64, 64, "native") == "convert"
    for mode in ("auto", "native", "convert"):
        for red in ("max", "min", "sum"):
            assert route(F32, red, 64, 64, mode) == "convert"                   # consulted for 16-bit features only
    # the mode comes from ISPLIB_HALF_MINMAX when it is not given; unset means convert, and ISPLIB_HALF=convert wins
    assert route(BF, "max", 64, 64) == "convert"
    monkeypatch.setenv("ISPLIB_HALF_MINMAX", "native")
    assert route(BF, "max", 64, 64) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert route(BF, "max", 64, 64) == "convert"
    monkeypatch.setenv("ISPLIB_HALF", "native")
    assert route(BF, "max", 64, 64) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF_MINMAX", "auto")
    assert route(BF, "max", 64, 64) == route(BF, "max", 64, 64, "auto")
    monkeypatch.setenv("ISPLIB_HALF_MINMAX", "convert")
    assert route(BF, "max", 64, 64) == "convert"


def test_auto_rule_mirror_matches_the_library():
    """cabi.rows16_minmax_native_pays restates isplib_rows16_minmax_native_pays (isplib_rows16_minmax_auto exports it)."""
    from isplib_amd import cabi
    for n, ldy in ((1000, 64), (BIG, 128), (BIG, 256), (2 ** 20, 128), (2 ** 20 + 1, 128)):
        for ordered in (False, True):
            for weighted in (False, True):
                for want_arg in (False, True):
                    lib = bool(cabi.lib().isplib_rows16_minmax_auto(n, ldy, int(ordered), int(weighted), int(want_arg)))
                    assert lib == cabi.rows16_minmax_native_pays(n, ldy, ordered, weighted, want_arg)


def test_header_declarations_match_the_exports():
    """Every non-static function the header declares is in cabi.EXPORTS and the other way round -- the new entry and its rule's symbol
    included (tests/test_host.py makes the same comparison for the whole header)."""
    import os
    import re
    from isplib_amd import cabi
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "isplib_hip.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|void|const char \*|float)\s+\*?(\w+)\(", header, re.M))
    assert {"fusedMM_csr_rows16_minmax_hip", "isplib_rows16_minmax_auto"} <= declared & set(cabi.EXPORTS)
    assert "static inline int isplib_rows16_minmax_native_pays(int64_t n, int64_t ldy, int ordered, int weighted, int want_arg)" in header
    for name in ("fusedMM_csr_rows16_minmax_hip", "isplib_rows16_minmax_auto"):
        getattr(cabi.lib(), name)


@pytest.mark.parametrize("dtype", (BF, FP), ids=("bf16", "fp16"))
def test_rounding_facts_of_the_contract(dtype):
    """Torch's CPU cast: -+FLT_MAX -> -+Inf in both types, NaN stays NaN, -0 stays -0, +-Inf stay, and widening is exact."""
    f = np.float32
    src = np.array([-mm.FLT_MAX, mm.FLT_MAX, np.nan, -0.0, 0.0, -np.inf, np.inf], f)
    got = half_ref.round16(src, dtype).to(F32).numpy()
    assert got[0] == -np.inf and got[1] == np.inf and np.isnan(got[2])
    assert got[3] == 0 and np.signbit(got[3]) and got[4] == 0 and not np.signbit(got[4])
    assert got[5] == -np.inf and got[6] == np.inf
    every = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)         # all 65,536 patterns
    back = every.to(F32).to(dtype)
    nan = torch.isnan(every)
    assert torch.equal(every.view(torch.int16)[~nan], back.view(torch.int16)[~nan]) and bool(torch.isnan(back[nan]).all())


@pytest.mark.parametrize("red", ("max", "min"))
@pytest.mark.parametrize("name,dtype", tuple(half_ref.DTYPES.items()))
@pytest.mark.parametrize("family", ("slot_cases", "length_cases", "tie_cases"))
def test_inputs_hold_what_the_gpu_tests_are_for(oracle_mod, family, name, dtype, red):
    """Per case of tests 1-3: the reference alone shows a tie (two edges reach the winning value of an element), a non-empty row in
    which nothing wins -- -+FLT_MAX, rounded -+Inf, position nnz -- and an empty row."""
    lose = -np.inf if red == "max" else np.inf
    seen = 0
    for case, rowptr, col, val, x16 in getattr(mm, family)(dtype, red):
        ref32, ref16, arg = mm.reference(oracle_mod, rowptr, col, val, x16, red)
        ties, nothing, empty = mm.census(rowptr, col, val, x16, ref32, arg)
        assert ties >= 1 and nothing.size >= 1 and empty.size >= 1, (case, ties, nothing, empty)
        r16 = ref16.to(F32).numpy()
        none = arg[nothing] == col.size
        assert np.all(r16[nothing][none] == lose) and np.all(np.abs(ref32[nothing][none]) == mm.FLT_MAX), case
        assert np.all(r16[empty] == 0) and np.all(arg[empty] == col.size), case
        seen += 1
    assert seen >= 4
