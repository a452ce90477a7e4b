"""Host side of the 16-bit (bf16 / fp16) SpMM path: the address domain of fusedMM_csr_stream16_hip as cabi.stream16_serves states it,
against a direct statement of the rule at every edge; the reference helper the GPU tests compare with; and the plug-in's choice
between the native kernel and the conversion route as a pure function.  No device."""
import numpy as np
import pytest
import torch

from tests import half_ref


def _rule(n, k, ldy, ldz, nnz):
    """include/isplib_hip.h, isplib_stream16_serves, stated directly."""
    return (n < 2 ** 24 and ldy < 2 ** 22 and n * ldy * 2 <= 0xE0000000 and k >= 4 and nnz < 2 ** 31 and
            k % 2 == 0 and ldy % 2 == 0 and ldz % 2 == 0)


ROW = 2 ** 21                                   # a pitch for the byte-size edge: 0xE0000000 / (2 * 2^21) = 896 rows exactly
EDGES = [
    # (n, k, ldy, ldz, nnz, served)
    (2 ** 24 - 1, 64, 64, 64, 10, True), (2 ** 24, 64, 64, 64, 10, False),
    (256, 64, 2 ** 22 - 2, 64, 10, True), (256, 64, 2 ** 22, 64, 10, False),
    (0xE0000000 // (2 * ROW), 64, ROW, 64, 10, True), (0xE0000000 // (2 * ROW) + 1, 64, ROW, 64, 10, False),
    (100, 2, 2, 2, 10, False), (100, 4, 4, 4, 10, True), (100, 41, 42, 42, 10, False), (100, 64, 64, 64, 10, True),
    (100, 64, 65, 64, 10, False), (100, 64, 66, 65, 10, False), (100, 64, 66, 130, 10, True),
    (100, 64, 64, 64, 2 ** 31 - 1, True), (100, 64, 64, 64, 2 ** 31, False),
]


@pytest.mark.parametrize("n,k,ldy,ldz,nnz,served", EDGES)
def test_stream16_serves_at_every_edge(n, k, ldy, ldz, nnz, served):
    from isplib_amd import cabi
    assert _rule(n, k, ldy, ldz, nnz) == served, "the test's own statement of the rule"
    assert cabi.stream16_serves(n, k, ldy, ldz, nnz) == served


def test_stream16_serves_matches_the_rule_on_a_grid():
    from isplib_amd import cabi
    assert 0xE0000000 == cabi.DENSE_BYTES_MAX
    for n in (1, 97, 2 ** 24 - 1, 2 ** 24):
        for k in (2, 3, 4, 6, 41, 64, 130):
            for ldy in (k, k + 1, k + 2, 2 ** 22 - 2, 2 ** 22):
                for ldz in (k, k + 1):
                    for nnz in (0, 2 ** 31 - 1, 2 ** 31):
                        assert cabi.stream16_serves(n, k, ldy, ldz, nnz) == _rule(n, k, ldy, ldz, nnz), (n, k, ldy, ldz, nnz)


def test_auto_rule_mirror_matches_the_library():
    """cabi.stream16_native_pays restates isplib_stream16_native_pays (the header's measured rule; isplib_stream16_auto exports it)."""
    from isplib_amd import cabi
    for streams in (2, 4, 8):
        for weighted in (False, True):
            assert bool(cabi.lib().isplib_stream16_auto(streams, int(weighted))) == cabi.stream16_native_pays(streams, weighted)


def test_reference_helper_rounds_once_to_nearest_even():
    bf, fp = torch.bfloat16, torch.float16
    got = half_ref.round16(np.array([966.0, 963.0, 962.0, np.nan, np.inf, -np.inf, 1e-40], np.float32), bf).to(torch.float32).numpy()
    assert got[0] == 968.0 and got[1] == 964.0 and got[2] == 960.0              # spacing 4 at 2^9: a tie goes to the even mantissa
    assert np.isnan(got[3]) and got[4] == np.inf and got[5] == -np.inf
    assert got[6] == np.float32(2.0 ** -133)                                     # a bf16 subnormal (their spacing is 2^-133) is kept
    got = half_ref.round16(np.array([70000.0, -70000.0, 65504.0, np.nan, 2049.0, 2051.0], np.float32), fp).to(torch.float32).numpy()
    assert got[0] == np.inf and got[1] == -np.inf and got[2] == 65504.0 and np.isnan(got[3])
    assert got[4] == 2048.0 and got[5] == 2052.0                                 # ties to even at spacing 2


def test_reference_is_the_oracle_on_the_widened_operand(oracle_mod):
    rowptr = np.array([0, 2, 2, 3], np.int64)
    col = np.array([0, 1, 1], np.int64)
    val = np.array([1.0, 1.0, 1.0], np.float32)
    for dtype, a, want in ((torch.bfloat16, 483.0, 968.0), (torch.float16, 35000.0, np.inf)):
        x16 = half_ref.to16(np.array([[a, np.nan], [a, 1.0]], np.float32), dtype)
        ref32, ref16 = half_ref.reference(oracle_mod, rowptr, col, val, x16, "sum")
        got = ref16.to(torch.float32).numpy()
        assert ref32[0, 0] == 2 * float(x16[0, 0]) and got[0, 0] == want        # 966 -> 968 in bf16, 70000 -> Inf in fp16
        assert np.isnan(got[0, 1]) and got[1, 0] == 0.0 and got[2, 1] == 1.0     # NaN kept; the empty row; an exact value


BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32


def test_half_route_is_a_pure_function_of_its_arguments(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import half_route
    for mode in ("auto", "native", "convert"):
        assert half_route(F32, "sum", 64, 64, mode) == "fp32"
        for dtype in (torch.float64, torch.int32, torch.int64):
            with pytest.raises(TypeError):
                half_route(dtype, "sum", 64, 64, mode)
    for dtype in (BF, FP):
        for red in ("sum", "add", "mean"):
            assert half_route(dtype, red, 64, 64, "native") == "native"
            assert half_route(dtype, red, 64, 64, "convert") == "convert"
            assert half_route(dtype, red, 64, 64, "native", streams=None) == "convert"      # no stream plan for the call
            for streams in (2, 4, 8):
                for weighted in (False, True):
                    want = "native" if cabi.stream16_native_pays(streams, weighted) else "convert"
                    assert half_route(dtype, red, 64, 64, "auto", streams, weighted) == want
        for red in ("max", "min"):
            assert half_route(dtype, red, 64, 64, "native") == "convert"
        # outside the domain: never an error, whatever the mode
        assert half_route(dtype, "sum", 41, 41, "native") == "convert"          # odd k
        assert half_route(dtype, "sum", 2, 2, "native") == "convert"            # narrow k
        assert half_route(dtype, "sum", 64, 65, "native") == "native"           # an odd pitch: the packed copy is served
        assert half_route(dtype, "sum", 64, 192, "native") == "native"          # a column view keeps its pitch
        assert half_route(dtype, "sum", 64, 64, "native", n=2 ** 24) == "convert"
        assert half_route(dtype, "sum", 64, 64, "native", nnz=2 ** 31) == "convert"
    # the mode comes from ISPLIB_HALF when it is not given; unset means auto
    monkeypatch.setenv("ISPLIB_HALF", "native")
    assert half_route(BF, "sum", 64, 64) == "native"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert half_route(BF, "sum", 64, 64) == "convert"
    monkeypatch.delenv("ISPLIB_HALF")
    assert half_route(BF, "sum", 64, 64) == half_route(BF, "sum", 64, 64, "auto")
