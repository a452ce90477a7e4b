"""Host side of the 16-bit row kernel (fusedMM_csr_rows16_hip): its address domain as cabi.rows16_serves states it, against the
header's own isplib_rows16_serves (exported as isplib_rows16_domain) and a direct statement of the rule at every edge; the measured
rule's mirror; the plug-in's choice between the kernel and the conversion route as a pure function; and the row-order threshold in
bytes.  No device."""
import pytest
import torch

BF, FP, F32 = torch.bfloat16, torch.float16, torch.float32


def _rule(n, k, ldy, ldz):
    """include/isplib_hip.h, isplib_rows16_serves, stated directly."""
    return 8 <= k < 2 ** 24 and k % 2 == 0 and ldy % 2 == 0 and ldz % 2 == 0 and n * ldy * 2 <= 0xE0000000 and n < 2 ** 31


ROW = 2 ** 21                                   # a pitch for the byte-size edge: 0xE0000000 / (2 * 2^21) = 896 rows exactly
EDGES = [
    # (n, k, ldy, ldz, served)
    (100, 6, 6, 6, False), (100, 8, 8, 8, True), (100, 9, 10, 10, False), (100, 10, 10, 10, True),
    (100, 64, 65, 64, False), (100, 64, 66, 65, False), (100, 64, 66, 130, True),
    (0xE0000000 // (2 * ROW), 64, ROW, 64, True), (0xE0000000 // (2 * ROW) + 1, 64, ROW, 64, False),
    (0xE0000000 // 128, 64, 64, 64, True), (0xE0000000 // 128 + 1, 64, 64, 64, False),
    (2 ** 31 - 1, 8, 0, 8, True), (2 ** 31, 8, 0, 8, False),
    (1, 2 ** 24 - 2, 2 ** 24 - 2, 2 ** 24 - 2, True), (1, 2 ** 24, 2 ** 24, 2 ** 24, False),
]


@pytest.mark.parametrize("n,k,ldy,ldz,served", EDGES)
def test_rows16_serves_at_every_edge(n, k, ldy, ldz, served):
    from isplib_amd import cabi
    assert _rule(n, k, ldy, ldz) == served, "the test's own statement of the rule"
    assert cabi.rows16_serves(n, k, ldy, ldz) == served
    assert bool(cabi.lib().isplib_rows16_domain(n, k, ldy, ldz)) == served


def test_rows16_serves_matches_the_header_on_a_grid():
    from isplib_amd import cabi
    L = cabi.lib()
    assert 0xE0000000 == cabi.DENSE_BYTES_MAX
    for n in (0, 1, 97, 0xE0000000 // 128, 0xE0000000 // 128 + 1, 2 ** 31 - 1, 2 ** 31):
        for k in (0, 2, 6, 7, 8, 9, 10, 41, 64, 130, 2 ** 24 - 2, 2 ** 24):
            for ldy in (k, k + 1, k + 2, 2 ** 22):
                for ldz in (k, k + 1):
                    got = cabi.rows16_serves(n, k, ldy, ldz)
                    assert got == _rule(n, k, ldy, ldz) == bool(L.isplib_rows16_domain(n, k, ldy, ldz)), (n, k, ldy, ldz)


def test_auto_rule_mirror_matches_the_library():
    """cabi.rows16_native_pays restates isplib_rows16_native_pays (the header's measured rule; isplib_rows16_auto exports it)."""
    from isplib_amd import cabi
    for n, ldy in ((1000, 64), (2_449_029, 128), (2_449_029, 256), (2 ** 20, 128), (2 ** 20 + 1, 128)):
        for ordered in (False, True):
            for weighted in (False, True):
                assert bool(cabi.lib().isplib_rows16_auto(n, ldy, int(ordered), int(weighted))) == cabi.rows16_native_pays(n, ldy, ordered, weighted)


def test_rows16_route_is_a_pure_function_of_its_arguments(monkeypatch):
    from isplib_amd import cabi
    from isplib_amd.plugin import rows16_route
    big = 2_449_029                                # the ogbn-products shape: 1.25 GB of bf16 at k = 256
    for dtype in (BF, FP):
        for red in ("sum", "add", "mean"):
            assert rows16_route(dtype, red, 64, 64, "native") == "rows16"
            assert rows16_route(dtype, red, 64, 64, "convert") == "convert"
            for n, k in ((2000, 64), (big, 128), (big, 256)):
                for ordered in (False, True):
                    for weighted in (False, True):
                        want = "rows16" if cabi.rows16_native_pays(n, k, ordered, weighted) else "convert"
                        assert rows16_route(dtype, red, k, k, "auto", n, ordered, weighted) == want
                        assert rows16_route(dtype, red, k, k, "native", n, ordered, weighted) == "rows16"
        for red in ("max", "min"):
            assert rows16_route(dtype, red, 64, 64, "native") == "convert"
        # outside the domain: never an error, whatever the mode
        for mode in ("auto", "native", "convert"):
            assert rows16_route(dtype, "sum", 41, 41, mode) == "convert"        # odd k
            assert rows16_route(dtype, "sum", 6, 6, mode) == "convert"          # narrow k
        assert rows16_route(dtype, "sum", 64, 65, "native") == "rows16"         # an odd pitch: served only packed
        assert rows16_route(dtype, "sum", 64, 192, "native") == "rows16"        # a column view keeps its pitch
        assert rows16_route(dtype, "sum", 64, 64, "native", n=0xE0000000 // 128 + 1) == "convert"
        # a pitch too wide for the descriptor, the packed operand inside it
        assert rows16_route(dtype, "sum", 64, 192, "native", n=0xE0000000 // 128) == "rows16"
    for mode in ("auto", "native", "convert"):
        assert rows16_route(F32, "sum", 64, 64, mode) == "convert"              # consulted for 16-bit features only
    # the mode comes from ISPLIB_HALF when it is not given; unset means auto
    monkeypatch.setenv("ISPLIB_HALF", "native")
    assert rows16_route(BF, "sum", 64, 64) == "rows16"
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert rows16_route(BF, "sum", 64, 64) == "convert"
    monkeypatch.delenv("ISPLIB_HALF")
    assert rows16_route(BF, "sum", 64, 64) == rows16_route(BF, "sum", 64, 64, "auto")


def test_half_route_is_unchanged():
    """What tests/test_half_host.py pins: without a stream plan half_route says "convert" -- the row kernel is a second question."""
    from isplib_amd.plugin import half_route
    for dtype in (BF, FP):
        for mode in ("auto", "native", "convert"):
            assert half_route(dtype, "sum", 64, 64, mode, streams=None) == "convert"
        assert half_route(dtype, "sum", 64, 64, "native") == "native"
        assert half_route(dtype, "max", 64, 64, "native") == "convert"
    assert half_route(F32, "sum", 64, 64, "native") == "fp32"


def test_row_order_threshold_is_on_bytes(monkeypatch):
    """SparseStorage.row_order judges the operand at its own element size: 1.5 M rows of 64 columns are 384 MB in fp32 (beyond the
    Infinity Cache: an order is looked for) and 192 MB in bf16 (inside it: declined without looking)."""
    from isplib_amd import reorder
    from isplib_amd.sparse import SparseStorage
    looked = []
    monkeypatch.setattr(reorder, "useful_order", lambda rp, cl: looked.append(1) or None)
    monkeypatch.delenv("ISPLIB_REORDER", raising=False)
    n, k = 1_500_000, 64
    s = SparseStorage.__new__(SparseStorage)
    s._sparse_sizes = (n, n)
    s._rowptr = torch.zeros(2, dtype=torch.int64)
    s._col = torch.zeros(1, dtype=torch.int64)
    assert n * k * 2 <= (256 << 20) < n * k * 4
    assert s.row_order(False, k, itemsize=2) == [] and not looked
    assert s.row_order(False, k) == [] and looked == [1]                        # the default is fp32's: it looked (and found none)
    assert s.row_order(False, k, itemsize=4) == [] and looked == [1]            # remembered per side
