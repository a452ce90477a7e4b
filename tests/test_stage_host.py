"""Staged column panels of the stream schedule, host side (no GPU): the rule isplib_stream_stage_panel of include/isplib_hip.h
over a table of calls, and what isplib_spmm_stream_workspace_bytes reserves for the copy."""
import ctypes

import pytest

from tests import stage_rule
from tests.stage_rule import AUTO, FORCE, OFF

PITCH = stage_rule.header_constant("STREAM_STAGE_PITCH")
BYTES_MAX = stage_rule.header_constant("STREAM_STAGE_BYTES_MAX")
MIN_DEGREE = stage_rule.header_constant("STREAM_STAGE_MIN_DEGREE")


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    return stage_rule.compile_rule(tmp_path_factory.mktemp("stage_rule"))


def test_the_constants_are_what_the_layout_needs():
    assert PITCH == 512 and BYTES_MAX == 1 << 30 and MIN_DEGREE >= 1


def test_rule_table(rule):
    n = 232965
    big, room = n * MIN_DEGREE, n * PITCH                       # a launch large enough; exactly enough room
    base = 0x7F0000000000                                       # 512-byte aligned
    # (address of y, ldy, c0, k, streams, n, nnz, room, mode) -> staged
    table = [
        # the headline: contiguous K = 128, panel 0 on bytes 0..255 of every 512 (fast), panel 1 on bytes 256..511 (slow)
        ((base, 128, 0, 128, 4, n, big, room, AUTO), False),
        ((base, 128, 64, 128, 4, n, big, room, AUTO), True),
        # the address decides, not the column: the same operand as columns 64..191 of a 256-wide tensor
        ((base + 256, 256, 0, 128, 4, n, big, room, AUTO), True),
        ((base + 256, 256, 64, 128, 4, n, big, room, AUTO), False),
        # K = 256 at ldy = 256 (1024-byte rows: bit 9 is the panel's own): panel 1 has the lines with bits [9:7] = 011 in every
        # row; panel 3 (bytes 768..1023: 110, 111) has none -- but it has them in every other row at a 1536-byte pitch
        ((base, 256, 0, 256, 4, n, big, room, AUTO), False), ((base, 256, 64, 256, 4, n, big, room, AUTO), True),
        ((base, 256, 128, 256, 4, n, big, room, AUTO), False), ((base, 256, 192, 256, 4, n, big, room, AUTO), False),
        ((base, 256, 192, 256, 4, n, big, room, FORCE), True), ((base, 384, 192, 256, 4, n, big, room, AUTO), True),
        ((base + 512, 128, 64, 128, 4, n, big, room, AUTO), True), ((base + 512, 256, 64, 128, 4, n, big, room, AUTO), False),
        # off: never; force: every eligible panel, whatever its class and the launch's size
        ((base, 128, 64, 128, 4, n, big, room, OFF), False),
        ((base, 128, 0, 128, 4, n, 1, room, FORCE), True), ((base, 128, 64, 128, 4, n, 1, room, FORCE), True),
        # the threshold of auto: nnz / n
        ((base, 128, 64, 128, 4, n, big - 1, room, AUTO), False),
        # partial panels: the 4-column sliver of K = 132, the 8 columns of K = 200 -- never, not even forced
        ((base, 256, 128, 132, 4, n, big, room, FORCE), False), ((base, 256, 64, 132, 4, n, big, room, FORCE), True),
        ((base, 256, 192, 200, 4, n, big, room, FORCE), False), ((base, 256, 128, 200, 4, n, big, room, FORCE), True),
        ((base, 128, 0, 48, 4, n, big, room, FORCE), False),
        # row pitch not a multiple of 512 bytes (ldy = 160, 132); a panel that does not start on a 256-byte boundary
        ((base, 160, 64, 128, 4, n, big, room, FORCE), False), ((base, 132, 64, 132, 4, n, big, room, FORCE), False),
        ((base + 128, 128, 64, 128, 4, n, big, room, FORCE), False), ((base + 16, 128, 0, 128, 4, n, big, room, FORCE), False),
        ((base, 128, 32, 128, 4, n, big, room, FORCE), False),
        # other slot widths: the 128-column geometry gathers all four lines in one pass; 32-column slots are not staged
        ((base, 128, 64, 128, 2, n, big, room, FORCE), False), ((base, 128, 64, 128, 8, n, big, room, FORCE), False),
        # room: one byte short; none; an operand whose copy would pass the cap
        ((base, 128, 64, 128, 4, n, big, room - 1, FORCE), False), ((base, 128, 64, 128, 4, n, big, 0, AUTO), False),
        ((base, 128, 64, 128, 4, BYTES_MAX // PITCH, 1 << 40, 1 << 40, FORCE), True),
        ((base, 128, 64, 128, 4, BYTES_MAX // PITCH + 1, 1 << 40, 1 << 40, FORCE), False),
        # degenerate
        ((base, 128, 64, 128, 4, 0, 0, room, FORCE), False), ((base, 128, -64, 128, 4, n, big, room, FORCE), False),
    ]
    for args, want in table:
        assert rule(*args) == want, args


def _plan_struct(cols, streams, n_parts):
    from isplib_amd import cabi
    s = cabi.StreamPlanStruct()
    s.rows, s.cols, s.streams, s.n_parts = cols, cols, streams, n_parts
    return s


def test_workspace_bytes_by_slot_width():
    """4-stream plans (the 64-column slots of sum / mean) get cols * 512 + 512 bytes behind the partial rows, up to 1 GiB; the
    other slot widths, max / min and a null plan are what they were."""
    from isplib_amd import cabi
    L = cabi.lib()
    L.isplib_spmm_stream_workspace_bytes.restype = ctypes.c_size_t
    L.isplib_spmm_stream_minmax_workspace_bytes.restype = ctypes.c_size_t
    new = lambda s: int(L.isplib_spmm_stream_workspace_bytes(ctypes.byref(s)))  # noqa: E731
    for cols, n_parts in ((3000, 0), (3000, 7), (232965, 301)):
        for streams in (2, 4, 8):
            old = stage_rule.old_workspace_bytes(n_parts, streams)
            assert new(_plan_struct(cols, streams, n_parts)) == old + (cols * PITCH + PITCH if streams == 4 else 0), (cols, n_parts, streams)
            assert int(L.isplib_spmm_stream_minmax_workspace_bytes(ctypes.byref(_plan_struct(cols, streams, n_parts)))) == 2 * old
    last = (BYTES_MAX - PITCH) // PITCH                           # the largest operand whose area is at most 1 GiB
    assert new(_plan_struct(last, 4, 5)) == stage_rule.old_workspace_bytes(5, 4) + BYTES_MAX
    assert new(_plan_struct(last + 1, 4, 5)) == stage_rule.old_workspace_bytes(5, 4)
    assert int(L.isplib_spmm_stream_workspace_bytes(None)) == 256


def test_workspace_never_shrinks():
    from isplib_amd import cabi
    L = cabi.lib()
    L.isplib_spmm_stream_workspace_bytes.restype = ctypes.c_size_t
    for cols in (1, 97, 4096, 1 << 21, (1 << 24) - 1):
        for n_parts in (0, 1, 63, 100000):
            for streams in (2, 4, 8):
                assert int(L.isplib_spmm_stream_workspace_bytes(ctypes.byref(_plan_struct(cols, streams, n_parts)))) >= stage_rule.old_workspace_bytes(n_parts, streams)


def test_a_staged_copy_fits_the_area_wherever_the_workspace_starts(rule):
    """The entry starts the copy at the first 512-byte boundary behind the partial rows: for a 256-byte aligned workspace of the
    advertised size that leaves at least n * 512 bytes."""
    n = 3001
    for n_parts in (0, 5):
        parts = stage_rule.old_workspace_bytes(n_parts, 4)
        total = parts + n * PITCH + PITCH
        for start in (0x10000, 0x10100):
            lo = (start + parts + PITCH - 1) & ~(PITCH - 1)
            assert rule(0x7F0000000000, 128, 64, 128, 4, n, n * MIN_DEGREE, start + total - lo, AUTO)
