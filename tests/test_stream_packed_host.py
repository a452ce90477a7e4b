"""The packed word stream of the sum / mean stream plans (include/isplib_hip.h, PACKED WORD STREAM), on the CPU: the numpy mirror of
the format in isplib_amd/plan.py -- stream_pack_words, what the library's packing pass writes, and stream_unpack_words, what its
kernel's decoder makes of it -- gives back the plan's words exactly, padding included, on random plans and at the format's edges;
the layout itself is pinned on a hand-made batch.  (tests/test_gpu_stream_packed.py compares the library's array with this one.)"""
import re

import numpy as np
import pytest
import torch

from tests import cases

RPW = 64            # rows per wave of the 64-column sum geometry (4 slots of 16 rows)


def _arrays(rowptr, col, n, slices, wpg, chunk):
    from isplib_amd.plan import stream_plan_arrays
    p = stream_plan_arrays(torch.from_numpy(rowptr), torch.from_numpy(col), n, slices, wpg, RPW, 4, chunk)
    return p["words"].numpy(), p["wave_step_off"].numpy(), p


def _round_trip(rowptr, col, n, slices, wpg, chunk, want=True):
    from isplib_amd.plan import STREAM_PACK_DWORDS, stream_pack_batches, stream_pack_words, stream_unpack_words
    words, off, p = _arrays(rowptr, col, n, slices, wpg, chunk)
    packed, ok = stream_pack_words(words, off, n, slices)
    assert ok == want
    assert packed.dtype == np.uint32 and packed.size == stream_pack_batches(off) * STREAM_PACK_DWORDS
    if ok:
        assert np.array_equal(stream_unpack_words(packed, off, n, slices), words)
    return words, off, packed, p


@pytest.mark.parametrize("seed", range(4))
def test_random_plans_round_trip(seed):
    rng = np.random.default_rng(seed)
    m, n = int(rng.integers(200, 1500)), int(rng.integers(100, 3000))
    rowptr, col = cases.random_csr(m, n, float(rng.uniform(2.0, 12.0)), seed=100 + seed, empty_rows=(0, m // 2),
                                   hub=(3, int(rng.integers(100, 600))), sort_cols=bool(seed % 2))
    _round_trip(rowptr, col, n, int(rng.integers(1, 12)), int(rng.integers(1, 6)), int(rng.integers(32, 256)))


def test_short_waves_ragged_batches_and_empty_waves():
    """A wave with fewer words than a batch, waves whose word count is no multiple of 128, and waves with no words at all (more
    waves than rows need: 8 waves of 4 streams for 10 rows -- a row per stream, the streams of five waves stay empty)."""
    rowptr, col = cases.random_csr(10, 500, 9.0, seed=5)
    words, off, packed, _ = _round_trip(rowptr, col, 500, 3, 8, 4096)
    nwords = (off[1:] - off[:-1]) * 4
    assert (nwords == 0).any() and ((nwords > 0) & (nwords < 128)).any() and (nwords % 128 != 0).any()
    rowptr, col = cases.random_csr(64, 300, 40.0, seed=6)
    words, off, packed, _ = _round_trip(rowptr, col, 300, 2, 1, 4096)
    assert (off[1] - off[0]) * 4 > 256 and ((off[1] - off[0]) * 4) % 128 != 0


@pytest.mark.parametrize("slices", (1, 40))
def test_one_slice_and_many_narrow_slices(slices):
    """40 slices of 75 columns on rows of ~6 entries: a slot's stream skips slices all the time, and the decoded slice lags behind
    the true one (the column field absorbs it)."""
    rowptr, col = cases.random_csr(300, 3000, 6.0, seed=7, empty_rows=(0, 17))
    words, off, packed, _ = _round_trip(rowptr, col, 3000, slices, 2, 4096)
    if slices == 40:
        width = 75
        lag = 0
        for w in range(len(off) - 1):           # some slot's true slice jumps by more than one between two of its entries
            for slot in range(4):
                ws = words[off[w] * 4 + slot:off[w + 1] * 4:4].astype(np.int64) & 0xFFFFFF
                sl = ws[ws != 3000] // width
                lag = max(lag, int(np.diff(sl).max(initial=0)))
        assert lag > 1


@pytest.mark.parametrize("n,slices,want", ((8192 * 2 - 1, 2, True), (8192 * 2, 2, True), (8192 * 2 + 1, 2, False),
                                           (8192 * 3, 3, True), (8192 * 3 + 1, 3, False)))
def test_slice_width_edge(n, slices, want):
    """Slices of 8,192 columns are the widest the 13-bit field holds; the last column and the last column of every slice are there."""
    rowptr, col = cases.random_csr(200, n, 12.0, seed=8)
    width = -(-n // slices)
    col = col.copy()
    for s in range(slices):          # row s: the first and the last column of slice s
        col[rowptr[s]:rowptr[s + 1]] = np.sort(np.resize(np.array([s * width, min((s + 1) * width, n) - 1]), rowptr[s + 1] - rowptr[s]))
    assert col.max() == n - 1
    _round_trip(rowptr, col, n, slices, 2, 4096, want)


def test_a_skip_over_a_wide_slice_is_not_representable():
    """Three slices of 8,000 columns and rows with entries in the first and the last only (a slot's 16 rows: 48 entries in slice 0,
    then slice 2 -- the skip falls inside the slot's second batch, where no header takes it): inside a batch the decoded slice cannot
    jump by two, and the 13-bit field cannot absorb a slice of 8,000 columns -- the packer says so and the plan runs on its words."""
    m, n = 64, 24000
    rowptr = np.arange(0, 5 * m + 1, 5, dtype=np.int64)
    col = np.tile(np.array([5, 70, 100, 17000, 23999], np.int64), m)
    _round_trip(rowptr, col, n, 3, 1, 4096, want=False)


def test_hub_rows_with_a_small_chunk():
    rowptr, col = cases.random_csr(400, 900, 8.0, seed=9, hub=(11, 700))
    _, _, _, p = _round_trip(rowptr, col, 900, 5, 3, 64)
    assert p["n_parts"] > 4 and p["n_hub"] >= 1


def test_layout_of_one_hand_made_batch():
    """One wave, 2 slices of 50 columns, n = 100.  Slot 0 holds 18 entries (so its 17th and 18th sit in the second batch register),
    slot 1 two entries in slice 1 only, slots 2 and 3 nothing."""
    from isplib_amd.plan import stream_pack_words, stream_unpack_words
    n = 100
    pad = [((s * 16) << 24) | n for s in range(4)]
    s0 = [(r << 24) | c for r, c in [(0, 3)] * 10 + [(1, 49), (1, 50), (2, 60)] + [(15, 99)] * 5]      # slice 0 x 11, then slice 1
    s1 = [((16 + 2) << 24) | 77, ((16 + 3) << 24) | 51]
    steps = len(s0)
    words = np.zeros(steps * 4, np.int64)
    for t in range(steps):
        words[t * 4:(t + 1) * 4] = [s0[t], s1[t] if t < 2 else pad[1], pad[2], pad[3]]
    off = np.array([0, steps], np.int64)
    packed, ok = stream_pack_words(words, off, n, 2)
    assert ok and packed.size == 2 * 76 and not packed[76:].any()             # (steps * 4) // 128 + 1 wave + 1 batches, the last unused
    assert [int(h) for h in packed[72:76]] == [0 | (18 << 12), 1 | (2 << 12), 0, 0]
    d = packed[:64].astype(np.int64)
    assert d[0] == 3 | (49 << 13) and d[4] == 3 | (49 << 13)                   # entries 16, 17 of slot 0 (column 99 = slice 1 + 49): bits 13..25, no flag
    assert d[4 * 10] == 49 | (1 << 26)
    assert d[4 * 11] == 0 | (1 << 26) | (1 << 30)                             # column 50: the slice advances, field 0
    assert d[4 * 12] == 10 | (2 << 26)                                        # column 60 = slice 1 + 10
    assert d[1] == (77 - 50) | (2 << 26) and d[5] == 1 | (3 << 26)            # slot 1 starts in slice 1: the header's, no flag
    assert int(packed[64]) == 15 | (15 << 4) and not packed[65:72].any()      # local rows of slot 0's entries 16 and 17
    assert np.array_equal(stream_unpack_words(packed, off, n, 2).view(np.uint32), words.astype(np.uint32))


def test_header_names_the_format_and_the_setting():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "isplib_hip.h")).read()
    from isplib_amd import plan
    assert int(re.search(r"#define\s+ISPLIB_STREAM_PACK_DWORDS\s+(\d+)", header).group(1)) == plan.STREAM_PACK_DWORDS
    assert int(re.search(r"#define\s+ISPLIB_STREAM_PACK_COL_BITS\s+(\d+)", header).group(1)) == plan.STREAM_PACK_COL_BITS
    assert "ISPLIB_STREAM_PACK" in header and re.search(r"const uint32_t \*packed;", header) and "has_packed" in header
