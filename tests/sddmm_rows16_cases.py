"""Inputs shared by tests/test_gpu_sddmm_rows16.py and the census and emulation of them in tests/test_sddmm_rows16_host.py: the
graphs are those of tests/test_gpu_rows16.py; the kernel's constants (isplib_amd/csrc/sddmm_rows16.hip, rows16_common.h) are
restated here."""
import numpy as np

from tests import cases
from tests.test_gpu_rows16 import _hub_graph

N = 200                                        # columns of both graphs
LONG_ROW = 2048                                # rows with more edges are split across a workgroup's four waves
U = 4                                          # SDDMM16_U: gathers per slot and step (tail steps: 2)
WIDTHS = (8, 10, 64, 66, 128, 130, 256, 258, 512, 514, 1022, 1024)
LENGTH_WIDTHS = (64, 256, 1024)
SUBNORMAL_SCALE = np.float32(1e-20)


def slot(k):
    """(LPR, NCH) of rows16_by_width: lanes per row slot and 8-column chunks per lane."""
    width = (k + 7) // 8
    for lpr in (8, 16, 32, 64):
        if width <= lpr:
            return lpr, 1
    return 64, 2


def slots_per_gather(k):
    """G: the edges one gather instruction of the wave serves."""
    return 64 // slot(k)[0]


def lane_columns(k):
    """Per (lane of a slot, chunk): (first column gathered, vfirst) as rows16_column gives them, or None beyond the row."""
    lpr, nch = slot(k)
    out = {}
    for lc in range(lpr):
        for j in range(nch):
            col = (j * lpr + lc) * 8
            if col >= k:
                out[lc, j] = None
            elif col + 8 > k:
                out[lc, j] = (k - 8, col + 8 - k)
            else:
                out[lc, j] = (col, 0)
    return out


def duplicated_columns(k):
    """The columns a shifted last vector gathers a second time (empty when k % 8 == 0)."""
    dup = []
    for v in lane_columns(k).values():
        if v is not None and v[1] > 0:
            dup += list(range(v[0], v[0] + v[1]))
    return sorted(dup)


def hub_graph():
    """random_csr(300, 200, 12, 31, empty_rows=(0, 150, 299), hub=(7, 2500), duplicates=True)."""
    return _hub_graph()


def edge_degrees():
    deg = {0, 1, 63, 64, 65, 127, 128, 129, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 3 * LONG_ROW}
    for k in LENGTH_WIDTHS:                    # G = 8, 2, 1
        g = slots_per_gather(k)
        deg |= {g - 1, g, g + 1, g * U - 1, g * U, g * U + 1}
    return sorted(deg)


def length_degrees():
    deg = edge_degrees()
    return deg + deg[::-1]                     # every length in two places of a workgroup's four rows


def length_graph():
    return cases.csr_of_degrees(length_degrees(), N, 17)


def ragged_trap(m, k=66, seed=43):
    """(y [N, k], g [m, k]) for the trap of a ragged K: y holds Inf -- one sign per row, in every third row -- in exactly the columns
    the shifted last vector gathers a second time, g is finite and positive there, everything else is finite.  An edge touching such
    a row of y is Inf of that sign; a kernel that zeroes g's duplicates but multiplies y's makes it Inf * 0 = NaN."""
    dup = duplicated_columns(k)
    y, g = cases.dense(N, k, seed, "uniform"), cases.dense(m, k, seed + 1, "uniform")
    g[:, dup] = np.abs(g[:, dup]) + np.float32(0.5)
    for r in range(0, N, 3):
        y[r, dup] = np.float32(np.inf) if (r // 3) % 2 == 0 else np.float32(-np.inf)
    return y, g


def subnormal_operands(m, k, seed=47):
    """Operands of magnitude ~1e-20 (bf16 holds them; fp16 does not): every product is an fp32 subnormal."""
    return cases.dense(N, k, seed, "uniform") * SUBNORMAL_SCALE, cases.dense(m, k, seed + 1, "uniform") * SUBNORMAL_SCALE


def emulate(rowptr, col, y, g, mean=False):
    """The kernel's summation order in numpy fp32: per lane its 8 (16: two chunks) columns in ascending order, one rounding per
    product-and-add as a fused multiply-add has (formed in double and rounded once: |operands| of 16 bits make every product exact
    in double), then a pairwise tree over the slot's lanes, then the mean's fp32 1.0f / deg."""
    y, g = np.asarray(y, np.float32), np.asarray(g, np.float32)
    k = y.shape[1]
    lpr, nch = slot(k)
    cols = lane_columns(k)
    deg = np.diff(rowptr)
    erow = np.repeat(np.arange(deg.size), deg)
    yy, gg = y[col].astype(np.float64), g[erow].astype(np.float64)
    part = np.zeros((lpr, col.size), np.float32)
    for lc in range(lpr):
        for j in range(nch):
            if cols[lc, j] is None:
                continue
            first, vfirst = cols[lc, j]
            for c in range(first + vfirst, first + 8):
                part[lc] = (part[lc].astype(np.float64) + yy[:, c] * gg[:, c]).astype(np.float32)
    while part.shape[0] > 1:                   # the butterfly: halves of the slot, widest first
        h = part.shape[0] // 2
        part = (part[:h] + part[h:]).astype(np.float32)
    out = part[0]
    if mean:
        out = (out * (np.float32(1.0) / np.maximum(deg, 1).astype(np.float32))[erow]).astype(np.float32)
    return out
