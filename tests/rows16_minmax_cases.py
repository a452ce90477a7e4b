"""Inputs of the 16-bit max / min row kernel's tests (tests/test_gpu_rows16_minmax.py runs them on the GPU, tests/test_rows16_minmax_host.py
proves on the CPU that they hold what the tests are for): graphs, operands with planted ties / specials, and the reference.

Every operand made by `operand` has
  * column 0 all zeros, +0 in even rows and -0 in odd ones: every candidate of that column ties (weighted: the sign of the weight flips
    the zero), so the winner must be the row's FIRST edge and the sign of the result is that edge's;
  * NaN in every column of the source rows of one short graph row (`victim`): in that graph row nothing wins -- value -+FLT_MAX, which
    rounds to -+Inf, position nnz -- and every other graph row that reads those sources has a NaN among finite candidates."""
import numpy as np

from tests import cases, half_ref
from tests.test_gpu_stream_edges import _weights

LONG_ROW = 2048
UNROLLS = (2, 3, 6)              # mm16_unroll (spmm_rows16_minmax.hip): weighted + positions, unit + positions / weighted values, unit values
WIDTHS = (8, 10, 64, 66, 128, 130, 256, 258, 512, 514, 1024, 1026)
FLT_MAX = np.float32(np.finfo(np.float32).max)


def hub_graph():
    return cases.random_csr(300, 200, 12, 31, empty_rows=(0, 150, 299), hub=(7, 2500), duplicates=True)


def edge_degrees():
    deg = {0, 1, 63, 64, 65, 127, 128, 129, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 3 * LONG_ROW}
    for lpr in (8, 32):                                      # the configurations of k = 64 and k = 256
        g = 64 // lpr
        deg |= {g - 1, g, g + 1}
        for u in UNROLLS:
            deg |= {g * u - 1, g * u, g * u + 1}
    return sorted(deg)


def lengths_graph():
    deg = edge_degrees()
    return cases.csr_of_degrees(deg + deg[::-1], 200, 17)    # every length in two places of a workgroup's four rows


def victim(rowptr):
    """The first of the shortest non-empty rows."""
    deg = np.diff(rowptr)
    return int(np.flatnonzero(deg == deg[deg > 0].min())[0])


def operand(rowptr, col, n, k, seed, kind, dtype):
    x = cases.dense(n, k, seed, kind)
    x[:, 0] = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    r = victim(rowptr)
    x[col[rowptr[r]:rowptr[r + 1]]] = np.nan
    return half_ref.to16(x, dtype)


def specials(x16, red):
    """Test 3's extra plants in an integer operand (rows 5, 9, 11, 13 of it, columns 1.. in steps of 7 and all of row 13): +-Inf
    winners, a value whose weighted product overflows fp16 but not fp32, and a source row that can never win unweighted."""
    x = half_ref.widen(x16).copy()
    x[5, 1::7] = np.inf
    x[9, 2::7] = -np.inf
    x[11, 3::7] = 30000.0
    x[13, 1:] = -np.inf if red == "max" else np.inf
    return half_ref.to16(x, x16.dtype)


def all_lose_graph(n):
    """Three rows: sources {13} only (all -Inf under max / +Inf under min after `specials`), an empty row, sources {13, 13, 20}."""
    return np.array([0, 3, 3, 6], np.int64), np.array([13, 13, 13, 13, 13, 20], np.int64)


def weights_of(col, unit):
    return np.ones(col.size, np.float32) if unit else _weights(col.size)


def reference(oracle, rowptr, col, val, x16, red):
    """(ref32, ref16, positions): half_ref.reference, and the positions of the same oracle call."""
    ref32, ref16 = half_ref.reference(oracle, rowptr, col, val, x16, red)
    again, arg = oracle.spmm_fw(rowptr, col, val, half_ref.widen(x16), red)
    assert np.array_equal(again.view(np.uint32), ref32.view(np.uint32))
    return ref32, ref16, arg


def slot_cases(dtype, red):
    """Test 1: (name, rowptr, col, val, x16)."""
    rowptr, col = hub_graph()
    for k in WIDTHS:
        x16 = operand(rowptr, col, 200, k, 3, "uniform", dtype)
        for unit in (False, True):
            yield (f"k{k}-{'unit' if unit else 'weighted'}", rowptr, col, weights_of(col, unit), x16)


def length_cases(dtype, red):
    """Test 2."""
    rowptr, col = lengths_graph()
    for k in (64, 256):
        x16 = operand(rowptr, col, 200, k, 3, "uniform", dtype)
        for unit in (False, True):
            yield (f"k{k}-{'unit' if unit else 'weighted'}", rowptr, col, weights_of(col, unit), x16)


def tie_cases(dtype, red):
    """Test 3: integer features in [-3, 3] on the duplicate-edge hub graph, with the specials; and the three-row graph."""
    rowptr, col = hub_graph()
    for k in (64, 130):
        x16 = specials(operand(rowptr, col, 200, k, 3, "integer", dtype), red)
        for unit in (False, True):
            yield (f"hub-k{k}-{'unit' if unit else 'weighted'}", rowptr, col, weights_of(col, unit), x16)
    rp3, col3 = all_lose_graph(200)
    x16 = specials(operand(rowptr, col, 200, 64, 3, "integer", dtype), red)
    yield ("all-lose-unit", rp3, col3, weights_of(col3, True), x16)


def census(rowptr, col, val, x16, ref32, arg):
    """What the reference holds: (elements of column 0 in which two or more edges reach the winning value, non-empty rows with an
    element nothing won, empty rows)."""
    x0 = half_ref.widen(x16)[:, 0]
    cand = val * x0[col]
    deg = np.diff(rowptr)
    ties = 0
    for r in np.flatnonzero(deg >= 2):
        c = cand[rowptr[r]:rowptr[r + 1]]
        ties += int(np.count_nonzero(c == ref32[r, 0]) >= 2 and arg[r, 0] != col.size)
    nothing = np.flatnonzero((deg > 0) & (arg == col.size).any(1))
    return ties, nothing, np.flatnonzero(deg == 0)
