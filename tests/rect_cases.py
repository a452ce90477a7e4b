"""Rectangular inputs (M != N) of the six attention families -- attention, gat, gatv2 and their 16-bit twins -- for
tests/test_rect_host.py and tests/test_gpu_attention_rect.py.  The cases are built with the families' own Case / Case16 classes, so the
fp64 references and the bounds are those of tests/attention_ref.py, gat_ref.py, gatv2_ref.py and the three *16_ref.py, computed once per
case and shared, unchanged.

Every entry of these families takes an M x N structure: x, g, z, lse, D and a_dst have M rows, y, dy, a_src and dasrc have N rows.  The
host entries size each gathered operand's buffer descriptor from one of the two counts and the launch grid from the other side's, so an
m / n mix-up clips rows (they read as 0), over-reads a neighbour, or leaves rows unwritten -- and is invisible on a square graph.  Two
shapes, both counts odd and no multiple of any block's wave count:

    tall  M = 233, N = 67     stored entries with a row id >= N: what a columns-kernel extent taken from n would clip
    wide  M = 67,  N = 233    stored entries with a column id >= M: what a forward / rows-kernel extent taken from m would clip

rect_graph(m, n, seed): rows 0..13 have exactly the lengths ROW_LENGTHS = attention_cases.LENGTHS + (HUB,) with columns drawn from
[0, n - 14); columns n - 14 .. n - 1 have exactly those values as in-degrees with rows drawn from [14, m); drawn with replacement and
left in drawing order after a stable sort by row.  So both the row kernels and the columns kernel meet every edge length, row 0 is empty,
column n - 14 is referenced by nothing, and row m - 1 and column n - 1 (the hub column) are gathered.  2720 entries at both shapes.

Operands are drawn as the square cases draw them (1.2 N(0, 1); att ~ N(0, 1) / sqrt(d); p = 1 / sqrt(K)); every case asserts
rho <= RHO_MAX when it is built (the bounds are first order in rho).  One configuration per kernel instantiation, not the whole list.
"""
import functools

import numpy as np
import torch

from tests import attention16_cases
from tests import attention_cases
from tests import attention_ref
from tests import gat16_cases
from tests import gat_cases
from tests import gatv2_16_cases
from tests import gatv2_cases

SHAPES = {"tall": (233, 67), "wide": (67, 233)}
SEEDS = {"tall": 0, "wide": 1}
ROW_LENGTHS = attention_cases.LENGTHS + (attention_cases.HUB,)
BLOCK = len(ROW_LENGTHS)
RHO_MAX = attention_ref.RHO_MAX
BF, FP = torch.bfloat16, torch.float16

ATTENTION_WIDTHS = (3, 33, 128, 257)                        # first instantiation, ragged, a full 32-lane one, two chunks per lane
GAT_CONFIGS = ((1, 47), (8, 8), (3, 128), (2, 256))         # H == 1 ragged, multi-head narrow, H no power of two, two chunks
ATTENTION16_WIDTHS = (8, 34, 128, 512)
GAT16_CONFIGS = ((1, 46), (8, 8), (4, 32), (8, 64))
GAT16_SPECS = tuple((h, d, BF) for h, d in GAT16_CONFIGS) + ((8, 8, FP),)       # bf16 everywhere, fp16 at one configuration
assert set(ATTENTION_WIDTHS) <= set(attention_cases.WIDTHS) and set(ATTENTION16_WIDTHS) <= set(attention16_cases.WIDTHS)
assert set(GAT_CONFIGS) <= set(gat_cases.CONFIGS) and set(GAT16_CONFIGS) <= set(gat16_cases.CONFIGS)

dtype_name = attention16_cases.dtype_name


@functools.lru_cache(maxsize=None)
def rect_graph(m, n, seed):
    """-> (rowptr [m + 1], col [nnz]) int64; CSR in drawing order."""
    assert m > 2 * BLOCK and n > 2 * BLOCK and m != n
    rng = np.random.default_rng(4000 + seed)
    lens = np.array(ROW_LENGTHS, dtype=np.int64)
    total = int(lens.sum())
    rows = [np.repeat(np.arange(BLOCK), lens), rng.integers(BLOCK, m, size=total)]       # rows 0..13: exact lengths
    cols = [rng.integers(0, n - BLOCK, size=total), np.repeat(np.arange(n - BLOCK, n), lens)]   # the last 14 columns: exact in-degrees
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = np.argsort(row, kind="stable")
    row, col = row[order], col[order]
    rowptr = np.zeros(m + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=m), out=rowptr[1:])
    deg, indeg = np.diff(rowptr), np.bincount(col, minlength=n)
    assert np.array_equal(deg[:BLOCK], lens) and np.array_equal(indeg[n - BLOCK:], lens)
    assert any(np.unique(col[rowptr[i]:rowptr[i + 1]]).size < deg[i] for i in range(m)), "duplicate entries"
    assert any(np.any(np.diff(col[rowptr[i]:rowptr[i + 1]]) < 0) for i in range(m)), "unsorted rows"
    assert deg[m - 1] > 0 and indeg[n - 1] > 0 and (deg == 0).any() and (indeg == 0).any()
    assert (row >= n).any() if m > n else (col >= m).any()
    rowptr.setflags(write=False)
    col.setflags(write=False)
    return rowptr, col


def graph(shape):
    return rect_graph(*SHAPES[shape], SEEDS[shape])


def _seed(shape, *parts):
    return 50000 * (1 + SEEDS[shape]) + sum(int(p) * w for p, w in zip(parts, (1000, 1)))


def _capped(case):
    top = float(case.bound["rho"].max())
    assert top <= RHO_MAX, (case.name, top)
    return case


@functools.lru_cache(maxsize=None)
def attention_case(shape, k):
    (m, n), (rowptr, col) = SHAPES[shape], graph(shape)
    f, s = attention_cases.features, _seed(shape, 0, k)
    return _capped(attention_cases.Case(f"{shape}-k{k}", rowptr, col, f(m, k, s + 10), f(n, k, s + 20), f(m, k, s + 30), 1.0 / np.sqrt(k)))


@functools.lru_cache(maxsize=None)
def attention16_case(shape, k, dtype):
    (m, n), (rowptr, col) = SHAPES[shape], graph(shape)
    f, s = attention_cases.features, _seed(shape, 0, k)
    return _capped(attention16_cases.Case16(f"{shape}-k{k}", rowptr, col, f(m, k, s + 10), f(n, k, s + 20), f(m, k, s + 30),
                                            1.0 / np.sqrt(k), dtype))


def _gat_operands(shape, heads, d):
    (m, n), s, normal = SHAPES[shape], _seed(shape, heads, d), gat_cases.normal
    k = heads * d
    return normal((n, k), s + 1), normal((m, heads), s + 2), normal((n, heads), s + 3), normal((m, k), s + 4)


@functools.lru_cache(maxsize=None)
def gat_case(shape, heads, d, ns=0.2):
    rowptr, col = graph(shape)
    y, a_dst, a_src, g = _gat_operands(shape, heads, d)
    return _capped(gat_cases.Case(f"{shape}-h{heads}d{d}", rowptr, col, y, a_dst, a_src, g, heads, ns))


@functools.lru_cache(maxsize=None)
def gat16_case(shape, heads, d, dtype=BF, ns=0.2):
    rowptr, col = graph(shape)
    y, a_dst, a_src, g = _gat_operands(shape, heads, d)
    return _capped(gat16_cases.Case16(f"{shape}-h{heads}d{d}", rowptr, col, y, a_dst, a_src, g, heads, ns, dtype))


def _gatv2_operands(shape, heads, d):
    (m, n), s, normal = SHAPES[shape], _seed(shape, heads, d), gatv2_cases.normal
    k = heads * d
    att = (np.random.default_rng(s + 5).standard_normal((heads, d)) / np.sqrt(d)).astype(np.float32)
    return normal((m, k), s + 1), normal((n, k), s + 2), att, normal((m, k), s + 4)


@functools.lru_cache(maxsize=None)
def gatv2_case(shape, heads, d, ns=0.2):
    rowptr, col = graph(shape)
    x, y, att, g = _gatv2_operands(shape, heads, d)
    return _capped(gatv2_cases.Case(f"{shape}-h{heads}d{d}", rowptr, col, x, y, att, g, heads, ns))


@functools.lru_cache(maxsize=None)
def gatv2_16_case(shape, heads, d, dtype=BF, ns=0.2):
    rowptr, col = graph(shape)
    x, y, att, g = _gatv2_operands(shape, heads, d)
    return _capped(gatv2_16_cases.Case16(f"{shape}-h{heads}d{d}", rowptr, col, x, y, att, g, heads, ns, dtype))


def all_cases():
    """Every case of both shapes, built (and its rho cap asserted) on first use."""
    out = []
    for shape in SHAPES:
        out += [attention_case(shape, k) for k in ATTENTION_WIDTHS]
        out += [attention16_case(shape, k, dtype) for k in ATTENTION16_WIDTHS for dtype in (BF, FP)]
        out += [gat_case(shape, h, d) for h, d in GAT_CONFIGS] + [gatv2_case(shape, h, d) for h, d in GAT_CONFIGS]
        out += [gat16_case(shape, h, d, dtype) for h, d, dtype in GAT16_SPECS]
        out += [gatv2_16_case(shape, h, d, dtype) for h, d, dtype in GAT16_SPECS]
    return out
