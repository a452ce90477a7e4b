"""Inputs of the attention tests (tests/test_attention_host.py, tests/test_gpu_attention.py), with their fp64 reference and bounds
computed once per case (tests/attention_ref.py) and shared, unchanged, by every test that needs them.

The kernels (isplib_amd/csrc/attention.hip) take one wave per row with G = 64 / LPR edge slots and U = 4 gathers per slot and step;
LPR is 8 / 16 / 32 / 64 / 64 (two chunks per lane) for K up to 32 / 64 / 128 / 256 / 512.  WIDTHS holds the first, last and ragged
width of every instantiation; LENGTHS holds 0, 1, G - 1, G, G + 1 for every G in (1, 2, 4, 8), the edges of the 64-entry batch, 129 and
one hub of 1000.  The graph is 200 x 200: rows 0..99 have exactly the LENGTHS (columns drawn from 0..99), columns 100..199 have exactly
the LENGTHS as in-degrees (rows drawn from 100..199) -- so both the row kernels and the column kernel meet every length.  Columns are
drawn with replacement and left in drawing order: duplicate entries and unsorted rows are part of every case.
"""
import functools

import numpy as np

from tests import attention_ref as ref

WIDTHS = (1, 3, 4, 31, 32, 33, 64, 65, 128, 129, 256, 257, 512)
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129)
HUB = 1000
HALF = 100
N = 2 * HALF


def slots(k):
    """G = 64 / LPR of the instantiation that serves width k."""
    w = (k + 3) // 4
    return 8 if w <= 8 else 4 if w <= 16 else 2 if w <= 32 else 1


def lengths():
    out = [LENGTHS[t % len(LENGTHS)] for t in range(HALF)]
    out[HALF - 1] = HUB
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def graph(seed=0):
    """-> (rowptr [N + 1], col [nnz]) int64; CSR in drawing order."""
    rng = np.random.default_rng(1000 + seed)
    lens = lengths()
    rows = [np.repeat(np.arange(HALF), lens)]                          # rows 0..99: exact row lengths, columns from 0..99
    cols = [rng.integers(0, HALF, size=int(lens.sum()))]
    cols.append(np.repeat(np.arange(HALF, N), lens))                   # columns 100..199: exact in-degrees, rows from 100..199
    rows.append(rng.integers(HALF, N, size=int(lens.sum())))
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = np.argsort(row, kind="stable")
    row, col = row[order], col[order]
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=N), out=rowptr[1:])
    deg, indeg = np.diff(rowptr), np.bincount(col, minlength=N)
    assert np.array_equal(deg[:HALF], lens) and np.array_equal(indeg[HALF:], lens)
    has_dup = any(np.unique(col[rowptr[i]:rowptr[i + 1]]).size < deg[i] for i in range(N))
    has_unsorted = any(np.any(np.diff(col[rowptr[i]:rowptr[i + 1]]) < 0) for i in range(N))
    assert has_dup and has_unsorted
    rowptr.setflags(write=False)
    col.setflags(write=False)
    return rowptr, col


class Case:
    def __init__(self, name, rowptr, col, x, y, g, p, kind="bounded"):
        self.name, self.rowptr, self.col, self.x, self.y, self.g, self.p, self.kind = name, rowptr, col, x, y, g, float(p), kind
        self.ref = ref.attention(rowptr, col, x, y, self.p, g)
        self.bound = ref.bounds(rowptr, col, x, y, self.p, self.ref, g)
        for a in (x, y, g):
            a.setflags(write=False)

    @property
    def m(self):
        return self.rowptr.size - 1

    @property
    def k(self):
        return self.x.shape[1]

    @property
    def live(self):
        return np.diff(self.rowptr) > 0


def features(rows, k, seed, spread=1.2):
    return (np.random.default_rng(seed).standard_normal((rows, k)) * spread).astype(np.float32)


@functools.lru_cache(maxsize=None)
def width_case(k):
    """Real-valued operands at width k, p = 1 / sqrt(k): scores of a few units, rho <= 1e-3 on every row, the hub included."""
    rowptr, col = graph()
    return Case(f"k{k}", rowptr, col, features(N, k, 10 + k), features(N, k, 20 + k), features(N, k, 30 + k), 1.0 / np.sqrt(k))


@functools.lru_cache(maxsize=None)
def large_case(k=33):
    """Scores spread over +-200 in real rows: exp of the raw score overflows fp32 from 88.7 on.  The products of one edge share a sign
    (x >= 0, a row of y of one sign), so sum_c |x_ic y_jc| = |s_e| / p and the score term of rho is as small as scores of this size
    allow: delta s_e = 1e-5 |s_e|, i.e. 2e-3 at |s_e| = 200.  rho <= 1e-3 is out of reach for ANY operands with such scores; this
    case is held to rho <= LARGE_RHO_MAX instead (tests/test_attention_host.py says why that keeps the bound first order)."""
    rowptr, col = graph()
    rng = np.random.default_rng(77)
    x = np.abs(rng.standard_normal((N, k))).astype(np.float32) + 0.5
    y = (np.abs(rng.standard_normal((N, k))) + 0.5).astype(np.float32)
    p = 1.0 / np.sqrt(k)
    # sign and size per row of y so that p <x_i, y_j> covers [-200, 200] over the columns
    top = float((x.astype(np.float64) @ y.astype(np.float64).T).max() * p)
    y = (y * (np.linspace(-1.0, 1.0, N) * 200.0 / top)[:, None]).astype(np.float32)
    return Case("large", rowptr, col, x, y, features(N, k, 78), p, kind="large")


LARGE_RHO_MAX = 4e-3


@functools.lru_cache(maxsize=None)
def single_case(k=33):
    """Every row has one entry or none; |s| reaches about 1e4.  z_i = y_j bit for bit whatever the score, lse_i = s_e."""
    rng = np.random.default_rng(5)
    deg = (np.arange(N) % 5 != 0).astype(np.int64)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, N, size=int(deg.sum()))
    x = features(N, k, 6, 30.0)
    y = features(N, k, 7, 30.0)
    case = Case("single", rowptr, col, x, y, features(N, k, 8), 1.0, kind="single")
    assert np.abs(case.ref["s"]).max() > 5e3
    return case


def bounded_cases():
    return [width_case(k) for k in WIDTHS]


def all_cases():
    return bounded_cases() + [large_case(), single_case()]
