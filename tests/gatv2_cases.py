"""Inputs of the GATv2 tests (tests/test_gatv2_host.py, tests/test_gpu_gatv2.py), with their fp64 reference and bounds computed once
per case (tests/gatv2_ref.py) and shared, unchanged, by every test that needs them.

The kernels (isplib_amd/csrc/gatv2.hip) take the mapping of gat.hip, so the configurations are those of tests/gat_cases.py: per
instantiation its first, last and a ragged width, heads of one lane up to a whole chunk, both chunks in one head and in two, head counts
that are no power of two, and the class-count widths with H = 1.  The graph is the 200 x 200 graph of tests/attention_cases.py: every
row length and column in-degree on a loop edge, a hub of 1000, duplicates, unsorted rows.  Every case asserts its rho cap when it is
built (RHO_MAX; the large case LARGE_RHO_MAX, as the attention large case): the bound is first order in rho.
"""
import functools

import numpy as np

from tests import attention_cases
from tests import gat_cases
from tests import gatv2_ref as ref

CONFIGS = gat_cases.CONFIGS
SLOPES = gat_cases.SLOPES
SLOPE_CONFIGS = ((1, 47), (8, 8), (3, 128))
N = attention_cases.N
LARGE_RHO_MAX = attention_cases.LARGE_RHO_MAX
graph = attention_cases.graph


class Case:
    def __init__(self, name, rowptr, col, x, y, att, g, heads, ns, kind="bounded", rho_max=ref.RHO_MAX):
        self.name, self.rowptr, self.col, self.x, self.y, self.att, self.g = name, rowptr, col, x, y, att, g
        self.heads, self.ns, self.kind, self.rho_max = int(heads), float(ns), kind, rho_max
        self.ref = ref.gatv2(rowptr, col, x, y, att, self.heads, self.ns, g)
        self.bound = ref.bounds(rowptr, col, x, y, att, self.heads, self.ns, self.ref, g)
        assert float(self.bound["rho"].max()) <= rho_max, (name, float(self.bound["rho"].max()))
        for a in (x, y, att, g):
            a.setflags(write=False)

    @property
    def m(self):
        return self.rowptr.size - 1

    @property
    def n(self):
        return self.y.shape[0]

    @property
    def k(self):
        return self.y.shape[1]

    @property
    def live(self):
        return np.diff(self.rowptr) > 0


def normal(shape, seed, spread=1.2):
    return (np.random.default_rng(seed).standard_normal(shape) * spread).astype(np.float32)


@functools.lru_cache(maxsize=None)
def config_case(heads, d, ns=0.2):
    """x, y, g drawn as 1.2 N(0, 1), att as N(0, 1) / sqrt(d): scores of a few units, u of both signs on every edge."""
    rowptr, col = graph()
    k, seed = heads * d, 1000 * heads + d + int(round(ns * 10)) * 100000
    att = (np.random.default_rng(seed + 5).standard_normal((heads, d)) / np.sqrt(d)).astype(np.float32)
    return Case(f"h{heads}d{d}ns{ns:g}", rowptr, col, normal((N, k), seed + 1), normal((N, k), seed + 2), att, normal((N, k), seed + 4),
                heads, ns)


def _head_scores(rowptr, col, x, y, att, heads, ns):
    return ref.gatv2(rowptr, col, x, y, att, heads, ns)["s"]


@functools.lru_cache(maxsize=None)
def large_case(heads=8, d=8, ns=0.2):
    """Scores spread beyond +-150 in real rows: exp of the raw score overflows fp32 from 88.7 on.  att > 0, x >= 0 small, and a row of
    y of one sign per head (a factor per (node, head) permuted from linspace(-1, 1, N), the negative half divided by ns so that the
    slope gives it back), so the products att_c v_ec of one edge and head share a sign and delta s_e is about 1e-5 |s_e| -- as small as
    scores of this size allow.  rho <= 1e-3 is out of reach for ANY operands with such scores; the case is held to LARGE_RHO_MAX."""
    rowptr, col = graph()
    rng = np.random.default_rng(77)
    k = heads * d
    att = ((np.abs(rng.standard_normal((heads, d))) + 0.5) / d).astype(np.float32)
    x = (0.25 * np.abs(rng.standard_normal((N, k)))).astype(np.float32)
    base = np.abs(rng.standard_normal((N, k))) + 0.5
    f = np.stack([rng.permutation(np.linspace(-1.0, 1.0, N)) for _ in range(heads)], 1)
    f = np.where(f < 0, f / ns, f)
    y0 = base * np.repeat(f, d, axis=1)
    scale = 1.0
    for _ in range(4):                                                      # the score is not linear in y (x shifts u): a few steps settle it
        y = (y0 * scale).astype(np.float32)
        scale *= 200.0 / float(_head_scores(rowptr, col, x, y, att, heads, ns).max())
    y = (y0 * scale).astype(np.float32)
    case = Case("large", rowptr, col, x, y, att, normal((N, k), 79), heads, ns, kind="large", rho_max=LARGE_RHO_MAX)
    s = case.ref["s"]
    assert s.max() > 150 and s.min() < -150
    spread = np.zeros(case.m)
    np.maximum.at(spread, case.ref["row"], np.abs(s).max(1))
    assert (spread > 100).sum() > case.m // 4                               # in real rows, not in one
    return case


@functools.lru_cache(maxsize=None)
def single_case(heads=4, d=8, ns=0.2):
    """Every row has one entry or none.  z_i = y_j bit for bit whatever the score; lse is the score."""
    rng = np.random.default_rng(5)
    deg = (np.arange(N) % 5 != 0).astype(np.int64)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, N, size=int(deg.sum()))
    k = heads * d
    att = (rng.standard_normal((heads, d)) / np.sqrt(d)).astype(np.float32)
    case = Case("single", rowptr, col, normal((N, k), 6, 10.0), normal((N, k), 7, 10.0), att, normal((N, k), 8), heads, ns, kind="single")
    assert np.abs(case.ref["s"]).max() > 30
    return case


def config_cases():
    return [config_case(h, d) for h, d in CONFIGS]


def slope_cases():
    """The three slopes at one configuration of each head form: ns = 0 (no gradient below 0), ns = 1 (no kink)."""
    return [config_case(h, d, ns) for h, d in SLOPE_CONFIGS for ns in SLOPES[1:]]


def all_cases():
    return config_cases() + slope_cases() + [large_case(), single_case()]
