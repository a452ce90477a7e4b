"""Inputs of the multi-head dot-product attention tests (tests/test_mha_host.py, tests/test_gpu_mha.py), with their fp64 reference and
bounds computed once per case (tests/mha_ref.py) and shared, unchanged, by every test that needs them.

The kernels (isplib_amd/csrc/mha.hip) take the mapping of gatv2.hip, so the configurations are those of tests/gat_cases.py: per
instantiation its first, last and a ragged width, heads of one lane up to a whole chunk, both chunks in one head and in two, head counts
that are no power of two, and the class-count widths with H = 1.  The graph is the 200 x 200 graph of tests/attention_cases.py: every
row length and column in-degree on a loop edge, a hub of 1000, duplicates, unsorted rows; the two rectangular shapes are those of
tests/rect_cases.py.  q, k, v, g are 1.2 N(0, 1) with the seeds 1000 H + d + {1, 2, 3, 4} and p = 1 / sqrt(d).  Every case asserts its
rho cap when it is built (RHO_MAX; the large case LARGE_RHO_MAX, as the attention large case): the bound is first order in rho.  The
cap is a condition on the inputs, not a measurement of the kernels: for the configurations the worst is 7.2e-4 at (1, 512), with |s|
below 10.5.
"""
import functools

import numpy as np

from tests import attention_cases
from tests import gat_cases
from tests import mha_ref as ref
from tests import rect_cases

CONFIGS = gat_cases.CONFIGS
N = attention_cases.N
LARGE_RHO_MAX = attention_cases.LARGE_RHO_MAX
graph = attention_cases.graph
RECT_CONFIGS = ((1, 47), (8, 8))
FUSED_CONFIGS = ((8, 16), (1, 47))
SCALES = (0.5, -0.3)                       # explicit scales at (8, 8), where 1 / sqrt(d) = 0.354: another magnitude, and a negative one


class Case:
    def __init__(self, name, rowptr, col, q, k, v, g, heads, p, kind="bounded", rho_max=ref.RHO_MAX):
        self.name, self.rowptr, self.col, self.q, self.k, self.v, self.g = name, rowptr, col, q, k, v, g
        self.heads, self.p, self.kind, self.rho_max = int(heads), float(p), kind, rho_max
        self.ref = ref.mha(rowptr, col, q, k, v, self.heads, self.p, g)
        self.bound = ref.bounds(rowptr, col, q, k, v, self.heads, self.p, self.ref, g)
        assert float(self.bound["rho"].max()) <= rho_max, (name, float(self.bound["rho"].max()))
        for a in (q, k, v, g):
            a.setflags(write=False)

    @property
    def m(self):
        return self.rowptr.size - 1

    @property
    def n(self):
        return self.k.shape[0]

    @property
    def width(self):
        return self.k.shape[1]

    @property
    def d(self):
        return self.width // self.heads

    @property
    def live(self):
        return np.diff(self.rowptr) > 0


def normal(shape, seed, spread=1.2):
    return (np.random.default_rng(seed).standard_normal(shape) * spread).astype(np.float32)


def _operands(m, n, heads, d, seed):
    width = heads * d
    return normal((m, width), seed + 1), normal((n, width), seed + 2), normal((n, width), seed + 3), normal((m, width), seed + 4)


@functools.lru_cache(maxsize=None)
def config_case(heads, d, scale=None):
    """q, k, v, g drawn as 1.2 N(0, 1), p = 1 / sqrt(d) (or the explicit `scale`): scores of a few units."""
    rowptr, col = graph()
    q, k, v, g = _operands(N, N, heads, d, 1000 * heads + d)
    p = 1.0 / np.sqrt(d) if scale is None else scale
    return Case(f"h{heads}d{d}" + ("" if scale is None else f"p{scale:g}"), rowptr, col, q, k, v, g, heads, p)


@functools.lru_cache(maxsize=None)
def shared_case(heads, d):
    """k is v: the operands of config_case with v replaced by k."""
    rowptr, col = graph()
    q, k, _, g = _operands(N, N, heads, d, 1000 * heads + d)
    return Case(f"h{heads}d{d}kv", rowptr, col, q, k, k, g, heads, 1.0 / np.sqrt(d))


@functools.lru_cache(maxsize=None)
def zero_q_case(heads, d):
    """q = 0: every score is 0, the weights are 1 / deg, lse = log deg."""
    rowptr, col = graph()
    _, k, v, g = _operands(N, N, heads, d, 1000 * heads + d)
    return Case(f"h{heads}d{d}q0", rowptr, col, np.zeros((N, heads * d), dtype=np.float32), k, v, g, heads, 1.0 / np.sqrt(d))


@functools.lru_cache(maxsize=None)
def rect_case(shape, heads, d):
    (m, n), (rowptr, col) = rect_cases.SHAPES[shape], rect_cases.graph(shape)
    q, k, v, g = _operands(m, n, heads, d, 50000 * (1 + rect_cases.SEEDS[shape]) + 1000 * heads + d)
    return Case(f"{shape}-h{heads}d{d}", rowptr, col, q, k, v, g, heads, 1.0 / np.sqrt(d))


@functools.lru_cache(maxsize=None)
def large_case(heads=8, d=8):
    """Scores spread beyond +-150 in real rows: exp of the raw score overflows fp32 from 88.7 on.  Built as attention_cases.large_case:
    q >= 0 and a row of k of one sign per head (a factor per (node, head) permuted from linspace(-1, 1, N)), so the products of one
    edge and head share a sign, sum_c |q_ic k_jc| = |s_e| / p and delta s_e = 1e-5 |s_e| -- as small as scores of this size allow.
    rho <= 1e-3 is out of reach for ANY operands with such scores; the case is held to LARGE_RHO_MAX."""
    rowptr, col = graph()
    rng = np.random.default_rng(77)
    width, p = heads * d, 1.0 / np.sqrt(d)
    q = (0.25 * np.abs(rng.standard_normal((N, width))) + 1.0).astype(np.float32)
    k0 = 0.25 * np.abs(rng.standard_normal((N, width))) + 1.0
    f = np.stack([rng.permutation(np.linspace(-1.0, 1.0, N)) for _ in range(heads)], 1)
    k = (k0 * np.repeat(f, d, axis=1)).astype(np.float32)
    top = float(np.abs(ref.mha(rowptr, col, q, k, k, heads, p)["s"]).max())
    k = (k.astype(np.float64) * (200.0 / top)).astype(np.float32)
    case = Case("large", rowptr, col, q, k, normal((N, width), 78), normal((N, width), 79), heads, p, kind="large", rho_max=LARGE_RHO_MAX)
    s = case.ref["s"]
    assert s.max() > 150 and s.min() < -150
    spread = np.zeros(case.m)
    np.maximum.at(spread, case.ref["row"], np.abs(s).max(1))
    assert (spread > 150).sum() > case.m // 4                               # in real rows, not in one
    return case


@functools.lru_cache(maxsize=None)
def single_case(heads=4, d=8):
    """Every row has one entry or none, |s| > 30.  z_i = v_j bit for bit whatever the score; lse is the score."""
    rng = np.random.default_rng(5)
    deg = (np.arange(N) % 5 != 0).astype(np.int64)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, N, size=int(deg.sum()))
    width = heads * d
    case = Case("single", rowptr, col, normal((N, width), 6, 3.5), normal((N, width), 7, 3.5), normal((N, width), 9, 3.5),
                normal((N, width), 8), heads, 1.0 / np.sqrt(d), kind="single")
    assert np.abs(case.ref["s"]).max() > 30
    return case


def config_cases():
    return [config_case(h, d) for h, d in CONFIGS]


def scale_cases():
    return [config_case(8, 8, s) for s in SCALES]


def all_cases():
    return config_cases() + scale_cases() + [large_case(), single_case()]
