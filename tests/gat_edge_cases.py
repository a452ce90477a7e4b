"""Inputs of the GAT edge-term tests (tests/test_gat_edge_host.py, tests/test_gpu_gat_edge.py), with their fp64 reference and bounds
computed once per case (tests/gat_edge_ref.py) and shared, unchanged, by every test that needs them.

Built on tests/gat_cases.py: the 200 x 200 graph (every row length, a hub of 1000, duplicates, unsorted rows), every (heads, d) of its
CONFIGS, the three slopes, and its operands -- plus a_edge [nnz, heads], one row per stored entry in CSR position order.  Every case
asserts rho <= 1e-3 when it is built, as gat_cases.Case does: the bound is first order in rho.
"""
import functools

import numpy as np

from tests import gat_cases
from tests import gat_edge_ref as ref
from tests import rect_cases

CONFIGS = gat_cases.CONFIGS
SLOPES = gat_cases.SLOPES
SLOPE_CONFIGS = ((1, 47), (8, 8), (3, 128))
N = gat_cases.N
graph = gat_cases.graph
normal = gat_cases.normal
RECT = ("wide", 8, 8)                   # one rectangular graph of tests/rect_cases.py: 67 rows, 233 columns


class Case:
    def __init__(self, name, rowptr, col, y, a_dst, a_src, a_edge, g, heads, ns, kind="bounded"):
        self.name, self.rowptr, self.col, self.y, self.a_dst, self.a_src, self.a_edge, self.g = name, rowptr, col, y, a_dst, a_src, a_edge, g
        self.heads, self.ns, self.kind = int(heads), float(ns), kind
        assert a_edge.shape == (col.size, self.heads) and a_edge.dtype == np.float32
        self.ref = ref.gat_edge(rowptr, col, y, a_dst, a_src, a_edge, self.heads, self.ns, g)
        self.bound = ref.bounds(rowptr, col, y, a_dst, a_src, a_edge, self.heads, self.ns, self.ref, g)
        assert float(self.bound["rho"].max()) <= ref.RHO_MAX, (name, float(self.bound["rho"].max()))
        for a in (y, a_dst, a_src, a_edge, g):
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
    def nnz(self):
        return self.col.size

    @property
    def live(self):
        return np.diff(self.rowptr) > 0


def _operands(heads, d, ns):
    """The operands of gat_cases.config_case (same seeds), and a_edge = 1.2 * N(0, 1)."""
    rowptr, col = graph()
    k, seed = heads * d, 1000 * heads + d + int(round(ns * 10)) * 100000
    return (rowptr, col, normal((N, k), seed + 1), normal((N, heads), seed + 2), normal((N, heads), seed + 3),
            normal((col.size, heads), seed + 5), normal((N, k), seed + 4))


@functools.lru_cache(maxsize=None)
def config_case(heads, d, ns=0.2):
    rowptr, col, y, a_dst, a_src, a_edge, g = _operands(heads, d, ns)
    return Case(f"h{heads}d{d}ns{ns:g}", rowptr, col, y, a_dst, a_src, a_edge, g, heads, ns)


@functools.lru_cache(maxsize=None)
def edge_only_case(heads=8, d=8, ns=0.2):
    """a_dst = a_src = 0: the score is the edge term alone."""
    rowptr, col, y, a_dst, a_src, a_edge, g = _operands(heads, d, ns)
    return Case("edge-only", rowptr, col, y, np.zeros_like(a_dst), np.zeros_like(a_src), a_edge, g, heads, ns, kind="edge-only")


def duplicate_pairs(rowptr, col):
    """[(e1, e2)]: CSR positions of two stored entries of one row with the same column."""
    out = []
    for i in range(rowptr.size - 1):
        seen = {}
        for e in range(int(rowptr[i]), int(rowptr[i + 1])):
            j = int(col[e])
            if j in seen:
                out.append((seen[j], e))
            else:
                seen[j] = e
    return out


@functools.lru_cache(maxsize=None)
def duplicate_case(heads=8, d=8, ns=0.2):
    """At least one duplicated (i, j) pair carries two different a_edge rows (asserted here): indexing a_edge or d a_edge per (i, j)
    instead of per stored entry cannot pass.  The first pair's second row is the first minus 2 on every head."""
    rowptr, col, y, a_dst, a_src, a_edge, g = _operands(heads, d, ns)
    pairs = duplicate_pairs(rowptr, col)
    assert pairs
    a_edge = np.array(a_edge)
    e1, e2 = pairs[0]
    a_edge[e2] = a_edge[e1] - np.float32(2.0)
    case = Case("duplicates", rowptr, col, y, a_dst, a_src, a_edge, g, heads, ns, kind="duplicates")
    case.pairs = pairs
    assert np.all(case.a_edge[e1] != case.a_edge[e2])
    assert sum(bool(np.any(case.a_edge[p] != case.a_edge[q])) for p, q in pairs) >= 1
    # and the reference tells the two entries apart by more than both bounds
    gap = np.abs(case.ref["daedge"][e1] - case.ref["daedge"][e2])
    assert np.any(gap > 10.0 * (case.bound["daedge"][e1] + case.bound["daedge"][e2]))
    return case


@functools.lru_cache(maxsize=None)
def large_case(heads=8, d=8, ns=0.2):
    """The edge term spread over +-200 in every row, node scores small (1.2 * N(0, 1)): exp of the raw score overflows fp32 from 88.7
    on.  delta s_e <= 3 eps 200 = 3.6e-5 and the range term 8 eps (R + deg + 4) stays below 7e-4 at R = 400 with the hub, so
    rho <= 1e-3 holds."""
    rowptr, col, y, a_dst, a_src, _, g = _operands(heads, d, ns)
    rng = np.random.default_rng(177)
    a_edge = np.stack([rng.permutation(np.linspace(-200.0, 200.0, col.size)) for _ in range(heads)], 1).astype(np.float32)
    case = Case("large", rowptr, col, y, a_dst, a_src, a_edge, g, heads, ns, kind="large")
    assert case.ref["u"].max() > 150 and case.ref["u"].min() < -150 and np.abs(case.ref["u0"]).max() < 15
    return case


@functools.lru_cache(maxsize=None)
def single_case(heads=4, d=8, ns=0.2):
    """Every row has one entry or none (the structure of gat_cases.single_case).  z_i = y_j bit for bit whatever the score, and
    d a_edge = a_e (t_e - D) slope is exactly 0: a_e = 1 and D = t_e bit for bit.  |u| reaches thousands; delta s_e =
    eps |u0| + 2 eps |u| with |u0| <= 4e3 and |u| <= 5e3 stays below 8.4e-4, inside rho <= 1e-3."""
    base = gat_cases.single_case(heads, d, ns)
    rng = np.random.default_rng(15)
    a_dst = rng.uniform(-2000.0, 2000.0, (N, heads)).astype(np.float32)
    a_src = rng.uniform(-2000.0, 2000.0, (N, heads)).astype(np.float32)
    a_edge = rng.uniform(-1000.0, 1000.0, (base.col.size, heads)).astype(np.float32)
    case = Case("single", base.rowptr, base.col, np.array(base.y), a_dst, a_src, a_edge, np.array(base.g), heads, ns, kind="single")
    assert np.abs(case.ref["u"]).max() > 3e3 and int(np.diff(case.rowptr).max()) == 1
    return case


@functools.lru_cache(maxsize=None)
def rect_case(shape=RECT[0], heads=RECT[1], d=RECT[2], ns=0.2):
    """M != N: the graph and operands of rect_cases.gat_case, and a_edge."""
    base = rect_cases.gat_case(shape, heads, d, ns)
    assert base.m != base.n
    a_edge = normal((base.col.size, heads), 61000 + 1000 * heads + d)
    return Case(f"{shape}-h{heads}d{d}", base.rowptr, base.col, np.array(base.y), np.array(base.a_dst), np.array(base.a_src), a_edge,
                np.array(base.g), heads, ns, kind="rect")


def config_cases():
    return [config_case(h, d) for h, d in CONFIGS]


def slope_cases():
    """The three slopes at one configuration of each head form (0.2 is in config_cases): ns = 0 and ns = 1."""
    return [config_case(h, d, ns) for h, d in SLOPE_CONFIGS for ns in SLOPES[1:]]


def all_cases():
    return config_cases() + slope_cases() + [edge_only_case(), duplicate_case(), large_case(), single_case(), rect_case()]
