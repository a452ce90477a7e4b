"""Inputs of the GAT dropout tests (tests/test_gat_dropout_host.py, tests/test_gpu_gat_dropout.py), with their reference and bounds
computed once per case (tests/gat_dropout_ref.py) and shared, unchanged, by every test that needs them.

Built on tests/gat_cases.py and tests/gat_edge_cases.py: the 200 x 200 graph (every row length, a hub of 1000, duplicates, unsorted
rows), their operands and their forward references (a_e, lse and the scores do not depend on the mask, so they are taken from the
base case, not computed again) -- plus a dropout probability p and a seed.  Every case asserts rho <= 1e-3 when it is built, as its
base case does, and that its mask keeps some entries and drops some.
"""
import functools

import numpy as np

from tests import gat_cases, gat_edge_cases
from tests import gat_dropout_ref as ref

CONFIGS = gat_cases.CONFIGS
SLOPES = gat_cases.SLOPES
SLOPE_CONFIGS = gat_edge_cases.SLOPE_CONFIGS
EDGE_CONFIGS = ((8, 4), (8, 8), (4, 32), (8, 32), (2, 256), (1, 47), (1, 512))   # the five width instantiations, both head forms
WIDTH_CONFIGS = ((8, 4), (1, 47), (4, 32), (8, 32), (1, 512))                    # one per width instantiation: LPR 8, 16, 32, 64, 64 x 2
P = 0.6
SEED = 0x1E3779B97F4A7C15


class Case:
    """A base case (gat_cases.Case or gat_edge_cases.Case) with dropout p under `seed`."""

    def __init__(self, base, p, seed, kind=None):
        self.base, self.p, self.seed = base, float(p), int(seed)
        self.name = f"{base.name}-p{p:g}"
        self.rowptr, self.col, self.y, self.a_dst, self.a_src, self.g = base.rowptr, base.col, base.y, base.a_dst, base.a_src, base.g
        self.a_edge = getattr(base, "a_edge", None)
        self.heads, self.ns, self.kind = base.heads, base.ns, kind or base.kind
        self.threshold, self.scale = ref.threshold(p), float(ref.scale(p))
        self.ref = ref.gat_drop(self.rowptr, self.col, self.y, self.a_dst, self.a_src, self.a_edge, self.heads, self.ns, p, seed, self.g,
                                fwd=base.ref)
        self.bound = ref.bounds(self.rowptr, self.col, self.y, self.a_dst, self.a_src, self.a_edge, self.heads, self.ns, self.ref, self.g)
        assert float(self.bound["rho"].max()) <= ref.RHO_MAX, (self.name, float(self.bound["rho"].max()))
        q = self.ref["q"]
        assert q.shape == (self.nnz, self.heads) and q.any() and not q.all(), self.name

    m = property(lambda self: self.rowptr.size - 1)
    n = property(lambda self: self.y.shape[0])
    k = property(lambda self: self.y.shape[1])
    nnz = property(lambda self: self.col.size)
    live = property(lambda self: np.diff(self.rowptr) > 0)


@functools.lru_cache(maxsize=None)
def config_case(heads, d, ns=0.2, p=P, seed=SEED):
    return Case(gat_cases.config_case(heads, d, ns), p, seed)


@functools.lru_cache(maxsize=None)
def edge_case(heads, d, ns=0.2, p=P, seed=SEED):
    return Case(gat_edge_cases.config_case(heads, d, ns), p, seed)


def config_cases():
    return [config_case(h, d) for h, d in CONFIGS]


def slope_cases():
    """p = 0.1 and p = 0.9 at the three slopes, at one configuration of each head form."""
    return [config_case(h, d, ns, p) for h, d in SLOPE_CONFIGS for ns in SLOPES for p in (0.1, 0.9)]


def edge_cases():
    return [edge_case(h, d) for h, d in EDGE_CONFIGS]


@functools.lru_cache(maxsize=None)
def single_case(heads=4, d=8, ns=0.2, p=P):
    """One-entry rows (gat_cases.single_case): a_e = 1, so a kept (row, head) has z = float32(y_j c) and a dropped one z = 0, exactly.
    The seed is the first for which some entries are kept and some dropped in every head, some column loses ALL its incoming entries in
    some head (its dy is exactly 0 there) and some column keeps one."""
    base = gat_cases.single_case(heads, d, ns)
    for seed in range(1, 1000):
        q = ref.keep(seed, base.col.size, heads, p)
        kept_in = np.zeros((base.n, heads), np.int64)
        np.add.at(kept_in, base.col, q.astype(np.int64))
        has_in = np.bincount(base.col, minlength=base.n) > 0
        if q.any(0).all() and (~q).any(0).all() and (kept_in[has_in] == 0).any() and (kept_in[has_in] > 0).any():
            case = Case(base, p, seed, kind="single")
            case.kept_in, case.has_in = kept_in, has_in
            return case
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def duplicate_case(heads=8, d=8, ns=0.2, p=P):
    """A duplicated (i, j) whose two stored entries carry the SAME a_edge row, so that only their keep bits tell them apart.  The seed is
    the first for which the bits of the pair differ in some head AND the reference's d a_edge of the two entries differs there by more
    than ten times both bounds (asserted here): a mask indexed per (i, j), or per row, cannot pass."""
    base = gat_edge_cases.config_case(heads, d, ns)
    pairs = gat_edge_cases.duplicate_pairs(base.rowptr, base.col)
    assert pairs
    e1, e2 = pairs[0]
    a_edge = np.array(base.a_edge)
    a_edge[e2] = a_edge[e1]
    same = gat_edge_cases.Case("duplicates-same-edge", base.rowptr, base.col, np.array(base.y), np.array(base.a_dst), np.array(base.a_src),
                               a_edge, np.array(base.g), heads, ns, kind="duplicates")
    for seed in range(1, 1000):
        q = ref.keep(seed, base.col.size, heads, p)
        differ = q[e1] != q[e2]
        if not differ.any():
            continue
        case = Case(same, p, seed, kind="duplicates")
        gap = np.abs(case.ref["daedge"][e1] - case.ref["daedge"][e2])
        wide = differ & (gap > 10.0 * (case.bound["daedge"][e1] + case.bound["daedge"][e2]))
        if wide.any():
            case.pairs, case.differ, case.wide = pairs, differ, wide
            assert np.array_equal(case.a_edge[e1], case.a_edge[e2]) and case.col[e1] == case.col[e2]
            return case
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def rect_case(p=P, seed=SEED):
    """M != N: rect_cases "wide" (67 x 233) with a_edge, as tests/gat_edge_cases.py builds it."""
    case = Case(gat_edge_cases.rect_case(), p, seed, kind="rect")
    assert case.m != case.n
    return case


def all_cases():
    return config_cases() + slope_cases() + edge_cases() + [single_case(), duplicate_case(), rect_case()]
