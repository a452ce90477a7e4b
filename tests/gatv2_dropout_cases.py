"""Inputs of the GATv2 dropout tests (tests/test_gatv2_dropout_host.py, tests/test_gpu_gatv2_dropout.py), with their reference and
bounds computed once per case (tests/gatv2_dropout_ref.py) and shared, unchanged, by every test that needs them.

Built on tests/gatv2_cases.py: the 200 x 200 graph (every row length, a hub of 1000, duplicates, unsorted rows), its operands and its
forward references (a_e, lse and the scores do not depend on the mask, so they are taken from the base case, not computed again) -- plus
a dropout probability p and a seed.  rho is a property of the unmasked scores, so every case asserts rho <= 1e-3 when it is built, as its
base case does, and that its mask keeps some entries and drops some.
"""
import functools

import numpy as np

from tests import gat_edge_cases, gatv2_cases, rect_cases
from tests import gatv2_dropout_ref as ref

CONFIGS = gatv2_cases.CONFIGS
SLOPES = gatv2_cases.SLOPES
SLOPE_CONFIGS = gatv2_cases.SLOPE_CONFIGS
WIDTH_CONFIGS = ((8, 4), (1, 47), (4, 32), (8, 32), (1, 512))                    # one per width instantiation: LPR 8, 16, 32, 64, 64 x 2
P = 0.6
SEED = 0x1E3779B97F4A7C15


class Case:
    """A base case (gatv2_cases.Case) with dropout p under `seed`."""

    def __init__(self, base, p, seed, kind=None):
        self.base, self.p, self.seed = base, float(p), int(seed)
        self.name = f"{base.name}-p{p:g}"
        self.rowptr, self.col, self.x, self.y, self.att, self.g = base.rowptr, base.col, base.x, base.y, base.att, base.g
        self.heads, self.ns, self.kind = base.heads, base.ns, kind or base.kind
        self.threshold, self.scale = ref.threshold(p), float(ref.scale(p))
        self.ref = ref.gatv2_drop(self.rowptr, self.col, self.x, self.y, self.att, self.heads, self.ns, p, seed, self.g, fwd=base.ref)
        self.bound = ref.bounds(self.rowptr, self.col, self.x, self.y, self.att, self.heads, self.ns, self.ref, self.g)
        assert float(self.bound["rho"].max()) <= ref.RHO_MAX, (self.name, float(self.bound["rho"].max()))
        q = self.ref["q"]
        assert q.shape == (self.nnz, self.heads) and q.any() and not q.all(), self.name

    m = property(lambda self: self.rowptr.size - 1)
    n = property(lambda self: self.y.shape[0])
    k = property(lambda self: self.y.shape[1])
    nnz = property(lambda self: self.col.size)
    live = property(lambda self: np.diff(self.rowptr) > 0)

    def with_mask(self, q):
        """The reference of this case's operands under another mask (a counter-example: what a wrong indexing of the bit would compute)."""
        return ref.gatv2_drop(self.rowptr, self.col, self.x, self.y, self.att, self.heads, self.ns, self.p, self.seed, self.g,
                              fwd=self.base.ref, q=q)

    def all_dropped(self):
        """bool [m, H]: a live row whose entries are all dropped for the head"""
        kept = np.zeros((self.m, self.heads), np.int64)
        np.add.at(kept, self.ref["row"], self.ref["q"].astype(np.int64))
        return self.live[:, None] & (kept == 0)


@functools.lru_cache(maxsize=None)
def config_case(heads, d, ns=0.2, p=P, seed=SEED):
    return Case(gatv2_cases.config_case(heads, d, ns), p, seed)


def config_cases():
    return [config_case(h, d) for h, d in CONFIGS]


@functools.lru_cache(maxsize=None)
def slope_cases():
    """p = 0.1 and p = 0.9 at the three slopes, at one configuration of each head form.  At p = 0.9 the (8, 8) case has live rows with
    an all-dropped head (82 of them): z = 0 exactly there, with a finite lse."""
    out = [config_case(h, d, ns, p) for h, d in SLOPE_CONFIGS for ns in SLOPES for p in (0.1, 0.9)]
    assert config_case(8, 8, 0.2, 0.9).all_dropped().any(1).sum() > 0
    return out


@functools.lru_cache(maxsize=None)
def single_case(heads=4, d=8, ns=0.2, p=P):
    """One-entry rows (gatv2_cases.single_case): a_e = 1, so a kept (row, head) has z = float32(y_j c) and a dropped one z = 0, exactly.
    The seed is the first for which some entries are kept and some dropped in every head, some column loses ALL its incoming entries in
    some head (the value part of its dy vanishes there) and some column keeps one."""
    base = gatv2_cases.single_case(heads, d, ns)
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
    """The first duplicated (i, j) of the graph: two stored entries of one row with the same column, which only their keep bits tell
    apart.  The seed is the first for which the bits of the pair differ in some head; asserted here: the reference z_i, recomputed with
    the second entry given the first one's bit, differs from the true one by more than ten bounds in such a head -- a mask indexed per
    (i, j), or per row, cannot pass."""
    base = gatv2_cases.config_case(heads, d, ns)
    pairs = gat_edge_cases.duplicate_pairs(base.rowptr, base.col)
    assert pairs
    e1, e2 = pairs[0]
    for seed in range(1, 1000):
        q = ref.keep(seed, base.col.size, heads, p)
        differ = q[e1] != q[e2]
        if differ.any():
            break
    else:
        raise AssertionError("no seed found")
    case = Case(base, p, seed, kind="duplicates")
    i = int(case.ref["row"][e1])
    assert case.ref["row"][e2] == i and case.col[e1] == case.col[e2]
    wrong = np.array(q)
    wrong[e2] = q[e1]
    gap = np.abs(ref.per_head(case.with_mask(wrong)["z"], heads)[i] - ref.per_head(case.ref["z"], heads)[i])     # [H, d]
    wide = differ & (gap > 10.0 * ref.per_head(case.bound["z"], heads)[i]).any(1)
    assert wide.any(), (seed, differ)
    case.pairs, case.differ, case.wide, case.row = pairs, differ, wide, i
    return case


def transposed_positions(col):
    """csr2csc of a stable transposition: the CSR position of every entry in column-major order."""
    return np.argsort(col, kind="stable")


@functools.lru_cache(maxsize=None)
def position_case(heads=8, d=8):
    """The columns kernel walks the transposed structure and must hash csr2csc[pos], not pos.  Asserted here: the reference dy with the
    mask indexed by the transposed position differs from the true one by more than ten bounds somewhere (rows are unsorted and columns
    interleave, so the two positions differ for almost every entry)."""
    case = config_case(heads, d)
    perm = transposed_positions(case.col)
    assert (perm != np.arange(case.nnz)).any()
    wrong = np.empty_like(case.ref["q"])
    wrong[perm] = case.ref["q"]                     # the entry at transposed position p (CSR position perm[p]) gets the bit of position p
    gap = np.abs(case.with_mask(wrong)["dy"] - case.ref["dy"])
    assert (gap > 10.0 * case.bound["dy"]).any()
    return case


@functools.lru_cache(maxsize=None)
def rect_case(heads=8, d=8, p=P, seed=SEED):
    """M != N: rect_cases "wide" (67 x 233)."""
    case = Case(rect_cases.gatv2_case("wide", heads, d), p, seed, kind="rect")
    assert (case.m, case.n) == (67, 233)
    return case


def all_cases():
    return config_cases() + slope_cases() + [single_case(), duplicate_case(), position_case(), rect_case()]
