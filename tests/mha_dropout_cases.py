"""Inputs of the multi-head attention dropout tests (tests/test_mha_dropout_host.py, tests/test_gpu_mha_dropout.py), with their reference
and bounds computed once per case (tests/mha_dropout_ref.py) and shared, unchanged, by every test that needs them.

Built on tests/mha_cases.py: the 200 x 200 graph (every row length, a hub of 1000, 8 empty rows, duplicates, unsorted rows), its operands
and its forward references (a_e, lse and the scores do not depend on the mask, so they are taken from the base case, not computed again)
-- plus a dropout probability p and a seed.  rho is a property of the unmasked scores, so every case asserts rho <= 1e-3 when it is
built, as its base case does, and that its mask keeps some entries and drops some.
"""
import functools

import numpy as np

from tests import gat_edge_cases, mha_cases
from tests import mha_dropout_ref as ref

CONFIGS = mha_cases.CONFIGS
SCALES = mha_cases.SCALES
FORM_CONFIGS = ((1, 47), (8, 8), (3, 128))                                       # one head, heads inside a chunk, a head of a whole chunk
WIDTH_CONFIGS = ((8, 4), (1, 47), (4, 32), (8, 32), (1, 512))                    # one per width instantiation: LPR 8, 16, 32, 64, 64 x 2
FUSED_CONFIGS = mha_cases.FUSED_CONFIGS
P = 0.6
SEED = 0x1E3779B97F4A7C15


class Case:
    """A base case (mha_cases.Case) with dropout p under `seed`.  `ps` is the score scale (the base case's p)."""

    def __init__(self, base, p, seed, kind=None):
        self.base, self.p, self.seed = base, float(p), int(seed)
        self.name = f"{base.name}-drop{p:g}"
        self.rowptr, self.col, self.q, self.k, self.v, self.g = base.rowptr, base.col, base.q, base.k, base.v, base.g
        self.heads, self.ps, self.kind = base.heads, base.p, kind or base.kind
        self.threshold, self.scale = ref.threshold(p), float(ref.scale(p))
        self.ref = ref.mha_drop(self.rowptr, self.col, self.q, self.k, self.v, self.heads, self.ps, p, seed, self.g, fwd=base.ref)
        self.bound = ref.bounds(self.rowptr, self.col, self.q, self.k, self.v, self.heads, self.ps, self.ref, self.g)
        assert float(self.bound["rho"].max()) <= ref.RHO_MAX, (self.name, float(self.bound["rho"].max()))
        mask = self.ref["q"]
        assert mask.shape == (self.nnz, self.heads) and mask.any() and not mask.all(), self.name

    m = property(lambda self: self.rowptr.size - 1)
    n = property(lambda self: self.k.shape[0])
    width = property(lambda self: self.k.shape[1])
    nnz = property(lambda self: self.col.size)
    live = property(lambda self: np.diff(self.rowptr) > 0)

    def with_mask(self, mask):
        """The reference of this case's operands under another mask (a counter-example: what a wrong indexing of the bit would compute)."""
        return ref.mha_drop(self.rowptr, self.col, self.q, self.k, self.v, self.heads, self.ps, self.p, self.seed, self.g,
                            fwd=self.base.ref, mask=mask)

    def all_dropped(self):
        """bool [m, H]: a live row whose entries are all dropped for the head"""
        kept = np.zeros((self.m, self.heads), np.int64)
        np.add.at(kept, self.ref["row"], self.ref["q"].astype(np.int64))
        return self.live[:, None] & (kept == 0)


@functools.lru_cache(maxsize=None)
def config_case(heads, d, scale=None, p=P, seed=SEED):
    return Case(mha_cases.config_case(heads, d, scale), p, seed)


def config_cases():
    return [config_case(h, d) for h, d in CONFIGS]


@functools.lru_cache(maxsize=None)
def scale_cases():
    """p = 0.1 and p = 0.9 at the two explicit score scales of (8, 8) (one is negative) and, with 1 / sqrt(d), at one configuration of
    each head form.  The (8, 8) graph has live (row, head) pairs whose entries are all dropped at every p used here: z = 0 exactly
    there, with a finite lse."""
    out = [config_case(8, 8, s, p) for s in SCALES for p in (0.1, 0.9)]
    out += [config_case(h, d, None, p) for h, d in FORM_CONFIGS for p in (0.1, 0.9)]
    for p in (0.1, P, 0.9):
        assert config_case(8, 8, None, p).all_dropped().any()
    return out


@functools.lru_cache(maxsize=None)
def single_case(heads=4, d=8, p=P):
    """One-entry rows (mha_cases.single_case): a_e = 1, so a kept (row, head) has z = float32(v_j c) and a dropped one z = 0, exactly.
    The seed is the first for which some entries are kept and some dropped in every head, some column loses ALL its incoming entries in
    some head (its dv vanishes there) and some column keeps one."""
    base = mha_cases.single_case(heads, d)
    for seed in range(1, 1000):
        mask = ref.keep(seed, base.col.size, heads, p)
        kept_in = np.zeros((base.n, heads), np.int64)
        np.add.at(kept_in, base.col, mask.astype(np.int64))
        has_in = np.bincount(base.col, minlength=base.n) > 0
        if mask.any(0).all() and (~mask).any(0).all() and (kept_in[has_in] == 0).any() and (kept_in[has_in] > 0).any():
            case = Case(base, p, seed, kind="single")
            case.kept_in, case.has_in = kept_in, has_in
            return case
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def duplicate_case(heads=8, d=8, p=P):
    """The first duplicated (i, j) of the graph: two stored entries of one row with the same column, which only their keep bits tell
    apart.  The seed is the first for which the bits of the pair differ in some head; asserted here: the reference z_i, recomputed with
    the second entry given the first one's bit, differs from the true one by more than ten bounds in such a head -- a mask indexed per
    (i, j), or per row, cannot pass."""
    base = mha_cases.config_case(heads, d)
    pairs = gat_edge_cases.duplicate_pairs(base.rowptr, base.col)
    assert pairs
    e1, e2 = pairs[0]
    for seed in range(1, 1000):
        mask = ref.keep(seed, base.col.size, heads, p)
        differ = mask[e1] != mask[e2]
        if differ.any():
            break
    else:
        raise AssertionError("no seed found")
    case = Case(base, p, seed, kind="duplicates")
    i = int(case.ref["row"][e1])
    assert case.ref["row"][e2] == i and case.col[e1] == case.col[e2]
    wrong = np.array(mask)
    wrong[e2] = mask[e1]
    gap = np.abs(ref.per_head(case.with_mask(wrong)["z"], heads)[i] - ref.per_head(case.ref["z"], heads)[i])     # [H, d]
    wide = differ & (gap > 10.0 * ref.per_head(case.bound["z"], heads)[i]).any(1)
    assert wide.any(), (seed, differ)
    case.pairs, case.differ, case.wide, case.row = pairs, differ, wide, i
    return case


def pair_mask(case):
    """The mask of a lookup keyed by (i, j): every stored entry takes the bit of the FIRST stored entry with its row and column."""
    key = case.ref["row"].astype(np.int64) * case.n + case.col
    _, first = np.unique(key, return_index=True)
    lookup = dict(zip(key[first].tolist(), first.tolist()))
    return case.ref["q"][np.array([lookup[x] for x in key.tolist()])]


def transposed_positions(col):
    """csr2csc of a stable transposition: the CSR position of every entry in column-major order."""
    return np.argsort(col, kind="stable")


@functools.lru_cache(maxsize=None)
def position_case(heads=8, d=8):
    """The columns kernel walks the transposed structure and must hash csr2csc[pos], not pos.  Asserted here: the reference dk or dv with
    the mask indexed by the transposed position differs from the true one by more than ten bounds somewhere (rows are unsorted and
    columns interleave, so the two positions differ for almost every entry)."""
    case = config_case(heads, d)
    perm = transposed_positions(case.col)
    assert (perm != np.arange(case.nnz)).any()
    wrong = np.empty_like(case.ref["q"])
    wrong[perm] = case.ref["q"]                     # the entry at transposed position p (CSR position perm[p]) gets the bit of position p
    other = case.with_mask(wrong)
    assert any((np.abs(other[name] - case.ref[name]) > 10.0 * case.bound[name]).any() for name in ("dk", "dv"))
    assert (np.abs(other["dv"] - case.ref["dv"]) > 10.0 * case.bound["dv"]).any()          # dv is what the GPU test looks at
    return case


@functools.lru_cache(maxsize=None)
def rect_case(heads=8, d=8, p=P, seed=SEED):
    """M != N: rect_cases "wide" (67 x 233)."""
    case = Case(mha_cases.rect_case("wide", heads, d), p, seed, kind="rect")
    assert (case.m, case.n) == (67, 233)
    return case


@functools.lru_cache(maxsize=None)
def shared_case(heads=8, d=8, p=P, seed=SEED):
    """k is v (mha_cases.shared_case): the one tensor's gradient is dk + dv."""
    case = Case(mha_cases.shared_case(heads, d), p, seed, kind="shared")
    assert case.k is case.v
    return case


@functools.lru_cache(maxsize=None)
def fused_case(heads, d, p=P, seed=SEED):
    """q, k, v as the three column blocks of one [N, 3K] projection (the graph is square): the operands of config_case, laid side by
    side in `case.fused`; the tests pass column views of it, at a pitch of 3K."""
    case = Case(mha_cases.config_case(heads, d), p, seed, kind="fused")
    assert case.m == case.n
    case.fused = np.ascontiguousarray(np.concatenate([case.q, case.k, case.v], axis=1))
    assert case.fused.shape == (case.n, 3 * case.width)
    return case


def all_cases():
    return config_cases() + scale_cases() + [single_case(), duplicate_case(), position_case(), rect_case(), shared_case()]
