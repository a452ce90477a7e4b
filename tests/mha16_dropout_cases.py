"""Inputs of the 16-bit multi-head attention dropout tests (tests/test_mha16_dropout_host.py, tests/test_gpu_mha16_dropout.py), with
their fp64 reference (tests/mha_dropout_ref.py, on the widened operands) and bounds (tests/mha16_dropout_ref.py) computed once per case
and shared, unchanged.

Built on tests/mha16_cases.py -- the 200 x 200 graphs and the 67 x 233 / 233 x 67 rectangles, its 16-bit operands and its forward
references (a_e, lse and the scores do not depend on the mask, so they are taken from the base case) -- plus a dropout probability p and
a seed, as tests/mha_dropout_cases.py is built on tests/mha_cases.py.  Conditions on the INPUTS, asserted when a case is built, none a
measurement of the kernels: the base case's rho cap (mha16_cases asserts it; rho is a property of the unmasked scores, the mask does not
enter it) and again here on the dropout bound's own rho; the mask keeps some entries and drops some; on (8, 8) some live (row, head) is
fully dropped at each p; for the duplicate and the position case the reference under the wrong mask misses the true one by more than ten
16-bit bounds somewhere (seeds are searched until it does).
"""
import functools

import numpy as np
import torch

from tests import gat_edge_cases
from tests import mha16_cases as c16
from tests import mha16_dropout_ref as ref16
from tests import mha_dropout_cases as c32
from tests import mha_dropout_ref as ref
from tests import rect_cases

CONFIGS, FP16_CONFIGS, GRAPH2_CONFIGS = c16.CONFIGS, c16.FP16_CONFIGS, c16.GRAPH2_CONFIGS
FORM_CONFIGS = ((1, 46), (8, 8), (3, 128))            # one head (ragged), heads of one lane, a head of sixteen lanes
RECT_CONFIGS = c16.RECT_CONFIGS
FUSED_CONFIGS = c16.FUSED_CONFIGS
PS = (0.1, 0.6, 0.9)
P = c32.P
SEED = c32.SEED
OUTPUTS, OUT16 = c16.OUTPUTS, c16.OUT16
BF, FP = torch.bfloat16, torch.float16
pair_mask = c32.pair_mask
transposed_positions = c32.transposed_positions
as_array = c16.as_array


class Case:
    """A base case (mha16_cases.Case16) with dropout p under `seed`.  `ps` is the score scale (the base case's p)."""

    def __init__(self, base, p, seed, kind=None):
        self.base, self.p, self.seed, self.dtype = base, float(p), int(seed), base.dtype
        self.name = f"{base.name}-drop{p:g}"
        self.rowptr, self.col, self.q, self.k, self.v, self.g = base.rowptr, base.col, base.q, base.k, base.v, base.g
        self.q16, self.k16, self.v16, self.g16 = base.q16, base.k16, base.v16, base.g16
        self.heads, self.ps, self.kind, self.shared = base.heads, base.p, kind or base.kind, base.shared
        self.m, self.n, self.width, self.d, self.live = base.m, base.n, base.width, base.d, base.live
        self.nnz = self.col.size
        self.threshold, self.scale = ref.threshold(p), float(ref.scale(p))
        self.ref = ref.mha_drop(self.rowptr, self.col, self.q, self.k, self.v, self.heads, self.ps, p, seed, self.g, fwd=base.ref)
        self.b32 = ref.bounds(self.rowptr, self.col, self.q, self.k, self.v, self.heads, self.ps, self.ref, self.g)
        self.bound = self.bound_of(self.ref, self.b32)
        assert float(self.bound["rho"].max()) <= base.rho_max, (self.name, float(self.bound["rho"].max()))
        mask = self.ref["q"]
        assert mask.shape == (self.nnz, self.heads) and mask.any() and not mask.all(), self.name

    def bound_of(self, r, b32):
        return ref16.bounds16(self.rowptr, self.col, self.q, self.k, self.v, self.heads, self.ps, r, b32, self.g, self.dtype)

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
def config_case(heads, d, dtype=BF, graph="g1", p=P, seed=SEED):
    return Case(c16.config_case(heads, d, dtype, graph), p, seed)


def config_specs():
    """(heads, d, dtype, graph) of every configuration case: mha16_cases' CONFIGS in bf16, FP16_CONFIGS in fp16, GRAPH2_CONFIGS on graph2."""
    return c16.config_cases()


case_id = c16.case_id


def p_specs():
    """(heads, d, p): every p at one configuration per head form."""
    return [(h, d, p) for h, d in FORM_CONFIGS for p in PS]


@functools.lru_cache(maxsize=None)
def check_fully_dropped_rows():
    """On (8, 8) some live (row, head) has every entry dropped at each p: z = 0 exactly there, with a finite lse."""
    for p in PS:
        assert config_case(8, 8, BF, "g1", p).all_dropped().any(), p
    return True


@functools.lru_cache(maxsize=None)
def large_case(dtype=BF):
    """mha16_cases.large_case (scores spread beyond +-150 in real rows): its own rho cap."""
    case = Case(c16.large_case(dtype), P, SEED)
    assert case.kind == "large" and case.base.rho_max == c16.LARGE_RHO_MAX
    return case


@functools.lru_cache(maxsize=None)
def single_case(dtype=BF, p=P):
    """One-entry rows (mha16_cases.single_case): a_e = 1, so a kept (row, head) has z = round16(float32(v_j c)) and a dropped one z = 0,
    exactly.  The seed is the first for which some entries are kept and some dropped in every head, some column loses ALL its incoming
    entries in some head (its dv vanishes there) and some column keeps one."""
    base = c16.single_case(dtype)
    for seed in range(1, 1000):
        mask = ref.keep(seed, base.col.size, base.heads, p)
        kept_in = np.zeros((base.n, base.heads), np.int64)
        np.add.at(kept_in, base.col, mask.astype(np.int64))
        has_in = np.bincount(base.col, minlength=base.n) > 0
        if mask.any(0).all() and (~mask).any(0).all() and (kept_in[has_in] == 0).any() and (kept_in[has_in] > 0).any():
            case = Case(base, p, seed, kind="single")
            case.kept_in, case.has_in = kept_in, has_in
            assert np.all(np.diff(case.rowptr) <= 1)
            return case
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def duplicate_case(heads=8, d=8, p=P):
    """The first duplicated (i, j) of the graph: two stored entries of one row with the same column, which only their keep bits tell
    apart.  The seed is the first for which the reference z_i, recomputed with the second entry given the first one's bit, differs from
    the true one by more than ten 16-bit bounds in a head where the bits differ; under the same seed the reference of a mask keyed by
    (i, j) (pair_mask) misses z by more than ten bounds too."""
    base = c16.config_case(heads, d)
    pairs = gat_edge_cases.duplicate_pairs(base.rowptr, base.col)
    assert pairs
    e1, e2 = pairs[0]
    for seed in range(1, 1000):
        mask = ref.keep(seed, base.col.size, heads, p)
        differ = mask[e1] != mask[e2]
        if not differ.any():
            continue
        case = Case(base, p, seed, kind="duplicates")
        i = int(case.ref["row"][e1])
        assert case.ref["row"][e2] == i and case.col[e1] == case.col[e2]
        wrong = np.array(mask)
        wrong[e2] = mask[e1]
        gap = np.abs(ref.per_head(case.with_mask(wrong)["z"], heads)[i] - ref.per_head(case.ref["z"], heads)[i])     # [H, d]
        wide = differ & (gap > 10.0 * ref.per_head(case.bound["z"], heads)[i]).any(1)
        if wide.any():
            keyed = case.with_mask(pair_mask(case))
            assert (np.abs(keyed["z"] - case.ref["z"]) > 10.0 * case.bound["z"]).any()
            case.pairs, case.differ, case.wide, case.row = pairs, differ, wide, i
            return case
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def position_case(heads=8, d=8, p=P):
    """The columns kernel walks the transposed structure and must hash csr2csc[pos], not pos.  The seed is the first for which the
    reference dv AND dk with the mask indexed by the transposed position differ from the true ones by more than ten 16-bit bounds
    somewhere (rows are unsorted and columns interleave, so the two positions differ for almost every entry).  `case.wrong`: that
    reference."""
    base = c16.config_case(heads, d)
    perm = transposed_positions(base.col)
    assert (perm != np.arange(base.col.size)).any()
    for seed in (SEED,) + tuple(range(1, 1000)):
        case = Case(base, p, seed, kind="position")
        wrong = np.empty_like(case.ref["q"])
        wrong[perm] = case.ref["q"]                 # the entry at transposed position t (CSR position perm[t]) gets the bit of position t
        other = case.with_mask(wrong)
        if all((np.abs(other[name] - case.ref[name]) > 10.0 * case.bound[name]).any() for name in ("dk", "dv")):
            case.wrong_mask, case.wrong = wrong, other
            return case
    raise AssertionError("no seed found")


@functools.lru_cache(maxsize=None)
def rect_case(shape, heads, d, dtype=BF, p=P, seed=SEED):
    """M != N: the 233 x 67 and 67 x 233 graphs of tests/rect_cases.py."""
    case = Case(c16.rect_case(shape, heads, d, dtype), p, seed, kind="rect")
    assert (case.m, case.n) == rect_cases.SHAPES[shape] and case.m != case.n
    return case


@functools.lru_cache(maxsize=None)
def shared_case(heads=8, d=8, p=P, seed=SEED):
    """k is v (mha16_cases.shared_case): the one tensor's gradient is dk + dv."""
    case = Case(c16.shared_case(heads, d), p, seed, kind="shared")
    assert case.v16 is case.k16 and case.shared
    return case


@functools.lru_cache(maxsize=None)
def fused_case(heads, d, dtype=BF, p=P, seed=SEED):
    """q, k, v as the three column blocks of one 16-bit [N, 3K] projection (the graph is square): the operands of config_case, laid
    side by side in `case.fused`; the tests pass column views of it, at a pitch of 3K."""
    case = Case(c16.config_case(heads, d, dtype), p, seed, kind="fused")
    assert case.m == case.n
    case.fused = torch.cat([case.q16, case.k16, case.v16], dim=1).contiguous()
    assert tuple(case.fused.shape) == (case.n, 3 * case.width)
    return case


def special_cases():
    """The large and the single case in both dtypes, the duplicate, position and shared cases, the rectangular cases of both shapes."""
    check_fully_dropped_rows()
    return ([large_case(dt) for dt in (BF, FP)] + [single_case(dt) for dt in (BF, FP)] + [duplicate_case(), position_case(), shared_case()] +
            [rect_case(shape, h, d) for shape in rect_cases.SHAPES for h, d in RECT_CONFIGS])


def referenced(case):
    hit = np.zeros(case.n, bool)
    hit[case.col] = True
    return hit


def fractions(case, got, names=OUTPUTS):
    """error / bound per named output, every element; lse and D over the rows that have entries (an empty row's -inf / 0 is compared
    for equality, as an unreferenced column's 0 in dk and dv)."""
    live, out = case.live, {}
    for name in names:
        v = as_array(got[name])
        if name == "lse":
            assert np.all(np.isneginf(v[~live])), "an empty row must have lse = -inf"
        if name in ("D", "dq", "z"):
            assert np.all(v[~live] == 0), f"an empty row must have {name} = 0"
        if name in ("dk", "dv"):
            assert np.all(v[~referenced(case)] == 0), f"a column no entry references must have {name} = 0"
        if name in ("lse", "D"):
            out[name] = ref.worst(v[live], case.ref[name][live], case.bound[name][live])
        else:
            out[name] = ref.worst(v, case.ref[name], case.bound[name])
    return out
