"""Inputs of the 16-bit multi-head attention tests (tests/test_mha16_host.py, tests/test_gpu_mha16.py), with their fp64 reference
(tests/mha_ref.py, on the widened operands) and bounds (tests/mha16_ref.py) computed once per case and shared, unchanged.

The kernels (isplib_amd/csrc/mha16.hip) take the mapping of gatv2_16.hip, so the configurations are those of tests/gat16_cases.py: the
first, last and a ragged width of every LPR (H == 1), heads of one lane (d = 8) up to half a slot, head counts that are no power of two
(lanes past K inside the slot).  Every configuration runs in bf16, FP16_CONFIGS (one per LPR) in fp16, on the 200 x 200 graph of
tests/attention_cases.py; GRAPH2_CONFIGS also on attention16_cases.graph2, whose row lengths sit at the edges of G and of a step.
Operands are mha_cases' draws (q, k, v, g as 1.2 N(0, 1) with the seeds 1000 H + d + {1, 2, 3, 4}, p = 1 / sqrt(d)), rounded by
half_ref.to16; the large, single, shared (k is v), zero-q and rectangular cases are mha_cases', rounded.  Every case asserts its rho cap
when it is built (RHO_MAX; the large case LARGE_RHO_MAX): the bound is first order in rho.  The caps are conditions on the inputs, not
measurements of the kernels: for the rounded operands the worst rho of the configuration cases is 7.19e-4 at (1, 512) in bf16 (|s|
below 10.3), of the large case 2.44e-3 (scores beyond +-150 in 179 of 200 rows), of the single case 7.5e-4 (|s| up to 63).
"""
import functools

import numpy as np
import torch

from tests import attention16_cases
from tests import gat16_cases
from tests import half_ref
from tests import mha16_ref as ref16
from tests import mha_cases
from tests import mha_ref as ref
from tests import rect_cases

CONFIGS = gat16_cases.CONFIGS
FP16_CONFIGS = gat16_cases.FP16_CONFIGS
GRAPH2_CONFIGS = gat16_cases.GRAPH2_CONFIGS
RECT_CONFIGS = ((1, 46), (8, 8))
FUSED_CONFIGS = ((8, 16), (1, 46))
DTYPES = (torch.bfloat16, torch.float16)
OUTPUTS = ("z", "lse", "dq", "D", "dk", "dv")
OUT16 = ("z", "dq", "dk", "dv")
N = mha_cases.N
RHO_MAX = ref.RHO_MAX
LARGE_RHO_MAX = mha_cases.LARGE_RHO_MAX
lanes_per_row = gat16_cases.lanes_per_row
dtype_name = attention16_cases.dtype_name
as_array = attention16_cases.as_array


def graphs():
    return {"g1": mha_cases.graph(), "g2": attention16_cases.graph2()}


class Case16:
    """One case: the 16-bit operands (CPU tensors q16, k16, v16, g16; v16 is k16 where `shared`), their widened fp32 arrays (q, k, v,
    g), the fp64 reference `ref`, the fp32 bound `b32` and the 16-bit bound `bound`.  mha_cases.Case asserts the rho cap when it is
    built."""

    def __init__(self, name, rowptr, col, q32, k32, v32, g32, heads, p, dtype, kind="bounded", rho_max=RHO_MAX):
        self.name, self.dtype, self.kind, self.rho_max = f"{name}-{dtype_name(dtype)}", dtype, kind, rho_max
        self.shared = v32 is k32
        self.q16, self.k16, self.g16 = half_ref.to16(q32, dtype), half_ref.to16(k32, dtype), half_ref.to16(g32, dtype)
        self.v16 = self.k16 if self.shared else half_ref.to16(v32, dtype)
        kw = half_ref.widen(self.k16)
        base = mha_cases.Case(self.name, rowptr, col, half_ref.widen(self.q16), kw, kw if self.shared else half_ref.widen(self.v16),
                              half_ref.widen(self.g16), heads, p, kind, rho_max)
        self.rowptr, self.col, self.q, self.k, self.v, self.g = base.rowptr, base.col, base.q, base.k, base.v, base.g
        self.heads, self.p, self.ref, self.b32 = base.heads, base.p, base.ref, base.bound
        self.m, self.n, self.width, self.d, self.live = base.m, base.n, base.width, base.d, base.live
        self.bound = ref16.bounds16(rowptr, col, self.q, self.k, self.v, self.heads, self.p, self.ref, self.b32, self.g, dtype)
        assert float(self.bound["rho"].max()) <= rho_max, (self.name, float(self.bound["rho"].max()))


def _rounded(c, dtype, kind="bounded", rho_max=RHO_MAX):
    """A case of mha_cases with its operands rounded to the dtype."""
    k32 = np.array(c.k)
    return Case16(c.name, c.rowptr, c.col, np.array(c.q), k32, k32 if c.v is c.k else np.array(c.v), np.array(c.g), c.heads, c.p, dtype,
                  kind, rho_max)


@functools.lru_cache(maxsize=None)
def config_case(heads, d, dtype=torch.bfloat16, graph="g1"):
    """mha_cases.config_case's draws, rounded to the dtype."""
    rowptr, col = graphs()[graph]
    k, seed, normal = heads * d, 1000 * heads + d, mha_cases.normal
    return Case16(f"h{heads}d{d}-{graph}", rowptr, col, normal((N, k), seed + 1), normal((N, k), seed + 2), normal((N, k), seed + 3),
                  normal((N, k), seed + 4), heads, 1.0 / np.sqrt(d), dtype)


@functools.lru_cache(maxsize=None)
def shared_case(heads, d, dtype=torch.bfloat16):
    """k is v: mha_cases.shared_case's operands, rounded."""
    rowptr, col = mha_cases.graph()
    k, seed, normal = heads * d, 1000 * heads + d, mha_cases.normal
    k32 = normal((N, k), seed + 2)
    return Case16(f"h{heads}d{d}kv", rowptr, col, normal((N, k), seed + 1), k32, k32, normal((N, k), seed + 4), heads, 1.0 / np.sqrt(d),
                  dtype)


@functools.lru_cache(maxsize=None)
def zero_q_case(heads, d, dtype=torch.bfloat16):
    """q = 0: every score is 0, the weights are 1 / deg, lse = log deg."""
    return _rounded(mha_cases.zero_q_case(heads, d), dtype)


@functools.lru_cache(maxsize=None)
def rect_case(shape, heads, d, dtype=torch.bfloat16):
    """The 233 x 67 and 67 x 233 graphs of tests/rect_cases.py with mha_cases.rect_case's seeds."""
    (m, n), (rowptr, col) = rect_cases.SHAPES[shape], rect_cases.graph(shape)
    k, seed, normal = heads * d, 50000 * (1 + rect_cases.SEEDS[shape]) + 1000 * heads + d, mha_cases.normal
    return Case16(f"{shape}-h{heads}d{d}", rowptr, col, normal((m, k), seed + 1), normal((n, k), seed + 2), normal((n, k), seed + 3),
                  normal((m, k), seed + 4), heads, 1.0 / np.sqrt(d), dtype)


@functools.lru_cache(maxsize=None)
def large_case(dtype=torch.bfloat16):
    """mha_cases.large_case (scores spread beyond +-150 in real rows), rounded to the dtype."""
    case = _rounded(mha_cases.large_case(), dtype, kind="large", rho_max=LARGE_RHO_MAX)
    s = case.ref["s"]
    assert s.max() > 150 and s.min() < -150
    return case


@functools.lru_cache(maxsize=None)
def single_case(dtype=torch.bfloat16):
    """mha_cases.single_case (one entry per row or none, |s| > 30), rounded to the dtype."""
    case = _rounded(mha_cases.single_case(), dtype, kind="single")
    assert np.abs(case.ref["s"]).max() > 30
    return case


def config_cases():
    """(heads, d, dtype, graph) of every bounded configuration case."""
    return ([(h, d, torch.bfloat16, "g1") for h, d in CONFIGS] + [(h, d, torch.float16, "g1") for h, d in FP16_CONFIGS] +
            [(h, d, torch.bfloat16, "g2") for h, d in GRAPH2_CONFIGS])


def special_cases():
    """The large and the single case in both dtypes, the shared and the zero-q case, the rectangular cases."""
    return ([large_case(dt) for dt in DTYPES] + [single_case(dt) for dt in DTYPES] + [shared_case(8, 8), zero_q_case(8, 8)] +
            [rect_case(shape, h, d) for shape in rect_cases.SHAPES for h, d in RECT_CONFIGS])


def case_id(spec):
    h, d, dtype, graph = spec
    return f"h{h}d{d}-{dtype_name(dtype)}-{graph}"


def referenced(case):
    """The columns that at least one stored entry references."""
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
