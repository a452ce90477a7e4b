"""Inputs of the 16-bit GATv2 tests (tests/test_gatv2_16_host.py, tests/test_gpu_gatv2_16.py), with their fp64 reference
(tests/gatv2_ref.py, on the widened operands) and bounds (tests/gatv2_16_ref.py) computed once per case and shared, unchanged.

The kernels (isplib_amd/csrc/gatv2_16.hip) take the mapping of gat16.hip, so the configurations are those of tests/gat16_cases.py: the
first, last and a ragged width of every LPR (H == 1), heads of one lane (d = 8) up to half a slot, head counts that are no power of two
(lanes past K inside the slot).  Every configuration runs in bf16, FP16_CONFIGS (one per LPR) in fp16, on the 200 x 200 graph of
tests/attention_cases.py; GRAPH2_CONFIGS also on attention16_cases.graph2, whose row lengths sit at the edges of G and of a step.
Operands are gatv2_cases' draws (x, y, g as 1.2 N(0, 1), att as N(0, 1) / sqrt(d) in fp32), x, y and g rounded by half_ref.to16.
Every case asserts its rho cap when it is built (RHO_MAX; the large case LARGE_RHO_MAX): the bound is first order in rho.
"""
import functools

import numpy as np
import torch

from tests import attention16_cases
from tests import gat16_cases
from tests import gatv2_16_ref as ref16
from tests import gatv2_cases
from tests import gatv2_ref as ref
from tests import half_ref

CONFIGS = gat16_cases.CONFIGS
FP16_CONFIGS = gat16_cases.FP16_CONFIGS
GRAPH2_CONFIGS = gat16_cases.GRAPH2_CONFIGS
SLOPE_CONFIGS = gat16_cases.SLOPE_CONFIGS
DTYPES = (torch.bfloat16, torch.float16)
OUTPUTS = ("z", "lse", "dx", "D", "dy", "datt")
N = gatv2_cases.N
RHO_MAX = ref.RHO_MAX
LARGE_RHO_MAX = gatv2_cases.LARGE_RHO_MAX
lanes_per_row = gat16_cases.lanes_per_row
dtype_name = attention16_cases.dtype_name
as_array = attention16_cases.as_array


def graphs():
    return {"g1": gatv2_cases.graph(), "g2": attention16_cases.graph2()}


class Case16:
    """One case: the 16-bit operands (CPU tensors x16, y16, g16), their widened fp32 arrays (x, y, g), the fp32 att, the fp64 reference
    `ref`, the fp32 bound `b32` and the 16-bit bound `bound`.  gatv2_cases.Case asserts the rho cap when it is built."""

    def __init__(self, name, rowptr, col, x32, y32, att, g32, heads, ns, dtype, kind="bounded", rho_max=RHO_MAX):
        self.name, self.dtype, self.kind, self.rho_max = f"{name}-{dtype_name(dtype)}", dtype, kind, rho_max
        self.x16, self.y16, self.g16 = half_ref.to16(x32, dtype), half_ref.to16(y32, dtype), half_ref.to16(g32, dtype)
        base = gatv2_cases.Case(self.name, rowptr, col, half_ref.widen(self.x16), half_ref.widen(self.y16), np.array(att, np.float32),
                                half_ref.widen(self.g16), heads, ns, kind, rho_max)
        self.rowptr, self.col, self.x, self.y, self.att, self.g = base.rowptr, base.col, base.x, base.y, base.att, base.g
        self.heads, self.ns, self.ref, self.b32 = base.heads, base.ns, base.ref, base.bound
        self.m, self.n, self.k, self.live = base.m, base.n, base.k, base.live
        self.bound = ref16.bounds16(rowptr, col, self.x, self.y, self.att, self.heads, self.ns, self.ref, self.b32, self.g, dtype)
        assert float(self.bound["rho"].max()) <= rho_max, (self.name, float(self.bound["rho"].max()))


@functools.lru_cache(maxsize=None)
def config_case(heads, d, dtype=torch.bfloat16, ns=0.2, graph="g1"):
    """gatv2_cases.config_case's draws, x, y and g rounded to the dtype."""
    rowptr, col = graphs()[graph]
    k, seed = heads * d, 1000 * heads + d + int(round(ns * 10)) * 100000
    att = (np.random.default_rng(seed + 5).standard_normal((heads, d)) / np.sqrt(d)).astype(np.float32)
    normal = gatv2_cases.normal
    return Case16(f"h{heads}d{d}ns{ns:g}-{graph}", rowptr, col, normal((N, k), seed + 1), normal((N, k), seed + 2), att,
                  normal((N, k), seed + 4), heads, ns, dtype)


@functools.lru_cache(maxsize=None)
def large_case(dtype=torch.bfloat16):
    """gatv2_cases.large_case (scores spread beyond +-150 in real rows), x, y and g rounded to the dtype."""
    c = gatv2_cases.large_case()
    case = Case16("large", c.rowptr, c.col, np.array(c.x), np.array(c.y), c.att, np.array(c.g), c.heads, c.ns, dtype, kind="large",
                  rho_max=LARGE_RHO_MAX)
    s = case.ref["s"]
    assert s.max() > 150 and s.min() < -150
    return case


@functools.lru_cache(maxsize=None)
def single_case(dtype=torch.bfloat16):
    """gatv2_cases.single_case (one entry per row or none), x, y and g rounded to the dtype."""
    c = gatv2_cases.single_case()
    case = Case16("single", c.rowptr, c.col, np.array(c.x), np.array(c.y), c.att, np.array(c.g), c.heads, c.ns, dtype, kind="single")
    assert np.abs(case.ref["s"]).max() > 30
    return case


def config_cases():
    """(heads, d, dtype, graph) of every bounded configuration case."""
    return ([(h, d, torch.bfloat16, "g1") for h, d in CONFIGS] + [(h, d, torch.float16, "g1") for h, d in FP16_CONFIGS] +
            [(h, d, torch.bfloat16, "g2") for h, d in GRAPH2_CONFIGS])


def slope_cases():
    return [config_case(h, d, torch.bfloat16, ns) for h, d in SLOPE_CONFIGS for ns in (0.0, 1.0)]


def special_cases():
    return slope_cases() + [large_case(), single_case()]


def case_id(spec):
    h, d, dtype, graph = spec
    return f"h{h}d{d}-{dtype_name(dtype)}-{graph}"


def fractions(case, got, names=OUTPUTS):
    """error / bound per named output, every element; lse and D over the rows that have entries (an empty row's -inf / 0 is compared
    for equality)."""
    live, out = case.live, {}
    for name in names:
        v = as_array(got[name])
        if name == "lse":
            assert np.all(np.isneginf(v[~live])), "an empty row must have lse = -inf"
        if name in ("D", "dx"):
            assert np.all(v[~live] == 0), f"an empty row must have {name} = 0"
        if name in ("lse", "D"):
            out[name] = ref.worst(v[live], case.ref[name][live], case.bound[name][live])
        else:
            out[name] = ref.worst(v, case.ref[name], case.bound[name])
    return out
