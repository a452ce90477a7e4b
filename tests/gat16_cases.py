"""Inputs of the 16-bit GAT tests (tests/test_gat16_host.py, tests/test_gpu_gat16.py), with their fp64 reference (tests/gat_ref.py, on
the widened operands) and bounds (tests/gat16_ref.py) computed once per case and shared, unchanged.

The kernels (isplib_amd/csrc/gat16.hip) take one wave per row with G = 64 / LPR edge slots and U = 4 gathers per slot and step; LPR is
4 / 8 / 16 / 32 / 64 for K = H*d up to 32 / 64 / 128 / 256 / 512, always one 16-byte chunk of eight columns per lane.  CONFIGS holds the
first, last and a ragged width of every LPR (H == 1), heads of one lane (d = 8) up to half a slot ((2, 256)), and head counts that are no
power of two ((5, 8), (33, 8), (3, 16), (3, 128): lanes past K inside the slot).  Every configuration runs in bf16, FP16_CONFIGS (one per
LPR) in fp16, on the 200 x 200 graph of tests/attention_cases.py; (8, 8) and (1, 34) also on attention16_cases.graph2, whose row
lengths sit at the edges of G and of a step.  Operands are gat_cases.normal(...) rounded by half_ref.to16; the scores are fp32.
"""
import functools

import numpy as np
import torch

from tests import attention16_cases
from tests import gat16_ref as ref16
from tests import gat_cases
from tests import gat_ref as ref
from tests import half_ref

CONFIGS = tuple((1, d) for d in (8, 10, 30, 32, 34, 46, 64, 66, 130, 258, 510, 512)) + (
    (2, 8), (4, 8), (5, 8), (8, 8), (33, 8), (64, 8), (3, 16), (8, 16), (4, 32), (3, 128), (2, 256), (8, 64))
FP16_CONFIGS = ((1, 10), (8, 8), (8, 16), (1, 130), (3, 128))          # LPR 4, 8, 16, 32, 64
GRAPH2_CONFIGS = ((8, 8), (1, 34))
SLOPE_CONFIGS = ((1, 46), (8, 8), (3, 128))
DTYPES = (torch.bfloat16, torch.float16)
OUTPUTS = ("z", "lse", "dadst", "D", "dy", "dasrc")
N = gat_cases.N
dtype_name = attention16_cases.dtype_name
as_array = attention16_cases.as_array


def lanes_per_row(k):
    """LPR of the instantiation that serves width k."""
    w = (k + 7) // 8
    return 4 if w <= 4 else 8 if w <= 8 else 16 if w <= 16 else 32 if w <= 32 else 64


def graphs():
    return {"g1": gat_cases.graph(), "g2": attention16_cases.graph2()}


class Case16:
    """One case: the 16-bit operands (CPU tensors y16, g16), their widened fp32 arrays (y, g), the fp32 scores, the fp64 reference `ref`,
    the fp32 bound `b32` and the 16-bit bound `bound`.  gat_cases.Case asserts rho <= RHO_MAX when it is built."""

    def __init__(self, name, rowptr, col, y32, a_dst, a_src, g32, heads, ns, dtype, kind="bounded"):
        self.name, self.dtype, self.kind = f"{name}-{dtype_name(dtype)}", dtype, kind
        self.y16, self.g16 = half_ref.to16(y32, dtype), half_ref.to16(g32, dtype)
        base = gat_cases.Case(self.name, rowptr, col, half_ref.widen(self.y16), np.array(a_dst), np.array(a_src), half_ref.widen(self.g16),
                              heads, ns, kind)
        self.rowptr, self.col, self.y, self.a_dst, self.a_src, self.g = base.rowptr, base.col, base.y, base.a_dst, base.a_src, base.g
        self.heads, self.ns, self.ref, self.b32 = base.heads, base.ns, base.ref, base.bound
        self.m, self.n, self.k, self.live = base.m, base.n, base.k, base.live
        self.bound = ref16.bounds16(rowptr, col, self.y, self.a_dst, self.a_src, self.heads, self.ns, self.ref, self.b32, self.g, dtype)
        assert float(self.bound["rho"].max()) <= ref.RHO_MAX, (self.name, float(self.bound["rho"].max()))


@functools.lru_cache(maxsize=None)
def config_case(heads, d, dtype=torch.bfloat16, ns=0.2, graph="g1"):
    """gat_cases.config_case's operands (scores 1.2 * N(0, 1) per node and head), y and g rounded to the dtype."""
    rowptr, col = graphs()[graph]
    k, seed = heads * d, 1000 * heads + d + int(round(ns * 10)) * 100000
    return Case16(f"h{heads}d{d}ns{ns:g}-{graph}", rowptr, col, gat_cases.normal((N, k), seed + 1), gat_cases.normal((N, heads), seed + 2),
                  gat_cases.normal((N, heads), seed + 3), gat_cases.normal((N, k), seed + 4), heads, ns, dtype)


@functools.lru_cache(maxsize=None)
def large_case(dtype=torch.bfloat16):
    """gat_cases.large_case (u spread over +-200), y and g rounded to the dtype."""
    c = gat_cases.large_case()
    case = Case16("large", c.rowptr, c.col, np.array(c.y), c.a_dst, c.a_src, np.array(c.g), c.heads, c.ns, dtype, kind="large")
    assert case.ref["u"].max() > 150 and case.ref["u"].min() < -150
    return case


@functools.lru_cache(maxsize=None)
def single_case(dtype=torch.bfloat16):
    """gat_cases.single_case (one entry per row or none, |u| to 8e3), y and g rounded to the dtype."""
    c = gat_cases.single_case()
    case = Case16("single", c.rowptr, c.col, np.array(c.y), c.a_dst, c.a_src, np.array(c.g), c.heads, c.ns, dtype, kind="single")
    assert np.abs(case.ref["u"]).max() > 5e3
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
        if name in ("D", "dadst"):
            assert np.all(v[~live] == 0), f"an empty row must have {name} = 0"
        if name in ("lse", "D"):
            out[name] = ref.worst(v[live], case.ref[name][live], case.bound[name][live])
        else:
            out[name] = ref.worst(v, case.ref[name], case.bound[name])
    return out
