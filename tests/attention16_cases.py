"""Inputs of the 16-bit attention tests (tests/test_attention16_host.py, tests/test_gpu_attention16.py), with their fp64 reference
(tests/attention_ref.py, on the widened operands) and bounds (tests/attention16_ref.py) computed once per case and shared, unchanged.

The kernels (isplib_amd/csrc/attention16.hip) take one wave per row with G = 64 / LPR edge slots; LPR is 4 / 8 / 16 / 32 / 64 for K up
to 32 / 64 / 128 / 256 / 512, always one 16-byte chunk of eight columns per lane.  The forward takes U = 4 gathers per slot and step,
the two backward kernels U = 2 at LPR = 4 and 4 elsewhere.  WIDTHS holds the first, last and a ragged width of every slot, and 16 and
24 inside the narrowest.  Two graphs of 200 x 200, built the same way (attention_cases.graph): the imported one has row lengths and
in-degrees 0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129 and a hub of 1000; the second adds 15, 16, 17 (G - 1, G, G + 1 of G = 16) and
31, 32, 33 (the edges of a step of G * U = 32 edges).  Operands are attention_cases.features rounded to the dtype by half_ref.to16.
"""
import functools

import numpy as np
import torch

from tests import attention16_ref as ref16
from tests import attention_cases as cases
from tests import half_ref

WIDTHS = (8, 10, 16, 24, 30, 32, 34, 64, 66, 128, 130, 256, 258, 510, 512)
DTYPES = (torch.bfloat16, torch.float16)
LENGTHS2 = (0, 1, 15, 16, 17, 31, 32, 33, 2, 66)
HUB2 = 300
N, HALF = cases.N, cases.HALF


def slots(k):
    """G = 64 / LPR of the instantiation that serves width k."""
    w = (k + 7) // 8
    return 16 if w <= 4 else 8 if w <= 8 else 4 if w <= 16 else 2 if w <= 32 else 1


def dtype_name(dtype):
    return {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype]


def lengths2():
    out = [LENGTHS2[t % len(LENGTHS2)] for t in range(HALF)]
    out[HALF - 1] = HUB2
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def graph2(seed=1):
    """attention_cases.graph's construction with the lengths of lengths2(): rows 0..99 have exactly these lengths (columns drawn from
    0..99), columns 100..199 exactly these in-degrees (rows drawn from 100..199); drawn with replacement, in drawing order."""
    rng = np.random.default_rng(1000 + seed)
    lens = lengths2()
    rows = [np.repeat(np.arange(HALF), lens), rng.integers(HALF, N, size=int(lens.sum()))]
    cols = [rng.integers(0, HALF, size=int(lens.sum())), np.repeat(np.arange(HALF, N), lens)]
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = np.argsort(row, kind="stable")
    row, col = row[order], col[order]
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=N), out=rowptr[1:])
    assert np.array_equal(np.diff(rowptr)[:HALF], lens) and np.array_equal(np.bincount(col, minlength=N)[HALF:], lens)
    rowptr.setflags(write=False)
    col.setflags(write=False)
    return rowptr, col


def graphs():
    return {"g1": cases.graph(), "g2": graph2()}


class Case16:
    """One case: the 16-bit operands (CPU tensors x16, y16, g16), their widened fp32 arrays (x, y, g), the fp64 reference `ref`, the
    fp32 bound `b32` and the 16-bit bound `bound`."""

    def __init__(self, name, rowptr, col, x32, y32, g32, p, dtype, kind="bounded"):
        self.name, self.dtype, self.kind = f"{name}-{dtype_name(dtype)}", dtype, kind
        self.x16, self.y16, self.g16 = (half_ref.to16(a, dtype) for a in (x32, y32, g32))
        base = cases.Case(self.name, rowptr, col, half_ref.widen(self.x16), half_ref.widen(self.y16), half_ref.widen(self.g16), p, kind)
        self.rowptr, self.col, self.x, self.y, self.g, self.p = base.rowptr, base.col, base.x, base.y, base.g, base.p
        self.ref, self.b32 = base.ref, base.bound
        self.bound = ref16.bounds16(rowptr, col, self.x, self.y, self.p, self.ref, self.b32, self.g, dtype)

    @property
    def m(self):
        return self.rowptr.size - 1

    @property
    def k(self):
        return self.x.shape[1]

    @property
    def live(self):
        return np.diff(self.rowptr) > 0


@functools.lru_cache(maxsize=None)
def width_case(k, dtype, graph="g1"):
    """Real-valued operands at width k, p = 1 / sqrt(k), on one of the two graphs."""
    rowptr, col = graphs()[graph]
    return Case16(f"k{k}-{graph}", rowptr, col, cases.features(N, k, 10 + k), cases.features(N, k, 20 + k), cases.features(N, k, 30 + k),
                  1.0 / np.sqrt(k), dtype)


@functools.lru_cache(maxsize=None)
def large_case(dtype, k=34):
    """attention_cases.large_case (scores spread over +-200) at an even ragged width, its operands rounded to the dtype."""
    c = cases.large_case(k)
    return Case16("large", c.rowptr, c.col, c.x, c.y, c.g, c.p, dtype, kind="large")


@functools.lru_cache(maxsize=None)
def single_case(dtype, k=34):
    """attention_cases.single_case (one entry per row or none, |s| of several thousand), its operands rounded to the dtype."""
    c = cases.single_case(k)
    case = Case16("single", c.rowptr, c.col, c.x, c.y, c.g, c.p, dtype, kind="single")
    assert np.abs(case.ref["s"]).max() > 5e3
    return case


def bounded_cases():
    return [width_case(k, dtype, graph) for k in WIDTHS for dtype in DTYPES for graph in ("g1", "g2")]


def worst(got, want, bound):
    from tests import attention_ref
    return attention_ref.worst(got, want, bound)


def as_array(v):
    """A tensor (any dtype, any device) or an array as an fp64 array."""
    if isinstance(v, torch.Tensor):
        return v.detach().to(torch.float32).cpu().numpy().astype(np.float64)
    return np.asarray(v, dtype=np.float64)


def fractions(case, got, names=("z", "lse", "dx", "dy", "D")):
    """error / bound per named output; lse and D over the rows that have entries (an empty row's -inf / 0 is compared for equality)."""
    live, out = case.live, {}
    for name in names:
        v = as_array(got[name])
        if name == "lse":
            assert np.all(np.isneginf(v[~live])), "an empty row must have lse = -inf"
        if name == "D":
            assert np.all(v[~live] == 0), "an empty row must have D = 0"
        if name in ("lse", "D"):
            out[name] = worst(v[live], case.ref[name][live], case.bound[name][live])
        else:
            out[name] = worst(v, case.ref[name], case.bound[name])
    return out
