"""Inputs and references shared by tests/test_gpu_rows16_gcn.py and tests/test_rows16_gcn_host.py: the 16-bit row kernel with an
epilogue (fusedMM_csr_rows16_epilogue_hip),

    z[i,c] = round16( act( rs_i * ( sum_e cs[col[e]] * y[col[e],c] + ss_i * y[i,c] ) + bias[c] ) ).

Both graphs are SQUARE (the self term reads y[i]); the tables are those of tests/rows16_colscale_cases.py at n = m."""
import numpy as np

from tests import cases
from tests import rows16_colscale_cases as cs
from tests.rows16_colscale_cases import LONG_ROW, U, integer_scale, scale_table, special_scale  # noqa: F401  (re-exported)

N_HUB = 300


def hub_graph():
    """300 x 300, three empty rows, duplicates, and a hub row of 2,500 edges: beyond long_row = 2048, so it runs phase 2."""
    return cases.random_csr(N_HUB, N_HUB, 12, 31, empty_rows=(0, 150, 299), hub=(7, 2500), duplicates=True)


def length_degrees():
    return cs.length_degrees()


def length_graph():
    """One row per length of test_gpu_rows16._edge_degrees(), each twice; as many columns as rows."""
    deg = length_degrees()
    return cases.csr_of_degrees(deg, len(deg), 17)


def row_scale_table(m, seed=43):
    """Factors in {+-0.5, +-1, +-2}: a product with them is exact."""
    return np.random.default_rng(seed).choice(np.array([-2, -1, -0.5, 0.5, 1, 2], np.float32), m).astype(np.float32)


def integer_bias(k, seed=47):
    return np.random.default_rng(seed).integers(-3, 4, k).astype(np.float32)


def real_bias(k, seed=53):
    return (np.random.default_rng(seed).random(k, np.float32) - np.float32(0.5)).astype(np.float32)


def segment_sum(rowptr, vals):
    """out[i] = +0.0 + the sum of vals[rowptr[i]:rowptr[i+1]] (fp64): a sum that starts from +0.0, as the kernel's does, is -0.0 never."""
    out = np.zeros((rowptr.size - 1,) + vals.shape[1:], np.float64)
    rows = np.flatnonzero(np.diff(rowptr) > 0)
    if rows.size:
        out[rows] = np.add.reduceat(vals.astype(np.float64), rowptr[rows], axis=0) + 0.0
    return out


def relu(v):
    """The kernel's ReLU, v > 0 ? v : 0: -0.0 and NaN give +0.0."""
    return np.where(v > 0, v, np.zeros((), v.dtype))


def formula64(rowptr, col, x, col_scale=None, self_scale=None, row_scale=None, bias=None, act=False):
    """(ref, mag) in fp64 on the widened operand x: the formula above before round16, and
    mag = |rs_i| * (sum_e |cs x| + |ss_i x_i|) + |b|, the magnitude its 1e-5 parity tolerance is taken from."""
    x = np.asarray(x, np.float64)
    w = np.ones(col.size) if col_scale is None else np.asarray(col_scale, np.float64)[col]
    with np.errstate(invalid="ignore", over="ignore"):
        prod = w[:, None] * x[col]
        ref, mag = segment_sum(rowptr, prod), segment_sum(rowptr, np.abs(prod))
        if self_scale is not None:
            own = np.asarray(self_scale, np.float64)[:, None] * x[:rowptr.size - 1]
            ref, mag = ref + own, mag + np.abs(own)
        if row_scale is not None:
            rs = np.asarray(row_scale, np.float64)[:, None]
            ref, mag = ref * rs, mag * np.abs(rs)
        if bias is not None:
            ref, mag = ref + np.asarray(bias, np.float64), mag + np.abs(np.asarray(bias, np.float64))
        if act:
            ref = relu(ref)
    return ref, mag


def epilogue_emulation(agg32, x32, self_scale=None, row_scale=None, bias=None, act=False):
    """The epilogue in the kernel's own order on a finished fp32 sum `agg32`: one fma(ss_i, x[i,c], sum) (the product of an fp32 and a
    16-bit value is exact in fp64, the sum is rounded once to fp32), * rs_i, + bias[c], v > 0 ? v : 0 -- every step rounded to fp32."""
    v = np.asarray(agg32, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        if self_scale is not None:
            v = (self_scale.astype(np.float64)[:, None] * x32[:v.shape[0]].astype(np.float64) + v.astype(np.float64)).astype(np.float32)
        if row_scale is not None:
            v = (v * row_scale.astype(np.float32)[:, None]).astype(np.float32)
        if bias is not None:
            v = (v + bias.astype(np.float32)).astype(np.float32)
        if act:
            v = relu(v)
    return v


def transpose_csr(rowptr, col, n):
    """(colptr, row_t) of the CSR's transpose, entries of a column in ascending row order."""
    rows = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    colptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=colptr[1:])
    return colptr, rows[order]


# the member sets of the integer test: all on, and each member absent in turn
MEMBER_SETS = ("all", "no_col_scale", "no_self_scale", "no_row_scale", "no_bias")


def integer_members(which, m, k):
    """{col_scale, self_scale, row_scale, bias} of the integer cases: integers in [-5, 5] (col, self), {+-0.5, +-1, +-2} (row),
    integers in [-3, 3] (bias); `which` names the member left out."""
    members = {"col_scale": integer_scale(m, 29), "self_scale": integer_scale(m, 31), "row_scale": row_scale_table(m), "bias": integer_bias(k)}
    if which != "all":
        members[which[3:]] = None
    return members
