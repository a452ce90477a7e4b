"""The front end the 16-bit row kernels share (isplib_amd/csrc/rows16_common.h): which row block a workgroup takes and which rows a
last, partly filled workgroup must leave alone.  The workgroups of one launch are dealt to the eight XCDs so that each walks a
contiguous range of row blocks: nb / 8 blocks each, the first nb % 8 XCDs one more.  The other rows16 modules reach that split only
at the row counts their graphs happen to have; here every count of row blocks nb = 1 .. 17 (both sides of 8 and of 16) is taken with a
full last block (m = 4 nb) and with one and three rows missing from it, on all three entries: sum with unit weights, sum with a column
table, max with positions.

bf16 integer features: every fp32 sum is exact in any order (|x| <= 3, factors <= 4, 2,049 edges: below 2^15), so the bar is BIT
EQUALITY with tests/half_ref.py's reference (max: tests/rows16_minmax_cases.reference, values and positions).  K = 8 is one chunk of
the narrowest slot, K = 1026 two chunks per lane and a second, ragged column panel.  Rows hold 2-5 edges, except the last row, 2,049
edges (over long_row: all four waves of its workgroup take it -- in index order that is the partly filled last workgroup, in the
reversed order the first).  Outputs are views of wider buffers: the pad columns beside them must keep their pre-fill."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref, rows16_minmax_cases

pytestmark = pytest.mark.gpu

N, PAD, LONG = 64, 2, 2049
COUNTS = tuple((nb, r) for nb in range(1, 18) for r in (0, 1, 3))
ARG_FILL = -7

_graphs, _refs = {}, {}


def _graph(nb, r):
    if (nb, r) not in _graphs:
        m = 4 * nb - r
        deg = np.random.default_rng(100 * nb + r).integers(2, 6, m)
        deg[m - 1] = LONG
        _graphs[nb, r] = cases.csr_of_degrees(deg, N, 7 * nb + r)
    return _graphs[nb, r]


def _scale():
    return (np.arange(N) % 4 + 1).astype(np.float32)


def _reference(oracle, entry, nb, r, x16):
    """(ref16, positions or None), once per (entry, graph, K), shared and left unchanged."""
    key = (entry, nb, r, x16.size(1))
    if key not in _refs:
        rowptr, col = _graph(nb, r)
        if entry == "max":
            _, ref16, arg = rows16_minmax_cases.reference(oracle, rowptr, col, np.ones(col.size, np.float32), x16, "max")
            arg.setflags(write=False)
        else:
            val = _scale()[col] if entry == "colscale" else np.ones(col.size, np.float32)
            (_, ref16), arg = half_ref.reference(oracle, rowptr, col, val, x16, "sum"), None
        _refs[key] = (half_ref.bits(ref16), arg)
    return _refs[key]


@pytest.mark.parametrize("k", (8, 1026))
@pytest.mark.parametrize("entry", ("unit", "colscale", "max"))
def test_every_count_of_row_blocks_with_a_full_and_a_ragged_last_workgroup(gpu, oracle_mod, entry, k):
    from isplib_amd import cabi
    x16 = half_ref.to16(cases.dense(N, k, 3, "integer"), torch.bfloat16)
    d_x, d_scale = x16.to(gpu), torch.from_numpy(_scale()).to(gpu)
    nan_bits = half_ref.bits(torch.full((1,), float("nan"), dtype=torch.bfloat16))[0]
    for nb, r in COUNTS:
        rowptr, col = _graph(nb, r)
        m = rowptr.size - 1
        assert m == 4 * nb - r and (m + 3) // 4 == nb and rowptr[m] - rowptr[m - 1] == LONG
        ref_bits, ref_arg = _reference(oracle_mod, entry, nb, r, x16)
        d_rowptr, d_col = torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu)
        for order in (None, torch.arange(m - 1, -1, -1, dtype=torch.int32, device=gpu)):
            z = torch.full((m, k + PAD), float("nan"), dtype=torch.bfloat16, device=gpu)
            z_arg = torch.full((m, k + PAD), ARG_FILL, dtype=torch.int64, device=gpu)
            if entry == "unit":
                cabi.spmm_rows16(d_rowptr, d_col, None, d_x, "sum", order=order, out=z[:, :k])
            elif entry == "colscale":
                cabi.spmm_rows16_colscale(d_rowptr, d_col, d_scale, d_x, "sum", order=order, out=z[:, :k])
            else:
                cabi.spmm_rows16_minmax(d_rowptr, d_col, None, d_x, "max", order=order, out=z[:, :k], arg=z_arg[:, :k])
            torch.cuda.synchronize()
            what = f"{entry}, k {k}, {nb} row blocks less {r} rows, {'index' if order is None else 'reversed'} order"
            got = half_ref.bits(z)
            bad = np.flatnonzero((got[:, :k] != ref_bits).any(1))
            assert bad.size == 0, f"{what}: rows {bad[:8].tolist()} differ from the reference"
            assert np.all(got[:, k:] == nan_bits), f"{what}: a pad column of z was written"
            got_arg = z_arg.cpu().numpy()
            if entry == "max":
                bad = np.flatnonzero((got_arg[:, :k] != ref_arg).any(1))
                assert bad.size == 0, f"{what}: positions of rows {bad[:8].tolist()} differ from the reference"
            assert np.all(got_arg[:, k:] == ARG_FILL), f"{what}: a pad column of z_arg was written"
