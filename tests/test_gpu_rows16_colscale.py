"""The column-scaled 16-bit row kernel (fusedMM_csr_rows16_colscale_hip): z[i] = round16(sum_e scale[col[e]] * y[col[e]]), and the
unit-weight mean backward that runs on it (ISPLIB_HALF_MEAN_BW), through the C ABI, the torch operators and the plug-in.

The contract is EQUALITY OF BITS with the weighted 16-bit row kernel given val[e] = scale[col[e]] (tests/test_gpu_rows16.py holds that
kernel to the oracle): the two differ only in where a lane's factor comes from.  Integer data is also compared with round16(oracle)
directly.  Every output is prefilled with NaN so an unwritten element shows, and every launch runs twice to equal bits."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests import rows16_colscale_cases as cs

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", tuple(half_ref.DTYPES.values()), ids=tuple(half_ref.DTYPES))
N = cs.N


def _nan_filled(m, k, dtype, dev):
    return torch.full((m, k), float("nan"), dtype=dtype, device=dev)


def _on(gpu, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays)


def _twice(fn, m, k, d_x):
    """fn(out) launched into two NaN-filled outputs: equal bits, returned once."""
    out, again = _nan_filled(m, k, d_x.dtype, d_x.device), _nan_filled(m, k, d_x.dtype, d_x.device)
    fn(out)
    fn(again)
    torch.cuda.synchronize()
    assert np.array_equal(half_ref.bits(out), half_ref.bits(again)), "two launches: equal bits"
    return out


def _colscale(d_rowptr, d_col, d_s, d_x, red, order=None):
    from isplib_amd import cabi
    return _twice(lambda o: cabi.spmm_rows16_colscale(d_rowptr, d_col, d_s, d_x, red, order=order, out=o), d_rowptr.numel() - 1, d_x.size(1), d_x)


def _weighted(d_rowptr, d_col, d_s, d_x, red, order=None):
    from isplib_amd import cabi
    d_val = d_s[d_col]
    return _twice(lambda o: cabi.spmm_rows16(d_rowptr, d_col, d_val, d_x, red, order=order, out=o), d_rowptr.numel() - 1, d_x.size(1), d_x)


def _assert_same_bits(got, want, what):
    g, w = half_ref.bits(got), half_ref.bits(want)
    bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(1))
    assert bad.size == 0, f"{what}: rows {bad[:8].tolist()} ... differ"


def _equal_to_weighted(gpu, rowptr, col, scale, x16, what):
    d_rowptr, d_col, d_s = _on(gpu, rowptr, col, scale)
    d_x = x16.to(gpu)
    for red in ("sum", "mean"):
        _assert_same_bits(_colscale(d_rowptr, d_col, d_s, d_x, red), _weighted(d_rowptr, d_col, d_s, d_x, red), f"{what}, {red}")


# ---- 1. bit equality with the weighted kernel, every slot width and its ragged edge ---------------------------------------------

@DT
@pytest.mark.parametrize("k", (8, 10, 64, 66, 128, 130, 256, 258, 512, 514, 1024, 1026))
def test_bits_of_the_weighted_kernel_on_real_valued_data(gpu, k, dtype):
    rowptr, col = cs.hub_graph()
    assert np.max(np.diff(rowptr)) > cs.LONG_ROW
    _equal_to_weighted(gpu, rowptr, col, cs.scale_table(), half_ref.to16(cases.dense(N, k, 3, "uniform"), dtype), f"k {k}")


# ---- 2. row lengths around every loop edge ---------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (64, 256))
def test_row_lengths_around_every_loop_edge(gpu, k, dtype):
    rowptr, col = cs.length_graph()
    _equal_to_weighted(gpu, rowptr, col, cs.scale_table(), half_ref.to16(cases.dense(N, k, 3, "uniform"), dtype), f"lengths, k {k}")


# ---- 3. right, not only equal ----------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (10, 64, 256, 1026))
def test_integer_data_has_the_bits_of_the_rounded_oracle(gpu, oracle_mod, k, dtype):
    """|x| <= 3 and integer scales |s| <= 5: every fp32 sum is exact in any order (a 6,144-edge row stays below 92,160 < 2^24), so the
    sum is round16 of the oracle's sum with val = s[col], bit for bit -- on the hub graph and on the graph of loop-edge lengths."""
    s = cs.integer_scale()
    x16 = half_ref.to16(cases.dense(N, k, 3, "integer"), dtype)
    for name, (rowptr, col) in (("hub", cs.hub_graph()), ("lengths", cs.length_graph())):
        ref32, _ = oracle_mod.spmm_fw(rowptr, col, s[col], half_ref.widen(x16), "sum")
        d_rowptr, d_col, d_s = _on(gpu, rowptr, col, s)
        _assert_same_bits(_colscale(d_rowptr, d_col, d_s, x16.to(gpu), "sum"), half_ref.round16(ref32, dtype), f"{name}, k {k}")


# ---- 4. row order ----------------------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (64, 256))
def test_any_row_order_gives_the_bits_of_index_order(gpu, k, dtype):
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    d_rowptr, d_col, d_s = _on(gpu, rowptr, col, cs.scale_table())
    d_x = half_ref.to16(cases.dense(N, k, 3, "uniform"), dtype).to(gpu)
    orders = (np.random.default_rng(5).permutation(m), np.arange(m)[::-1].copy())
    for red in ("sum", "mean"):
        base = _colscale(d_rowptr, d_col, d_s, d_x, red)
        for o in orders:
            d_o = torch.from_numpy(o.astype(np.int32)).to(gpu)
            _assert_same_bits(_colscale(d_rowptr, d_col, d_s, d_x, red, d_o), base, red)


# ---- 5. pitch --------------------------------------------------------------------------------------------------------------------

@DT
def test_column_view_and_output_pitch(gpu, dtype):
    """A [n, 64] column view of a [n, 192] tensor is gathered at its own pitch, and an output view with pitch 130 is written at its
    own: nothing beside the 64 columns is touched."""
    from isplib_amd import cabi
    rowptr, col = cs.hub_graph()
    m, k = rowptr.size - 1, 64
    d_rowptr, d_col, d_s = _on(gpu, rowptr, col, cs.scale_table())
    d_view = half_ref.to16(cases.dense(N, 192, 5, "uniform"), dtype).to(gpu)[:, 64:128]
    assert d_view.stride(0) == 192
    big = _nan_filled(m, 130, dtype, gpu)
    out = cabi.spmm_rows16_colscale(d_rowptr, d_col, d_s, d_view, "sum", out=big[:, :k])
    torch.cuda.synchronize()
    assert out.data_ptr() == big.data_ptr() and out.stride(0) == 130
    _assert_same_bits(out.contiguous(), _weighted(d_rowptr, d_col, d_s, d_view.contiguous(), "sum"), "column view, output pitch 130")
    assert bool(torch.isnan(big[:, k:]).all()), "columns beyond k must not be touched"


# ---- 6. special values -----------------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("where", ("scale", "operand"))
@pytest.mark.parametrize("kind", ("nonfinite", "denormal"))
def test_nonfinite_and_small_values(gpu, kind, where, dtype):
    """Inf, NaN and subnormals in the table or in the operand: still the bits of the weighted kernel, NaN payloads included
    (tests/test_rows16_colscale_host.py: the references of these cases do hold NaN, Inf and subnormal results)."""
    n, k = 97, 64
    rowptr, col = cases.random_csr(64, n, 3.0, 41)
    scale = cs.special_scale(kind, n) if where == "scale" else cs.scale_table(n)
    x16 = half_ref.to16(cases.dense(n, k, 3, kind if where == "operand" else "uniform"), dtype)
    d_rowptr, d_col, d_s = _on(gpu, rowptr, col, scale)
    for red in ("sum", "mean"):
        _assert_same_bits(_colscale(d_rowptr, d_col, d_s, x16.to(gpu), red), _weighted(d_rowptr, d_col, d_s, x16.to(gpu), red), f"{kind} in the {where}, {red}")


# ---- 7. refusals before any launch -----------------------------------------------------------------------------------------------

@DT
def test_entry_refuses_before_any_launch(gpu, dtype):
    """Each refused call returns the documented status, leaves the output as it was, and isplib_hip_last_error names the cause."""
    from isplib_amd import cabi
    rowptr, col = cases.random_csr(150, 120, 9.0, 21, empty_rows=(4,), hub=(9, 700), duplicates=True)
    m, n, k = 150, 120, 64
    d_rowptr, d_col, d_s = _on(gpu, rowptr, col, cs.scale_table(n))
    y = torch.ones((n, k), dtype=dtype, device=gpu)
    flat = torch.ones(n * k + 2, dtype=dtype, device=gpu)
    SUM, MAX, FAIL, NO = cabi.MSG_SPMM_SUM, cabi.MSG_SPMM_MAX, cabi.FAIL, cabi.NO_OPT_IMPL
    calls = (
        ("null col_scale", FAIL, SUM, None, y, {}),                                                # null table, nnz > 0
        ("isplib_rows16_serves", FAIL, SUM, d_s, y, {"k": 63}),                                   # odd k
        ("isplib_rows16_serves", FAIL, SUM, d_s, y, {"k": 6}),                                    # k < 8
        ("dtype", FAIL, SUM, d_s, y, {"dtype": 0}),                                               # what an fp32 tensor maps to
        ("sum and mean only", NO, MAX, d_s, y, {}),
        ("4-byte aligned", FAIL, SUM, d_s, flat[1:1 + n * k].view(n, k), {}),                     # a base at 2 bytes mod 4
    )
    for cause, status, msg, scale, yy, extra in calls:
        z = _nan_filled(m, 66, dtype, gpu)
        st = cabi.fusedMM_csr_rows16_colscale_hip(msg, d_rowptr, d_col, scale, None, yy, z[:, :k], check=False, **extra)
        torch.cuda.synchronize()
        assert st == status and cause in cabi.last_error(), (cause, st, cabi.last_error())
        assert "fusedMM_csr_rows16_colscale_hip" in cabi.last_error()
        assert bool(torch.isnan(z).all()), cause
    # nothing to do is a success, a null table included when there is no edge
    empty_rp = torch.zeros(1, dtype=torch.int64, device=gpu)
    assert cabi.fusedMM_csr_rows16_colscale_hip(SUM, empty_rp, d_col[:0], None, None, y, torch.empty((0, k), dtype=dtype, device=gpu),
                                                check=False) == cabi.SUCCESS
    # the wrapper raises before the call
    with pytest.raises(ValueError):
        cabi.spmm_rows16_colscale(d_rowptr, d_col, None, y)
    with pytest.raises(ValueError):
        cabi.spmm_rows16_colscale(d_rowptr, d_col, d_s[:-1], y)                # one factor per column
    with pytest.raises(ValueError):
        cabi.spmm_rows16_colscale(d_rowptr, d_col, d_s, y[:, :6])
    with pytest.raises(ValueError):
        cabi.spmm_rows16_colscale(d_rowptr, d_col, d_s[:100], y[:100])         # column ids beyond n
    with pytest.raises(TypeError):
        cabi.spmm_rows16_colscale(d_rowptr, d_col, d_s, y.to(torch.float32))
    with pytest.raises(ValueError):
        cabi.spmm_rows16_colscale(d_rowptr, d_col, d_s, y, "max")


# ---- 8-11. operator and autograd, through patch_pyg() / matmul -------------------------------------------------------------------

M_OP, K_OP = 2000, 64
FP32_COPY = M_OP * K_OP * 4


def _matmul(adj, x, red):
    import isplib_amd
    isplib_amd.iSpLibPlugin.patch_pyg()
    try:
        return torch.sparse.mm(adj, x, red)
    finally:
        isplib_amd.iSpLibPlugin.unpatch_pyg()


def _peak_during(fn):
    """(bytes allocated at the peak of fn() beyond what was allocated before it, fn's result)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, r


@pytest.fixture(scope="module")
def op_graph():
    return cases.random_csr(M_OP, M_OP, 8.0, 51, empty_rows=(0, 1999), hub=(11, 1500), duplicates=True)


def _adj(gpu, op_graph, val):
    import isplib_amd
    rowptr, col = op_graph
    d_val = None if val is None else torch.from_numpy(val).to(gpu)
    return isplib_amd.SparseTensor.from_csr(torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), d_val, (M_OP, M_OP))


def _operands(dtype):
    return half_ref.to16(cases.dense(M_OP, K_OP, 3, "integer"), dtype), half_ref.to16(cases.dense(M_OP, K_OP, 5, "integer"), dtype)


def _grad(gpu, adj, x16, g16, red="mean"):
    """(x.grad, peak allocation of the backward, the forward's schedule, the output) of matmul(adj, x, red).backward(g)."""
    x = x16.to(gpu).requires_grad_(True)
    out = _matmul(adj, x, red)
    schedule = adj.storage._last_schedule
    g = g16.to(gpu)
    peak, _ = _peak_during(lambda: out.backward(g))
    return x.grad.detach(), peak, schedule, out.detach()


def _setenv(monkeypatch, mean_bw):
    monkeypatch.setenv("ISPLIB_STREAM", "0")
    monkeypatch.setenv("ISPLIB_HALF", "native")
    if mean_bw is None:
        monkeypatch.delenv("ISPLIB_HALF_MEAN_BW", raising=False)
    else:
        monkeypatch.setenv("ISPLIB_HALF_MEAN_BW", mean_bw)


def _assert_mean_bw_bound(oracle, op_graph, grad, g16, dtype, what):
    rowptr, col = op_graph
    ones = np.ones(col.size, np.float32)
    g32 = half_ref.widen(g16)
    colptr, new_row, new_w = oracle.mean_bw_weights(rowptr, col, ones, M_OP)
    gref = oracle.spmm_mean_bw(rowptr, col, ones, M_OP, g32).astype(np.float64)
    gtol = cases.sum_tolerance(oracle, colptr, new_row, new_w, g32).astype(np.float64)
    got = grad.cpu().to(torch.float32).numpy().astype(np.float64)
    bound = half_ref.rounding_bound(gref, gtol, dtype)
    err = np.abs(got - gref)
    assert np.all(np.isfinite(got)) and np.all(err <= bound), f"{what}: max err / bound = {np.max(err / bound)}"


@DT
def test_native_mean_backward_on_an_unweighted_graph(gpu, oracle_mod, op_graph, monkeypatch, dtype):
    """ISPLIB_HALF_MEAN_BW=native: x.grad of mean on the unweighted graph has x's dtype, the bits of the same call on the graph with
    explicit all-ones weights (the weighted mean backward: the 16-bit kernel with 1 / max(deg, 1) per edge), meets the bound against
    the oracle, and the backward allocates less than an fp32 copy of dY."""
    x16, g16 = _operands(dtype)
    _setenv(monkeypatch, "native")
    grad, peak, schedule, out = _grad(gpu, _adj(gpu, op_graph, None), x16, g16)
    assert schedule == ("rows16",), schedule
    assert out.dtype == dtype and grad.dtype == dtype
    ones_grad, ones_peak, _, ones_out = _grad(gpu, _adj(gpu, op_graph, np.ones(op_graph[1].size, np.float32)), x16, g16)
    print(f"peak of the backward: unit {peak}, all-ones weights {ones_peak}, an fp32 copy of dY {FP32_COPY}")
    _assert_same_bits(out, ones_out, "forward, unit against all-ones weights")
    _assert_same_bits(grad, ones_grad, "x.grad, unit against all-ones weights")
    _assert_mean_bw_bound(oracle_mod, op_graph, grad, g16, dtype, "x.grad")
    assert peak < FP32_COPY, f"the backward allocated {peak} bytes: an fp32 copy of dY is {FP32_COPY}"


@DT
def test_default_is_unchanged(gpu, oracle_mod, op_graph, monkeypatch, dtype):
    """The variable unset: the fp32 dY / deg is still formed (the peak shows it) and x.grad has the bits of ISPLIB_HALF_MEAN_BW=convert;
    ISPLIB_HALF=convert wins over ISPLIB_HALF_MEAN_BW=native."""
    x16, g16 = _operands(dtype)
    adj = _adj(gpu, op_graph, None)
    _setenv(monkeypatch, None)
    grad, peak, schedule, _ = _grad(gpu, adj, x16, g16)
    assert schedule == ("rows16",) and grad.dtype == dtype
    print(f"peak of the backward: default {peak}, an fp32 copy of dY {FP32_COPY}")
    assert peak >= FP32_COPY, f"the default backward allocated {peak} bytes only: no fp32 dY / deg of {FP32_COPY}?"
    _setenv(monkeypatch, "convert")
    conv, conv_peak, _, _ = _grad(gpu, adj, x16, g16)
    _assert_same_bits(grad, conv, "unset against convert")
    assert conv_peak >= FP32_COPY
    _assert_mean_bw_bound(oracle_mod, op_graph, grad, g16, dtype, "x.grad")
    monkeypatch.setenv("ISPLIB_HALF_MEAN_BW", "native")
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    both, _, schedule, _ = _grad(gpu, adj, x16, g16)
    assert schedule[0] == "convert", schedule
    _assert_mean_bw_bound(oracle_mod, op_graph, both, g16, dtype, "x.grad under ISPLIB_HALF=convert")


@DT
def test_direct_operator_call(gpu, op_graph, monkeypatch, dtype):
    """torch.ops.isplib.fusedmm_spmm_mean_planned: the three-element plan_t gives the native backward's bits without an fp32 copy,
    today's two-element plan the default's, and an fp32 call on the three-element plan the fp32 result unchanged."""
    x16, g16 = _operands(dtype)
    adj = _adj(gpu, op_graph, None)
    s = adj.storage
    colptr, row_t = s.colptr(), s.row_t()
    row_plan = [torch.empty(0, dtype=torch.int32, device=gpu), torch.tensor([16], dtype=torch.int32)]
    three = row_plan + [s.inv_rowcount()]
    assert s.inv_rowcount().dtype == torch.float32 and s.inv_rowcount().numel() == M_OP

    def run(x0, g0, plan_t):
        x = x0.to(gpu).requires_grad_(True)
        out = torch.ops.isplib.fusedmm_spmm_mean_planned(s._rowptr, s._col, None, colptr, x, row_t, None, row_plan, plan_t)
        g = g0.to(gpu)
        peak, _ = _peak_during(lambda: out.backward(g))
        return out.detach(), x.grad.detach(), peak

    _setenv(monkeypatch, "native")
    want_native, _, _, _ = _grad(gpu, adj, x16, g16)
    _setenv(monkeypatch, None)
    want_default, _, _, _ = _grad(gpu, adj, x16, g16)
    out3, grad3, peak3 = run(x16, g16, three)
    out2, grad2, peak2 = run(x16, g16, row_plan)
    print(f"peak of the backward: three-element plan {peak3}, two-element plan {peak2}, an fp32 copy of dY {FP32_COPY}")
    assert grad3.dtype == dtype and grad2.dtype == dtype
    _assert_same_bits(out3, out2, "the forward does not read plan_t")
    _assert_same_bits(grad3, want_native, "three-element plan_t")
    _assert_same_bits(grad2, want_default, "two-element plan_t")
    assert peak3 < FP32_COPY <= peak2, (peak3, peak2, FP32_COPY)
    # a table of another length is not the mean's: the route it always took, nothing raises
    _, grad_bad, peak_bad = run(x16, g16, row_plan + [s.inv_rowcount()[:-1]])
    _assert_same_bits(grad_bad, want_default, "a table of another length")
    assert peak_bad >= FP32_COPY
    # fp32 operands
    x32, g32 = x16.to(torch.float32), g16.to(torch.float32)
    o3, d3, _ = run(x32, g32, three)
    o2, d2, _ = run(x32, g32, row_plan)
    assert o3.dtype == torch.float32 and d3.dtype == torch.float32
    assert torch.equal(o3, o2) and torch.equal(d3, d2)


@DT
def test_weighted_graphs_and_sum_are_untouched_by_the_variable(gpu, op_graph, monkeypatch, dtype):
    from tests.test_gpu_stream_edges import _weights
    x16, g16 = _operands(dtype)
    unit, weighted = _adj(gpu, op_graph, None), _adj(gpu, op_graph, _weights(op_graph[1].size))
    for adj, red in ((weighted, "mean"), (weighted, "sum"), (unit, "sum")):
        seen = []
        for mode in (None, "convert", "native", "auto"):
            _setenv(monkeypatch, mode)
            grad, _, schedule, out = _grad(gpu, adj, x16, g16, red)
            assert schedule == ("rows16",), schedule
            seen.append((half_ref.bits(out).copy(), half_ref.bits(grad).copy()))
        for o, g in seen[1:]:
            assert np.array_equal(o, seen[0][0]) and np.array_equal(g, seen[0][1]), red
