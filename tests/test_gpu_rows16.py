"""16-bit features (bf16, fp16) for SpMM sum / mean on the plain row-per-wave kernel: fusedMM_csr_rows16_hip (16-byte gathers of
eight columns), through the C ABI, the torch operators and the plug-in.

The contract is the 16-bit stream kernel's (include/isplib_hip.h): products, sums and the mean's division in fp32, the finished row
rounded ONCE to nearest even.  The reference of every test is tests/half_ref.py: the oracle on the widened operand, then torch's CPU
`.to(dtype)`.  Where the operands are small integers every fp32 sum is exact in any order (|x| <= 3, |w| <= 5: a 6,144-edge row stays
below 92,160 < 2^24), so the bar for sums is BIT EQUALITY with that reference; real-valued data and the mean meet
half_ref.rounding_bound.  Every output is prefilled with NaN so an unwritten element shows, and every launch runs twice to equal
bits.  The kernel's loop constants: a slot is LPR lanes (8 / 16 / 32 / 64 up to 64 / 128 / 256 / 512 columns), G = 64 / LPR slots per
wave, U = 6 gathers per slot and step (rows16_unroll, spmm_rows16.hip), long_row = 2048."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests.test_gpu_stream_edges import _weights

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", tuple(half_ref.DTYPES.values()), ids=tuple(half_ref.DTYPES))
U, LONG_ROW = 6, 2048

_refs = {}


def _ref(oracle, key, rowptr, col, val, x16, red):
    """(ref32, ref16, tol) once per (graph, operands, reduction), shared and left unchanged."""
    key = key + (x16.dtype, red)
    if key not in _refs:
        ref32, ref16 = half_ref.reference(oracle, rowptr, col, val, x16, red)
        tol = cases.sum_tolerance(oracle, rowptr, col, val, half_ref.widen(x16))
        ref32.setflags(write=False)
        tol.setflags(write=False)
        _refs[key] = (ref32, ref16, tol)
    return _refs[key]


def _nan_filled(m, k, dtype, dev):
    return torch.full((m, k), float("nan"), dtype=dtype, device=dev)


def _launch_twice(d_rowptr, d_col, d_val, d_x, red, order=None):
    from isplib_amd import cabi
    m, k = d_rowptr.numel() - 1, d_x.size(1)
    out, again = _nan_filled(m, k, d_x.dtype, d_x.device), _nan_filled(m, k, d_x.dtype, d_x.device)
    cabi.spmm_rows16(d_rowptr, d_col, d_val, d_x, red, order=order, out=out)
    cabi.spmm_rows16(d_rowptr, d_col, d_val, d_x, red, order=order, out=again)
    torch.cuda.synchronize()
    assert np.array_equal(half_ref.bits(out), half_ref.bits(again)), "two launches: equal bits"
    return out


def _assert_bits(got, ref16, what):
    bad = np.flatnonzero((half_ref.bits(got) != half_ref.bits(ref16)).reshape(ref16.shape[0], -1).any(1))
    assert bad.size == 0, f"{what}: rows {bad[:8].tolist()} ... differ from round16(oracle)"


def _assert_bound(got, ref32, tol, dtype, what):
    g = got.detach().cpu().to(torch.float32).numpy().astype(np.float64)
    bound = half_ref.rounding_bound(ref32.astype(np.float64), tol.astype(np.float64), dtype)
    err = np.abs(g - ref32.astype(np.float64))
    assert np.all(np.isfinite(g)) and np.all(err <= bound), f"{what}: max err / bound = {np.max(err / bound)}"


def _on(gpu, *arrays):
    return tuple(None if a is None else torch.from_numpy(a).to(gpu) for a in arrays)


def _sum_and_mean(gpu, oracle, key, rowptr, col, n, k, dtype, order=None):
    """Weighted and unit, integer data: sum bit-equal to round16(oracle), mean within the bound."""
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    d_rowptr, d_col = _on(gpu, rowptr, col)
    d_x = x16.to(gpu)
    for unit in (False, True):
        val = np.ones(col.size, np.float32) if unit else _weights(col.size)
        d_val = None if unit else torch.from_numpy(val).to(gpu)
        for red in ("sum", "mean"):
            out = _launch_twice(d_rowptr, d_col, d_val, d_x, red, order)
            ref32, ref16, tol = _ref(oracle, key + (k, unit), rowptr, col, val, x16, red)
            what = f"{red}, k {k}, {'unit' if unit else 'weighted'}"
            if red == "sum":
                _assert_bits(out, ref16, what)
            else:
                _assert_bound(out, ref32, tol, dtype, what)


# ---- 1. every slot width and its ragged edge -------------------------------------------------------------------------------------

def _hub_graph():
    return cases.random_csr(300, 200, 12, 31, empty_rows=(0, 150, 299), hub=(7, 2500), duplicates=True)


@DT
@pytest.mark.parametrize("k", (8, 10, 64, 66, 128, 130, 256, 258, 512, 514, 1024, 1026))
def test_every_slot_width_and_its_ragged_edge(gpu, oracle_mod, k, dtype):
    """One whole slot of every width and two columns more; 1024 is the widest single pass (64 lanes x 2 chunks x 8 columns) and 1026
    needs a second grid.y panel.  The hub row (2,500 edges) exceeds long_row: all four waves of its workgroup take it."""
    rowptr, col = _hub_graph()
    assert np.max(np.diff(rowptr)) > LONG_ROW
    _sum_and_mean(gpu, oracle_mod, ("hub",), rowptr, col, 200, k, dtype)


# ---- 2. row lengths around every loop edge ---------------------------------------------------------------------------------------

def _edge_degrees():
    deg = {0, 1, 63, 64, 65, 127, 128, 129, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 3 * LONG_ROW}
    for lpr in (8, 32):                                      # the configurations of k = 64 and k = 256
        g = 64 // lpr
        deg |= {g - 1, g, g + 1, g * U - 1, g * U, g * U + 1}
    return sorted(deg)


@DT
@pytest.mark.parametrize("k", (64, 256))
def test_row_lengths_around_every_loop_edge(gpu, oracle_mod, k, dtype):
    deg = _edge_degrees()
    deg = deg + deg[::-1]                                    # every length in two places of a workgroup's four rows
    rowptr, col = cases.csr_of_degrees(deg, 200, 17)
    _sum_and_mean(gpu, oracle_mod, ("lengths",), rowptr, col, 200, k, dtype)


# ---- 3. row order ----------------------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (64, 256))
def test_any_row_order_gives_the_bits_of_index_order(gpu, oracle_mod, k, dtype):
    rowptr, col = _hub_graph()
    m = rowptr.size - 1
    d_rowptr, d_col, d_val = _on(gpu, rowptr, col, cases.weights(col.size, 4, "uniform"))
    d_x = half_ref.to16(cases.dense(200, k, 3, "uniform"), dtype).to(gpu)
    orders = (np.random.default_rng(5).permutation(m), np.arange(m)[::-1].copy())
    for red in ("sum", "mean"):
        base = half_ref.bits(_launch_twice(d_rowptr, d_col, d_val, d_x, red))
        for o in orders:
            d_o = torch.from_numpy(o.astype(np.int32)).to(gpu)
            assert np.array_equal(half_ref.bits(_launch_twice(d_rowptr, d_col, d_val, d_x, red, d_o)), base), red
    # and the ordered launch is right, not only equal: integer data against the oracle
    _sum_and_mean(gpu, oracle_mod, ("hub",), rowptr, col, 200, k, dtype, order=torch.from_numpy(orders[0].astype(np.int32)).to(gpu))


# ---- 4. pitch --------------------------------------------------------------------------------------------------------------------

@DT
def test_column_view_and_output_pitch(gpu, oracle_mod, dtype):
    """A [n, 64] column view of a [n, 192] tensor is gathered at its own pitch, and an output view with pitch 130 is written at its
    own: nothing beside the 64 columns is touched."""
    from isplib_amd import cabi
    rowptr, col = _hub_graph()
    m, n, k = rowptr.size - 1, 200, 64
    val = _weights(col.size)
    d_rowptr, d_col, d_val = _on(gpu, rowptr, col, val)
    wide = half_ref.to16(cases.dense(n, 192, 5, "integer"), dtype)
    x16 = wide[:, 64:128].contiguous()
    d_view = wide.to(gpu)[:, 64:128]
    assert d_view.stride(0) == 192
    big = _nan_filled(m, 130, dtype, gpu)
    out = cabi.spmm_rows16(d_rowptr, d_col, d_val, d_view, "sum", out=big[:, :k])
    torch.cuda.synchronize()
    assert out.data_ptr() == big.data_ptr() and out.stride(0) == 130
    _, ref16, _ = _ref(oracle_mod, ("view",), rowptr, col, val, x16, "sum")
    _assert_bits(out.contiguous(), ref16, "column view, output pitch 130")
    assert bool(torch.isnan(big[:, k:]).all()), "columns beyond k must not be touched"


# ---- 5. the rounding bound on real-valued data -----------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (8, 64, 100, 256))
def test_rounding_bound_on_real_valued_data(gpu, oracle_mod, k, dtype):
    """|got - ref32| <= tol + u * (|ref32| + tol) (+ 2^-25 for fp16) for EVERY element (half_ref.rounding_bound)."""
    rowptr, col = _hub_graph()
    val = cases.weights(col.size, 4, "uniform")
    x16 = half_ref.to16(cases.dense(200, k, 3, "uniform"), dtype)
    d_rowptr, d_col, d_val = _on(gpu, rowptr, col, val)
    for red in ("sum", "mean"):
        out = _launch_twice(d_rowptr, d_col, d_val, x16.to(gpu), red)
        ref32, _, tol = _ref(oracle_mod, ("real", k), rowptr, col, val, x16, red)
        _assert_bound(out, ref32, tol, dtype, f"{red}, k {k}")


# ---- 6. special values -----------------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("kind", ("nonfinite", "denormal"))
def test_nonfinite_and_small_values(gpu, oracle_mod, kind, dtype):
    """NaN stays NaN, +-Inf stay, in exactly the elements the reference marks; bf16 subnormals are kept (in fp16 the denormal operand
    is all zeros after rounding).  Degrees are about 1 and the terms are in (-1, 1): nothing overflows, so the masks do not depend
    on the order."""
    m, n, k = 64, 97, 64
    rowptr, col = cases.random_csr(m, n, 1.0, 41)
    val = np.ones(col.size, np.float32)
    x16 = half_ref.to16(cases.dense(n, k, 3, kind), dtype)
    if kind == "denormal":
        assert bool((x16 == 0).all()) == (dtype == torch.float16)
    d_rowptr, d_col = _on(gpu, rowptr, col)
    for red in ("sum", "mean"):
        got = _launch_twice(d_rowptr, d_col, None, x16.to(gpu), red).cpu().to(torch.float32).numpy()
        _, ref16, _ = _ref(oracle_mod, ("small", kind), rowptr, col, val, x16, red)
        ref = ref16.to(torch.float32).numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)), red
        assert np.array_equal(got == np.inf, ref == np.inf) and np.array_equal(got == -np.inf, ref == -np.inf), red
        fin = np.isfinite(ref)
        assert np.array_equal(got[fin], ref[fin]), red
        if kind == "denormal" and dtype == torch.bfloat16 and red == "sum":
            assert np.any((got != 0) & (np.abs(got) < np.float32(2.0 ** -126))), "bf16 keeps subnormal results"


@DT
def test_a_sum_beyond_the_largest_fp16_is_infinite_in_fp16(gpu, oracle_mod, dtype):
    """40 x 2048 = 81,920 > 65,504: +-Inf in fp16, the exact value in bf16; 31 x 2048 = 63,488 is finite in both."""
    n, k = 4, 16
    rowptr = np.array([0, 40, 80, 111], np.int64)
    col = np.concatenate([np.zeros(40), np.ones(40), np.zeros(31)]).astype(np.int64)
    val = np.ones(col.size, np.float32)
    x = np.zeros((n, k), np.float32)
    x[0], x[1] = 2048.0, -2048.0
    x16 = half_ref.to16(x, dtype)
    d_rowptr, d_col = _on(gpu, rowptr, col)
    out = _launch_twice(d_rowptr, d_col, None, x16.to(gpu), "sum")
    ref32, ref16, _ = _ref(oracle_mod, ("overflow",), rowptr, col, val, x16, "sum")
    assert ref32[0, 0] == 81920.0 and ref32[1, 0] == -81920.0 and ref32[2, 0] == 63488.0
    _assert_bits(out, ref16, "overflow")
    got = out.cpu().to(torch.float32).numpy()
    if dtype == torch.float16:
        assert np.all(got[0] == np.inf) and np.all(got[1] == -np.inf) and np.all(got[2] == 63488.0)
    else:
        assert np.all(got[0] == 81920.0) and np.all(got[1] == -81920.0)


# ---- 7. refusals before any launch -----------------------------------------------------------------------------------------------

@DT
def test_entry_refuses_before_any_launch(gpu, dtype):
    """Each refused call returns the documented status, leaves the output as it was, and isplib_hip_last_error names the cause."""
    from isplib_amd import cabi
    rowptr, col = cases.random_csr(150, 120, 9.0, 21, empty_rows=(4,), hub=(9, 700), duplicates=True)
    m, n, k = 150, 120, 64
    d_rowptr, d_col, d_val = _on(gpu, rowptr, col, _weights(col.size))
    y = torch.ones((n, k), dtype=dtype, device=gpu)
    y66 = torch.ones((n, 66), dtype=dtype, device=gpu)
    flat = torch.ones(n * k + 2, dtype=dtype, device=gpu)
    SUM, MAX, FAIL, NO = cabi.MSG_SPMM_SUM, cabi.MSG_SPMM_MAX, cabi.FAIL, cabi.NO_OPT_IMPL
    calls = (
        ("isplib_rows16_serves", FAIL, SUM, y, {"k": 63}),                                        # odd k
        ("isplib_rows16_serves", FAIL, SUM, y, {"k": 6}),                                         # k < 8
        ("isplib_rows16_serves", FAIL, SUM, torch.ones((n, 65), dtype=dtype, device=gpu)[:, :k], {}),   # odd ldy
        ("isplib_rows16_serves", FAIL, SUM, y, {"ldz": 65}),                                      # odd ldz
        ("4-byte aligned", FAIL, SUM, flat[1:1 + n * k].view(n, k), {}),                          # a base at 2 bytes mod 4
        ("sum and mean only", NO, MAX, y, {}),
        ("dtype", FAIL, SUM, y, {"dtype": 0}),                                                    # what an fp32 tensor maps to
        ("leading dimension", FAIL, SUM, y66[:, :k], {"ldz": 62}),                                # ldz < k
    )
    for cause, status, msg, yy, extra in calls:
        z = _nan_filled(m, 66, dtype, gpu)
        before = half_ref.bits(z).copy()
        st = cabi.fusedMM_csr_rows16_hip(msg, d_rowptr, d_col, d_val, None, yy, z[:, :k], check=False, **extra)
        torch.cuda.synchronize()
        assert st == status and cause in cabi.last_error(), (cause, st, cabi.last_error())
        assert np.array_equal(half_ref.bits(z), before), cause
    # nothing to do is a success
    empty_rp = torch.zeros(1, dtype=torch.int64, device=gpu)
    assert cabi.fusedMM_csr_rows16_hip(SUM, empty_rp, d_col[:0], None, None, y, torch.empty((0, k), dtype=dtype, device=gpu), check=False) == cabi.SUCCESS
    assert cabi.fusedMM_csr_rows16_hip(SUM, d_rowptr, d_col, None, None, y[:, :0], torch.empty((m, 0), dtype=dtype, device=gpu), check=False) == cabi.SUCCESS
    # the wrapper raises before the call
    with pytest.raises(ValueError):
        cabi.spmm_rows16(d_rowptr, d_col, d_val, y[:, :6])
    with pytest.raises(ValueError):
        cabi.spmm_rows16(d_rowptr, d_col, d_val, y[:100])                      # column ids beyond n
    with pytest.raises(ValueError):
        cabi.spmm_rows16(d_rowptr, d_col[:-1], d_val, y)
    with pytest.raises(TypeError):
        cabi.spmm_rows16(d_rowptr, d_col, d_val, y.to(torch.float32))
    with pytest.raises(ValueError):
        cabi.spmm_rows16(d_rowptr, d_col, d_val, y, out=torch.empty((m, 65), dtype=dtype, device=gpu)[:, :k])
    with pytest.raises(ValueError):
        cabi.spmm_rows16(d_rowptr, d_col, d_val, y, "max")
    with pytest.raises(ValueError):
        cabi.spmm_rows16(d_rowptr, d_col, d_val, y, order=torch.zeros(m - 1, dtype=torch.int32, device=gpu))


# ---- 8. byte offsets past 2 GiB, up to the descriptor's limit --------------------------------------------------------------------

def test_gather_offsets_up_to_the_descriptor_limit_in_a_bf16_operand(gpu, oracle_mod):
    """n x 64 bf16 with n * ldy * 2 = 0xE0000000 exactly (the largest operand isplib_rows16_serves admits): the 32-bit byte offsets of
    the gathers run up to 3.5 GiB.  The operand is allocated uninitialised and only the rows the graph touches are written (integers):
    the first rows, the last rows, the rows either side of byte 2^31, and a long row over all of them.  Bit equality with
    round16(oracle) on the compacted rows.  Peak device memory: ~3.8 GB."""
    import gc
    from isplib_amd import cabi
    k = 64
    n = 0xE0000000 // (2 * k)
    assert cabi.rows16_serves(n, k, k, k) and not cabi.rows16_serves(n + 1, k, k, k)
    mid = (1 << 31) // (2 * k)
    touched = np.concatenate([np.arange(10), mid + np.arange(-3, 4), n - 1 - np.arange(10)]).astype(np.int64)
    rows = [touched[:10], touched[-10:], touched[10:17], np.array([0, 0, n - 1, n - 1, mid], np.int64), np.zeros(0, np.int64),
            np.sort(np.tile(touched, 90))]                                     # 2,430 edges: beyond long_row
    rowptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([r.size for r in rows], out=rowptr[1:])
    col = np.concatenate([np.sort(r) for r in rows])
    uniq, inv = np.unique(col, return_inverse=True)
    inv = inv.astype(np.int64).reshape(-1)
    xs16 = half_ref.to16(cases.dense(uniq.size, k, 3, "integer"), torch.bfloat16)
    x = torch.empty((n, k), dtype=torch.bfloat16, device=gpu)
    try:
        x[torch.from_numpy(uniq).to(gpu)] = xs16.to(gpu)
        d_rowptr, d_col = _on(gpu, rowptr, col)
        for weighted in (True, False):
            w = _weights(col.size) if weighted else np.ones(col.size, np.float32)
            d_w = torch.from_numpy(w).to(gpu) if weighted else None
            out = _launch_twice(d_rowptr, d_col, d_w, x, "sum")
            ref32, _ = oracle_mod.spmm_fw(rowptr, inv, w, half_ref.widen(xs16), "sum")
            _assert_bits(out, half_ref.round16(ref32, torch.bfloat16), f"up to 3.5 GiB, weighted={weighted}")
    finally:
        del x
        gc.collect()
        torch.cuda.empty_cache()


# ---- 9. operator and autograd, through patch_pyg() / matmul ----------------------------------------------------------------------

def _matmul(adj, x, red):
    import isplib_amd
    isplib_amd.iSpLibPlugin.patch_pyg()
    try:
        return torch.sparse.mm(adj, x, red)
    finally:
        isplib_amd.iSpLibPlugin.unpatch_pyg()


@pytest.fixture(scope="module")
def op_graph():
    rowptr, col = cases.random_csr(2000, 2000, 8.0, 51, empty_rows=(0, 1999), hub=(11, 1500), duplicates=True)
    return rowptr, col


def _adj(gpu, op_graph, weighted):
    import isplib_amd
    rowptr, col = op_graph
    val = _weights(col.size) if weighted else np.ones(col.size, np.float32)
    d_val = torch.from_numpy(val).to(gpu) if weighted else None
    return isplib_amd.SparseTensor.from_csr(torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), d_val, (2000, 2000)), val


@DT
@pytest.mark.parametrize("weighted", (True, False), ids=("weighted", "unit"))
@pytest.mark.parametrize("red", ("sum", "mean"))
def test_matmul_forward_and_backward(gpu, oracle_mod, op_graph, monkeypatch, red, weighted, dtype):
    """With the stream schedule off the plain kernel serves this graph (fp32: `_last_schedule`); ISPLIB_HALF=native then runs the
    16-bit row kernel forward and backward: output and x.grad have x's dtype, with integer operands the sum and its x.grad are
    bit-equal to round16 of the oracle, the mean meets the rounding bound against the oracle with fp32 scaling.  ISPLIB_HALF=convert
    converts, on the plain kernel, as before."""
    rowptr, col = op_graph
    m = n = 2000
    k = 64
    adj, val = _adj(gpu, op_graph, weighted)
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    g16 = half_ref.to16(cases.dense(m, k, 5, "integer"), dtype)
    monkeypatch.setenv("ISPLIB_STREAM", "0")
    _matmul(adj, x16.to(gpu).to(torch.float32), red)
    assert adj.storage._last_schedule == ("plain",), adj.storage._last_schedule
    results = {}
    for mode in ("native", "convert"):
        monkeypatch.setenv("ISPLIB_HALF", mode)
        x = x16.to(gpu).requires_grad_(True)
        out = _matmul(adj, x, red)
        schedule = adj.storage._last_schedule
        g = g16.to(gpu)
        peak, _ = _peak_during(lambda: out.backward(g))
        assert out.dtype == dtype and x.grad.dtype == dtype
        assert schedule == (("rows16",) if mode == "native" else ("convert", "plain")), schedule
        if mode == "native" and (weighted or red == "sum"):
            # `_last_schedule` is the forward's; that the BACKWARD ran on the row kernel too shows in what it allocates: the 16-bit
            # gradient and nothing the size of an fp32 copy of dY (the unit-weight mean backward forms dY / deg in fp32 on purpose)
            assert peak < n * k * 4, f"the backward allocated {peak} bytes: an fp32 copy of dY is {n * k * 4}"
        results[mode] = (out.detach(), x.grad.detach())
    ref32, ref16, tol = _ref(oracle_mod, ("op", weighted), rowptr, col, val, x16, red)
    g32 = half_ref.widen(g16)
    for mode, (out, grad) in results.items():
        if red == "sum":
            _assert_bits(out, ref16, f"forward, {mode}")
            _assert_bits(grad, half_ref.round16(oracle_mod.spmm_sum_bw(rowptr, col, val, n, g32), dtype), f"x.grad, {mode}")
        else:
            _assert_bound(out, ref32, tol, dtype, f"forward, {mode}")
            colptr, new_row, new_w = oracle_mod.mean_bw_weights(rowptr, col, val, n)
            gref = oracle_mod.spmm_mean_bw(rowptr, col, val, n, g32)
            gtol = cases.sum_tolerance(oracle_mod, colptr, new_row, new_w, g32)
            _assert_bound(grad, gref, gtol, dtype, f"x.grad, {mode}")


def _peak_during(fn):
    """(bytes allocated at the peak of fn() beyond what was allocated before it, fn's result)."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, r


@DT
def test_planned_operator_takes_the_row_plan_forward_and_backward_without_an_fp32_copy(gpu, oracle_mod, op_graph, dtype):
    """torch.ops.isplib.fusedmm_spmm_planned with an explicit 16-bit row plan -- [empty int32 (index order), host int32 [16]] -- for
    the forward and for A^T dY: bit-equal to the rounded oracle, and neither pass allocates as much as an fp32 copy of its operand;
    the empty plan (the plain kernel: the conversion route for a 16-bit operand) does, which is what tells the two apart."""
    rowptr, col = op_graph
    n, k = 2000, 64
    adj, val = _adj(gpu, op_graph, True)
    s = adj.storage
    colptr, row_t, val_t = s.colptr(), s.row_t(), s.val_t()
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    g = half_ref.to16(cases.dense(n, k, 5, "integer"), dtype).to(gpu)
    _, ref16, _ = _ref(oracle_mod, ("op", True), rowptr, col, val, x16, "sum")
    gref = half_ref.round16(oracle_mod.spmm_sum_bw(rowptr, col, val, n, half_ref.widen(g.cpu())), dtype)
    row_plan = [torch.empty(0, dtype=torch.int32, device=gpu), torch.tensor([16], dtype=torch.int32)]
    peaks = {}
    for name, plan in (("rows16", row_plan), ("convert", [])):
        x = x16.to(gpu).requires_grad_(True)
        fw, out = _peak_during(lambda: torch.ops.isplib.fusedmm_spmm_planned(s._rowptr, s._col, s._value, colptr, x, val_t, row_t, plan, plan))
        bw, _ = _peak_during(lambda: out.backward(g))
        peaks[name] = (fw, bw)
        _assert_bits(out, ref16, f"forward, {name}")
        _assert_bits(x.grad, gref, f"x.grad, {name}")
    fp32_copy = n * k * 4
    assert max(peaks["rows16"]) < fp32_copy <= min(peaks["convert"]), (peaks, fp32_copy)


@DT
@pytest.mark.parametrize("mode", ("auto", "native"))
def test_an_operand_two_bytes_past_a_four_byte_boundary_is_served(gpu, oracle_mod, op_graph, monkeypatch, mode, dtype):
    """A contiguous x (and dY) that starts at an odd element of a flat buffer: `contiguous()` leaves it where it is and the entry
    refuses such a base, so the operators copy it (16 bits) -- nothing raises, forward and x.grad are bit-equal to the rounded oracle."""
    from isplib_amd import cabi
    rowptr, col = op_graph
    n, k = 2000, 64
    adj, val = _adj(gpu, op_graph, True)
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    g16 = half_ref.to16(cases.dense(n, k, 5, "integer"), dtype)

    def odd(t16):
        flat = torch.zeros(n * k + 2, dtype=dtype, device=gpu)
        flat[1:1 + n * k] = t16.to(gpu).reshape(-1)
        v = flat[1:1 + n * k].view(n, k)
        assert v.is_contiguous() and v.data_ptr() % 4 == 2
        return v
    monkeypatch.setenv("ISPLIB_STREAM", "0")
    monkeypatch.setenv("ISPLIB_HALF", mode)
    for red in ("sum", "mean"):
        x = odd(x16).detach().requires_grad_(True)
        assert x.data_ptr() % 4 == 2
        out = _matmul(adj, x, red)
        want = "rows16" if mode == "native" or cabi.rows16_native_pays(n, k, False, True) else "convert"
        assert adj.storage._last_schedule[0] == want, adj.storage._last_schedule
        out.backward(odd(g16))
        torch.cuda.synchronize()
        assert out.dtype == dtype and x.grad.dtype == dtype
        if red == "sum":
            _, ref16, _ = _ref(oracle_mod, ("op", True), rowptr, col, val, x16, "sum")
            _assert_bits(out, ref16, "forward")
            _assert_bits(x.grad, half_ref.round16(oracle_mod.spmm_sum_bw(rowptr, col, val, n, half_ref.widen(g16)), dtype), "x.grad")
        else:
            ref32, _, tol = _ref(oracle_mod, ("op", True), rowptr, col, val, x16, "mean")
            _assert_bound(out, ref32, tol, dtype, "forward")


@DT
def test_odd_k_and_max_min_convert_under_every_mode(gpu, op_graph, monkeypatch, dtype):
    """k = 41 is outside isplib_rows16_serves and max / min are not served: the conversion route, whatever ISPLIB_HALF says, and the
    default (auto) follows the measured rule."""
    from isplib_amd import cabi
    adj, _ = _adj(gpu, op_graph, True)
    monkeypatch.setenv("ISPLIB_STREAM", "0")
    x41 = half_ref.to16(cases.dense(2000, 41, 3, "uniform"), dtype).to(gpu)
    x64 = half_ref.to16(cases.dense(2000, 64, 3, "uniform"), dtype).to(gpu)
    for mode in ("native", "auto", "convert"):
        monkeypatch.setenv("ISPLIB_HALF", mode)
        for x, red in ((x41, "sum"), (x41, "mean"), (x64, "max"), (x64, "min")):
            out = _matmul(adj, x, red)
            assert out.dtype == dtype and adj.storage._last_schedule[0] == "convert", (mode, red, adj.storage._last_schedule)
    monkeypatch.delenv("ISPLIB_HALF")
    _matmul(adj, x64, "sum")
    want = "rows16" if cabi.rows16_native_pays(2000, 64, False, True) else "convert"
    assert adj.storage._last_schedule[0] == want


@DT
def test_captured_graph_replays_to_the_same_bits(gpu, oracle_mod, op_graph, monkeypatch, dtype):
    import isplib_amd
    rowptr, col = op_graph
    n, k = 2000, 64
    adj, val = _adj(gpu, op_graph, True)
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    monkeypatch.setenv("ISPLIB_STREAM", "0")
    monkeypatch.setenv("ISPLIB_HALF", "native")
    x = x16.to(gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        eager = isplib_amd.matmul(adj, x, "sum")                  # decides the schedule: nothing is built under capture
    torch.cuda.current_stream().wait_stream(side)
    assert adj.storage._last_schedule == ("rows16",)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        captured = isplib_amd.matmul(adj, x, "sum")
    replays = []
    for _ in range(2):
        captured.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        replays.append(half_ref.bits(captured).copy())
    assert np.array_equal(replays[0], replays[1]) and np.array_equal(replays[0], half_ref.bits(eager))
    _, ref16, _ = _ref(oracle_mod, ("op", True), rowptr, col, val, x16, "sum")
    _assert_bits(captured, ref16, "replayed graph")
