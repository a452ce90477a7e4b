"""16-bit features (bf16, fp16) for SpMM sum / mean on the stream kernel: fusedMM_csr_stream16_hip, through the C ABI, the torch
operators and the plug-in.

The contract (include/isplib_hip.h): products, sums and the mean's division in fp32, the finished row rounded ONCE to nearest even
to the operand's type.  The reference of every test is tests/half_ref.py: the oracle on the widened operand, then torch's CPU
`.to(dtype)`.  Where the operands are small integers every fp32 sum is exact in any order, so the bar is BIT EQUALITY with that
reference (sums above 256 are not representable in bf16: this pins the rounding mode too); real-valued data meets
half_ref.rounding_bound.  Every output is prefilled with NaN so an unwritten row shows, and every launch runs twice to equal bits."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests.test_gpu_stream_edges import CHUNK, N, UNEVEN, _graph, _plans, _steps, _weights

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", tuple(half_ref.DTYPES.values()), ids=tuple(half_ref.DTYPES))
PANEL_K = {8: (32, 34), 4: (64, 66), 2: (128, 130)}         # one whole panel, and one panel plus a 2-column sliver

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


def _launch_twice(cabi, d_rowptr, nnz, plan, d_x, red):
    m, k = d_rowptr.numel() - 1, d_x.size(1)
    out, again = _nan_filled(m, k, d_x.dtype, d_x.device), _nan_filled(m, k, d_x.dtype, d_x.device)
    cabi.spmm_stream16(d_rowptr, nnz, plan, d_x, red, out=out)
    cabi.spmm_stream16(d_rowptr, nnz, plan, d_x, red, out=again)
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


def _sum_mean16(gpu, oracle, key, rowptr, col, streams, wpg, k, unit, want_steps, dtype):
    from isplib_amd import cabi
    val = np.ones(col.size, np.float32) if unit else _weights(col.size)
    x16 = half_ref.to16(cases.dense(N, k, 3, "integer"), dtype)
    d_rowptr, d_x = torch.from_numpy(rowptr).to(gpu), x16.to(gpu)
    for builder, plan in _plans(gpu, rowptr, col, None if unit else val, streams, wpg, slices=3):
        assert _steps(plan) == want_steps and plan.gens == 1 and plan.n_hub == 0, builder
        for red in ("sum", "mean"):
            out = _launch_twice(cabi, d_rowptr, col.size, plan, d_x, red)
            ref32, ref16, tol = _ref(oracle, key + (k, unit), rowptr, col, val, x16, red)
            if red == "sum":
                _assert_bits(out, ref16, f"sum, {builder} plan, streams {streams}, k {k}")
            else:
                _assert_bound(out, ref32, tol, dtype, f"mean, {builder} plan, streams {streams}, k {k}")
        if builder == "native":
            plan.close()


# ---- 1. every wave length ----------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("unit", (False, True), ids=("weighted", "unit"))
@pytest.mark.parametrize("streams", (2, 4, 8))
def test_ladder_every_wave_length(gpu, oracle_mod, streams, unit, dtype):
    (rowptr, col), wpg = _graph("ladder", streams)
    for k in PANEL_K[streams]:
        _sum_mean16(gpu, oracle_mod, ("ladder", streams), rowptr, col, streams, wpg, k, unit, list(cases.LADDER), dtype)


@DT
@pytest.mark.parametrize("length", UNEVEN)
def test_uneven_wave(gpu, oracle_mod, length, dtype):
    for streams in (2, 4, 8):
        (rowptr, col), wpg = _graph("uneven", streams, length)
        for k in PANEL_K[streams]:
            for unit in (False, True):
                _sum_mean16(gpu, oracle_mod, ("uneven", streams, length), rowptr, col, streams, wpg, k, unit, [length], dtype)


# ---- 2. every plan shape: hub rows (the 16-bit fold), two generations, empty rows, fewer rows than streams ------------------------

SHAPES = {c[0]: c[1:] for c in cases.stream_shape_cases(64)}


@DT
@pytest.mark.parametrize("name", tuple(SHAPES))
def test_every_plan_shape(gpu, oracle_mod, name, dtype):
    from isplib_amd import cabi
    from isplib_amd.plan import build_stream_plan
    rowptr, col, n, (slices, wpg, streams, chunk) = SHAPES[name]
    val = _weights(col.size)
    d_rowptr, d_col, d_val = torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), torch.from_numpy(val).to(gpu)
    plans = (("torch", build_stream_plan(d_rowptr, d_col, d_val, n, slices, wpg, None, streams, chunk)),
             ("native", cabi.NativeStreamPlan(d_rowptr, d_col, d_val, n, streams, slices, chunk, wpg)))
    try:
        for k in (64, 6):
            x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
            for builder, plan in plans:
                for red in ("sum", "mean"):
                    out = _launch_twice(cabi, d_rowptr, col.size, plan, x16.to(gpu), red)
                    ref32, ref16, tol = _ref(oracle_mod, ("shape", name, k), rowptr, col, val, x16, red)
                    if red == "sum":
                        _assert_bits(out, ref16, f"{name} sum, {builder} plan, k {k}")
                    else:
                        _assert_bound(out, ref32, tol, dtype, f"{name} mean, {builder} plan, k {k}")
    finally:
        plans[1][1].close()


# ---- 3. the rounding bound on real-valued data -----------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (4, 64, 100, 128))
def test_rounding_bound_on_real_valued_data(gpu, oracle_mod, k, dtype):
    """|got - ref32| <= tol + u * (|ref32| + tol) (+ 2^-25 for fp16) for EVERY element: another order of summation moves the fp32
    value by at most the project's own bound tol (cases.sum_tolerance), rounding to nearest adds one unit roundoff of it."""
    from isplib_amd import cabi
    m, n = 300, 200
    rowptr, col = cases.random_csr(m, n, 12, 31, empty_rows=(0, 150, 299), hub=(7, 900), duplicates=True)
    val = cases.weights(col.size, 4, "uniform")
    x16 = half_ref.to16(cases.dense(n, k, 3, "uniform"), dtype)
    d_rowptr, d_col, d_val = torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), torch.from_numpy(val).to(gpu)
    for streams in (2, 4, 8):
        plan = cabi.NativeStreamPlan(d_rowptr, d_col, d_val, n, streams, 3, CHUNK, 2)
        try:
            assert plan.n_hub == 1 and plan.gens >= 1
            for red in ("sum", "mean"):
                out = _launch_twice(cabi, d_rowptr, col.size, plan, x16.to(gpu), red)
                ref32, _, tol = _ref(oracle_mod, ("real", k), rowptr, col, val, x16, red)
                _assert_bound(out, ref32, tol, dtype, f"{red}, streams {streams}, k {k}")
        finally:
            plan.close()


# ---- 4. non-finite and small values ----------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("kind", ("nonfinite", "denormal"))
def test_nonfinite_and_small_values(gpu, oracle_mod, kind, dtype):
    """NaN stays NaN, +-Inf stay, bf16 subnormals are kept; in fp16 the denormal operand is all zeros after rounding (nothing traps).
    Degrees are about 1 and the terms are in (-1, 1): neither fp32 nor fp16 can overflow, so the masks do not depend on the order."""
    from isplib_amd import cabi
    m, n, k = 64, 97, 64
    rowptr, col = cases.random_csr(m, n, 1.0, 41)
    val = np.ones(col.size, np.float32)
    x16 = half_ref.to16(cases.dense(n, k, 3, kind), dtype)
    if kind == "denormal":
        assert bool((x16 == 0).all()) == (dtype == torch.float16)
    d_rowptr, d_col = torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu)
    plan = cabi.NativeStreamPlan(d_rowptr, d_col, None, n, 4, 2, CHUNK, 2)
    try:
        for red in ("sum", "mean"):
            got = _launch_twice(cabi, d_rowptr, col.size, plan, x16.to(gpu), red).cpu().to(torch.float32).numpy()
            _, ref16, _ = _ref(oracle_mod, ("small", kind), rowptr, col, val, x16, red)
            ref = ref16.to(torch.float32).numpy()
            assert np.array_equal(np.isnan(got), np.isnan(ref)), red
            assert np.array_equal(got == np.inf, ref == np.inf) and np.array_equal(got == -np.inf, ref == -np.inf), red
            fin = np.isfinite(ref)
            assert np.array_equal(got[fin], ref[fin]), red
    finally:
        plan.close()


# ---- 5. pitch and views ----------------------------------------------------------------------------------------------------------

def _small_graph(gpu, weighted=True, m=150, n=120, seed=21):
    rowptr, col = cases.random_csr(m, n, 9.0, seed, empty_rows=(4,), hub=(9, 700), duplicates=True)
    val = _weights(col.size) if weighted else np.ones(col.size, np.float32)
    d = (torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), torch.from_numpy(val).to(gpu) if weighted else None)
    return rowptr, col, val, d


@DT
def test_column_view_and_output_pitch(gpu, oracle_mod, dtype):
    """A [n, 64] column view of a [n, 192] tensor is gathered at its own pitch, and an output view with pitch 130 is written at its
    own: nothing beside the 64 columns is touched."""
    from isplib_amd import cabi
    rowptr, col, val, (d_rowptr, d_col, d_val) = _small_graph(gpu)
    m, n, k = rowptr.size - 1, 120, 64
    wide = half_ref.to16(cases.dense(n, 192, 5, "integer"), dtype)
    x16 = wide[:, 64:128].contiguous()
    d_view = wide.to(gpu)[:, 64:128]
    assert d_view.stride(0) == 192
    plan = cabi.NativeStreamPlan(d_rowptr, d_col, d_val, n, 4, 3, 64, 2)
    try:
        big = _nan_filled(m, 130, dtype, gpu)
        out = cabi.spmm_stream16(d_rowptr, col.size, plan, d_view, "sum", out=big[:, :k])
        torch.cuda.synchronize()
        assert out.data_ptr() == big.data_ptr() and out.stride(0) == 130
        _, ref16, _ = _ref(oracle_mod, ("view",), rowptr, col, val, x16, "sum")
        _assert_bits(out.contiguous(), ref16, "column view, output pitch 130")
        assert bool(torch.isnan(big[:, k:]).all()), "columns beyond k must not be touched"
    finally:
        plan.close()


def _planned(adj, geom, mat, reduce="sum"):
    """torch.ops.isplib.fusedmm_spmm[_mean]_planned on the graph's stream plan of `geom` (forward only)."""
    s = adj.storage
    plan = s.stream_plan(False, geom)
    op = torch.ops.isplib.fusedmm_spmm_mean_planned if reduce == "mean" else torch.ops.isplib.fusedmm_spmm_planned
    return op(s._rowptr, s._col, s._value, None, mat, None, None, plan, [])


@DT
def test_odd_pitch_and_odd_k_take_the_conversion_route(gpu, oracle_mod, dtype):
    """An odd pitch (65) and k = 41 are outside isplib_stream16_serves: through the operator they give the answer of the conversion
    route -- the fp32 operator on the widened operand, rounded once -- and no error."""
    import isplib_amd
    rowptr, col, val, (d_rowptr, d_col, d_val) = _small_graph(gpu)
    m, n = rowptr.size - 1, 120
    adj = isplib_amd.SparseTensor.from_csr(d_rowptr, d_col, d_val, (m, n))
    for k, pitch in ((64, 65), (41, 41), (64, 64)):
        wide = half_ref.to16(cases.dense(n, pitch, 6, "integer"), dtype).to(gpu)
        mat = wide[:, :k]
        for red in ("sum", "mean"):
            got = _planned(adj, (4, 3, 64), mat, red)
            want = _planned(adj, (4, 3, 64), mat.to(torch.float32), red).to(dtype)
            torch.cuda.synchronize()
            assert got.dtype == dtype and np.array_equal(half_ref.bits(got), half_ref.bits(want)), (k, pitch, red)
        _, ref16, _ = _ref(oracle_mod, ("odd", k, pitch), rowptr, col, val, mat.cpu().contiguous(), "sum")
        _assert_bits(_planned(adj, (4, 3, 64), mat, "sum"), ref16, f"k {k}, pitch {pitch}")


# ---- 6. operator and autograd, through patch_pyg() / matmul ----------------------------------------------------------------------

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


@DT
@pytest.mark.parametrize("weighted", (True, False), ids=("weighted", "unit"))
@pytest.mark.parametrize("red", ("sum", "mean"))
def test_matmul_forward_and_backward(gpu, oracle_mod, op_graph, monkeypatch, red, weighted, dtype):
    """Output and x.grad have x's dtype; the forward runs natively (`_last_schedule`); with integer operands the sum's x.grad is
    bit-equal to round16 of the oracle's A^T dY on the widened dY; mean meets the rounding bound against the oracle with fp32 scaling
    (a 1/deg-scaled dY kept in 16 bits would not); ISPLIB_HALF=convert gives the same bits."""
    import isplib_amd
    rowptr, col = op_graph
    m = n = 2000
    k = 64
    val = _weights(col.size) if weighted else np.ones(col.size, np.float32)
    d_val = torch.from_numpy(val).to(gpu) if weighted else None
    adj = isplib_amd.SparseTensor.from_csr(torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), d_val, (m, n))
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    g16 = half_ref.to16(cases.dense(m, k, 5, "integer"), dtype)
    monkeypatch.setenv("ISPLIB_STREAM_GEOM", "4:3:256")
    results = {}
    for mode in ("native", "convert"):
        monkeypatch.setenv("ISPLIB_HALF", mode)
        x = x16.to(gpu).requires_grad_(True)
        out = _matmul(adj, x, red)
        schedule = adj.storage._last_schedule
        out.backward(g16.to(gpu))
        torch.cuda.synchronize()
        assert out.dtype == dtype and x.grad.dtype == dtype
        assert schedule[0] == ("stream16" if mode == "native" else "convert"), schedule
        if mode == "convert":
            assert schedule[1] == "stream", schedule
        results[mode] = (out.detach(), x.grad.detach())
    for a, b in zip(results["native"], results["convert"]):
        assert np.array_equal(half_ref.bits(a), half_ref.bits(b)), "ISPLIB_HALF=convert: the same bits"
    out, grad = results["native"]
    ref32, ref16, tol = _ref(oracle_mod, ("op", weighted), rowptr, col, val, x16, red)
    g32 = half_ref.widen(g16)
    if red == "sum":
        _assert_bits(out, ref16, "forward")
        _assert_bits(grad, half_ref.round16(oracle_mod.spmm_sum_bw(rowptr, col, val, n, g32), dtype), "x.grad")
    else:
        _assert_bound(out, ref32, tol, dtype, "forward")
        colptr, new_row, new_w = oracle_mod.mean_bw_weights(rowptr, col, val, n)
        gref = oracle_mod.spmm_mean_bw(rowptr, col, val, n, g32)
        gtol = cases.sum_tolerance(oracle_mod, colptr, new_row, new_w, g32)
        _assert_bound(grad, gref, gtol, dtype, "x.grad")


@DT
def test_reference_schema_operator_with_16_bit_weights(gpu, oracle_mod, op_graph, dtype):
    """The reference-schema operator (no plan: the conversion route) with 16-bit weights, which it brings to fp32 (exact): forward
    and x.grad bit-equal to the rounded oracle; the A^T operands are built in the backward."""
    rowptr, col = op_graph
    n, k = 2000, 64
    val = _weights(col.size)
    d_rowptr, d_col = torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu)
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    g32 = cases.dense(n, k, 5, "integer")
    x = x16.to(gpu).requires_grad_(True)
    out = torch.ops.isplib.fusedmm_spmm(None, d_rowptr, d_col, torch.from_numpy(val).to(gpu).to(dtype), None, None, x, None, None)
    out.backward(torch.from_numpy(g32).to(gpu).to(dtype))
    torch.cuda.synchronize()
    _, ref16, _ = _ref(oracle_mod, ("op", True), rowptr, col, val, x16, "sum")
    _assert_bits(out, ref16, "forward with 16-bit weights")
    assert x.grad.dtype == dtype
    _assert_bits(x.grad, half_ref.round16(oracle_mod.spmm_sum_bw(rowptr, col, val, n, g32), dtype), "x.grad")


@DT
@pytest.mark.parametrize("red", ("max", "min"))
def test_max_min_take_the_conversion_route(gpu, op_graph, red, dtype):
    """max / min of a 16-bit x: 16-bit values equal to round16 of the fp32 operator's, positions equal to the fp32 operator's; the
    backward returns a 16-bit gradient equal to the rounded fp32 one."""
    rowptr, col = op_graph
    n, k = 2000, 64
    d_rowptr, d_col = torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu)
    d_val = torch.from_numpy(_weights(col.size)).to(gpu)
    x16 = half_ref.to16(cases.dense(n, k, 3, "uniform"), dtype).to(gpu)
    g16 = half_ref.to16(cases.dense(n, k, 5, "integer"), dtype).to(gpu)
    op = torch.ops.isplib.fusedmm_spmm_max if red == "max" else torch.ops.isplib.fusedmm_spmm_min
    x = x16.clone().requires_grad_(True)
    out, arg = op(d_rowptr, d_col, d_val, x)
    out.backward(g16)
    x32 = x16.to(torch.float32).requires_grad_(True)
    out32, arg32 = op(d_rowptr, d_col, d_val, x32)
    out32.backward(g16.to(torch.float32))
    torch.cuda.synchronize()
    assert out.dtype == dtype and x.grad.dtype == dtype
    assert np.array_equal(half_ref.bits(out), half_ref.bits(out32.detach().to(dtype))) and torch.equal(arg, arg32)
    assert np.array_equal(half_ref.bits(x.grad), half_ref.bits(x32.grad.to(dtype)))


@DT
def test_other_dtypes_are_refused_as_before(gpu, op_graph, dtype):
    import isplib_amd
    rowptr, col = op_graph
    d_rowptr, d_col = torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu)
    adj = isplib_amd.SparseTensor.from_csr(d_rowptr, d_col, None, (2000, 2000))
    x = torch.zeros((2000, 8), dtype=dtype, device=gpu)
    for bad in (x.to(torch.float64), x.to(torch.int32)):
        with pytest.raises(TypeError):
            isplib_amd.matmul(adj, bad, "sum")
        with pytest.raises(RuntimeError):
            torch.ops.isplib.fusedmm_spmm(None, d_rowptr, d_col, None, None, None, bad, None, None)
    with pytest.raises(RuntimeError):
        isplib_amd.matmul(adj, x.cpu(), "sum")
    with pytest.raises(RuntimeError):
        isplib_amd.gcn_norm_matmul(adj, x)                       # the fused epilogue stays fp32-only


@DT
def test_captured_graph_replays_to_the_same_bits(gpu, oracle_mod, op_graph, monkeypatch, dtype):
    import isplib_amd
    rowptr, col = op_graph
    n, k = 2000, 64
    val = _weights(col.size)
    adj = isplib_amd.SparseTensor.from_csr(torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), torch.from_numpy(val).to(gpu), (n, n))
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    monkeypatch.setenv("ISPLIB_STREAM_GEOM", "4:3:256")
    monkeypatch.setenv("ISPLIB_HALF", "native")
    x = x16.to(gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        eager = isplib_amd.matmul(adj, x, "sum")                  # builds the plan: nothing is built under capture
    torch.cuda.current_stream().wait_stream(side)
    assert adj.storage._last_schedule[0] == "stream16"
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


# ---- 7. refusals before any launch -----------------------------------------------------------------------------------------------

@DT
def test_entry_refuses_before_any_launch(gpu, dtype):
    """Each refused call returns a status, leaves the output as it was, and isplib_hip_last_error names the cause."""
    from isplib_amd import cabi
    rowptr, col, val, (d_rowptr, d_col, d_val) = _small_graph(gpu)
    m, n, k = rowptr.size - 1, 120, 64
    nnz = col.size
    plan = cabi.NativeStreamPlan(d_rowptr, d_col, d_val, n, 4, 3, 64, 2)
    mm_plan = cabi.NativeStreamPlan(d_rowptr, d_col, d_val, n, 4, 3, 64, 2, minmax=True)
    y = torch.ones((n, k), dtype=dtype, device=gpu)
    flat = torch.ones(n * k + 2, dtype=dtype, device=gpu)
    work = plan.workspace()
    SUM, MAX = cabi.MSG_SPMM_SUM, cabi.MSG_SPMM_MAX
    calls = (
        ("another shape", SUM, plan, torch.ones((n + 1, k), dtype=dtype, device=gpu), {}),
        ("isplib_stream16_serves", SUM, plan, y[:, :2], {}),                                      # k = 2
        ("isplib_stream16_serves", SUM, plan, torch.ones((n, 65), dtype=dtype, device=gpu)[:, :k], {}),   # odd ldy
        ("4-byte aligned", SUM, plan, flat[1:1 + n * k].view(n, k), {}),                          # a base at 2 bytes mod 4
        ("sum and mean only", MAX, plan, y, {}),
        ("bad plan geometry", SUM, mm_plan, y, {}),
        ("dtype", SUM, plan, y, {"dtype": 7}),
    )
    try:
        for cause, msg, p, yy, extra in calls:
            z = _nan_filled(m, yy.size(1), dtype, gpu)
            before = half_ref.bits(z).copy()
            st = cabi.fusedMM_csr_stream16_hip(msg, d_rowptr, nnz, p, yy, z, work, check=False, **extra)
            torch.cuda.synchronize()
            assert st != cabi.SUCCESS and cause in cabi.last_error(), (cause, st, cabi.last_error())
            assert np.array_equal(half_ref.bits(z), before), cause
        # the wrapper raises before the call
        with pytest.raises(ValueError):
            cabi.spmm_stream16(d_rowptr, nnz, plan, torch.ones((n + 1, k), dtype=dtype, device=gpu))
        with pytest.raises(ValueError):
            cabi.spmm_stream16(d_rowptr[:-1], nnz, plan, y)
        with pytest.raises(TypeError):
            cabi.spmm_stream16(d_rowptr, nnz, plan, y.to(torch.float32))
        with pytest.raises(ValueError):
            cabi.spmm_stream16(d_rowptr, nnz, plan, y, out=torch.empty((m, 65), dtype=dtype, device=gpu)[:, :k])
        with pytest.raises(ValueError):
            cabi.spmm_stream16(d_rowptr, nnz, plan, y, out=torch.empty((m, k), dtype=torch.float32, device=gpu))
        with pytest.raises(ValueError):
            cabi.spmm_stream16(d_rowptr, nnz, plan, y, "max")
    finally:
        plan.close()
        mm_plan.close()


# ---- 8. bit 31 of a gather offset ------------------------------------------------------------------------------------------------

def test_gather_offsets_past_2_gib_in_a_bf16_operand(gpu, oracle_mod):
    """n = 13.5 M rows of 80 bf16 columns: n * ldy * 2 = 2.16 GB, just above 2^31, so the 32-bit byte offsets of the gathers have
    bit 31 set for the top of X.  The operand is allocated uninitialised and only the rows the graph touches are written (integers);
    the graph is tests/test_gpu_address_edges.py's: first rows, last rows, the rows either side of byte 2^31, a 12,345-edge hub over
    the top of X.  Bit equality with round16(oracle) on the compacted rows.  Peak device memory: ~2.4 GB."""
    import gc
    from isplib_amd import cabi
    from tests.test_gpu_address_edges import _Graph
    n, k = 13_500_000, 80
    assert (1 << 31) < n * k * 2 < 0xE0000000 and n < (1 << 24)
    g = _Graph(n, k * 2, gpu, seed=15)
    assert g.far == [((1 << 31) + k * 2 - 1) // (k * 2)]
    xs16 = half_ref.to16(cases.dense(g.uniq.size, k, 3, "integer"), torch.bfloat16)
    x = torch.empty((n, k), dtype=torch.bfloat16, device=gpu)
    x[g.d_uniq] = xs16.to(gpu)
    try:
        for weighted in (True, False):
            d_w, w = g.weights(weighted)
            plan = cabi.NativeStreamPlan(g.rowptr, g.col, d_w, n, 4, 6, 512)
            try:
                out = _launch_twice(cabi, g.rowptr, g.nnz, plan, x, "sum")
            finally:
                plan.close()
            ref32, _ = oracle_mod.spmm_fw(g.rp, g.inv, w, half_ref.widen(xs16), "sum")
            _assert_bits(out, half_ref.round16(ref32, torch.bfloat16), f"past 2 GiB, weighted={weighted}")
    finally:
        del x
        gc.collect()
        torch.cuda.empty_cache()
