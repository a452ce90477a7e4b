"""16-bit features (bf16, fp16) for SpMM max / min on the plain row-per-wave kernel: fusedMM_csr_rows16_minmax_hip, through the C ABI,
the torch operators and the plug-in (opt-in: ISPLIB_HALF_MINMAX).

The contract needs no tolerance (include/isplib_hip.h): widening is exact, every comparison is fp32, the candidate replaces the running
value only if strictly better -- the first edge wins a tie, NaN never wins -- and the fp32 winner is rounded once.  So the bar of every
test is BIT EQUALITY of the 16-bit values with half_ref.reference (the oracle on the widened operand, rounded by torch's CPU cast) and
torch.equal of the positions with the same oracle call's, on real-valued data as on integers.  Outputs are prefilled with NaN and -1 so
an unwritten element shows, every launch runs twice to equal bits, and the values-only launch (no positions) must give the with-position
launch's value bits.  The inputs are tests/rows16_minmax_cases.py's: tests/test_rows16_minmax_host.py proves on the CPU that each holds
ties, a row in which nothing wins and an empty row.  The kernel's loop constants: a slot is LPR lanes (8 / 16 / 32 / 64 up to 64 / 128
/ 256 / 512 columns), G = 64 / LPR slots per wave, U = 2 / 3 / 6 gathers per slot and step by form (mm16_unroll), long_row = 2048."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests import rows16_minmax_cases as mm
from tests.test_gpu_stream_edges import _weights

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", tuple(half_ref.DTYPES.values()), ids=tuple(half_ref.DTYPES))
RED = pytest.mark.parametrize("red", ("max", "min"))

_refs = {}


def _ref(oracle, key, rowptr, col, val, x16, red):
    """(ref16, positions) once per (inputs, reduction), shared and left unchanged."""
    key = key + (x16.dtype, red)
    if key not in _refs:
        _, ref16, arg = mm.reference(oracle, rowptr, col, val, x16, red)
        arg.setflags(write=False)
        _refs[key] = (ref16, arg)
    return _refs[key]


def _on(gpu, *arrays):
    return tuple(None if a is None else torch.from_numpy(a).to(gpu) for a in arrays)


def _launch(d_rowptr, d_col, d_val, d_x, red, order=None):
    """With positions twice and values-only twice: (out, arg); all four value results bit-equal, both position results equal."""
    from isplib_amd import cabi
    m, k = d_rowptr.numel() - 1, d_x.size(1)
    outs, args = [], []
    for want_arg in (True, True, False, False):
        out = torch.full((m, k), float("nan"), dtype=d_x.dtype, device=d_x.device)
        arg = torch.full((m, k), -1, dtype=torch.int64, device=d_x.device) if want_arg else None
        o, a = cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, d_x, red, order=order, out=out, arg=arg, want_arg=want_arg)
        assert o is out and a is arg
        outs.append(half_ref.bits(out))
        args.append(arg)
    torch.cuda.synchronize()
    assert np.array_equal(outs[0], outs[1]) and torch.equal(args[0], args[1]), "two launches: equal bits"
    assert np.array_equal(outs[2], outs[3]), "two values-only launches: equal bits"
    bad = np.flatnonzero((outs[0] != outs[2]).reshape(m, -1).any(1))
    assert bad.size == 0, f"values-only differs from the launch with positions in rows {bad[:8].tolist()}"
    return out, args[0]


def _assert_equal(out, arg, ref16, ref_arg, what):
    bad = np.flatnonzero((half_ref.bits(out) != half_ref.bits(ref16)).reshape(ref16.shape[0], -1).any(1))
    assert bad.size == 0, f"{what}: values of rows {bad[:8].tolist()} ... differ from round16(oracle)"
    bad = np.flatnonzero((arg.cpu().numpy() != ref_arg).any(1))
    assert bad.size == 0, f"{what}: positions of rows {bad[:8].tolist()} ... differ from the oracle's"


def _run_case(gpu, oracle, key, rowptr, col, val, x16, red, order=None):
    unit = bool(np.all(val == 1.0))
    d_rowptr, d_col = _on(gpu, rowptr, col)
    d_val = None if unit else torch.from_numpy(val).to(gpu)
    out, arg = _launch(d_rowptr, d_col, d_val, x16.to(gpu), red, order)
    ref16, ref_arg = _ref(oracle, key, rowptr, col, val, x16, red)
    _assert_equal(out, arg, ref16, ref_arg, f"{key}, {red}")
    return out, arg, ref16, ref_arg


# ---- 1. every slot width and its ragged edge -------------------------------------------------------------------------------------

@DT
@RED
@pytest.mark.parametrize("k", mm.WIDTHS)
def test_every_slot_width_and_its_ragged_edge(gpu, oracle_mod, k, red, dtype):
    """One whole slot of every width and two columns more; 1024 is the widest single pass (64 lanes x 2 chunks x 8 columns) and 1026
    needs a second grid.y panel.  The hub row (2,500 edges) exceeds long_row.  Real-valued data, unit and weighted (negative weights
    flip the order)."""
    n_cases = 0
    for name, rowptr, col, val, x16 in mm.slot_cases(dtype, red):
        if name.startswith(f"k{k}-"):
            assert np.max(np.diff(rowptr)) > mm.LONG_ROW
            _run_case(gpu, oracle_mod, ("slot", name), rowptr, col, val, x16, red)
            n_cases += 1
    assert n_cases == 2


# ---- 2. row lengths around every loop edge ---------------------------------------------------------------------------------------

@DT
@RED
@pytest.mark.parametrize("k", (64, 256))
def test_row_lengths_around_every_loop_edge(gpu, oracle_mod, k, red, dtype):
    n_cases = 0
    for name, rowptr, col, val, x16 in mm.length_cases(dtype, red):
        if name.startswith(f"k{k}-"):
            _run_case(gpu, oracle_mod, ("lengths", name), rowptr, col, val, x16, red)
            n_cases += 1
    assert n_cases == 2


# ---- 3. ties and specials --------------------------------------------------------------------------------------------------------

@DT
@RED
def test_ties_and_specials(gpu, oracle_mod, red, dtype):
    """Integer features in [-3, 3] on the duplicate-edge hub graph: nearly every element ties and the position must be the oracle's
    lowest edge.  Planted: a column of alternating +0 / -0, a graph row whose sources are all NaN, a source row of -Inf under max
    (+Inf under min) and a graph row reading nothing else, NaN among finite values, +-Inf winners, and a weighted product beyond the
    largest fp16 (30000 x 3 and more) that is finite in fp32.  Rows in which nothing wins show -+Inf and position nnz."""
    lose = float("-inf") if red == "max" else float("inf")
    for name, rowptr, col, val, x16 in mm.tie_cases(dtype, red):
        out, arg, ref16, ref_arg = _run_case(gpu, oracle_mod, ("ties", name), rowptr, col, val, x16, red)
        nnz = col.size
        none = torch.from_numpy((ref_arg == nnz) & (np.diff(rowptr) > 0)[:, None])
        assert bool(none.any()), name
        assert bool((out.cpu().to(torch.float32)[none] == lose).all()) and bool((arg.cpu()[none] == nnz).all()), name
        got = out.cpu().to(torch.float32)
        if name.startswith("hub"):
            assert bool(torch.isinf(got[~none]).any()), f"{name}: an infinite winner"
        if name.startswith("hub") and name.endswith("weighted"):
            assert bool(((got[:, 0] == 0) & torch.signbit(got[:, 0])).any()) and bool(((got[:, 0] == 0) & ~torch.signbit(got[:, 0])).any())
            if dtype == torch.float16:
                ref32, _, _ = mm.reference(oracle_mod, rowptr, col, val, x16, red)
                over = np.isfinite(ref32) & (np.abs(ref32) > 65520.0) & (np.abs(ref32) < mm.FLT_MAX)
                assert over.any() and bool(torch.isinf(got[torch.from_numpy(over)]).all()), "beyond fp16, finite in fp32"


# ---- 4. the empty-row switch -----------------------------------------------------------------------------------------------------

@DT
@RED
def test_empty_row_switch(gpu, oracle_mod, red, dtype):
    """isplib_hip_set_empty_row: an empty row is 0, or the identity -+FLT_MAX, which rounds to -+Inf; its position is nnz either way."""
    from isplib_amd import cabi
    rowptr, col = mm.hub_graph()
    val = mm.weights_of(col, False)
    x16 = mm.operand(rowptr, col, 200, 64, 3, "uniform", dtype)
    empty = torch.from_numpy(np.flatnonzero(np.diff(rowptr) == 0))
    try:
        for mode, value in (("init", float("-inf") if red == "max" else float("inf")), ("zero", 0.0)):
            cabi.set_empty_row(mode)
            oracle_mod.set_empty_row(mode)
            out, arg, _, _ = _run_case(gpu, oracle_mod, ("empty", mode), rowptr, col, val, x16, red)
            assert bool((out.cpu().to(torch.float32)[empty] == value).all()) and bool((arg.cpu()[empty] == col.size).all()), mode
    finally:
        cabi.set_empty_row("zero")
        oracle_mod.set_empty_row("zero")


# ---- 5. row order ----------------------------------------------------------------------------------------------------------------

@DT
@RED
@pytest.mark.parametrize("k", (64, 256))
def test_any_row_order_gives_the_bits_of_index_order(gpu, oracle_mod, k, red, dtype):
    rowptr, col = mm.hub_graph()
    m = rowptr.size - 1
    val = mm.weights_of(col, False)
    x16 = mm.operand(rowptr, col, 200, k, 3, "uniform", dtype)
    base_out, base_arg, _, _ = _run_case(gpu, oracle_mod, ("slot", f"k{k}-weighted"), rowptr, col, val, x16, red)
    d_rowptr, d_col, d_val = _on(gpu, rowptr, col, val)
    for o in (np.random.default_rng(5).permutation(m), np.arange(m)[::-1].copy()):
        out, arg = _launch(d_rowptr, d_col, d_val, x16.to(gpu), red, torch.from_numpy(o.astype(np.int32)).to(gpu))
        assert np.array_equal(half_ref.bits(out), half_ref.bits(base_out)) and torch.equal(arg, base_arg)


# ---- 6. pitches and pads ---------------------------------------------------------------------------------------------------------

@DT
@RED
def test_pitches_and_pads(gpu, oracle_mod, red, dtype):
    """y a [n, 64] column block of a [n, 192] tensor, z a block of a [m, 130] buffer, the positions a block of a [m, 132] buffer: each
    at its own pitch, nothing beside the 64 columns touched.  And k = 130 with every base 4-byte but not 16-byte aligned."""
    from isplib_amd import cabi
    rowptr, col = mm.hub_graph()
    m, n, k = rowptr.size - 1, 200, 64
    val = mm.weights_of(col, False)
    d_rowptr, d_col, d_val = _on(gpu, rowptr, col, val)
    wide = mm.operand(rowptr, col, n, 192, 5, "uniform", dtype)
    x16 = wide[:, 64:128].contiguous()
    d_view = wide.to(gpu)[:, 64:128]
    assert d_view.stride(0) == 192
    big = torch.full((m, 130), float("nan"), dtype=dtype, device=gpu)
    big_arg = torch.full((m, 132), -1, dtype=torch.int64, device=gpu)
    out, arg = cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, d_view, red, out=big[:, 2:2 + k], arg=big_arg[:, 3:3 + k])
    torch.cuda.synchronize()
    assert out.data_ptr() == big[:, 2:].data_ptr() and out.stride(0) == 130 and arg.stride(0) == 132
    ref16, ref_arg = _ref(oracle_mod, ("view",), rowptr, col, val, x16, red)
    _assert_equal(out.contiguous(), arg.contiguous(), ref16, ref_arg, "column view, output pitches 130 / 132")
    assert bool(torch.isnan(big[:, :2]).all()) and bool(torch.isnan(big[:, 2 + k:]).all()), "z pads must not be touched"
    assert bool((big_arg[:, :3] == -1).all()) and bool((big_arg[:, 3 + k:] == -1).all()), "position pads must not be touched"
    # k = 130: a ragged last vector; y, z at 4 bytes mod 16 and the positions at 8 bytes mod 16
    k = 130
    x16 = mm.operand(rowptr, col, n, k, 7, "uniform", dtype)
    fy = torch.zeros(n * k + 8, dtype=dtype, device=gpu)
    fz = torch.full((m * k + 8,), float("nan"), dtype=dtype, device=gpu)
    fa = torch.full((m * k + 8,), -1, dtype=torch.int64, device=gpu)
    fy[2:2 + n * k] = x16.to(gpu).reshape(-1)
    y, z, a = fy[2:2 + n * k].view(n, k), fz[2:2 + m * k].view(m, k), fa[1:1 + m * k].view(m, k)
    assert y.data_ptr() % 16 == 4 and z.data_ptr() % 16 == 4 and a.data_ptr() % 16 == 8
    cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, y, red, out=z, arg=a)
    torch.cuda.synchronize()
    ref16, ref_arg = _ref(oracle_mod, ("offset",), rowptr, col, val, x16, red)
    _assert_equal(z, a, ref16, ref_arg, "k = 130 at a 4-byte-aligned base")
    assert bool(torch.isnan(fz[:2]).all()) and bool(torch.isnan(fz[2 + m * k:]).all()) and bool((fa[:1] == -1).all()) and bool((fa[1 + m * k:] == -1).all())


# ---- 7. refusals before any launch -----------------------------------------------------------------------------------------------

@DT
def test_entry_refuses_before_any_launch(gpu, dtype):
    """Each refused call returns the documented status, leaves both outputs as they were, and isplib_hip_last_error names the cause."""
    from isplib_amd import cabi
    rowptr, col = cases.random_csr(150, 120, 9.0, 21, empty_rows=(4,), hub=(9, 700), duplicates=True)
    m, n, k = 150, 120, 64
    d_rowptr, d_col, d_val = _on(gpu, rowptr, col, _weights(col.size))
    y = torch.ones((n, k), dtype=dtype, device=gpu)
    y66 = torch.ones((n, 66), dtype=dtype, device=gpu)
    flat = torch.ones(n * k + 2, dtype=dtype, device=gpu)
    SUM, MAX, MIN, FAIL, NO = cabi.MSG_SPMM_SUM, cabi.MSG_SPMM_MAX, cabi.MSG_SPMM_MIN, cabi.FAIL, cabi.NO_OPT_IMPL
    calls = (
        ("max and min only", NO, SUM, y, {}),
        ("max and min only", NO, cabi.MSG_SPMM_MEAN, y, {}),
        ("isplib_rows16_serves", FAIL, MAX, y, {"k": 63}),                                        # odd k
        ("isplib_rows16_serves", FAIL, MIN, y, {"k": 6}),                                         # k < 8
        ("isplib_rows16_serves", FAIL, MAX, torch.ones((n, 65), dtype=dtype, device=gpu)[:, :k], {}),   # odd ldy
        ("isplib_rows16_serves", FAIL, MIN, y, {"ldz": 65}),                                      # odd ldz
        ("4-byte aligned", FAIL, MAX, flat[1:1 + n * k].view(n, k), {}),                          # a base at 2 bytes mod 4
        ("dtype", FAIL, MAX, y, {"dtype": 0}),                                                    # what an fp32 tensor maps to
        ("leading dimension", FAIL, MIN, y66[:, :k], {"ldz": 62}),                                # ldz < k
        ("leading dimension", FAIL, MAX, y, {"ldarg": 62}),                                       # ldarg < k
    )
    for cause, status, msg, yy, extra in calls:
        z = torch.full((m, 66), float("nan"), dtype=dtype, device=gpu)
        za = torch.full((m, 66), -1, dtype=torch.int64, device=gpu)
        st = cabi.fusedMM_csr_rows16_minmax_hip(msg, d_rowptr, d_col, d_val, None, yy, z[:, :k], za[:, :k], check=False, **extra)
        torch.cuda.synchronize()
        assert st == status and cause in cabi.last_error(), (cause, st, cabi.last_error())
        assert bool(torch.isnan(z).all()) and bool((za == -1).all()), cause
    # nothing to do is a success
    empty_rp = torch.zeros(1, dtype=torch.int64, device=gpu)
    assert cabi.fusedMM_csr_rows16_minmax_hip(MAX, empty_rp, d_col[:0], None, None, y, torch.empty((0, k), dtype=dtype, device=gpu), check=False) == cabi.SUCCESS
    assert cabi.fusedMM_csr_rows16_minmax_hip(MIN, d_rowptr, d_col, None, None, y[:, :0], torch.empty((m, 0), dtype=dtype, device=gpu), check=False) == cabi.SUCCESS
    # the wrapper raises before the call
    with pytest.raises(ValueError):
        cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, y[:, :6])
    with pytest.raises(ValueError):
        cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, y[:100])                      # column ids beyond n
    with pytest.raises(ValueError):
        cabi.spmm_rows16_minmax(d_rowptr, d_col[:-1], d_val, y)
    with pytest.raises(TypeError):
        cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, y.to(torch.float32))
    with pytest.raises(ValueError):
        cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, y, out=torch.empty((m, 65), dtype=dtype, device=gpu)[:, :k])
    with pytest.raises(ValueError):
        cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, y, arg=torch.empty((m, k), dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError):
        cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, y, "sum")
    with pytest.raises(ValueError):
        cabi.spmm_rows16_minmax(d_rowptr, d_col, d_val, y, order=torch.zeros(m - 1, dtype=torch.int32, device=gpu))


# ---- 8. byte offsets past 2 GiB, up to the descriptor's limit --------------------------------------------------------------------

def test_gather_offsets_up_to_the_descriptor_limit_in_a_bf16_operand(gpu, oracle_mod):
    """n x 64 bf16 with n * ldy * 2 = 0xE0000000 exactly (the largest operand isplib_rows16_serves admits): the 32-bit byte offsets of
    the gathers run up to 3.5 GiB.  The operand is allocated uninitialised and only the rows the graph touches are written: the first
    rows, the last rows, the rows either side of byte 2^31, and a long row over all of them.  Values and positions equal the oracle's
    on the compacted rows.  Peak device memory: ~3.8 GB."""
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
    xs16 = half_ref.to16(cases.dense(uniq.size, k, 3, "uniform"), torch.bfloat16)
    x = torch.empty((n, k), dtype=torch.bfloat16, device=gpu)
    try:
        x[torch.from_numpy(uniq).to(gpu)] = xs16.to(gpu)
        d_rowptr, d_col = _on(gpu, rowptr, col)
        for red in ("max", "min"):
            for weighted in (True, False):
                w = mm.weights_of(col, not weighted)
                out, arg = _launch(d_rowptr, d_col, torch.from_numpy(w).to(gpu) if weighted else None, x, red)
                _, ref16, ref_arg = mm.reference(oracle_mod, rowptr, inv, w, xs16, red)
                _assert_equal(out, arg, ref16, ref_arg, f"up to 3.5 GiB, {red}, weighted={weighted}")
    finally:
        del x
        gc.collect()
        torch.cuda.empty_cache()


# ---- 9. operators ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def op_graph():
    rowptr, col = cases.random_csr(2000, 2000, 8.0, 51, empty_rows=(0, 1999), hub=(11, 1500), duplicates=True)
    return rowptr, col


def _adj(gpu, op_graph, weighted):
    import isplib_amd
    rowptr, col = op_graph
    val = mm.weights_of(col, not weighted)
    d_val = torch.from_numpy(val).to(gpu) if weighted else None
    return isplib_amd.SparseTensor.from_csr(torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), d_val, (2000, 2000)), val


def _row_plan(gpu):
    return [torch.empty(0, dtype=torch.int32, device=gpu), torch.tensor([16], dtype=torch.int32)]


@DT
@RED
@pytest.mark.parametrize("weighted", (True, False), ids=("weighted", "unit"))
def test_planned_operators_on_a_row_plan(gpu, oracle_mod, op_graph, weighted, red, dtype):
    """fusedmm_spmm_{max,min}_planned with a 16-bit row plan: a 16-bit output bit-equal to the rounded oracle, the oracle's positions,
    and positions and x.grad equal to the fp32 operator's on the widened x (its x.grad rounded once); the _values operator returns
    the same value bits; an x that starts at an odd element is copied, and nothing raises."""
    rowptr, col = op_graph
    n, k = 2000, 64
    adj, val = _adj(gpu, op_graph, weighted)
    s = adj.storage
    ops = torch.ops.isplib
    planned = ops.fusedmm_spmm_max_planned if red == "max" else ops.fusedmm_spmm_min_planned
    values = ops.fusedmm_spmm_max_values if red == "max" else ops.fusedmm_spmm_min_values
    x16 = mm.operand(rowptr, col, n, k, 3, "uniform", dtype)
    g16 = half_ref.to16(cases.dense(n, k, 5, "uniform"), dtype).to(gpu)
    ref16, ref_arg = _ref(oracle_mod, ("op", weighted), rowptr, col, val, x16, red)
    x32 = x16.to(gpu).to(torch.float32).requires_grad_(True)
    out32, arg32 = planned(s._rowptr, s._col, s._value, x32, [])
    out32.backward(g16.to(torch.float32))
    flat = torch.zeros(n * k + 2, dtype=dtype, device=gpu)
    flat[1:1 + n * k] = x16.to(gpu).reshape(-1)
    odd = flat[1:1 + n * k].view(n, k)
    assert odd.is_contiguous() and odd.data_ptr() % 4 == 2
    for name, x in (("aligned", x16.to(gpu)), ("odd offset", odd.detach())):
        x = x.requires_grad_(True)
        out, arg = planned(s._rowptr, s._col, s._value, x, _row_plan(gpu))
        out.backward(g16)
        torch.cuda.synchronize()
        assert out.dtype == dtype and x.grad.dtype == dtype and arg.dtype == torch.int64
        _assert_equal(out, arg, ref16, ref_arg, f"planned, {name}")
        assert torch.equal(arg, arg32) and np.array_equal(half_ref.bits(out), half_ref.bits(out32.detach().to(dtype)))
        assert np.array_equal(half_ref.bits(x.grad), half_ref.bits(x32.grad.to(dtype))), f"x.grad, {name}"
        with torch.no_grad():
            only = values(s._rowptr, s._col, s._value, x.detach(), _row_plan(gpu))
        assert only.dtype == dtype and np.array_equal(half_ref.bits(only), half_ref.bits(out)), f"_values, {name}"


# ---- 10. plug-in -----------------------------------------------------------------------------------------------------------------

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


@DT
@RED
def test_plugin_route_is_opt_in(gpu, oracle_mod, op_graph, monkeypatch, red, dtype):
    """With the stream schedule off the plain kernel serves this graph.  ISPLIB_HALF_MINMAX=native runs the 16-bit kernel, forward and
    (through the positions it saved) backward; unset and `convert` convert as before; `auto` follows the measured rule;
    ISPLIB_HALF=convert wins over `native`.  Every route gives the same bits, and only the conversion route allocates an fp32 copy."""
    from isplib_amd import cabi
    rowptr, col = op_graph
    n, k = 2000, 64
    adj, val = _adj(gpu, op_graph, True)
    x16 = mm.operand(rowptr, col, n, k, 3, "uniform", dtype)
    g16 = half_ref.to16(cases.dense(n, k, 5, "uniform"), dtype).to(gpu)
    ref16, _ = _ref(oracle_mod, ("op", True), rowptr, col, val, x16, red)
    monkeypatch.setenv("ISPLIB_STREAM", "0")
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_MINMAX", raising=False)
    results = {}
    for mode in (None, "convert", "native", "auto"):
        if mode is not None:
            monkeypatch.setenv("ISPLIB_HALF_MINMAX", mode)
        x = x16.to(gpu).requires_grad_(True)
        out = _matmul(adj, x, red)
        schedule = adj.storage._last_schedule
        out.backward(g16)
        with torch.no_grad():
            peak, only = _peak_during(lambda: _matmul(adj, x.detach(), red))
        inference = adj.storage._last_schedule
        native = mode == "native"
        assert schedule[0] == ("rows16mm" if native or (mode == "auto" and cabi.rows16_minmax_native_pays(n, k, False, True, True)) else "convert"), (mode, schedule)
        assert inference[0] == ("rows16mm" if native or (mode == "auto" and cabi.rows16_minmax_native_pays(n, k, False, True, False)) else "convert"), (mode, inference)
        if inference[0] == "rows16mm":
            assert peak < n * k * 4, f"{mode}: a no-grad native call allocated {peak} bytes, an fp32 copy of X is {n * k * 4}"
        else:
            assert peak >= n * k * 4, (mode, peak)
        assert out.dtype == dtype and x.grad.dtype == dtype
        assert np.array_equal(half_ref.bits(out), half_ref.bits(ref16)) and np.array_equal(half_ref.bits(only), half_ref.bits(ref16)), mode
        results[mode] = half_ref.bits(x.grad).copy()
    for mode in ("convert", "native", "auto"):
        assert np.array_equal(results[mode], results[None]), f"x.grad, {mode}"
    monkeypatch.setenv("ISPLIB_HALF_MINMAX", "native")
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    _matmul(adj, x16.to(gpu), red)
    assert adj.storage._last_schedule[0] == "convert", adj.storage._last_schedule
