"""The five kernels on the stream front end (sweep_common.h: StreamWave, stream_bounds, stream_load_batch, stream_issue and the
three-batch word rotation with the weights one batch behind) at every wave length, plan shape and builder edge that the
Poisson-degree graphs of the other modules meet only by accident: tests/cases.py builds inputs whose plan is KNOWN
(tests/test_host.py proves the step counts and plan shapes on the CPU), and here they run against the oracle.

Operands are small integers throughout, and the weights differ between neighbouring CSR positions (1 + pos % 5, signed by
parity): every sum is exact in fp32 whatever its order, a weight paired with another word changes the answer, and so does a
step dropped or taken twice.  The bar is therefore BIT EQUALITY with the oracle -- sum, max / min values and positions, the
FusedMM words with the `scale` menu function at 0.25, the SDDMM's dot products -- and cases.sum_tolerance (BASELINE.md
section 3) for mean, which divides."""
import numpy as np
import pytest
import torch

from tests import cases
from tests.test_gpu_sweep import _check, _stream_all, _stream_minmax_all, _t

pytestmark = pytest.mark.gpu

N = 97                       # columns of the ladder and uneven-wave graphs
CHUNK = 256                  # above the longest row of either: no hub rows
UNEVEN = (1, 31, 32, 33, 64, 97)


def _weights(nnz):
    pos = np.arange(nnz)
    return ((1 + pos % 5) * np.where(pos % 2 == 0, 1, -1)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_refs = {}


def _ref(oracle, key, rowptr, col, val, x, red):
    """The oracle's answer, computed once per (graph, operands, reduction) and shared by the tests that ask for it."""
    key = key + (red,)
    if key not in _refs:
        out, arg = oracle.spmm_fw(rowptr, col, val, x, red)
        out.setflags(write=False)
        if arg is not None:
            arg.setflags(write=False)
        _refs[key] = (out, arg)
    return _refs[key]


def _graph(kind, streams, length=None):
    if kind == "ladder":
        return cases.stream_ladder(streams, cases.LADDER, N, seed=streams), len(cases.LADDER)
    return cases.stream_uneven_wave(streams, length, N, seed=streams + length), 1


def _rungs(rowptr, streams, bad_rows):
    """The steps of the waves that own `bad_rows` (row r of a ladder graph is on wave r // streams): what a failure names."""
    deg = np.diff(rowptr)
    return sorted({int(deg[r]) for r in bad_rows}, reverse=True)


def _exact(name, rowptr, streams, got, ref):
    bad = np.flatnonzero((_bits(got) != _bits(ref)).reshape(ref.shape[0], -1).any(1))
    assert bad.size == 0, f"{name}: rows of {_rungs(rowptr, streams, bad)} edges differ from the oracle (rows {bad[:8].tolist()} ...)"


def _plans(gpu, rowptr, col, val, streams, wpg, slices, minmax=False, fusedmm=False):
    """The same plan from both builders, with the step counts the constructor promises."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_stream_plan
    d_rowptr, d_col = _t(rowptr, gpu), _t(col, gpu)
    d_val = None if val is None else _t(val, gpu)
    plans = []
    if not fusedmm:
        plans.append(("torch", build_stream_plan(d_rowptr, d_col, d_val, N, slices, wpg, None, streams, CHUNK, minmax=minmax)))
    plans.append(("native", cabi.NativeStreamPlan(d_rowptr, d_col, d_val, N, streams, slices, CHUNK, wpg, minmax=minmax, fusedmm=fusedmm)))
    return plans


def _steps(plan):
    off = plan.array("wave_step_off") if hasattr(plan, "array") else plan.wave_step_off
    return np.diff(off.cpu().numpy()).tolist()


def _sum_mean(gpu, oracle, key, rowptr, col, streams, wpg, k, unit, want_steps):
    from isplib_amd import cabi
    val = np.ones(col.size, np.float32) if unit else _weights(col.size)
    x = cases.dense(N, k, 3, "integer")
    d_rowptr, d_x = _t(rowptr, gpu), _t(x, gpu)
    for builder, plan in _plans(gpu, rowptr, col, None if unit else val, streams, wpg, slices=3):
        assert _steps(plan) == want_steps and plan.gens == 1 and plan.n_hub == 0, builder
        for red in ("sum", "mean"):
            out = cabi.spmm_stream(d_rowptr, col.size, plan, d_x, red)
            again = cabi.spmm_stream(d_rowptr, col.size, plan, d_x, red)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "bitwise reproducible"
            ref, _ = _ref(oracle, key + (k, unit), rowptr, col, val, x, red)
            if red == "sum":
                _exact(f"sum, {builder} plan", rowptr, streams, out.cpu().numpy(), ref)
            else:
                _check(oracle, rowptr, col, val, x, red, out, None)
        if builder == "native":
            plan.close()


def _max_min(gpu, oracle, key, rowptr, col, streams, wpg, k, unit, want_steps):
    from isplib_amd import cabi
    val = np.ones(col.size, np.float32) if unit else _weights(col.size)
    x = cases.dense(N, k, 3, "integer")
    d_rowptr, d_x = _t(rowptr, gpu), _t(x, gpu)
    for builder, plan in _plans(gpu, rowptr, col, None if unit else val, streams, wpg, slices=3, minmax=True):
        assert _steps(plan) == want_steps and plan.gens == 1 and plan.n_hub == 0, builder
        for red in ("max", "min"):
            out, arg = cabi.spmm_stream_minmax(d_rowptr, col.size, plan, d_x, red)
            values, none = cabi.spmm_stream_minmax(d_rowptr, col.size, plan, d_x, red, want_arg=False)
            torch.cuda.synchronize()
            ref, ref_arg = _ref(oracle, key + (k, unit), rowptr, col, val, x, red)
            _exact(f"{red}, {builder} plan", rowptr, streams, out.cpu().numpy(), ref)
            _exact(f"{red} positions, {builder} plan", rowptr, streams, arg.cpu().numpy().astype(np.int32), ref_arg.astype(np.int32))
            assert none is None and torch.equal(out.view(torch.int32), values.view(torch.int32)), "values-only launch: the same values"
        if builder == "native":
            plan.close()


def _fusedmm_words(gpu, oracle, rowptr, col, streams, wpg, k, want_steps):
    from isplib_amd import cabi
    m = rowptr.size - 1
    x, y = cases.dense(m, k, 3, "integer"), cases.dense(N, k, 5, "integer")
    d_rowptr = _t(rowptr, gpu)
    (_, plan), = _plans(gpu, rowptr, col, None, streams, wpg, slices=3, fusedmm=True)
    assert _steps(plan) == want_steps and plan.rows_per_wave == cabi.fusedmm_stream_geometry(streams)[0]
    for name in ("sigmoid_embedding", "tdist_embedding"):
        word = cabi.PATTERNS[name][0]
        st, ref, _ = oracle.fusedmm_general(word, rowptr, col, None, x, y, cabi.SOP_UDEF["scale"], 0.25)
        st2, z = cabi.fusedmm_stream(word, d_rowptr, col.size, plan, _t(x, gpu), _t(y, gpu), sop_udef="scale", sop_param=0.25)
        assert st == 0 and st2 == 0
        _exact(name, rowptr, streams, z.cpu().numpy(), ref)
    plan.close()


def _sddmm(gpu, oracle, rowptr, col, streams, wpg, k, want_steps):
    """The SDDMM writes per edge: a step lost, doubled or paired with another position names itself."""
    from isplib_amd import cabi
    m = rowptr.size - 1
    y, g = cases.dense(N, k, 3, "integer"), cases.dense(m, k, 5, "integer")
    d_rowptr = _t(rowptr, gpu)
    ref = oracle.sddmm(rowptr, col, y, g)
    erow = np.repeat(np.arange(m), np.diff(rowptr))
    for builder, plan in _plans(gpu, rowptr, col, None, streams, wpg, slices=3):
        assert _steps(plan) == want_steps, builder
        got = cabi.sddmm_stream(d_rowptr, col.size, plan, _t(y, gpu), _t(g, gpu), False).cpu().numpy()
        bad = np.flatnonzero(_bits(got) != _bits(ref))
        assert bad.size == 0, f"sddmm, {builder} plan: edges of rows of {_rungs(rowptr, streams, erow[bad])} edges differ (positions {bad[:8].tolist()} ...)"
        if builder == "native":
            plan.close()


def _hybrid(gpu, oracle, rowptr, col, streams, wpg, k, want_steps):
    """Unit weights.  Without hot rows (min_refs beyond any in-degree) the cold stream IS the plan of the ladder; with them the
    deal goes by cold length and the hot chunks run beside it: the same exact answer either way."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_hybrid_plan
    val = np.ones(col.size, np.float32)
    x = cases.dense(N, k, 3, "integer")
    d_rowptr, d_col, d_x = _t(rowptr, gpu), _t(col, gpu), _t(x, gpu)
    ref, _ = oracle.spmm_fw(rowptr, col, val, x, "sum")
    for min_refs in (1 << 30, 2):
        plan = build_hybrid_plan(d_rowptr, d_col, N, 3, streams, CHUNK, waves_per_gen=wpg, min_refs=min_refs)
        assert plan is not None and plan.hot_edges + int((plan.cold.perm >= 0).sum()) == col.size
        if min_refs > 2:
            assert plan.hot_edges == 0 and _steps(plan.cold) == want_steps
        elif col.size > 2 * N:
            assert plan.hot_edges > 0
        for red in ("sum", "mean"):
            out = cabi.spmm_hybrid(d_rowptr, col.size, plan, d_x, red)
            again = cabi.spmm_hybrid(d_rowptr, col.size, plan, d_x, red)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "bitwise reproducible"
            if red == "sum":
                _exact(f"hybrid sum, min_refs {min_refs}", rowptr, streams, out.cpu().numpy(), ref)
            else:
                _check(oracle, rowptr, col, val, x, red, out, None)


# ---- the ladder: wave w walks exactly cases.LADDER[w] steps ------------------------------------------------------------------

@pytest.mark.parametrize("unit", (False, True), ids=("weighted", "unit"))
@pytest.mark.parametrize("streams,k", ((2, 128), (2, 100), (4, 64), (8, 32)))
def test_ladder_sum_mean(gpu, oracle_mod, streams, k, unit):
    (rowptr, col), wpg = _graph("ladder", streams)
    _sum_mean(gpu, oracle_mod, ("ladder", streams), rowptr, col, streams, wpg, k, unit, list(cases.LADDER))


@pytest.mark.parametrize("unit", (False, True), ids=("weighted", "unit"))
@pytest.mark.parametrize("streams,k", ((4, 64), (8, 32)))
def test_ladder_max_min(gpu, oracle_mod, streams, k, unit):
    (rowptr, col), wpg = _graph("ladder", streams)
    _max_min(gpu, oracle_mod, ("ladder", streams), rowptr, col, streams, wpg, k, unit, list(cases.LADDER))


@pytest.mark.parametrize("streams,k", ((2, 128), (4, 64), (8, 32)))
def test_ladder_fusedmm_words(gpu, oracle_mod, streams, k):
    (rowptr, col), wpg = _graph("ladder", streams)
    _fusedmm_words(gpu, oracle_mod, rowptr, col, streams, wpg, k, list(cases.LADDER))


@pytest.mark.parametrize("streams,k", ((2, 128), (4, 64), (8, 32)))
def test_ladder_sddmm(gpu, oracle_mod, streams, k):
    (rowptr, col), wpg = _graph("ladder", streams)
    _sddmm(gpu, oracle_mod, rowptr, col, streams, wpg, k, list(cases.LADDER))


@pytest.mark.parametrize("streams,k", ((4, 64), (8, 32)))
def test_ladder_hybrid(gpu, oracle_mod, streams, k):
    """The hybrid's workgroups are eight waves: the ladder with two more waves of no steps (24 waves per generation)."""
    lengths = cases.LADDER + (0, 0)
    rowptr, col = cases.stream_ladder(streams, lengths, N, seed=streams)
    _hybrid(gpu, oracle_mod, rowptr, col, streams, len(lengths), k, list(lengths))


# ---- one wave whose slots are of very different lengths: most words of all slots but one are padding -----------------------------

@pytest.mark.parametrize("length", UNEVEN)
def test_uneven_wave_sum_mean(gpu, oracle_mod, length):
    for streams, k in ((2, 128), (4, 64), (8, 32)):
        (rowptr, col), wpg = _graph("uneven", streams, length)
        for unit in (False, True):
            _sum_mean(gpu, oracle_mod, ("uneven", streams, length), rowptr, col, streams, wpg, k, unit, [length])


@pytest.mark.parametrize("length", UNEVEN)
def test_uneven_wave_max_min(gpu, oracle_mod, length):
    for streams, k in ((4, 64), (8, 32)):
        (rowptr, col), wpg = _graph("uneven", streams, length)
        for unit in (False, True):
            _max_min(gpu, oracle_mod, ("uneven", streams, length), rowptr, col, streams, wpg, k, unit, [length])


@pytest.mark.parametrize("length", UNEVEN)
def test_uneven_wave_fusedmm_sddmm_hybrid(gpu, oracle_mod, length):
    for streams, k in ((2, 128), (4, 64), (8, 32)):
        (rowptr, col), wpg = _graph("uneven", streams, length)
        _fusedmm_words(gpu, oracle_mod, rowptr, col, streams, wpg, k, [length])
        _sddmm(gpu, oracle_mod, rowptr, col, streams, wpg, k, [length])
    for streams, k in ((4, 64), (8, 32)):                       # eight waves per generation: the wave and seven without rows
        rowptr, col = cases.stream_uneven_wave(streams, length, N, seed=streams + length)
        _hybrid(gpu, oracle_mod, rowptr, col, streams, 8, k, [length] + [0] * 7)


# ---- the plan's shape: both builders, every array identical, every row written ---------------------------------------------------

SHAPE_NAMES = tuple(c[0] for c in cases.stream_shape_cases())
PLAN_ARRAYS = ("words", "perm", "vals", "wave_step_off", "wave_row", "wave_part", "hub_row", "hub_off")
PLAN_FIELDS = ("gens", "waves_per_gen", "rows_per_wave", "streams", "n_steps", "n_parts", "n_hub", "slices")


@pytest.mark.parametrize("minmax", (False, True), ids=("sum_mean", "max_min"))
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_shape_cases_from_both_builders(gpu, oracle_mod, name, minmax):
    """Every case of cases.stream_shape_cases through isplib_amd.plan.build_stream_plan and the library's own builder (what the
    plug-in and the C handle use): the same plan, array by array, and the oracle's answer through either.  z is prefilled with
    7 and z_arg with -5, so a row that nobody wrote shows as a mismatch; the plain kernel is held to the same answer."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_stream_plan
    geometry = cabi.stream_minmax_geometry if minmax else cabi.stream_geometry
    shapes = {c[0]: c[1:] for c in cases.stream_shape_cases(geometry(4)[0])}
    rowptr, col, n, (slices, wpg, streams, chunk) = shapes[name]
    m, k = rowptr.size - 1, 37
    val = _weights(col.size)
    x = cases.dense(n, k, 3, "integer")
    d_rowptr, d_col, d_val, d_x = _t(rowptr, gpu), _t(col, gpu), _t(val, gpu), _t(x, gpu)
    ref_plan = build_stream_plan(d_rowptr, d_col, d_val, n, slices, wpg, None, streams, chunk, minmax=minmax)
    nat = cabi.NativeStreamPlan(d_rowptr, d_col, d_val, n, streams, slices, chunk, wpg, minmax=minmax)
    try:
        assert ref_plan is not None and ref_plan.rows_per_wave == geometry(streams)[0]
        for field in PLAN_FIELDS:
            assert getattr(nat, field) == getattr(ref_plan, field), field
        for array in PLAN_ARRAYS:
            want = getattr(ref_plan, array)
            got = nat.array(array)
            assert torch.equal(got.to(want.dtype), want), array
        for red in (("max", "min") if minmax else ("sum", "mean")):
            ref, ref_arg = oracle_mod.spmm_fw(rowptr, col, val, x, red)
            for builder, plan in (("torch", ref_plan), ("native", nat)):
                z = torch.full((m, k), 7.0, device=gpu)
                z_arg = torch.full((m, k), -5, dtype=torch.int64, device=gpu) if minmax else None
                if minmax:
                    st = cabi.fusedMM_csr_stream_minmax_hip(cabi.MESSAGE[red], d_rowptr, col.size, plan, d_x, z, z_arg, plan.workspace(minmax=True), check=False)
                else:
                    st = cabi.fusedMM_csr_stream_hip(cabi.MESSAGE[red], d_rowptr, col.size, plan, d_x, z, plan.workspace(), check=False)
                torch.cuda.synchronize()
                assert st == cabi.SUCCESS, (builder, red, cabi.last_error())
                if red == "mean":
                    _check(oracle_mod, rowptr, col, val, x, red, z, None)
                else:
                    assert np.array_equal(_bits(z.cpu().numpy()), _bits(ref)), (builder, red)
                if minmax:
                    assert np.array_equal(z_arg.cpu().numpy(), ref_arg), (builder, red)
            z = torch.full((m, k), 7.0, device=gpu)
            z_arg = torch.full((m, k), -5, dtype=torch.int64, device=gpu) if minmax else None
            cabi.fusedMM_csr_hip(cabi.MESSAGE[red], d_rowptr, d_col, d_val, d_x, z, z_arg)
            _check(oracle_mod, rowptr, col, val, x, red, z, z_arg)
    finally:
        nat.close()


# ---- a last panel of ONE column: run_stream_panels widens it backwards, the write-out folds one column per thread -----------------

@pytest.mark.parametrize("streams,k", ((8, 33), (4, 65), (2, 129)))
def test_sliver_panel_of_one_column(gpu, oracle_mod, streams, k):
    """k = one column more than the slot width, on the hub case of test_stream_hub_row_is_cut_into_virtual_rows (k = 66, 67 and
    130 are there: slivers of two and three): the last panel is z + k - 4, unaligned, and the hub fold takes its VEC = 1 form."""
    rowptr, col = cases.random_csr(64, 400, 6.0, seed=9, empty_rows=(0, 63), hub=(17, 12345), duplicates=True)
    val = cases.weights(col.size, 4, "signed_int")
    x = cases.dense(400, k, 3, "integer")
    _stream_all(gpu, oracle_mod, rowptr, col, val, x, geoms=((8, 16, streams, 64), (3, 3, streams, 300)))
    if streams != 2:
        _stream_minmax_all(gpu, oracle_mod, rowptr, col, val, x, geoms=((streams, 8, 16, 64), (streams, 3, 3, 300)))
        _stream_minmax_all(gpu, oracle_mod, rowptr, col, val, x, native=True, geoms=((streams, 3, 5, 200),))
