"""The packed word stream of the sum / mean stream kernel (include/isplib_hip.h, PACKED WORD STREAM; ISPLIB_STREAM_PACK): a launch that
decodes the plan's packed stream gives the bits of the launch that reads the plan's words, and stays within the sum bound of the
oracle; the library's packing pass writes the array that isplib_amd/plan.py's numpy mirror writes.  Graphs of a few thousand rows
forced onto 4-stream plans with explicit geometry (as tests/test_gpu_sweep.py does); the mode is switched through the library's
undeclared test entries isplib_stream_pack_set / isplib_stream_pack_last and put back after every test."""
import os

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

OFF, FORCE, AUTO = 0, 1, 2
_MODE_OF_THE_PROCESS = {"0": OFF, "1": FORCE}.get(os.environ.get("ISPLIB_STREAM_PACK", ""), AUTO)           # as runtime.hip reads it
_STAGE_OF_THE_PROCESS = {"0": 0, "1": 1}.get(os.environ.get("ISPLIB_STREAM_STAGE", ""), 2)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(autouse=True)
def _modes_back_to_what_they_were():
    yield
    from isplib_amd import cabi
    cabi.stream_pack_set(_MODE_OF_THE_PROCESS)
    cabi.lib().isplib_stream_stage_set(_STAGE_OF_THE_PROCESS)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _run(plan, d_rowptr, nnz, y, red, mode):
    """One call in `mode`; (out, whether it read the packed stream)."""
    from isplib_amd import cabi
    cabi.stream_pack_set(mode)
    out = torch.full((d_rowptr.numel() - 1, y.size(1)), float("nan"), dtype=torch.float32, device=y.device)
    cabi.fusedMM_csr_stream_hip(cabi.MESSAGE[red], d_rowptr, nnz, plan, y, out, plan.workspace())
    torch.cuda.synchronize()
    return out, cabi.stream_pack_last()


def _packed_equals_unpacked(gpu, oracle, rowptr, col, val, n, geom, ks=(64,), reds=("sum",), packable=True, native=False, stage=None):
    """geom: (slices, waves_per_gen, chunk).  The plan carries a packed stream exactly where `packable`; the native array is the
    numpy mirror's; per k and reduction: packed == unpacked bit for bit (an unpackable plan runs unpacked in every mode and says so),
    twice the same bits, within the oracle's sum bound."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_stream_plan, build_stream_plan_native, stream_pack_words
    slices, wpg, chunk = geom
    d_rowptr, d_col = _t(rowptr, gpu), _t(col, gpu)
    if native:
        plan = build_stream_plan_native(d_rowptr, d_col, n, slices, 4, chunk, waves_per_gen=wpg)
        if val is not None:
            plan.set_values(_t(val, gpu))
    else:
        plan = build_stream_plan(d_rowptr, d_col, None if val is None else _t(val, gpu), n, slices, wpg, None, 4, chunk)
    assert plan is not None and plan.streams == 4
    want, ok = stream_pack_words(plan.words.cpu().numpy(), plan.wave_step_off.cpu().numpy(), n, slices)
    assert ok == packable and (plan.packed is not None) == packable and plan.struct().has_packed == int(packable)
    if packable:
        assert np.array_equal(plan.packed.cpu().numpy().view(np.uint32), want)
    if stage is not None:
        assert cabi.lib().isplib_stream_stage_set(stage) == 0
    weights = np.ones(col.size, np.float32) if val is None else val
    for k in ks:
        x = cases.dense(n, k, 3 + k)
        y = _t(x, gpu)
        tol = cases.sum_tolerance(oracle, rowptr, col, weights, x)
        for red in reds:
            plain, was = _run(plan, d_rowptr, col.size, y, red, OFF)
            assert not was
            packed, was = _run(plan, d_rowptr, col.size, y, red, FORCE)
            assert was == packable
            assert _same_bits(packed, plain), f"k={k} {red}"
            again, _ = _run(plan, d_rowptr, col.size, y, red, FORCE)
            assert _same_bits(again, packed), "two packed launches must give the same bits"
            ref, _ = oracle.spmm_fw(rowptr, col, weights, x, red)
            err = np.abs(packed.cpu().numpy().astype(np.float64) - ref.astype(np.float64))
            assert np.all(err <= tol), f"k={k} {red}: max err/tol = {np.max(err / tol)}"
    return plan


@pytest.mark.parametrize("weights", ("unit", "uniform"))
@pytest.mark.parametrize("k", (64, 128, 41, 4))
def test_widths_reductions_and_weights(gpu, oracle_mod, k, weights):
    """3,000 rows, mean degree 24, empty rows, a hub row cut into virtual rows; sum and mean; K = 128 runs two panels, 41 a ragged one."""
    rowptr, col = cases.random_csr(3000, 3000, 24.0, seed=61, empty_rows=(0, 1500), hub=(17, 1500))
    val = None if weights == "unit" else cases.weights(col.size, 4)
    plan = _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, val, 3000, (4, 16, 512), ks=(k,), reds=("sum", "mean"))
    assert plan.n_parts > 0 and int((plan.perm < 0).sum()) > 0           # partial rows and a fold; padding words


def test_short_waves_ragged_batches_and_empty_waves(gpu, oracle_mod):
    """10 rows on 8 waves: waves of fewer words than one batch, waves with none; 64 rows of ~40 entries on one wave: several
    batches, the last one ragged."""
    rowptr, col = cases.random_csr(10, 500, 9.0, seed=5)
    plan = _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, None, 500, (3, 8, 4096))
    nwords = ((plan.wave_step_off[1:] - plan.wave_step_off[:-1]) * 4).cpu().numpy()
    assert (nwords == 0).any() and ((nwords > 0) & (nwords < 128)).any()
    rowptr, col = cases.random_csr(64, 300, 40.0, seed=6)
    plan = _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, cases.weights(col.size, 2), 300, (2, 1, 4096))
    assert plan.n_steps * 4 > 256 and (plan.n_steps * 4) % 128 != 0


@pytest.mark.parametrize("slices", (1, 40))
def test_one_slice_and_many_narrow_slices(gpu, oracle_mod, slices):
    """3,000 columns in 1 and in 40 slices, rows of ~6 entries: with 40, rows have no entry in most slices and a slot's stream skips
    several slices between two entries (tests/test_stream_packed_host.py counts them on the same graph)."""
    rowptr, col = cases.random_csr(300, 3000, 6.0, seed=7, empty_rows=(0, 17))
    _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, None, 3000, (slices, 2, 4096), ks=(64, 41))


@pytest.mark.parametrize("n,slices,packable", ((8192 * 2 - 1, 2, True), (8192 * 2, 2, True), (8192 * 2 + 1, 2, False),
                                               (8192 * 3, 3, True), (8192 * 3 + 1, 3, False)))
def test_slice_width_edge(gpu, oracle_mod, n, slices, packable):
    """Slices of 8,192 columns are the widest the format holds: one column more and the plan has no packed stream, says so through
    its flag and runs on its words in every mode.  The first and last column of every slice are in the graph."""
    rowptr, col = cases.random_csr(2000, n, 12.0, seed=8)
    width = -(-n // slices)
    col = col.copy()
    for s in range(slices):
        col[rowptr[s]:rowptr[s + 1]] = np.sort(np.resize(np.array([s * width, min((s + 1) * width, n) - 1]), rowptr[s + 1] - rowptr[s]))
    assert col.max() == n - 1
    _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, None, n, (slices, 8, 4096), packable=packable)


def test_a_skip_over_a_wide_slice_runs_unpacked(gpu, oracle_mod):
    """Slices of 8,000 columns and rows with entries in the first and the last only: not representable, and not an error."""
    m, n = 64, 24000
    rowptr = np.arange(0, 5 * m + 1, 5, dtype=np.int64)
    col = np.tile(np.array([5, 70, 100, 17000, 23999], np.int64), m)
    _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, None, n, (3, 1, 4096), packable=False)
    _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, None, n, (3, 1, 4096), packable=False, native=True)


def test_hub_rows_with_a_small_chunk_native_builder(gpu, oracle_mod):
    """A hub row of 2,000 entries cut at 64, through the library's own builder (which attaches the packed stream itself)."""
    rowptr, col = cases.random_csr(2500, 2500, 10.0, seed=9, hub=(11, 2000))
    plan = _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, cases.weights(col.size, 5), 2500, (5, 12, 64), ks=(64, 128),
                                   reds=("sum", "mean"), native=True)
    assert plan.n_parts > 20 and plan.n_hub >= 1


def test_a_staged_second_panel(gpu, oracle_mod):
    """K = 128 with staging forced (ISPLIB_STREAM_STAGE=1): both panels are gathered from their copies, packed and unpacked alike."""
    from isplib_amd import cabi
    rowptr, col = cases.random_csr(3000, 3000, 24.0, seed=62, hub=(5, 900))
    _packed_equals_unpacked(gpu, oracle_mod, rowptr, col, cases.weights(col.size, 6), 3000, (3, 16, 256), ks=(128,), stage=1)
    cabi.lib().isplib_stream_stage_last.restype = __import__("ctypes").c_uint
    assert int(cabi.lib().isplib_stream_stage_last()) == 0b11


def test_auto_packs_from_the_size_on_where_the_stream_schedule_is_offered(gpu):
    """auto: a small graph runs on its words (the plan has a packed stream all the same); 0 never packs; 1 packs it."""
    rowptr, col = cases.random_csr(500, 500, 8.0, seed=12)
    from isplib_amd.plan import build_stream_plan
    d_rowptr = _t(rowptr, gpu)
    plan = build_stream_plan(d_rowptr, _t(col, gpu), None, 500, 2, 4, None, 4, 4096)
    assert plan.packed is not None
    y = _t(cases.dense(500, 64, 1), gpu)
    assert [_run(plan, d_rowptr, col.size, y, "sum", mode)[1] for mode in (AUTO, OFF, FORCE)] == [False, False, True]
