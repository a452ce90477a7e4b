"""The levelled deal of the stream plans on the GPU (include/isplib_hip.h: isplib_stream_capacities_hip,
isplib_stream_plan_build_caps_hip): the capacities decide which wave holds a row and nothing else, so both builders give the
same plan under the same capacities and a levelled launch gives the bits of the unlevelled one (in every row that no stream
carries across a slice boundary: all rows of the cases here but the last test's).  700 rows over 300 columns --
two generations at waves_per_gen = 8 --, one row of 2,000 entries (cut at chunk = 256 and folded), empty rows, and enough
entries per column for the rule to stage the second panel of a K = 128 call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cases
from tests.stage_rule import AUTO, FORCE, OFF

pytestmark = pytest.mark.gpu

M, N, CHUNK, WPG, STREAMS, SLICES = 700, 300, 256, 8, 4, 3
ONE = 4096
SKEWED = {"0.5 to 1.5": [ONE // 2 + (ONE * w) // 7 for w in range(WPG)],
          "one at a tenth": [ONE] * 3 + [ONE // 10] + [ONE] * 4}
ARRAYS = ("words", "perm", "wave_step_off", "wave_row", "wave_part", "hub_row", "hub_off")
_STAGE_OF_THE_PROCESS = {"0": OFF, "1": FORCE}.get(os.environ.get("ISPLIB_STREAM_STAGE", ""), AUTO)
_LEVEL_OF_THE_PROCESS = {"0": 0, "1": 1}.get(os.environ.get("ISPLIB_STREAM_LEVEL", ""), 2)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Graph:
    pass


@pytest.fixture(scope="module")
def g(gpu):
    s = _Graph()
    s.rowptr, s.col = cases.random_csr(M, N, 64.0, seed=23, empty_rows=(0, 350, 699), hub=(17, 2000))
    s.nnz = int(s.col.size)
    assert s.nnz >= N * 128 and s.rowptr[18] - s.rowptr[17] > CHUNK
    s.val = cases.weights(s.nnz, 4)
    s.d_rowptr, s.d_col, s.d_val = _t(s.rowptr, gpu), _t(s.col, gpu), _t(s.val, gpu)
    raw = torch.empty(N * 128 + 1024, dtype=torch.float32, device=gpu)          # y on a 4096-byte boundary: the rule then stages panel 1
    first = (-raw.data_ptr() % 4096) // 4
    s.y = {128: raw[first:first + N * 128].view(N, 128), 4: _t(cases.dense(N, 4, 5), gpu)}
    s.y[128].copy_(_t(cases.dense(N, 128, 3), gpu))
    return s


@pytest.fixture(autouse=True)
def _modes_back_to_what_they_were():
    yield
    from isplib_amd import cabi
    cabi.lib().isplib_stream_stage_set(_STAGE_OF_THE_PROCESS)
    cabi.stream_level_set(_LEVEL_OF_THE_PROCESS)


def _native(g, caps, weighted):
    from isplib_amd import cabi
    return cabi.NativeStreamPlan(g.d_rowptr, g.d_col, g.d_val if weighted else None, N, STREAMS, SLICES, CHUNK, WPG, capacities=caps)


def _launch(g, plan, k):
    from isplib_amd import cabi
    L = cabi.lib()
    L.isplib_stream_stage_last.restype = ctypes.c_uint
    assert L.isplib_stream_stage_set(AUTO) == 0
    out = torch.full((M, k), float("nan"), dtype=torch.float32, device=g.y[k].device)
    cabi.fusedMM_csr_stream_hip(cabi.MSG_SPMM_SUM, g.d_rowptr, g.nnz, plan, g.y[k], out, plan.workspace())
    torch.cuda.synchronize()
    return out, int(L.isplib_stream_stage_last())


@pytest.mark.parametrize("name", sorted(SKEWED))
@pytest.mark.parametrize("weighted", (False, True), ids=("unit", "weighted"))
@pytest.mark.parametrize("k", (128, 4))
def test_levelled_plan_and_launch(gpu, oracle_mod, g, k, weighted, name):
    from isplib_amd import cabi
    from isplib_amd.plan import stream_plan_arrays
    caps = SKEWED[name]
    rpw, _ = cabi.stream_geometry(STREAMS)
    lev, base = _native(g, caps, weighted), _native(g, None, weighted)
    assert lev.gens == 2 and lev.n_parts > 1 and lev.n_hub == 1
    # both builders, the same capacities: identical arrays (and they are not the unlevelled plan's)
    torch_built = stream_plan_arrays(g.d_rowptr, g.d_col, N, SLICES, WPG, rpw, STREAMS, CHUNK, capacities=caps)
    for a in ARRAYS:
        assert torch.equal(lev.array(a).to(torch.int64), torch_built[a].to(torch.int64)), a
    assert lev.n_steps != base.n_steps or not torch.equal(lev.array("words"), base.array("words"))
    # the levelled launch: the unlevelled launch's bits, and its own on a second run
    out0, staged0 = _launch(g, base, k)
    out1, staged1 = _launch(g, lev, k)
    out2, _ = _launch(g, lev, k)
    assert staged0 == staged1 == (0b10 if k == 128 else 0), "K = 128: two panels, the second one staged"
    assert not torch.isnan(out0).any()
    assert torch.equal(out1.view(torch.int32), out0.view(torch.int32)) and torch.equal(out2.view(torch.int32), out1.view(torch.int32))
    val = g.val if weighted else np.ones(g.nnz, np.float32)
    x = g.y[k].cpu().numpy()
    ref, _ = oracle_mod.spmm_fw(g.rowptr, g.col, val, x, "sum")
    assert np.all(np.abs(out1.cpu().numpy().astype(np.float64) - ref) <= cases.sum_tolerance(oracle_mod, g.rowptr, g.col, val, x))


def test_capacities_rule_and_calibration(gpu, g):
    """isplib_stream_capacities_hip: none with the switch off, for another waves_per_gen than the resident waves, and under auto
    for a small graph; switched on, one capacity per resident wave within the clamp (8 %) of nominal, equal inside a workgroup,
    the same on a second call (calibrated once per process) and not all equal -- and under them both builders give the same plan
    of the kernel's own geometry, which is not the unlevelled plan; its launch gives the unlevelled plan's bits in every row that
    neither plan carries across a slice boundary, and the sum within its bound in all."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_stream_plan, build_stream_plan_native
    _, resident = cabi.stream_geometry(STREAMS)
    cabi.stream_level_set(0)
    assert cabi.stream_capacities(gpu, STREAMS, 0, 1 << 30) is None
    cabi.stream_level_set(2)
    assert cabi.stream_capacities(gpu, STREAMS, 0, g.nnz) is None, "auto: not for a graph the stream schedule is not offered"
    cabi.stream_level_set(1)
    assert cabi.stream_capacities(gpu, STREAMS, WPG, 1 << 30) is None
    caps = cabi.stream_capacities(gpu, STREAMS, 0, g.nnz)
    assert caps is not None and len(caps) == resident and caps == cabi.stream_capacities(gpu, STREAMS, resident, g.nnz)
    c = np.array(caps).reshape(-1, 4)
    assert (c == c[:, :1]).all() and c.min() >= ONE / 1.08 - 1 and c.max() <= ONE / 0.92 + 1
    assert len(set(caps)) > 1, "the calibration found no difference between the places at all: nothing below would be levelled"
    first, second = c[:c.shape[0] // 2, 0].mean(), c[c.shape[0] // 2:, 0].mean()
    print(f"capacities {c.min()} .. {c.max()}; first workgroups of the CUs {first:.0f}, second {second:.0f}")
    # a graph with more rows than the generation has streams (8,192): two rounds, so the capacities do decide who gets what
    rowptr, col = cases.random_csr(20000, N, 8.0, seed=29, empty_rows=(0, 9999), hub=(17, 2000))
    d_rowptr, d_col = _t(rowptr, gpu), _t(col, gpu)
    cabi.stream_level_set(0)
    base2 = build_stream_plan_native(d_rowptr, d_col, N, SLICES, STREAMS, CHUNK)
    cabi.stream_level_set(1)
    nat = build_stream_plan_native(d_rowptr, d_col, N, SLICES, STREAMS, CHUNK)
    tor = build_stream_plan(d_rowptr, d_col, None, N, SLICES, None, None, STREAMS, CHUNK)
    assert nat.waves_per_gen == resident and nat.gens == 1
    assert nat.n_steps != base2.n_steps or not torch.equal(nat.words, base2.words), "the levelled plan is another plan"
    for a in ARRAYS:
        assert torch.equal(getattr(nat, a).to(torch.int64), getattr(tor, a).to(torch.int64)), a
    outs = []
    for plan in (base2, nat):
        out = torch.full((20000, 128), float("nan"), dtype=torch.float32, device=gpu)
        cabi.fusedMM_csr_stream_hip(cabi.MSG_SPMM_SUM, d_rowptr, int(col.size), plan, g.y[128], out, plan.workspace())
        torch.cuda.synchronize()
        outs.append(out)
    assert not torch.isnan(outs[0]).any() and not torch.isnan(outs[1]).any()
    # Which wave holds a row is all the deal decides -- but the kernel adds a row's running sum to its LDS line when the stream
    # CHANGES rows, so a row whose stream has no other row between its last word of one column slice and its first of the next is
    # summed straight through that boundary, and whether that happens depends on the rows it shares a stream with.  With two or
    # three short rows per stream, as here, it does happen; rows that are flushed at every boundary in both plans have the same
    # bits, and every row is within the bound of the sum either way.  (Streams of many rows with entries in every slice -- the
    # plans above, the headline -- carry nothing: there the whole output is bitwise the unlevelled one.)
    differ = (outs[0].view(torch.int32) != outs[1].view(torch.int32)).any(dim=1).cpu().numpy()
    carried = _carried_rows(base2, N) | _carried_rows(nat, N)
    print(f"rows with other bits under the levelled plan: {int(differ.sum())}; rows carried across a slice boundary in either plan: {len(carried)}")
    assert set(np.nonzero(differ)[0].tolist()) <= carried
    x = g.y[128].cpu().numpy()
    ones = np.ones(col.size, np.float32)
    import oracle
    ref, _ = oracle.spmm_fw(rowptr, col, ones, x, "sum")
    tol = cases.sum_tolerance(oracle, rowptr, col, ones, x)
    for out in outs:
        assert np.all(np.abs(out.cpu().numpy().astype(np.float64) - ref) <= tol)


def _carried_rows(plan, ncols):
    """Rows that some stream of the plan walks from one column slice into the next without another row in between."""
    streams, rpw = plan.streams, plan.rows_per_wave
    width = -(-ncols // plan.slices)
    words = (plan.words.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).reshape(-1, streams)
    real = plan.perm.cpu().numpy().reshape(-1, streams) >= 0
    off = plan.wave_step_off.cpu().numpy()
    rows = plan.wave_row.cpu().numpy().reshape(-1, rpw)
    out = set()
    for w in range(off.size - 1):
        for q in range(streams):
            wd = words[off[w]:off[w + 1], q][real[off[w]:off[w + 1], q]]
            sl, lr = (wd & 0xFFFFFF) // width, wd >> 24
            at = np.nonzero((sl[1:] != sl[:-1]) & (lr[1:] == lr[:-1]))[0]
            out.update(rows[w, lr[at]].tolist())
    return out


def test_capacities_out_of_range_are_refused(gpu, g):
    from isplib_amd import cabi
    with pytest.raises(cabi.IsplibError):
        _native(g, [ONE] * (WPG - 1) + [ONE * 17], False)
    with pytest.raises(cabi.IsplibError):
        _native(g, [ONE // 17] + [ONE] * (WPG - 1), False)
    with pytest.raises(ValueError):
        _native(g, [ONE] * (WPG + 1), False)
