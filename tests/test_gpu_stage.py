"""Staged column panels of the stream schedule (fusedMM_csr_stream_hip; include/isplib_hip.h, isplib_stream_stage_panel): a panel
gathered from its copy in the workspace gives the bits the panel itself gives.  One graph of 3,000 rows, mean degree 32, with a
row longer than the plan's chunk (partial rows and the fold) and an edge to column n - 1; forced staging (mode 1) against none
(mode 0) through the library's undeclared test entries isplib_stream_stage_set / isplib_stream_stage_last."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cases, stage_rule
from tests.stage_rule import AUTO, FORCE, OFF

pytestmark = pytest.mark.gpu

N, CHUNK = 3000, 256
_MODE_OF_THE_PROCESS = {"0": OFF, "1": FORCE}.get(os.environ.get("ISPLIB_STREAM_STAGE", ""), AUTO)      # as runtime.hip reads it


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class _Graph:
    pass


@pytest.fixture(scope="module")
def g(gpu):
    from isplib_amd.plan import build_stream_plan
    s = _Graph()
    s.rowptr, s.col = cases.random_csr(N, N, 32.0, seed=41, empty_rows=(0, 1500), hub=(17, 2000))
    s.col[s.rowptr[N] - 1] = N - 1                      # the last row's last (= largest) column: the highest id there is
    assert s.col.max() == N - 1 and s.rowptr[18] - s.rowptr[17] > CHUNK
    s.nnz = int(s.col.size)
    s.val = {"unit": np.ones(s.nnz, np.float32), "uniform": cases.weights(s.nnz, 4)}
    s.d_rowptr, s.d_col = _t(s.rowptr, gpu), _t(s.col, gpu)
    s.plan = {"unit": build_stream_plan(s.d_rowptr, s.d_col, None, N, 4, 16, None, 4, CHUNK),
              "uniform": build_stream_plan(s.d_rowptr, s.d_col, _t(s.val["uniform"], gpu), N, 3, 16, None, 4, CHUNK)}
    for p in s.plan.values():
        assert p.streams == 4 and p.n_parts > 0 and p.n_hub > 0 and int((p.perm < 0).sum()) > 0      # partial rows, a fold, padding words
    s.wide = cases.dense(N, 256, 3)                     # every operand of the cases below is a column view of this
    raw = torch.empty(N * 256 + 1024, dtype=torch.float32, device=gpu)      # start d_wide on a 4096-byte boundary: the class of a line
    first = (-raw.data_ptr() % 4096) // 4                                   # in 1024-byte rows depends on address bit 9
    s.d_wide = raw[first:first + N * 256].view(N, 256)
    s.d_wide.copy_(_t(s.wide, gpu))
    assert s.d_wide.data_ptr() % 4096 == 0
    return s


@pytest.fixture(autouse=True)
def _mode_back_to_what_it_was():
    yield
    from isplib_amd import cabi
    cabi.lib().isplib_stream_stage_set(_MODE_OF_THE_PROCESS)


def _run(g, weights, red, y, mode, workspace=None, ep=None):
    """One call in `mode`; (out, bit mask of the panels it staged)."""
    from isplib_amd import cabi
    L = cabi.lib()
    L.isplib_stream_stage_last.restype = ctypes.c_uint
    assert L.isplib_stream_stage_set(mode) == 0
    plan = g.plan[weights]
    out = torch.empty((N, y.size(1)), dtype=torch.float32, device=y.device)
    cabi.fusedMM_csr_stream_hip(cabi.MESSAGE[red], g.d_rowptr, g.nnz, plan, y, out, plan.workspace() if workspace is None else workspace, ep)
    torch.cuda.synchronize()
    return out, int(L.isplib_stream_stage_last())


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _within_bound(oracle, g, weights, x, red, out):
    ref, _ = oracle.spmm_fw(g.rowptr, g.col, g.val[weights], x, red)
    tol = cases.sum_tolerance(oracle, g.rowptr, g.col, g.val[weights], x)
    err = np.abs(out.cpu().numpy().astype(np.float64) - ref.astype(np.float64))
    assert np.all(err <= tol), f"{red}: max err/tol = {np.max(err / tol)}"


def _staged_equals_unstaged(g, weights, red, y, want_mask, **kw):
    plain, none = _run(g, weights, red, y, OFF, **kw)
    staged, mask = _run(g, weights, red, y, FORCE, **kw)
    assert none == 0 and mask == want_mask, (none, mask)
    assert _same_bits(staged, plain)
    return staged


@pytest.mark.parametrize("weights", ("unit", "uniform"))
@pytest.mark.parametrize("red", ("sum", "mean"))
def test_contiguous_k128(gpu, oracle_mod, g, red, weights):
    """#1: K = 128 at ldy = 128, both panels forced through the copy; with and without the fused epilogue."""
    from isplib_amd import cabi
    x = np.ascontiguousarray(g.wide[:, :128])
    y = _t(x, gpu)
    out = _staged_equals_unstaged(g, weights, red, y, 0b11)
    _within_bound(oracle_mod, g, weights, x, red, out)
    rs, bias = cases.dense(N, 1, 8)[:, 0].copy(), cases.dense(1, 128, 9)[0].copy()
    d_rs, d_bias = _t(rs, gpu), _t(bias, gpu)
    ep = cabi.Epilogue(d_rs.data_ptr(), y.data_ptr(), 128, d_bias.data_ptr(), 1)
    out = _staged_equals_unstaged(g, weights, red, y, 0b11, ep=ep)
    ref, _ = oracle_mod.spmm_fw(g.rowptr, g.col, g.val[weights], x, red)
    want = np.maximum(rs[:, None] * (ref + x) + bias[None, :], 0.0)
    tol = cases.sum_tolerance(oracle_mod, g.rowptr, g.col, g.val[weights], x) * np.abs(rs[:, None]) + 1e-6
    assert np.all(np.abs(out.cpu().numpy() - want) <= tol)


def test_column_view_the_first_panel_is_the_slow_one(gpu, oracle_mod, g, tmp_path):
    """#2: X = wide[:, 64:192]: panel 0 starts 256 bytes into a 1024-byte row (address bit 8 set), panel 1 on a 512-byte boundary.
    The rule looks at the address: (1, 0), where the contiguous operand of #1 gets (0, 1)."""
    y = g.d_wide[:, 64:192]
    assert y.data_ptr() % 512 == 256 and y.stride(0) == 256
    out = _staged_equals_unstaged(g, "uniform", "sum", y, 0b11)
    _within_bound(oracle_mod, g, "uniform", np.ascontiguousarray(g.wide[:, 64:192]), "sum", out)
    rule = stage_rule.compile_rule(tmp_path)
    big, room = N * stage_rule.header_constant("STREAM_STAGE_MIN_DEGREE"), N * 512
    assert [rule(y.data_ptr(), 256, c0, 128, 4, N, big, room, AUTO) for c0 in (0, 64)] == [True, False]
    assert [rule(g.d_wide.data_ptr(), 128, c0, 128, 4, N, big, room, AUTO) for c0 in (0, 64)] == [False, True]


@pytest.mark.parametrize("k,ld,view,want_mask", ((132, 256, 0, 0b011), (132, 132, None, 0), (200, 256, 0, 0b0111), (128, 160, None, 0)))
def test_partial_panels_and_other_pitches(gpu, oracle_mod, g, k, ld, view, want_mask):
    """#3 K = 132: the 4-column sliver is never staged (at ldy = 256 the two whole panels are; at ldy = 132 the pitch rules all out);
    #4 K = 200 at ldy = 256: the 8-column last panel is not; #5 ldy = 160 (640-byte rows): nothing is."""
    x = np.ascontiguousarray(g.wide[:, :k])
    if view is None:
        pad = torch.zeros((N, ld), dtype=torch.float32, device=gpu)
        pad[:, :k] = _t(x, gpu)
        y = pad[:, :k]
    else:
        y = g.d_wide[:, :k]
    assert y.stride(0) == ld
    out = _staged_equals_unstaged(g, "uniform", "mean", y, want_mask)
    _within_bound(oracle_mod, g, "uniform", x, "mean", out)


def _poisoned(nbytes, dev):
    return torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)[:nbytes]


def test_padding_words_read_zero_through_the_staged_descriptor(gpu, oracle_mod, g):
    """#6 (and #9): the plan's streams end in padding words (column n) and the graph reaches column n - 1.  Integer operands and unit
    weights make every sum exact, the workspace is full of NaN behind the copy's last row: anything a padding word read from
    inside the staging area would show."""
    from isplib_amd import cabi
    L = cabi.lib()
    x = cases.dense(N, 128, 5, "integer")
    y = _t(x, gpu)
    plan = g.plan["unit"]
    L.isplib_spmm_stream_workspace_bytes.restype = ctypes.c_size_t
    nbytes = int(L.isplib_spmm_stream_workspace_bytes(ctypes.byref(plan.struct())))
    assert nbytes == stage_rule.old_workspace_bytes(plan.n_parts, 4) + N * 512 + 512
    plain, _ = _run(g, "unit", "sum", y, OFF)
    staged, mask = _run(g, "unit", "sum", y, FORCE, workspace=_poisoned(nbytes, gpu))
    assert mask == 0b11 and _same_bits(staged, plain)
    ref, _ = oracle_mod.spmm_fw(g.rowptr, g.col, g.val["unit"], x, "sum")
    assert np.array_equal(staged.cpu().numpy(), ref)


def test_the_operand_is_only_read(gpu, g):
    """#7"""
    y = g.d_wide[:, :128].contiguous()
    before = y.clone()
    _, mask = _run(g, "uniform", "sum", y, FORCE)
    assert mask == 0b11 and _same_bits(y, before)


def test_workspace_of_the_old_size_runs_unstaged(gpu, g):
    """#8: a caller that sizes the workspace by the partial rows alone is served as before."""
    y = g.d_wide[:, :128].contiguous()
    plan = g.plan["uniform"]
    small = torch.empty(stage_rule.old_workspace_bytes(plan.n_parts, 4), dtype=torch.uint8, device=gpu)
    plain, _ = _run(g, "uniform", "sum", y, OFF)
    out, mask = _run(g, "uniform", "sum", y, FORCE, workspace=small)
    assert mask == 0 and _same_bits(out, plain)


def test_poisoned_workspace_of_the_new_size(gpu, g):
    """#9: nothing of the workspace is read before the call wrote it."""
    y = g.d_wide[:, :128].contiguous()
    plan = g.plan["uniform"]
    plain, _ = _run(g, "uniform", "mean", y, OFF)
    out, mask = _run(g, "uniform", "mean", y, FORCE, workspace=_poisoned(plan.workspace().numel(), gpu))
    assert mask == 0b11 and _same_bits(out, plain)
