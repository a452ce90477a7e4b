"""Host side of the fp32 SDDMM tests (tests/test_gpu_sddmm_fp32.py): a census of their inputs against the kernels' selection rules
and loop edges, a numpy emulation of the kernels' summation order held to the bounds the GPU tests assert (with two broken copies
that must miss them), and the operand checks of cabi.sddmm, cabi.sddmm_tasks and GraphHandle.sddmm.  No device."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import cases
from tests import sddmm_fp32_cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = 64 * 2.0 ** -149                        # the bound's absolute term: roundings in the subnormal range, each at most 2^-150


def _source(name):
    return open(os.path.join(ROOT, "isplib_amd", "csrc", name)).read()


def test_constants_and_selection_rules_match_the_source():
    src = _source("backward.hip")
    assert re.search(r"a\.long_row = 4096;", src) and cs.LONG_ROW == 4096
    assert len(re.findall(r"constexpr int U = 4;|constexpr int G = 64 / LPR, U = 4;", src)) == 2 and cs.U == 4
    # the row entry's ladder and the task entry's, as written
    for line in ("if (w <= 8) return launch_sddmm<4, 8>(a, st);", "if (w <= 16) return launch_sddmm<4, 16>(a, st);",
                 "if (w <= 32) return launch_sddmm<4, 32>(a, st);", "return launch_sddmm<4, 64>(a, st);",
                 "if (k <= 16) return launch_sddmm<1, 16>(a, st);", "if (k <= 32) return launch_sddmm<1, 32>(a, st);",
                 "return launch_sddmm<1, 64>(a, st);", "if (w <= 8) rc = launch_sddmm_tasks<8, 1>(p, st, acc);",
                 "else if (w <= 16) rc = launch_sddmm_tasks<16, 1>(p, st, acc);", "else if (w <= 32) rc = launch_sddmm_tasks<32, 1>(p, st, acc);",
                 "else if (w <= 64) rc = launch_sddmm_tasks<64, 1>(p, st, acc);", "else if (w <= 128) rc = launch_sddmm_tasks<64, 2>(p, st, acc);",
                 "else rc = launch_sddmm_tasks<64, 4>(p, st, acc);",
                 "const bool v4 = (k % 4 == 0) && (ldy % 4 == 0) && (ldg % 4 == 0) && ((al & 15) == 0);"):
        assert line in src, line
    header = open(os.path.join(ROOT, "include", "isplib_hip.h")).read()
    assert re.search(r"#define\s+ISPLIB_K_MIN\s+4\b", header) and re.search(r"#define\s+ISPLIB_SDDMM_TASKS_K_MAX\s+1024\b", header)
    assert (cs.K_MIN, cs.TASKS_K_MAX) == (4, 1024) and min(cs.TASK_WIDTHS) == 4 and max(cs.TASK_WIDTHS) == 1024


def test_widths_reach_every_instantiation_and_its_ragged_form():
    # the row kernel's seven instantiations, each at its first and its last width
    slots = {}
    for k, vec4 in cs.ROW_WIDTHS:
        slots.setdefault(cs.row_slot(k, vec4), []).append(k)
    assert slots == {(4, 8): [4, 32], (4, 16): [36, 64], (4, 32): [68, 128], (4, 64): [132, 256, 260, 1024],
                     (1, 16): [1, 3, 16], (1, 32): [17, 31, 32], (1, 64): [33, 41, 65, 130]}
    assert all(k % 4 == 0 for k in cs.ROW_WIDTHS_VEC4) and [k for k in cs.ROW_WIDTHS_SCALAR if k % 4 == 0] == [16, 32]
    assert 260 % 256 != 0 and 1024 % 256 == 0 and 65 > 64                  # a second trip, partial and whole; the scalar form's second trip
    assert {cs.row_slot(k, v) for k, v in cs.ROW_LENGTH_WIDTHS} == {(4, 8), (4, 16), (4, 32), (4, 64), (1, 16), (1, 32), (1, 64)}
    # the task kernel's six, whole and ragged, with every vfirst
    whole, ragged, vfirsts = set(), set(), set()
    for k in cs.TASK_WIDTHS:
        (whole if k % 4 == 0 else ragged).add(cs.task_slot(k))
        vfirsts |= {v[1] for v in cs.task_lane_columns(k).values() if v is not None}
    six = {(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)}
    assert whole == six and ragged == six and vfirsts == {0, 1, 2, 3}
    assert {cs.task_slot(k) for k in cs.TASK_LENGTH_WIDTHS} == six
    # where the shifted vector sits: chunk j of its lane
    where = {k: [j for (lc, j), v in cs.task_lane_columns(k).items() if v is not None and v[1] > 0] for k in cs.TASK_WIDTHS if k % 4}
    assert where[130] == [0] and where[258] == [1] and where[259] == [1] and where[514] == [2] and where[1021] == [3]
    assert all(len(v) == 1 for v in where.values())
    assert all(j >= cs.task_slot(k)[1] // 2 for k, v in where.items() for j in v), "the kernel masks the upper half of a lane's chunks"
    for k in range(cs.K_MIN, cs.TASKS_K_MAX + 1):                          # ... for every width the entry takes, not only the tested ones
        if k % 4:
            lpr, nch = cs.task_slot(k)
            assert (k // 4) // lpr >= nch // 2 and (k // 4) // lpr < nch, k
    assert {cs.task_slot(k) for k in cs.TRAP_WIDTHS} == six and all(k % 4 for k in cs.TRAP_WIDTHS)


def test_duplicated_columns_follow_the_kernels_column_rule():
    for k in cs.TASK_WIDTHS + cs.TRAP_WIDTHS + (cs.PANEL_TRAP_WIDTH,):
        walked, seen = [], []
        for v in cs.task_lane_columns(k).values():
            if v is not None:
                walked += list(range(v[0], v[0] + v[1]))
                seen += list(range(v[0] + v[1], v[0] + 4))
        assert sorted(walked) == cs.duplicated_columns(k), k
        assert sorted(seen) == list(range(k)), f"k {k}: every column is multiplied exactly once"
    assert cs.duplicated_columns(41) == [37, 38, 39] and cs.duplicated_columns(64) == [] and cs.duplicated_columns(5) == [1, 2, 3]
    # the column panels: k = 129 in 64-column panels is 64 + 65, and the last panel's shifted vector duplicates the same columns
    k, pw = cs.PANEL_TRAP_WIDTH, cs.PANEL_COLS
    assert k >= 2 * pw and cs.PANEL_PITCH % 32 == 0 and cs.PANEL_PITCH >= k
    panels, c0 = [], 0
    while c0 < k:
        c1 = c0 + pw
        if c1 + 4 > k:
            c1 = k
        panels.append((c0, c1))
        c0 = c1
    assert panels == [(0, 64), (64, 129)]
    assert [64 + c for c in cs.duplicated_columns(65)] == cs.duplicated_columns(129) == [125, 126, 127]


def test_graphs_hold_every_length_the_kernels_have_an_edge_at():
    rowptr, col = cs.hub_graph()
    deg = np.diff(rowptr)
    assert rowptr.size - 1 == 300 and col.max() < cs.N and col.min() >= 0
    assert all(deg[r] == 0 for r in (0, 150, 299)) and deg[7] == deg.max() == 5000 > cs.LONG_ROW
    assert any(np.any(np.diff(col[rowptr[r]:rowptr[r + 1]]) == 0) for r in range(300)), "duplicate columns"
    want = {0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 4160, 12293}
    for g in (8, 4, 2, 1):
        want |= {g - 1, g, g + 1, 4 * g - 1, 4 * g, 4 * g + 1}
    rp2, col2 = cs.length_graph()
    deg2 = np.diff(rp2)
    assert set(deg2.tolist()) == want == set(cs.edge_degrees()) and col2.max() < cs.N
    assert 40_000 < col2.size < 70_000
    for d in want:                                                         # each length in two different wave positions of a workgroup
        at = np.flatnonzero(deg2 == d)
        assert len({int(r) % 4 for r in at}) >= 2, d
    # a row over long_row is cut into four chunks of ceil(deg / 4) rounded up to 64: the last wave's is shorter, a whole number of
    # 64-edge batches (4160) or not (4097, 12293)
    for d, chunks in ((4097, [1088, 1088, 1088, 833]), (4160, [1088, 1088, 1088, 896]), (12293, [3136, 3136, 3136, 2885])):
        chunk = (-(-d // 4) + 63) // 64 * 64
        assert [max(0, min(d, (w + 1) * chunk) - min(d, w * chunk)) for w in range(4)] == chunks, d
    # the integer cases: |x| <= 3, so |dot| <= 9 * 1024 < 2^24 -- exact in fp32 in any order
    assert np.abs(cases.dense(cs.N, 64, 3, "integer")).max() <= 3 and 9 * 1024 < 2 ** 24


def test_trap_and_subnormal_operands_are_what_they_claim(oracle_mod):
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    for k in cs.TRAP_WIDTHS + (cs.PANEL_TRAP_WIDTH,):
        y, g = cs.ragged_trap(m, k)
        dup = cs.duplicated_columns(k)
        assert sorted(set(np.nonzero(np.isinf(y))[1].tolist())) == dup
        hot = np.isinf(y).any(1)
        assert np.array_equal(np.flatnonzero(hot), cs.trap_rows()[0]) and np.any(y[hot, dup[0]] > 0) and np.any(y[hot, dup[0]] < 0)
        assert np.all(np.isfinite(g)) and np.all(g[:, dup] >= 0.5) and np.all(np.isfinite(np.delete(y, dup, axis=1)))
        for mean in (False, True):
            ref = oracle_mod.sddmm(rowptr, col, y, g, mean=mean)
            assert np.array_equal(np.isinf(ref), hot[col]) and not np.any(np.isnan(ref)) and np.any(hot[col]) and not np.all(hot[col])
            assert np.array_equal(np.sign(ref[hot[col]]), np.sign(y[:, dup[0]])[col][hot[col]])
    for k in (41, 64):
        y, g = cs.subnormal_operands(m, k)
        assert np.abs(y).max() < 4e-38 and np.abs(g).max() <= 1
        ref = oracle_mod.sddmm(rowptr, col, y, g)
        assert np.count_nonzero(ref) > 0.99 * ref.size and np.mean(np.abs(ref[ref != 0]) < 2.0 ** -126) > 0.05
        # non-finite operands: the reference holds NaN, Inf and finite results
        with np.errstate(invalid="ignore"):
            ref = oracle_mod.sddmm(rowptr, col, cases.dense(cs.N, k, 3, "nonfinite"), cases.dense(m, k, 5, "uniform"))
        assert np.any(np.isnan(ref)) and np.any(np.isinf(ref)) and np.any(np.isfinite(ref))


FORMS = [("row4", k) for k in cs.ROW_WIDTHS_VEC4] + [("row1", k) for k in cs.ROW_WIDTHS_SCALAR] + [("task", k) for k in cs.TASK_WIDTHS]


@pytest.mark.parametrize("form,k", FORMS, ids=[f"{f}-{k}" for f, k in FORMS])
def test_emulated_summation_order_meets_the_bounds(oracle_mod, form, k):
    """The kernels' order of additions in numpy fp32 against oracle.sddmm on the GPU tests' own inputs: real-valued data within
    1e-5 * mag + 64 * 2^-149 per edge (printed: the largest err / bound, and err / mag against the 24 roundings of the derivation),
    integer data exact and its mean within 1e-6 * mag."""
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    y, g = cases.dense(cs.N, k, 3, "uniform"), cases.dense(m, k, 5, "uniform")
    for mean in (False, True):
        ref = oracle_mod.sddmm(rowptr, col, y, g, mean=mean).astype(np.float64)
        mag = oracle_mod.sddmm(rowptr, col, np.abs(y), np.abs(g), mean=mean).astype(np.float64)
        err = np.abs(cs.emulate(rowptr, col, y, g, mean, form).astype(np.float64) - ref)
        bound = 1e-5 * mag + TINY
        print(f"{form} k {k} mean {mean}: max err / bound = {np.max(err / bound):.3g}, max err / mag = {np.max(err / (mag + 1e-30)) / 2.0 ** -24:.3g} * 2^-24")
        assert np.all(err <= bound), (form, k, mean, np.max(err / bound))
        assert np.max(err / (mag + 1e-30)) <= 24 * 2.0 ** -24, "the derivation: at most about 24 roundings of 2^-24"
    yi, gi = cases.dense(cs.N, k, 3, "integer"), cases.dense(m, k, 5, "integer")
    assert np.array_equal(cs.emulate(rowptr, col, yi, gi, False, form), oracle_mod.sddmm(rowptr, col, yi, gi))
    magi = oracle_mod.sddmm(rowptr, col, np.abs(yi), np.abs(gi), mean=True).astype(np.float64)
    erri = np.abs(cs.emulate(rowptr, col, yi, gi, True, form).astype(np.float64) - oracle_mod.sddmm(rowptr, col, yi, gi, mean=True))
    assert np.all(erri <= 1e-6 * magi + 1e-30), (form, k, np.max(erri / (1e-6 * magi + 1e-30)))


@pytest.mark.parametrize("form,k", (("task", 41), ("row1", 41), ("task", 64), ("row4", 64)))
def test_emulated_subnormal_operands_meet_the_bound_and_a_flush_misses_it(oracle_mod, form, k):
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    y, g = cs.subnormal_operands(m, k)
    for mean in (False, True):
        ref = oracle_mod.sddmm(rowptr, col, y, g, mean=mean).astype(np.float64)
        bound = 1e-5 * oracle_mod.sddmm(rowptr, col, np.abs(y), np.abs(g), mean=mean).astype(np.float64) + TINY
        err = np.abs(cs.emulate(rowptr, col, y, g, mean, form).astype(np.float64) - ref)
        print(f"{form} k {k} mean {mean}: subnormal max err / bound = {np.max(err / bound):.3g}")
        assert np.all(err <= bound), (form, k, mean, np.max(err / bound))
        flushed = np.abs(cs.emulate(rowptr, col, y, g, mean, form, flush=True).astype(np.float64) - ref)
        print(f"{form} k {k} mean {mean}: flushed max err / bound = {np.max(flushed / bound):.3g}")
        assert np.mean(flushed > 100 * bound) > 0.5, "a kernel that flushes subnormals must miss the bound by orders of magnitude"


@pytest.mark.parametrize("k", cs.TRAP_WIDTHS)
def test_emulated_trap_gives_inf_and_the_unmasked_copy_nan(oracle_mod, k):
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    y, g = cs.ragged_trap(m, k)
    hot = np.isinf(y).any(1)[col]
    sign = np.sign(y[:, cs.duplicated_columns(k)[0]])[col]
    for mean in (False, True):
        good = cs.emulate(rowptr, col, y, g, mean, "task")
        assert not np.any(np.isnan(good)) and np.array_equal(np.isinf(good), hot) and np.array_equal(np.sign(good[hot]), sign[hot])
        mag = oracle_mod.sddmm(rowptr, col, np.abs(y), np.abs(g), mean=mean).astype(np.float64)
        ref = oracle_mod.sddmm(rowptr, col, y, g, mean=mean).astype(np.float64)
        assert np.all(np.abs(good[~hot].astype(np.float64) - ref[~hot]) <= 1e-5 * mag[~hot] + TINY)
        broken = cs.emulate(rowptr, col, y, g, mean, "task", zero_times_dup=True)
        assert np.array_equal(np.isnan(broken), hot), "Inf * 0 in the duplicated components: every trapped edge is NaN"
        row = cs.emulate(rowptr, col, y, g, mean, "row1")                  # the row kernel has no shifted vector
        assert not np.any(np.isnan(row)) and np.array_equal(np.isinf(row), hot)


# ---- the wrappers' operand checks -------------------------------------------------------------------------------------------------

def _plan(m, slices=3, ncols=cs.N):
    """What sddmm_tasks reads of a TaskPlan before the library is touched."""
    return types.SimpleNamespace(slices=slices, seg_off=torch.zeros(slices * m + 1, dtype=torch.int32), ncols=ncols, n_tasks=0,
                                 lane_off=[0] * 9, task_row=torch.zeros(0, dtype=torch.int32), task_b=torch.zeros(0, dtype=torch.int64),
                                 task_len=torch.zeros(0, dtype=torch.int32), col32=None)


def _handle(rowptr, col, ncols):
    """A GraphHandle as its checks see it, without the library's object (there is no device to make one on)."""
    from isplib_amd import cabi
    h = object.__new__(cabi.GraphHandle)
    h.rowptr, h.col, h.val, h.m, h.n, h._cols_ok, h._h = rowptr, col, None, rowptr.numel() - 1, ncols, None, None
    return h


def _bad_operands(rowptr, col, y, g):
    F64, BF = torch.float64, torch.bfloat16
    m, k = g.shape
    wide_y, wide_g = torch.zeros((cs.N, 2 * k)), torch.zeros((m, 2 * k))
    return (
        ("g one row short", rowptr, col, y, g[:-1], None, ValueError),
        ("g one row long", rowptr, col, y, torch.zeros((m + 1, k)), None, ValueError),
        ("g narrower than y", rowptr, col, y, g[:, :k - 2], None, ValueError),
        ("g wider than y", rowptr, col, y, wide_g, None, ValueError),
        ("g 1-D", rowptr, col, y, g.reshape(-1), None, ValueError),
        ("g 3-D", rowptr, col, y, g.reshape(m, k, 1), None, ValueError),
        ("g not a tensor", rowptr, col, y, g.numpy(), None, ValueError),
        ("y 1-D", rowptr, col, y.reshape(-1), g, None, ValueError),
        ("y not a tensor", rowptr, col, None, g, None, ValueError),
        ("y float64", rowptr, col, y.to(F64), g.to(F64), None, TypeError),
        ("y bfloat16", rowptr, col, y.to(BF), g, None, TypeError),
        ("g float64", rowptr, col, y, g.to(F64), None, TypeError),
        ("g bfloat16", rowptr, col, y, g.to(BF), None, TypeError),
        ("y column-major", rowptr, col, y.t().contiguous().t(), g, None, ValueError),
        ("g column-major", rowptr, col, y, g.t().contiguous().t(), None, ValueError),
        ("y every other column", rowptr, col, wide_y[:, ::2], g, None, ValueError),
        ("g rows overlap", rowptr, col, y, torch.zeros(k).expand(m, k), None, ValueError),
        ("rowptr int32", rowptr.to(torch.int32), col, y, g, None, TypeError),
        ("col int32", rowptr, col.to(torch.int32), y, g, None, TypeError),
        ("rowptr 2-D", rowptr.reshape(1, -1), col, y, g, None, ValueError),
        ("rowptr empty", rowptr[:0], col, y, g[:0], None, ValueError),
        ("out too short", rowptr, col, y, g, torch.zeros(col.numel() - 1), ValueError),
        ("out float64", rowptr, col, y, g, torch.zeros(col.numel(), dtype=F64), ValueError),
        ("out 2-D", rowptr, col, y, g, torch.zeros((col.numel(), 1)), ValueError),
        ("out strided", rowptr, col, y, g, torch.zeros(2 * col.numel())[::2], ValueError),
        ("well-shaped, but not on a GPU", rowptr, col, y, g, None, ValueError),
        ("well-shaped views, but not on a GPU", rowptr, col, wide_y[:, 1:1 + k], wide_g[:, 3:3 + k], torch.zeros(col.numel() + 64), ValueError),
    )


def test_wrappers_refuse_every_mis_shaped_operand_before_the_library_is_touched(monkeypatch):
    from isplib_amd import cabi
    rowptr, col = (torch.from_numpy(a) for a in cases.random_csr(30, cs.N, 3.0, 1))
    m, k = 30, 64
    y, g = torch.zeros((cs.N, k)), torch.zeros((m, k))

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(cabi, "lib", no_library)
    for what, rp, cl, yy, gg, out, err in _bad_operands(rowptr, col, y, g):
        with pytest.raises(err):
            cabi.sddmm(rp, cl, yy, gg, out=out)
        with pytest.raises(err):
            cabi.sddmm(rp, cl, yy, gg, True, out=out, check=False)
        with pytest.raises(err):
            cabi.sddmm_tasks(rp, cl, _plan(m), yy, gg, out=out)
        if rp is rowptr and cl is col:                                     # the handle owns its rowptr and col
            with pytest.raises(err):
                _handle(rowptr, col, cs.N).sddmm(yy, gg, out=out)
    # the task and handle forms: y must hold a row for every column the plan / handle was built for, the plan one segment list
    # per row of this graph
    with pytest.raises(ValueError, match="built for 200 columns"):
        cabi.sddmm_tasks(rowptr, col, _plan(m), y[:150], g)
    with pytest.raises(ValueError, match="built for 200 columns"):
        _handle(rowptr, col, cs.N).sddmm(y[:150], g)
    with pytest.raises(ValueError, match="built for 29 rows"):
        cabi.sddmm_tasks(rowptr, col, _plan(m - 1), y, g)
    with pytest.raises(ValueError, match="built for 31 rows"):
        cabi.sddmm_tasks(rowptr, col, _plan(m + 1), y, g)
    # column ids, behind check=True: looked at before the device is (a CPU tensor answers), and not with check=False
    low, high = col.clone(), col.clone()
    low[3], high[5] = -1, cs.N
    for bad in (low, high):
        with pytest.raises(ValueError, match="column ids"):
            cabi.sddmm(rowptr, bad, y, g)
        with pytest.raises(ValueError, match="column ids"):
            cabi.sddmm_tasks(rowptr, bad, _plan(m), y, g)
        with pytest.raises(ValueError, match="GPU tensor"):
            cabi.sddmm(rowptr, bad, y, g, check=False)
    with pytest.raises(ValueError, match="column ids"):
        cabi.sddmm(rowptr, col, y[:int(col.max())], g)                     # y one row short of the largest column id
