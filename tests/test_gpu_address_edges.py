"""Parity at the address-width edges of the kernel families.

A gather offset of the stream, task-list, sliced, SDDMM and generic FusedMM kernels is an unsigned 32-bit byte offset
through a buffer descriptor (up to BUF_LIMIT = 3.5 GiB); the plain kernel falls back to 64-bit addresses past that; the
deterministic max / min backward sorts 32-bit keys.  The rest of the suite runs on operands of a few hundred MB, where
bit 31 of an offset is never set.  Here every family runs on dense operands of 2-4.4 GB (and outputs past 4 GiB) with
small graphs built to hit the far end of X on purpose: the first rows, the last rows, the first row whose byte offset
is >= 2^31 (and >= 2^32 where the operand reaches it), a hub row of 12,345 edges over the top of X, empty rows,
duplicate columns and degrees that are not multiples of 64.

The reference is exact: only the rows of X a graph touches are copied to the host (`_Graph.compact`), ascending, so
each row's edges keep their CSR order, and the oracle runs on the compacted operand.  X and the weights are integer
valued, so every fp32 sum is exact in any order: sum and SDDMM must equal the oracle, max / min values and CSR
positions bit for bit; an fp64 sum on the device over the uncompacted operand is the second arbiter.

Each test states its peak device memory; the 2.30 GB operand is shared through a module fixture.

The attention families (attention, gat, gatv2, mha, their EDGE / DROP forms and 16-bit twins) came after this module: their gathers past
2^31 bytes, up to the last pitch their domains admit, are in tests/test_gpu_attention_address_edges.py.
"""
import gc

import numpy as np
import pytest
import torch

from tests import cases

pytestmark = pytest.mark.gpu

BUF_LIMIT = 0xE0000000          # gather.h: bytes one buffer descriptor addresses
PANEL_BYTES = 256 << 20         # spmm.hip: the index-order plain launch runs K > 128 in panels past this operand size
HUB_DEG = 12345


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _int_features(n, k, seed, dev):
    """Integer-valued X in {-3..3} made in place (no int64 temporary of the whole operand)."""
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    return torch.randint(-3, 4, (n, k), generator=gen, device=dev, dtype=torch.float32)


class _Graph:
    """m rows over n columns, rows column-sorted, with the far end of X hit on purpose.  `row_bytes`: the byte pitch of
    a row of X (ldy * 4), to place the edges to the first rows at or past 2^31 and 2^32 bytes."""

    def __init__(self, n, row_bytes, dev, m=20000, mean_deg=48, seed=0, top=None):
        rng = np.random.default_rng(seed)
        top = n if top is None else top                     # columns are < top (<= n)
        self.far = sorted({r for b in (1 << 31, 1 << 32) for r in ((b + row_bytes - 1) // row_bytes,) if r < top})
        special = {
            0: np.arange(10),                                                    # the first rows of X
            1: top - 1 - np.arange(10),                                          # the last rows
            2: np.array([r + d for r in self.far for d in (-1, 0, 1) if 0 <= r + d < top], np.int64),
            3: rng.integers(max(0, top - top // 8), top, HUB_DEG),               # the hub, over the top eighth
            5: np.array([0, 0] + [r for r in self.far for _ in range(3)] + [top - 1, top - 1], np.int64),   # duplicates
        }
        deg = rng.integers(0, 2 * mean_deg, m).astype(np.int64)
        deg[deg % 64 == 0] += 1                                                  # masked lanes everywhere
        for r in (4, 100, m // 2, m - 1):
            deg[r] = 0                                                           # empty rows, the last one included
        for r, c in special.items():
            deg[r] = c.size
        rowptr = np.zeros(m + 1, np.int64)
        np.cumsum(deg, out=rowptr[1:])
        col = rng.integers(0, top, int(rowptr[-1])).astype(np.int64)
        hi = rng.random(col.size) < 0.3                                          # a third of the edges over the top quarter
        col[hi] = rng.integers(max(0, top - top // 4), top, int(hi.sum()))
        for r, c in special.items():
            col[rowptr[r]:rowptr[r + 1]] = c
        row = np.repeat(np.arange(m, dtype=np.int64), deg)
        col = col[np.lexsort((col, row))]
        self.m, self.n, self.nnz = m, n, col.size
        self.rp, self.cl = rowptr, col
        self.uniq, self.inv = np.unique(col, return_inverse=True)
        self.inv = self.inv.astype(np.int64).reshape(-1)
        assert self.uniq[0] == 0 and self.uniq[-1] == top - 1 and all(r in self.uniq for r in self.far)
        self.rowptr = torch.from_numpy(rowptr).to(dev)
        self.col = torch.from_numpy(col).to(dev)
        self.d_uniq = torch.from_numpy(self.uniq.astype(np.int64)).to(dev)
        self.w = cases.weights(col.size, seed + 1, "signed_int")
        self.d_w = torch.from_numpy(self.w).to(dev)

    def compact(self, x):
        """The rows of x the graph touches, ascending, on the host."""
        return x[self.d_uniq].cpu().numpy()

    def weights(self, weighted):
        return (self.d_w, self.w) if weighted else (None, np.ones(self.nnz, np.float32))

    def fp64_sum(self, x, d_w=None, mean=False):
        """Second arbiter: the fp64 sum on the device over the uncompacted operand."""
        rows = torch.repeat_interleave(torch.arange(self.m, device=x.device), self.rowptr.diff())
        out = torch.zeros((self.m, x.size(1)), dtype=torch.float64, device=x.device)
        for b in range(0, self.nnz, 1 << 19):
            t = x[self.col[b:b + (1 << 19)]].double()
            if d_w is not None:
                t *= d_w[b:b + (1 << 19), None].double()
            out.index_add_(0, rows[b:b + (1 << 19)], t)
        if mean:
            out /= self.rowptr.diff().clamp(min=1).double()[:, None]
        return out.cpu().numpy()


def _exact(got, ref, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert np.array_equal(got, ref), f"{what}: {np.count_nonzero(got != ref)} elements differ"


def _bits(got, ref, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), what


def _mean_close(oracle, g, xs, w, got, what):
    ref, _ = oracle.spmm_fw(g.rp, g.inv, w, xs, "mean")
    mag, _ = oracle.spmm_fw(g.rp, g.inv, np.abs(w), np.abs(xs), "mean")
    got = got.cpu().numpy()
    assert np.all(np.abs(got - ref) <= 1e-5 * mag + 1e-30), what


def _check_spmm(oracle, g, xs, w, red, out, arg, what):
    ref, ref_arg = oracle.spmm_fw(g.rp, g.inv, w, xs, red)
    if red == "sum":
        _exact(out, ref, what)
    elif red == "mean":
        _mean_close(oracle, g, xs, w, out, what)
    else:
        _bits(out, ref, what)
        if arg is not None:
            _exact(arg, ref_arg, what + " positions")


@pytest.fixture(scope="module")
def tall(gpu):
    """X [9.0 M, 64] fp32 (2.30 GB: offsets past 2^31, rows below 2^24) and a graph hitting its far end."""
    n, k = 9_000_000, 64
    assert (1 << 31) < n * k * 4 < BUF_LIMIT and n < (1 << 24)
    x = _int_features(n, k, 3, gpu)
    g = _Graph(n, k * 4, gpu, seed=11)
    assert g.far == [(1 << 31) // (k * 4)]
    return x, g, g.compact(x)


# ---- stream schedule ---------------------------------------------------------------------------------------------------

def _stream_plans(g, n, weighted, streams_list=(2, 4, 8), slices=6):
    from isplib_amd import cabi
    from isplib_amd.plan import build_stream_plan
    d_w = g.d_w if weighted else None
    for streams in streams_list:
        p = build_stream_plan(g.rowptr, g.col, d_w, n, slices, None, None, streams, 512)
        assert p is not None
        yield f"torch-built streams={streams}", p
        nat = cabi.NativeStreamPlan(g.rowptr, g.col, d_w, n, streams, slices, 512)
        yield f"native streams={streams}", nat
        nat.close()


def _stream_sum_mean(oracle, g, x, xs, weighted, label):
    from isplib_amd import cabi
    _, w = g.weights(weighted)
    ref64 = g.fp64_sum(x, g.d_w if weighted else None)
    for name, plan in _stream_plans(g, x.size(0), weighted):
        for red in ("sum", "mean"):
            out = cabi.spmm_stream(g.rowptr, g.nnz, plan, x, red)
            again = cabi.spmm_stream(g.rowptr, g.nnz, plan, x, red)
            assert torch.equal(out.view(torch.int32), again.view(torch.int32)), (label, name, red)
            _check_spmm(oracle, g, xs, w, red, out, None, f"{label} {name} {red}")
            if red == "sum":
                assert np.array_equal(out.cpu().numpy().astype(np.float64), ref64), (label, name)


@pytest.mark.parametrize("weighted", (True, False))
def test_stream_sum_mean_on_a_tall_operand_past_2_gib(gpu, oracle_mod, tall, weighted):
    """Boundary: gather offsets past 2^31 on the stream schedule (n = 9.0 M, K = 64, 2.30 GB), torch-built and native
    plans on 2, 4 and 8 streams, weighted and unit.  Exact against the oracle and the fp64 arbiter; two launches bitwise
    equal.  Peak device memory: ~3 GB."""
    x, g, xs = tall
    _stream_sum_mean(oracle_mod, g, x, xs, weighted, "tall")


def test_stream_at_the_widest_24_bit_column_and_one_past(gpu, oracle_mod):
    """Boundary: the stream word's 24-bit column id.  Inside: n = 2^24 - 1, K = 48 (3.22 GB, the widest column x pitch
    offset), the graph reaching column 2^24 - 2: exact on both plan builders.  Outside: n = 2^24 is refused by both plan
    builders (the native one with status FAIL, decided before any launch) and the graph handle serves it on another schedule with the
    same answer.  Peak device memory: ~3.4 GB."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_stream_plan
    k, n_out = 48, 1 << 24
    n_in = n_out - 1
    big = _int_features(n_out, k, 5, gpu)
    x = big[:n_in]
    assert x.is_contiguous() and n_in * k * 4 < BUF_LIMIT
    g = _Graph(n_in, k * 4, gpu, seed=12)
    xs = g.compact(x)
    assert g.uniq[-1] == n_in - 1
    _, w = g.weights(True)
    out_in = None
    for name, plan in _stream_plans(g, n_in, True, streams_list=(2, 4)):
        out = cabi.spmm_stream(g.rowptr, g.nnz, plan, x, "sum")
        _check_spmm(oracle_mod, g, xs, w, "sum", out, None, f"n=2^24-1 {name}")
        out_in = out
    # one past: n = 2^24 (the same graph: X's extra last row is never touched)
    assert build_stream_plan(g.rowptr, g.col, g.d_w, n_out, 6, None, None, 4, 512) is None
    with pytest.raises(cabi.IsplibError) as e:
        cabi.NativeStreamPlan(g.rowptr, g.col, g.d_w, n_out, 4, 6, 512)
    assert e.value.status == cabi.ISPLIB_FAIL and cabi.last_error()
    h = cabi.GraphHandle(g.rowptr, g.col, g.d_w, n_out)
    try:
        served, _ = h.spmm(big, "sum")
    finally:
        h.close()
    _exact(served, out_in.cpu().numpy(), "handle at n = 2^24")


def test_stream_sum_on_a_padded_operand_with_the_widest_pitch(gpu, oracle_mod):
    """Boundary: ldy = 2^22 - 4 (3.36 GB operand of n = 200 rows, a K = 64 column block at column 4096), the widest row
    pitch the stream entries accept, through the raw entry (the block is not copied).  Exact, both plan builders.
    Peak device memory: ~3.4 GB."""
    from isplib_amd import cabi
    n, ld, k, c0 = 200, (1 << 22) - 4, 64, 4096
    assert n * ld * 4 < BUF_LIMIT
    wide = torch.zeros((n, ld), dtype=torch.float32, device=gpu)
    wide[:, c0:c0 + k] = _int_features(n, k, 6, gpu)
    block = wide[:, c0:c0 + k]
    assert block.stride(0) == ld
    g = _Graph(n, ld * 4, gpu, m=6000, mean_deg=40, seed=13)
    assert g.far and g.far[0] < n
    xs = g.compact(block)
    _, w = g.weights(True)
    for name, plan in _stream_plans(g, n, True, streams_list=(4,)):
        out = torch.empty((g.m, k), device=gpu)
        cabi.fusedMM_csr_stream_hip(cabi.MSG_SPMM_SUM, g.rowptr, g.nnz, plan, block, out, plan.workspace())
        _check_spmm(oracle_mod, g, xs, w, "sum", out, None, f"ldy=2^22-4 {name}")


def test_stream_and_plain_at_exactly_buf_limit_and_one_row_past(gpu, oracle_mod):
    """Boundary: n * ldy * 4 == BUF_LIMIT exactly (n = 229,376, ldy = 4096, a K = 64 block): the stream schedule and the
    plain kernel on its buffer path; one row more (n = 229,377) takes the plain kernel's 64-bit path, and the stream
    entry refuses it (status FAIL before any launch).  Exact; the ordered kernel equals the plain one bitwise.
    Peak device memory: ~3.8 GB."""
    from isplib_amd import cabi
    n, ld, k, c0 = 229_376, 4096, 64, 1000
    assert n * ld * 4 == BUF_LIMIT
    wide = torch.zeros((n + 1, ld), dtype=torch.float32, device=gpu)
    wide[:, c0:c0 + k] = _int_features(n + 1, k, 7, gpu)
    g = _Graph(n, ld * 4, gpu, m=8000, mean_deg=40, seed=14)
    _, w = g.weights(True)
    for rows in (n, n + 1):
        block = wide[:rows, c0:c0 + k]
        xs = g.compact(block)
        for red in cases.REDUCES:
            out = torch.empty((g.m, k), device=gpu)
            arg = torch.empty((g.m, k), dtype=torch.int64, device=gpu) if red in ("max", "min") else None
            cabi.fusedMM_csr_hip(cabi.MESSAGE[red], g.rowptr, g.col, g.d_w, block, out, arg)
            _check_spmm(oracle_mod, g, xs, w, red, out, arg, f"plain rows={rows} {red}")
            out2 = torch.empty_like(out)
            arg2 = None if arg is None else torch.empty_like(arg)
            order = torch.arange(g.m, dtype=torch.int32, device=gpu)
            cabi.fusedMM_csr_ordered_hip(cabi.MESSAGE[red], g.rowptr, g.col, g.d_w, order, block, out2, arg2)
            assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and (arg is None or torch.equal(arg, arg2)), (rows, red)
        plan = cabi.NativeStreamPlan(g.rowptr, g.col, g.d_w, rows, 4, 6, 512)
        try:
            out = torch.empty((g.m, k), device=gpu)
            st = cabi.fusedMM_csr_stream_hip(cabi.MSG_SPMM_SUM, g.rowptr, g.nnz, plan, block, out, plan.workspace(), check=False)
            if rows == n:
                assert st == cabi.SUCCESS
                _check_spmm(oracle_mod, g, xs, w, "sum", out, None, "stream at BUF_LIMIT")
            else:
                assert st == cabi.ISPLIB_FAIL and "3.5 GiB" in cabi.last_error()
        finally:
            plan.close()


@pytest.mark.parametrize("red", ("max", "min"))
def test_stream_max_min_just_under_2_gib_and_at_2_gib(gpu, oracle_mod, tall, red):
    """Boundary: the max / min stream entry stops below 2 GiB.  Inside: the rows of the 2.30 GB tensor cut to
    n = 2^31 / 256 - 1 (the last row ends one row short of 2^31 bytes), graph reaching row n - 1: values and positions
    bit-exact, with and without positions, both plan builders.  Outside: n = 2^31 / 256 is not offered the schedule (the
    rule asked for a graph it would otherwise take) and the entry refuses it; the graph handle serves it on another schedule with the same bits.  Peak device memory: ~3 GB."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_stream_plan
    x, _, _ = tall
    k = x.size(1)
    n_out = (1 << 31) // (k * 4)
    n_in = n_out - 1
    y = x[:n_in]
    g = _Graph(n_in, k * 4, gpu, seed=15)
    assert g.uniq[-1] == n_in - 1
    xs = g.compact(y)
    _, w = g.weights(True)
    ref, ref_arg = oracle_mod.spmm_fw(g.rp, g.inv, w, xs, red)
    for streams in (4, 8):
        plans = [("torch-built", build_stream_plan(g.rowptr, g.col, g.d_w, n_in, 6, None, None, streams, 512, minmax=True)),
                 ("native", cabi.NativeStreamPlan(g.rowptr, g.col, g.d_w, n_in, streams, 6, 512, minmax=True))]
        for name, plan in plans:
            assert plan is not None
            out, arg = cabi.spmm_stream_minmax(g.rowptr, g.nnz, plan, y, red)
            _bits(out, ref, (name, streams, red))
            _exact(arg, ref_arg, f"{name} streams={streams} {red} positions")
            out2, none = cabi.spmm_stream_minmax(g.rowptr, g.nnz, plan, y, red, want_arg=False)
            assert none is None
            _bits(out2, ref, (name, streams, red, "no positions"))
        plans[1][1].close()
    # at 2 GiB
    y_out = x[:n_out]
    assert n_out * k * 4 == 1 << 31
    assert cabi.suggest_stream_minmax(g.m, n_in, 1 << 28, k) is not None and cabi.suggest_stream_minmax(g.m, n_out, 1 << 28, k) is None
    plan = cabi.NativeStreamPlan(g.rowptr, g.col, g.d_w, n_out, 4, 6, 512, minmax=True)
    try:
        out = torch.empty((g.m, k), device=gpu)
        arg = torch.empty((g.m, k), dtype=torch.int64, device=gpu)
        st = cabi.fusedMM_csr_stream_minmax_hip(cabi.MESSAGE[red], g.rowptr, g.nnz, plan, y_out, out, arg, plan.workspace(minmax=True), check=False)
        assert st == cabi.ISPLIB_FAIL and "2 GiB" in cabi.last_error()
    finally:
        plan.close()
    h = cabi.GraphHandle(g.rowptr, g.col, g.d_w, n_out)
    try:
        out, arg = h.spmm(y_out, red)
    finally:
        h.close()
    _bits(out, ref, "handle at 2 GiB")
    _exact(arg, ref_arg, "handle at 2 GiB positions")


# ---- task list, sliced form, plain and ordered kernels -----------------------------------------------------------------

def test_task_list_and_sliced_form_every_reduce_past_2_gib(gpu, oracle_mod, tall):
    """Boundary: the task list and the sliced plain kernel on the 2.30 GB operand (buffer offsets past 2^31), slice counts
    1, 7 and 16, every reduce, weighted.  Exact / bit-exact.  Peak device memory: ~3 GB."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_task_plan
    x, g, xs = tall
    n = x.size(0)
    _, w = g.weights(True)
    for slices in (1, 7, 16):
        plan = build_task_plan(g.rowptr, g.col, n, slices)
        assert plan is not None and int(plan.task_len.sum()) == g.nnz
        table, ok = cabi.spmm_slices(g.rowptr, g.col, n, slices)
        assert ok
        for red in cases.REDUCES:
            out, arg = cabi.spmm_tasks(g.rowptr, g.col, g.d_w, plan, x, red)
            _check_spmm(oracle_mod, g, xs, w, red, out, arg, f"tasks slices={slices} {red}")
            out, arg = cabi.spmm_sliced(g.rowptr, g.col, g.d_w, table, slices, x, red)
            _check_spmm(oracle_mod, g, xs, w, red, out, arg, f"sliced slices={slices} {red}")


def test_task_list_refuses_past_buf_limit_and_the_handle_serves_it(gpu, oracle_mod):
    """Boundary: the task list stops at 3.5 GiB of dense operand.  One row past (n = 229,377 rows of a 4096-float pitch,
    a K = 64 block): status FAIL from the entry, before any launch; the graph handle serves the same call on the plain
    kernel's 64-bit path, exact.  Peak device memory: ~3.8 GB."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_task_plan
    n, ld, k, c0 = 229_377, 4096, 64, 64
    assert n * ld * 4 > BUF_LIMIT
    wide = torch.zeros((n, ld), dtype=torch.float32, device=gpu)
    wide[:, c0:c0 + k] = _int_features(n, k, 8, gpu)
    block = wide[:, c0:c0 + k]
    g = _Graph(n, ld * 4, gpu, m=8000, mean_deg=40, seed=16)
    xs = g.compact(block)
    _, w = g.weights(True)
    plan = build_task_plan(g.rowptr, g.col, n, 4)
    out = torch.empty((g.m, k), device=gpu)
    st = cabi.fusedMM_csr_tasks_hip(cabi.MSG_SPMM_SUM, g.rowptr, g.col, g.d_w, plan, block, out, None, plan.workspace("sum", k), check=False)
    assert st == cabi.ISPLIB_FAIL and "3.5 GiB" in cabi.last_error()
    h = cabi.GraphHandle(g.rowptr, g.col, g.d_w, n)
    try:
        for red in cases.REDUCES:
            out, arg = h.spmm(block, red)
            _check_spmm(oracle_mod, g, xs, w, red, out, arg, f"handle past BUF_LIMIT {red}")
    finally:
        h.close()


def test_plain_and_ordered_kernels_past_4_gib(gpu, oracle_mod):
    """Boundary: 64-bit addresses with offsets past 2^32 (n = 17 M, K = 64: 4.35 GB, graph reaching the first row at or
    past 2^31 and 2^32 bytes): the plain kernel, the ordered kernel (identity and shuffled order: bitwise the plain result)
    and the graph handle, every reduce; ragged K = 61 (a column block) on the same path.  Exact / bit-exact.
    Peak device memory: ~4.6 GB."""
    from isplib_amd import cabi
    n, k = 17_000_000, 64
    assert n * k * 4 > (1 << 32)
    x = _int_features(n, k, 9, gpu)
    g = _Graph(n, k * 4, gpu, seed=17)
    assert len(g.far) == 2
    xs = g.compact(x)
    _, w = g.weights(True)
    shuffled = torch.randperm(g.m, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(gpu)
    ident = torch.arange(g.m, dtype=torch.int32, device=gpu)
    h = cabi.GraphHandle(g.rowptr, g.col, g.d_w, n)
    try:
        for red in cases.REDUCES:
            out, arg = cabi.spmm(g.rowptr, g.col, g.d_w, x, red)
            _check_spmm(oracle_mod, g, xs, w, red, out, arg, f"plain {red}")
            for name, order in (("identity", ident), ("shuffled", shuffled)):
                o2, a2 = cabi.spmm_ordered(g.rowptr, g.col, g.d_w, order, x, red)
                assert torch.equal(out.view(torch.int32), o2.view(torch.int32)) and (arg is None or torch.equal(arg, a2)), (name, red)
            o3, a3 = h.spmm(x, red)
            _check_spmm(oracle_mod, g, xs, w, red, o3, a3, f"handle {red}")
        ref64 = g.fp64_sum(x, g.d_w)
        assert np.array_equal(cabi.spmm(g.rowptr, g.col, g.d_w, x, "sum")[0].cpu().numpy().astype(np.float64), ref64)
        block = x[:, :61]                                  # ragged K on the 64-bit path
        for red in cases.REDUCES:
            out = torch.empty((g.m, 61), device=gpu)
            arg = torch.empty((g.m, 61), dtype=torch.int64, device=gpu) if red in ("max", "min") else None
            cabi.fusedMM_csr_hip(cabi.MESSAGE[red], g.rowptr, g.col, g.d_w, block, out, arg)
            _check_spmm(oracle_mod, g, np.ascontiguousarray(xs[:, :61]), w, red, out, arg, f"ragged {red}")
    finally:
        h.close()


@pytest.mark.parametrize("red", ("sum", "max"))
def test_output_offsets_past_4_gib(gpu, oracle_mod, red):
    """Boundary: z (and for max z_arg, which shares z's leading dimension) written past 4 GiB: z is a K = 64 column block
    of a [300, 4 M] fp32 tensor (4.8 GB; z_arg [300, 4 M] int64, 9.6 GB).  Exact / bit-exact, and the columns outside the
    block are untouched (checked on the device).  Peak device memory: sum ~5 GB, max ~15 GB."""
    from isplib_amd import cabi
    m, ld, k, c0, n = 300, 4 << 20, 64, (4 << 20) - 128, 100_000
    assert (m - 1) * ld * 4 > (1 << 32)
    x = _int_features(n, k, 10, gpu)
    g = _Graph(n, k * 4, gpu, m=m, mean_deg=60, seed=18)
    xs = g.compact(x)
    _, w = g.weights(True)
    zw = torch.full((m, ld), 7.0, dtype=torch.float32, device=gpu)
    aw = torch.full((m, ld), -5, dtype=torch.int64, device=gpu) if red == "max" else None
    z = zw[:, c0:c0 + k]
    za = None if aw is None else aw[:, c0:c0 + k]
    cabi.fusedMM_csr_hip(cabi.MESSAGE[red], g.rowptr, g.col, g.d_w, x, z, za)
    _check_spmm(oracle_mod, g, xs, w, red, z.cpu().numpy(), None if za is None else za.cpu().numpy(), f"z past 4 GiB {red}")
    zw[:, c0:c0 + k] = 7.0
    assert bool((zw == 7.0).all()), "a column outside the block was written"
    if aw is not None:
        aw[:, c0:c0 + k] = -5
        assert bool((aw == -5).all()), "a position outside the block was written"


# ---- SDDMM and the generic FusedMM pipeline ----------------------------------------------------------------------------

@pytest.mark.parametrize("mean", (False, True))
def test_sddmm_plain_and_task_forms_past_2_gib(gpu, oracle_mod, tall, mean):
    """Boundary: isplib_sddmm_csr_hip and isplib_sddmm_csr_tasks_hip gathering y rows past 2^31 bytes (2.30 GB y).
    Integer operands: sum exact against the oracle; mean within the oracle bound.  Peak device memory: ~3 GB."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_task_plan
    x, g, xs = tall
    k = x.size(1)
    gm = _int_features(g.m, k, 19, gpu)
    ref = oracle_mod.sddmm(g.rp, g.inv, xs, gm.cpu().numpy(), mean)
    mag = oracle_mod.sddmm(g.rp, g.inv, np.abs(xs), np.abs(gm.cpu().numpy()), mean)
    plan = build_task_plan(g.rowptr, g.col, x.size(0), 7)
    for name, got in (("plain", cabi.sddmm(g.rowptr, g.col, x, gm, mean)), ("tasks", cabi.sddmm_tasks(g.rowptr, g.col, plan, x, gm, mean))):
        got = got.cpu().numpy()
        if mean:
            assert np.all(np.abs(got - ref) <= 1e-6 * mag + 1e-30), name
        else:
            _exact(got, ref, f"sddmm {name}")


def test_generic_pipeline_and_stream_fusedmm_past_2_gib(gpu, oracle_mod, tall):
    """Boundary: the generic FusedMM pipeline (plain and task forms, sigmoid and t-distribution words) and the stream
    FusedMM front end gathering y rows past 2^31 bytes (2.30 GB y).  Within the oracle bound.  Peak device memory: ~5 GB."""
    from isplib_amd import cabi
    from isplib_amd.plan import build_task_plan
    y, g, ys = tall
    n, k = y.size(0), y.size(1)
    ys = ys * np.float32(0.2)
    yr = y * 0.2                        # 2.30 GB more: scaled so that the sigmoid is not saturated
    xl = torch.from_numpy(cases.dense(g.m, k, 20) * np.float32(0.2)).to(gpu)
    xh = xl.cpu().numpy()
    plan = build_task_plan(g.rowptr, g.col, n, 7)
    geom = cabi.fusedmm_stream_geometry(4)
    assert geom[0] > 0
    fplan = cabi.NativeStreamPlan(g.rowptr, g.col, None, n, 4, 6, 512, fusedmm=True)
    try:
        for pattern in ("sigmoid_embedding", "tdist_embedding"):
            word, fn = cabi.PATTERNS[pattern]
            st, ref, _ = oracle_mod.fusedmm_general(word, g.rp, g.inv, None, xh, ys, cabi.SOP_UDEF[fn], 0.0)
            assert st == 0
            bound = 1e-4 * np.abs(ref).max() + 1e-7
            for name, p in (("plain", None), ("tasks", plan)):
                st, z, _ = cabi.fusedmm(word, g.rowptr, g.col, None, xl, yr, sop_udef=fn, plan=p)
                assert np.all(np.abs(z.cpu().numpy() - ref) <= bound), (pattern, name)
            _, z = cabi.fusedmm_stream(word, g.rowptr, g.nnz, fplan, xl, yr, sop_udef=fn)
            assert np.all(np.abs(z.cpu().numpy() - ref) <= bound), (pattern, "stream")
    finally:
        fplan.close()


# ---- deterministic max / min backward ----------------------------------------------------------------------------------

def test_det_minmax_backward_and_row_scatter_with_sort_keys_past_2_31(gpu, oracle_mod):
    """Boundary: the deterministic max / min backward sorts 32-bit keys dest * k + c; with n = 35 M, k = 64
    (n * k = 2.24e9) keys of the far rows are >= 2^31.  Positions come from the compacted oracle's forward, so no forward
    runs on the device.  dX: exact against oracle.spmm_minmax_bw on the touched rows, every other row exactly zero, equal
    to the atomic form, bitwise reproducible.  isplib_scatter_rows_det_hip with lo > 0 on the same keys: exact against an
    fp64 np.add.at.  Peak device memory: ~18 GB."""
    from isplib_amd import cabi
    n, k = 35_000_000, 64
    assert (1 << 31) < n * k < (1 << 32) - 1
    mat = _int_features(n, k, 21, gpu)
    g = _Graph(n, k * 4, gpu, seed=22)
    xs = g.compact(mat)
    _, w = g.weights(True)
    grad_out = _int_features(g.m, k, 23, gpu)
    go = grad_out.cpu().numpy()
    keys = (g.uniq[-1]) * k
    assert keys >= (1 << 31)
    for red in ("max", "min"):
        _, ref_arg = oracle_mod.spmm_fw(g.rp, g.inv, w, xs, red)
        _, ref_dx = oracle_mod.spmm_minmax_bw(g.inv, w, xs, ref_arg, go)
        arg = torch.from_numpy(ref_arg).to(gpu)
        got = []
        for det in (True, True, False):
            _, dx = cabi.spmm_minmax_bw(g.col, g.d_w, mat, arg, grad_out, need_mat=True, need_val=False, deterministic=det)
            rows = dx[g.d_uniq].cpu().numpy()
            dx[g.d_uniq] = 0
            assert not bool(dx.any()), (red, det, "a row no edge points at is not zero")
            del dx
            _exact(rows, ref_dx, f"{red} det={det}")
            got.append(rows)
        assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)), "det backward not bitwise reproducible"
    del mat
    # the row partition's local scatter: destinations in [lo, lo + nrows), sort keys past 2^31
    lo, nrows = 1000, n - 2000
    dest = torch.from_numpy(np.where(ref_arg == g.nnz, -1, g.cl[np.minimum(ref_arg, g.nnz - 1)]).astype(np.int32)).to(gpu)
    dest[(dest < lo) | (dest >= lo + nrows)] = -1
    out = cabi.scatter_rows_det(dest, grad_out, lo, nrows)
    d = dest.cpu().numpy()
    ok = d >= 0
    touched = np.unique(d[ok])
    ref = np.zeros((touched.size, k), np.float64)
    np.add.at(ref, (np.searchsorted(touched, d[ok]), np.broadcast_to(np.arange(k), d.shape)[ok]), go[ok].astype(np.float64))
    assert int(touched[-1] - lo) * k >= (1 << 31)
    t = torch.from_numpy(touched - lo).to(gpu)
    _exact(out[t].cpu().numpy().astype(np.float64), ref, "scatter_rows_det")
    out[t] = 0
    assert not bool(out.any())
    again = cabi.scatter_rows_det(dest, grad_out, lo, nrows)
    again[t] = 0
    assert not bool(again.any())


# ---- row partition across the plain kernel's panel switch --------------------------------------------------------------

def _skewed_square(n, dense_rows, dense_deg, sparse_deg, seed, dev):
    rng = np.random.default_rng(seed)
    deg = np.where(np.arange(n) < dense_rows, dense_deg, sparse_deg).astype(np.int64)
    deg += rng.integers(0, 3, n)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(deg, out=rowptr[1:])
    col = rng.integers(0, n, int(rowptr[-1])).astype(np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), deg)
    col = col[np.lexsort((col, row))]
    return torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)


@pytest.mark.parametrize("n,side", ((100_000, "both one-pass"), (250_000, "straddle"), (300_000, "both panels")))
def test_row_partition_is_bit_identical_across_the_plain_panel_switch(gpu, n, side):
    """Boundary: the plain kernel's index-order launch runs K > 128 in 128-column panels when n * ldy * 4 > 256 MiB, and
    a shard reads a padded gather buffer of world * max_rows >= n rows.  Straddle: n * K * 4 <= 256 MiB < world * max_rows
    * K * 4 (n = 250,000, K = 256, world = 2, a dense first block so that the nnz-balanced cut gives shard 1 over 131,072
    rows); and one shape on each side.  Real-valued X and weights (on integers every association gives the same bits).
    For every reduce and rank, RowPartition.spmm (its all-gather replaced by the fill it would leave) and local_spmm on
    the plain schedule equal the single-device rows bit for bit.  Peak device memory: ~1.5 GB."""
    from isplib_amd import cabi, synth
    from isplib_amd.dist import RowPartition
    k, world = 256, 2
    rowptr, col = _skewed_square(n, n // 5, 40, 4, 30, gpu)
    val = synth.edge_weights(col.numel(), device=gpu)
    x = synth.features(n, k, device=gpu)
    parts = [RowPartition(rowptr, col, val, n, r, world) for r in range(world)]
    padded = parts[0].ncols_padded
    one_dev, shard = n * k * 4 > PANEL_BYTES, padded * k * 4 > PANEL_BYTES
    assert (one_dev, shard) == {"both one-pass": (False, False), "straddle": (False, True), "both panels": (True, True)}[side]
    buf = parts[0].gather_buffer(k)
    buf.zero_()
    for p in range(world):
        r0, r1 = parts[0].x_cuts[p], parts[0].x_cuts[p + 1]
        buf[p * parts[0].max_rows: p * parts[0].max_rows + (r1 - r0)] = x[r0:r1]
    for red in cases.REDUCES:
        whole, whole_arg = cabi.spmm(rowptr, col, val, x, red)
        for part in parts:
            r0, r1 = part.row_cuts[part.rank], part.row_cuts[part.rank + 1]
            part.all_gather = lambda x_shard, b: b.copy_(buf)
            out, arg = part.spmm(part.shard(x), red)
            assert torch.equal(out.view(torch.int32), whole[r0:r1].view(torch.int32)), (side, red, part.rank, "spmm")
            if arg is not None:
                assert torch.equal(arg, whole_arg[r0:r1]), (side, red, part.rank, "spmm positions")
            out = torch.empty((part.rows, k), device=gpu)
            arg = torch.empty((part.rows, k), dtype=torch.int64, device=gpu) if whole_arg is not None else None
            part.local_spmm(("plain", None, None), buf, out, red, arg)
            assert torch.equal(out.view(torch.int32), whole[r0:r1].view(torch.int32)), (side, red, part.rank, "local_spmm")
            if arg is not None:
                assert torch.equal(part.global_arg(arg), whole_arg[r0:r1]), (side, red, part.rank, "local_spmm positions")
    assert cabi.plain_panels(n, k) == one_dev and cabi.plain_panels(padded, k) == shard
