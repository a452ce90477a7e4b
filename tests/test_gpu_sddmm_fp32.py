"""The fp32 value gradient dval[e] = <y[col[e], :], g[row(e), :]> (mean: / max(deg, 1)) in its three forms -- the row kernel
(cabi.sddmm), the task kernel (cabi.sddmm_tasks) and the route through isplib_graph_sddmm (GraphHandle.sddmm) -- edge by edge
against oracle.sddmm (double-precision sums, one rounding).

Small-integer operands (|values| <= 3, |dot| <= 9 * 1024 < 2^24): the sum is exact in any order, so it equals the oracle bit for bit,
and the mean lies within 1e-6 * mag (two fp32 roundings against the oracle's one).  Real operands: |got - ref| <= 1e-5 * mag +
64 * 2^-149 per edge, mag = oracle.sddmm(|y|, |g|, mean) -- BASELINE.md section 3's parity rule; no instantiation performs more than
about 24 roundings of 2^-24 on an edge at k <= 1024 (1.5e-6; tests/test_sddmm_fp32_host.py shows it on these very inputs), and the
absolute term covers roundings in the subnormal range.  Every dval goes through `out=`, a NaN-filled buffer of nnz + 64 entries, so
an unwritten edge and a write past the end both show, and every launch runs twice to equal bits.  The inputs, and the loop edges they
are placed on, are tests/sddmm_fp32_cases.py's."""
import numpy as np
import pytest
import torch

from tests import cases
from tests import sddmm_fp32_cases as cs

pytestmark = pytest.mark.gpu

N = cs.N
PAD = 64
TINY = 64 * 2.0 ** -149


def _on(gpu, *arrays):
    return tuple(torch.from_numpy(np.array(a)).to(gpu) for a in arrays)         # (a copy: the shared references are read-only)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _twice(call, nnz, gpu, written=True):
    """call(out) launched into two NaN-filled buffers of nnz + 64 entries: equal bits, the tail untouched, every edge written
    (`written`: no NaN may remain; off where the data holds NaN of its own).  Returns the nnz results as a numpy array."""
    outs = [torch.full((nnz + PAD,), float("nan"), dtype=torch.float32, device=gpu) for _ in range(2)]
    for o in outs:
        assert call(o) is o, "a given `out` is written in place and returned"
    torch.cuda.synchronize()
    a, b = (o.cpu().numpy() for o in outs)
    assert np.array_equal(_bits(a), _bits(b)), "two launches: equal bits"
    assert np.all(np.isnan(a[nnz:])), "the 64 entries behind dval must not be touched"
    if written:
        left = np.flatnonzero(np.isnan(a[:nnz]))
        assert left.size == 0, f"edges {left[:8].tolist()} ... were not written (or are NaN)"
    return a[:nnz]


def _lengths_of(rowptr, bad):
    deg = np.diff(rowptr)
    erow = np.repeat(np.arange(deg.size), deg)
    return sorted(set(deg[erow[bad]].tolist()))


def _assert_exact(got, ref, rowptr, what):
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{what}: edges of rows of {_lengths_of(rowptr, bad)} edges differ (positions {bad[:8].tolist()} ...)"


def _assert_within(got, ref, bound, rowptr, what, where=None):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    miss = ~(err <= bound) if where is None else where & ~(err <= bound)
    bad = np.flatnonzero(miss)
    shown = err / bound if where is None else (err / bound)[where]
    print(f"{what}: max err / bound = {np.max(shown) if shown.size else 0.0:.3g}")
    assert bad.size == 0, f"{what}: edges of rows of {_lengths_of(rowptr, bad)} edges miss the bound (positions {bad[:8].tolist()} ...)"


# ---- graphs, plans and references: made once, shared, left unchanged --------------------------------------------------------------

@pytest.fixture(scope="module")
def graphs(gpu):
    """name -> (rowptr, col, device rowptr, device col)."""
    out = {}
    for name, (rowptr, col) in (("hub", cs.hub_graph()), ("lengths", cs.length_graph())):
        out[name] = (rowptr, col) + _on(gpu, rowptr, col)
    return out


@pytest.fixture(scope="module")
def plans(gpu, graphs):
    """name -> the task plan the issue places on that graph; the lengths the cases below need must occur."""
    from isplib_amd.plan import build_task_plan
    hub = build_task_plan(graphs["hub"][2], graphs["hub"][3], N, *cs.HUB_PLAN)
    lengths = build_task_plan(graphs["lengths"][2], graphs["lengths"][3], N, *cs.LENGTH_PLAN)
    assert hub is not None and lengths is not None
    have = set(hub.task_len.cpu().tolist())
    assert 64 in have and min(have) < 64 and max(have) <= 64 and min(have) >= 1, sorted(have)
    have = set(lengths.task_len.cpu().tolist())
    want = {1, 63, 64, 65} | {g * cs.U + d for g in (8, 4, 2, 1) for d in (-1, 0, 1)}
    assert want <= have and max(have) <= 4096, sorted(want - have)
    return {"hub": hub, "lengths": lengths}


_REFS = {}


def _case(oracle, graphs, name, k, kind):
    """(y, g, {mean: ref}, {mean: mag}) for cases.dense operands of `kind` on graph `name`: computed once per module run."""
    key = (name, k, kind)
    if key not in _REFS:
        rowptr, col = graphs[name][:2]
        m = rowptr.size - 1
        if kind == "subnormal":
            y, g = cs.subnormal_operands(m, k)
        elif kind == "trap":
            y, g = cs.ragged_trap(m, k)
        else:
            y, g = cases.dense(N, k, 3, kind), cases.dense(m, k, 5, "uniform" if kind == "nonfinite" else kind)
        with np.errstate(invalid="ignore"):
            ref = {mean: oracle.sddmm(rowptr, col, y, g, mean=mean) for mean in (False, True)}
            mag = {mean: oracle.sddmm(rowptr, col, np.abs(y), np.abs(g), mean=mean).astype(np.float64) for mean in (False, True)}
        for a in (y, g, *ref.values(), *mag.values()):
            a.setflags(write=False)
        _REFS[key] = (y, g, ref, mag)
    return _REFS[key]


def _misaligned(t):
    """The same values at a base 4 bytes off a 16-byte boundary: the row kernel's scalar form at k % 4 == 0."""
    flat = torch.empty(t.numel() + 5, dtype=t.dtype, device=t.device)
    off = 1 + (-(flat.data_ptr() // 4) % 4)                                # flat[off] sits at 4 bytes past a 16-byte boundary
    v = flat[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _pitched(t, pitch, first=0):
    """The same values as columns [first, first + k) of a [rows, pitch] tensor filled with NaN around them."""
    wide = torch.full((t.size(0), pitch), float("nan"), dtype=t.dtype, device=t.device)
    wide[:, first:first + t.size(1)] = t
    v = wide[:, first:first + t.size(1)]
    assert v.stride(0) == pitch and v.stride(1) == 1
    return v


def _row(gpu, graph, d_y, d_g, mean, written=True):
    from isplib_amd import cabi
    return _twice(lambda o: cabi.sddmm(graph[2], graph[3], d_y, d_g, mean, out=o), graph[1].size, gpu, written)


def _tasks(gpu, graph, plan, d_y, d_g, mean, written=True, col32=True):
    from isplib_amd import cabi
    return _twice(lambda o: cabi.sddmm_tasks(graph[2], graph[3], plan, d_y, d_g, mean, out=o, col32=col32), graph[1].size, gpu, written)


def _handle(gpu, graph, slices):
    from isplib_amd import cabi
    h = cabi.GraphHandle(graph[2], graph[3], None, N)
    h.set_slices(slices)
    return h


def _integer_checks(run, oracle, graphs, name, k, what):
    """`run(d_y, d_g, mean)` on the integer operands: the sum is the oracle's bit for bit, the mean two roundings off."""
    y, g, ref, mag = _case(oracle, graphs, name, k, "integer")
    rowptr = graphs[name][0]
    return y, g, (lambda d_y, d_g: (_assert_exact(run(d_y, d_g, False), ref[False], rowptr, f"{what}, sum"),
                                    _assert_within(run(d_y, d_g, True), ref[True], 1e-6 * mag[True] + 1e-30, rowptr, f"{what}, mean")))


# ---- 1. the row kernel at every width ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,vec4", cs.ROW_WIDTHS, ids=[f"{k}-{'vec4' if v else 'scalar'}" for k, v in cs.ROW_WIDTHS])
def test_row_kernel_every_width(gpu, oracle_mod, graphs, k, vec4):
    """Each of the seven instantiations at its first and last width on the hub graph (its hub of 5,000 edges exceeds long_row: all
    four waves of its workgroup take a chunk).  A width that is a multiple of 4 reaches the scalar form by a misaligned base."""
    graph = graphs["hub"]
    y, g, check = _integer_checks(lambda d_y, d_g, mean: _row(gpu, graph, d_y, d_g, mean), oracle_mod, graphs, "hub", k, f"row kernel, k {k}")
    d_y, d_g = _on(gpu, y, g)
    if not vec4 and k % 4 == 0:
        d_y = _misaligned(d_y)
    assert (k % 4 == 0 and d_y.data_ptr() % 16 == 0 and d_g.data_ptr() % 16 == 0) == vec4
    check(d_y, d_g)


@pytest.mark.parametrize("k", (16, 32, 64))
def test_row_kernel_scalar_form_at_a_multiple_of_four(gpu, oracle_mod, graphs, k):
    """ldy % 4 != 0, ldg % 4 != 0 and a base 4 bytes off a 16-byte boundary each send k % 4 == 0 to the scalar form; the operands
    are column views of wider NaN-filled tensors, and the oracle sees the viewed columns."""
    graph = graphs["hub"]
    y, g, check = _integer_checks(lambda d_y, d_g, mean: _row(gpu, graph, d_y, d_g, mean), oracle_mod, graphs, "hub", k, f"row kernel, k {k}")
    d_y, d_g = _on(gpu, y, g)
    check(_pitched(d_y, k + 1), d_g)                                       # y's pitch is no multiple of 4
    check(d_y, _pitched(d_g, k + 3))                                       # g's
    check(d_y, _misaligned(d_g))                                           # g's base
    check(_misaligned(d_y), d_g)                                           # y's base
    check(_pitched(d_y, k + 8, 4), _pitched(d_g, k + 12, 8))               # aligned views at pitches that are multiples of 4: the float4 form
    check(_pitched(d_y, k + 5, 2), _pitched(d_g, k + 7, 3))                # both views, odd pitches, bases off by 8 and 12 bytes


# ---- 2. the row kernel at every row length ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,vec4", cs.ROW_LENGTH_WIDTHS, ids=[f"{k}-{'vec4' if v else 'scalar'}" for k, v in cs.ROW_LENGTH_WIDTHS])
def test_row_kernel_every_row_length(gpu, oracle_mod, graphs, k, vec4):
    """Row lengths on every loop edge (G = 64 / LPR edges per gather, 4 G per step, 64 per store batch, long_row and its chunks),
    each in two wave positions of a workgroup."""
    graph = graphs["lengths"]
    y, g, check = _integer_checks(lambda d_y, d_g, mean: _row(gpu, graph, d_y, d_g, mean), oracle_mod, graphs, "lengths", k, f"row lengths, k {k}")
    d_y, d_g = _on(gpu, y, g)
    check(_misaligned(d_y) if (not vec4 and k % 4 == 0) else d_y, d_g)


# ---- 3. the task kernel at every width --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", cs.TASK_WIDTHS)
def test_task_kernel_every_width(gpu, oracle_mod, graphs, plans, k):
    """All six instantiations whole and ragged on slice pieces of at most 64 edges; with the plan's packed 32-bit column ids and
    with the int64 ones (indx32 = NULL), to equal bits."""
    graph, plan = graphs["hub"], plans["hub"]
    assert plan.col32 is not None and plan.col32.numel() == graph[1].size
    y, g, check = _integer_checks(lambda d_y, d_g, mean: _tasks(gpu, graph, plan, d_y, d_g, mean), oracle_mod, graphs, "hub", k, f"task kernel, k {k}")
    d_y, d_g = _on(gpu, y, g)
    check(d_y, d_g)
    for mean in (False, True):
        a, b = _tasks(gpu, graph, plan, d_y, d_g, mean), _tasks(gpu, graph, plan, d_y, d_g, mean, col32=False)
        bad = np.flatnonzero(_bits(a) != _bits(b))
        assert bad.size == 0, f"k {k}, mean {mean}: 64-bit column ids change edges of rows of {_lengths_of(graph[0], bad)} edges"
    if k in (64, 130):                                                     # pitched views of both operands: ldy and ldg are passed on
        check(_pitched(d_y, k + 24, 8), _pitched(d_g, k + 7, 3))


# ---- 4. the task kernel at every task length --------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", cs.TASK_LENGTH_WIDTHS)
def test_task_kernel_every_task_length(gpu, oracle_mod, graphs, plans, k):
    """One slice, chunk 4096, no short rows: a row of at most 4096 edges is one task, so the task lengths are the row lengths."""
    graph, plan = graphs["lengths"], plans["lengths"]
    y, g, check = _integer_checks(lambda d_y, d_g, mean: _tasks(gpu, graph, plan, d_y, d_g, mean), oracle_mod, graphs, "lengths", k, f"task lengths, k {k}")
    check(*_on(gpu, y, g))


# ---- 5. real-valued operands, per edge --------------------------------------------------------------------------------------------

def _three_forms(gpu, graphs, plans, name="hub", slices=(0, 1, 3)):
    """[(what, run(d_y, d_g, mean, written))] for the row kernel, the task kernel and the handle at each slice count."""
    graph = graphs[name]
    forms = [("row kernel", lambda d_y, d_g, mean, written=True: _row(gpu, graph, d_y, d_g, mean, written)),
             ("task kernel", lambda d_y, d_g, mean, written=True: _tasks(gpu, graph, plans[name], d_y, d_g, mean, written))]
    for s in slices:
        h = _handle(gpu, graph, s)
        forms.append((f"handle, {s} slices", lambda d_y, d_g, mean, written=True, h=h: _twice(lambda o: h.sddmm(d_y, d_g, mean, out=o), graph[1].size, gpu, written)))
    return forms


@pytest.mark.parametrize("k", cs.REAL_WIDTHS)
def test_real_valued_operands_within_the_bound_per_edge(gpu, oracle_mod, graphs, plans, k):
    y, g, ref, mag = _case(oracle_mod, graphs, "hub", k, "uniform")
    d_y, d_g = _on(gpu, y, g)
    for what, run in _three_forms(gpu, graphs, plans):
        for mean in (False, True):
            _assert_within(run(d_y, d_g, mean), ref[mean], 1e-5 * mag[mean] + TINY, graphs["hub"][0], f"{what}, k {k}, mean {mean}")


# ---- 6. the ragged-K trap ---------------------------------------------------------------------------------------------------------

def _assert_trap(got, y, ref, mag, rowptr, col, k, what):
    """Exactly +-Inf on the edges that touch a trapped row of y, every other edge within the bound, no NaN."""
    hot = np.isinf(y).any(1)[col]
    sign = np.sign(y[:, cs.duplicated_columns(k)[0]])[col]
    assert hot.any() and not hot.all()
    nan = np.flatnonzero(np.isnan(got))
    assert nan.size == 0, f"{what}: {nan.size} edges are NaN ({np.count_nonzero(hot)} touch a trapped row), in rows of {_lengths_of(rowptr, nan)[:12]} edges"
    bad = np.flatnonzero(np.isinf(got) != hot)
    assert bad.size == 0, f"{what}: Inf on the wrong edges, rows of {_lengths_of(rowptr, bad)} edges"
    assert np.array_equal(np.sign(got[hot]), sign[hot]), f"{what}: the sign of the Inf"
    _assert_within(np.where(hot, 0, got), np.where(hot, 0, ref), 1e-5 * mag + TINY, rowptr, what, where=~hot)


@pytest.mark.parametrize("k", cs.TRAP_WIDTHS)
def test_ragged_k_does_not_turn_inf_into_nan(gpu, oracle_mod, graphs, plans, monkeypatch, k):
    """y holds +-Inf in exactly the columns the task form's shifted last vector gathers a second time, g is at least 0.5 there: IEEE
    arithmetic on the k columns gives Inf of the row's sign.  Through the task kernel on both plans, the handle at 3 slices, the
    operator's backward on the forward's task plan (ISPLIB_SLICES=8), and the row kernel, which has no shifted vector."""
    import isplib_amd
    for name in ("hub", "lengths"):
        rowptr, col = graphs[name][:2]
        y, g, ref, mag = _case(oracle_mod, graphs, name, k, "trap")
        d_y, d_g = _on(gpu, y, g)
        forms = _three_forms(gpu, graphs, plans, name, slices=(3,)) if name == "hub" else _three_forms(gpu, graphs, plans, name, slices=())[1:]
        for what, run in forms:
            for mean in (False, True):
                _assert_trap(run(d_y, d_g, mean, False), y, ref[mean], mag[mean], rowptr, col, k, f"{what} on the {name} graph, k {k}, mean {mean}")
    # (d_y, d_g and the references are the length graph's from here on: swap back to the hub graph for the operator)
    rowptr, col, d_rowptr, d_col = graphs["hub"]
    y, g, ref, mag = _case(oracle_mod, graphs, "hub", k, "trap")
    d_y, d_g = _on(gpu, y, g)
    monkeypatch.setenv("ISPLIB_SLICES", "8")
    for red, mean in (("sum", False), ("mean", True)):
        value = torch.from_numpy(cases.weights(col.size, 4)).to(gpu).requires_grad_(True)
        adj = isplib_amd.SparseTensor.from_csr(d_rowptr, d_col, value, (rowptr.size - 1, N))
        isplib_amd.matmul(adj, d_y.clone().requires_grad_(True), red).backward(d_g)
        _assert_trap(value.grad.cpu().numpy(), y, ref[mean], mag[mean], rowptr, col, k, f"matmul('{red}').backward, k {k}")


def test_ragged_last_column_panel_does_not_turn_inf_into_nan(gpu, oracle_mod, graphs, plans):
    """The experimental column panels (64 columns): k = 129 runs as a panel of 64 and one of 65, whose shifted vector duplicates
    columns 125..127 -- where the trap's Inf sits.  Pitches that are multiples of 32 keep the call on panels."""
    from isplib_amd import cabi
    k = cs.PANEL_TRAP_WIDTH
    rowptr, col = graphs["hub"][:2]
    y, g, ref, mag = _case(oracle_mod, graphs, "hub", k, "trap")
    d_y, d_g = (_pitched(t, cs.PANEL_PITCH) for t in _on(gpu, y, g))
    try:
        assert cabi.exp_lib().isplib_hip_tune_experimental(12, cs.PANEL_COLS) == 0
        for mean in (False, True):
            got = _tasks(gpu, graphs["hub"], plans["hub"], d_y, d_g, mean, written=False)
            _assert_trap(got, y, ref[mean], mag[mean], rowptr, col, k, f"task kernel in 64-column panels, k {k}, mean {mean}")
    finally:
        cabi.exp_lib().isplib_hip_tune_experimental(12, 0)


# ---- 7. non-finite and subnormal operands -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (41, 64))
def test_nonfinite_operands(gpu, oracle_mod, graphs, plans, k):
    """NaN and +-Inf scattered over y: NaN exactly where the oracle has NaN, Inf of the oracle's sign where it has Inf, the rest within
    the bound -- a non-finite value in column c reaches an edge through the product of column c only."""
    rowptr = graphs["hub"][0]
    y, g, ref, mag = _case(oracle_mod, graphs, "hub", k, "nonfinite")
    d_y, d_g = _on(gpu, y, g)
    for what, run in _three_forms(gpu, graphs, plans, slices=(3,)):
        for mean in (False, True):
            r = ref[mean]
            assert np.any(np.isnan(r)) and np.any(np.isinf(r)) and np.any(np.isfinite(r))
            got = run(d_y, d_g, mean, False)
            bad = np.flatnonzero(np.isnan(got) != np.isnan(r))
            assert bad.size == 0, f"{what}, k {k}, mean {mean}: NaN positions differ in rows of {_lengths_of(rowptr, bad)} edges"
            inf = np.isinf(r)
            assert np.array_equal(np.isinf(got), inf) and np.array_equal(np.sign(got[inf]), np.sign(r[inf])), f"{what}, k {k}, mean {mean}: Inf positions and signs"
            fin = np.isfinite(r)
            _assert_within(np.where(fin, got, 0), np.where(fin, r, 0), 1e-5 * np.where(fin, mag[mean], 0) + TINY, rowptr, f"{what}, k {k}, mean {mean}", where=fin)


@pytest.mark.parametrize("k", (41, 64))
def test_subnormal_operands_are_not_flushed(gpu, oracle_mod, graphs, plans, k):
    """y of magnitude ~3e-38: products at the bottom of the normal range, partial sums below it.  Within the bound; a kernel that
    flushes subnormals misses it by four orders of magnitude (the host test shows that on the emulation)."""
    rowptr = graphs["hub"][0]
    y, g, ref, mag = _case(oracle_mod, graphs, "hub", k, "subnormal")
    d_y, d_g = _on(gpu, y, g)
    for what, run in _three_forms(gpu, graphs, plans, slices=(3,)):
        for mean in (False, True):
            got = run(d_y, d_g, mean)
            assert np.count_nonzero(got) > 0.99 * got.size, f"{what}: subnormal results were flushed"
            _assert_within(got, ref[mean], 1e-5 * mag[mean] + TINY, rowptr, f"{what}, subnormal, k {k}, mean {mean}")


# ---- 8. empty things --------------------------------------------------------------------------------------------------------------

def test_empty_graphs_and_plans_write_nothing(gpu, oracle_mod):
    from isplib_amd import cabi
    from isplib_amd.plan import TaskPlan, build_task_plan
    k = 41
    # m rows, all empty, and a task plan of zero tasks
    m = 9
    rowptr = torch.zeros(m + 1, dtype=torch.int64, device=gpu)
    col = torch.zeros(0, dtype=torch.int64, device=gpu)
    y, g = _on(gpu, cases.dense(N, k, 3), cases.dense(m, k, 5))
    i32 = dict(dtype=torch.int32, device=gpu)
    none = TaskPlan(1, 0, torch.zeros(0, **i32), torch.zeros(0, dtype=torch.int64, device=gpu), torch.zeros(0, **i32),
                    torch.zeros(m + 1, **i32), [0] * 9, 64, 0, None, N)
    for mean in (False, True):
        assert _twice(lambda o: cabi.sddmm(rowptr, col, y, g, mean, out=o), 0, gpu).size == 0
        assert _twice(lambda o: cabi.sddmm_tasks(rowptr, col, none, y, g, mean, out=o), 0, gpu).size == 0
    assert cabi.sddmm(rowptr, col, y, g).numel() == 0 and cabi.sddmm_tasks(rowptr, col, none, y, g).numel() == 0
    # zero tasks over a graph that has edges: the entry has nothing to do, succeeds, and writes nothing at all
    rp_np, col_np = cases.random_csr(m, N, 4.0, 3)
    d_rp, d_col = _on(gpu, rp_np, col_np)
    out = torch.full((col_np.size + PAD,), float("nan"), dtype=torch.float32, device=gpu)
    assert cabi.sddmm_tasks(d_rp, d_col, none, y, g, out=out) is out
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # one row, one edge: all three forms
    rp1, col1 = np.array([0, 1], np.int64), np.array([N - 1], np.int64)
    d_rp1, d_col1 = _on(gpu, rp1, col1)
    g1 = g[4:5]
    ref = oracle_mod.sddmm(rp1, col1, y.cpu().numpy(), g1.cpu().numpy())
    bound = 1e-5 * oracle_mod.sddmm(rp1, col1, np.abs(y.cpu().numpy()), np.abs(g1.cpu().numpy())).astype(np.float64) + TINY
    plan1 = build_task_plan(d_rp1, d_col1, N, 1, 64, 0)
    assert plan1 is not None and plan1.n_tasks == 1
    h = cabi.GraphHandle(d_rp1, d_col1, None, N)
    for slices in (0, 1):
        h.set_slices(slices)
        for mean in (False, True):                                          # a degree of 1: the mean is the sum
            for what, call in (("row kernel", lambda o: cabi.sddmm(d_rp1, d_col1, y, g1, mean, out=o)),
                               ("task kernel", lambda o: cabi.sddmm_tasks(d_rp1, d_col1, plan1, y, g1, mean, out=o)),
                               (f"handle, {slices} slices", lambda o: h.sddmm(y, g1, mean, out=o))):
                _assert_within(_twice(call, 1, gpu), ref, bound, rp1, f"one edge, {what}, mean {mean}")
