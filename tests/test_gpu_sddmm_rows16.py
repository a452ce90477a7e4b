"""The 16-bit SDDMM row kernel (isplib_sddmm_csr_rows16_hip): dval[j] = <y[col[j], :], g[i, :]> (/ max(deg_i, 1)) for bf16 / fp16
y and g, dval fp32 -- through the C ABI, the torch operators and the plug-in (ISPLIB_HALF_DA).

The reference is oracle.sddmm on the widened operands (widening is exact).  Small-integer operands: the sum is exact in fp32 in any
order, so it equals the oracle bit for bit, and the mean lies within 1e-6 * mag (two fp32 roundings against the oracle's double);
real-valued data within 1e-5 * mag, mag = oracle.sddmm(|y|, |g|).  Every dval is allocated with 64 extra elements and prefilled with
NaN, so an unwritten edge and a write past the end both show, and every launch runs twice to equal bits."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests import sddmm_rows16_cases as cs

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", tuple(half_ref.DTYPES.values()), ids=tuple(half_ref.DTYPES))
N = cs.N
PAD = 64


def _on(gpu, *arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in arrays)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _twice(call, nnz, gpu, written=True):
    """call(out) launched into two NaN-filled buffers of nnz + 64 entries: equal bits, the tail untouched, every edge written
    (`written`: no NaN may remain; off where the data holds NaN of its own).  Returns the nnz results as a numpy array."""
    outs = [torch.full((nnz + PAD,), float("nan"), dtype=torch.float32, device=gpu) for _ in range(2)]
    for o in outs:
        call(o)
    torch.cuda.synchronize()
    a, b = (o.cpu().numpy() for o in outs)
    assert np.array_equal(_bits(a), _bits(b)), "two launches: equal bits"
    assert np.all(np.isnan(a[nnz:])), "the 64 entries behind dval must not be touched"
    if written:
        left = np.flatnonzero(np.isnan(a[:nnz]))
        assert left.size == 0, f"edges {left[:8].tolist()} ... were not written"
    return a[:nnz]


def _sddmm(gpu, d_rowptr, d_col, d_y, d_g, mean, order=None, written=True):
    from isplib_amd import cabi
    return _twice(lambda o: cabi.sddmm_rows16(d_rowptr, d_col, d_y, d_g, mean, order=order, out=o), d_col.numel(), gpu, written)


def _lengths_of(rowptr, bad):
    deg = np.diff(rowptr)
    erow = np.repeat(np.arange(deg.size), deg)
    return sorted(set(deg[erow[bad]].tolist()))


def _assert_exact(got, ref, rowptr, what):
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, f"{what}: edges of rows of {_lengths_of(rowptr, bad)} edges differ (positions {bad[:8].tolist()} ...)"


def _assert_within(got, ref, bound, rowptr, what):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bad = np.flatnonzero(~(err <= bound))
    print(f"{what}: max err / bound = {np.max(err / bound) if err.size else 0.0:.3g}")
    assert bad.size == 0, f"{what}: edges of rows of {_lengths_of(rowptr, bad)} edges miss the bound (positions {bad[:8].tolist()} ...)"


def _integer_case(gpu, oracle, rowptr, col, k, dtype, what):
    """|y|, |g| <= 3: |dot| <= 9 * 1024 < 2^24, so the sum equals the oracle's bit for bit and the mean is two roundings off."""
    m = rowptr.size - 1
    y16, g16 = half_ref.to16(cases.dense(N, k, 3, "integer"), dtype), half_ref.to16(cases.dense(m, k, 5, "integer"), dtype)
    y32, g32 = half_ref.widen(y16), half_ref.widen(g16)
    d_rowptr, d_col = _on(gpu, rowptr, col)
    d_y, d_g = y16.to(gpu), g16.to(gpu)
    _assert_exact(_sddmm(gpu, d_rowptr, d_col, d_y, d_g, False), oracle.sddmm(rowptr, col, y32, g32), rowptr, f"{what}, sum")
    mag = oracle.sddmm(rowptr, col, np.abs(y32), np.abs(g32), mean=True)
    _assert_within(_sddmm(gpu, d_rowptr, d_col, d_y, d_g, True), oracle.sddmm(rowptr, col, y32, g32, mean=True), 1e-6 * mag + 1e-30, rowptr,
                   f"{what}, mean")


# ---- 1. every slot width and its ragged edge -------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", cs.WIDTHS)
def test_every_slot_width_and_its_ragged_edge(gpu, oracle_mod, k, dtype):
    """One whole slot of every width and two columns more (1022: the ragged end of the two-chunk form, 1024 its whole width).  The
    hub row (2,500 edges) exceeds long_row: all four waves of its workgroup take a chunk of it."""
    rowptr, col = cs.hub_graph()
    assert np.max(np.diff(rowptr)) > cs.LONG_ROW
    _integer_case(gpu, oracle_mod, rowptr, col, k, dtype, f"hub, k {k}")


# ---- 2. row lengths around every loop edge ---------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", cs.LENGTH_WIDTHS)
def test_row_lengths_around_every_loop_edge(gpu, oracle_mod, k, dtype):
    rowptr, col = cs.length_graph()
    _integer_case(gpu, oracle_mod, rowptr, col, k, dtype, f"lengths, k {k}")


# ---- 3. row order ----------------------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (64, 130))
def test_any_row_order_gives_the_bits_of_index_order(gpu, k, dtype):
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    d_rowptr, d_col = _on(gpu, rowptr, col)
    d_y = half_ref.to16(cases.dense(N, k, 3, "uniform"), dtype).to(gpu)
    d_g = half_ref.to16(cases.dense(m, k, 5, "uniform"), dtype).to(gpu)
    orders = (np.random.default_rng(5).permutation(m), np.arange(m)[::-1].copy())
    for mean in (False, True):
        base = _sddmm(gpu, d_rowptr, d_col, d_y, d_g, mean)
        for o in orders:
            d_o = torch.from_numpy(o.astype(np.int32)).to(gpu)
            got = _sddmm(gpu, d_rowptr, d_col, d_y, d_g, mean, d_o)
            bad = np.flatnonzero(_bits(got) != _bits(base))
            assert bad.size == 0, f"mean {mean}: edges of rows of {_lengths_of(rowptr, bad)} edges differ under a row order"


# ---- 4. pitches ------------------------------------------------------------------------------------------------------------------

@DT
def test_column_views_of_both_operands(gpu, oracle_mod, dtype):
    """y as a [n, 64] column view of a [n, 192] tensor through the wrapper, and g as a column view (ldg = 130) through the raw
    boundary call: each is read at its own pitch."""
    from isplib_amd import cabi
    rowptr, col = cs.hub_graph()
    m, k = rowptr.size - 1, 64
    d_rowptr, d_col = _on(gpu, rowptr, col)
    y_big = half_ref.to16(cases.dense(N, 192, 7, "integer"), dtype)
    g_big = half_ref.to16(cases.dense(m, 130, 9, "integer"), dtype)
    d_y, d_g = y_big.to(gpu)[:, 64:128], g_big.to(gpu)[:, 2:2 + k]
    assert d_y.stride(0) == 192 and d_g.stride(0) == 130
    ref = oracle_mod.sddmm(rowptr, col, half_ref.widen(y_big)[:, 64:128], half_ref.widen(g_big)[:, 2:2 + k])
    _assert_exact(_sddmm(gpu, d_rowptr, d_col, d_y, d_g.contiguous(), False), ref, rowptr, "y at pitch 192")
    got = _twice(lambda o: cabi.isplib_sddmm_csr_rows16_hip(d_rowptr, d_col, None, d_y, d_g, o), col.size, gpu)
    _assert_exact(got, ref, rowptr, "y at pitch 192, g at pitch 130")
    _assert_exact(_sddmm(gpu, d_rowptr, d_col, d_y, d_g, False), ref, rowptr, "both views through the wrapper")


# ---- 5. real-valued data ---------------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (66, 256, 1024))
def test_real_valued_data_within_the_bound(gpu, oracle_mod, k, dtype):
    """1e-5 * mag: the project's SDDMM bound; a lane sums at most 16 products and the slot reduction adds 6 levels -- at most 23
    roundings of 2^-24, about 1.4e-6 of mag."""
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    y16, g16 = half_ref.to16(cases.dense(N, k, 3, "uniform"), dtype), half_ref.to16(cases.dense(m, k, 5, "uniform"), dtype)
    y32, g32 = half_ref.widen(y16), half_ref.widen(g16)
    d_rowptr, d_col = _on(gpu, rowptr, col)
    for mean in (False, True):
        got = _sddmm(gpu, d_rowptr, d_col, y16.to(gpu), g16.to(gpu), mean)
        bound = 1e-5 * oracle_mod.sddmm(rowptr, col, np.abs(y32), np.abs(g32), mean=mean) + 1e-30
        _assert_within(got, oracle_mod.sddmm(rowptr, col, y32, g32, mean=mean), bound, rowptr, f"k {k}, mean {mean}")


# ---- 6. non-finite and small values ----------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (64, 66))
def test_nonfinite_operands(gpu, oracle_mod, k, dtype):
    """NaN and Inf in y and in g: NaN where the oracle has NaN, Inf of the oracle's sign where it has Inf, the rest within the bound."""
    rowptr, col = cases.random_csr(64, N, 6.0, 41, empty_rows=(5,), hub=(9, 300))
    m = rowptr.size - 1
    y16, g16 = half_ref.to16(cases.dense(N, k, 3, "nonfinite"), dtype), half_ref.to16(cases.dense(m, k, 5, "nonfinite"), dtype)
    y32, g32 = half_ref.widen(y16), half_ref.widen(g16)
    d_rowptr, d_col = _on(gpu, rowptr, col)
    for mean in (False, True):
        with np.errstate(invalid="ignore"):
            ref = oracle_mod.sddmm(rowptr, col, y32, g32, mean=mean)
            mag = oracle_mod.sddmm(rowptr, col, np.abs(y32), np.abs(g32), mean=mean)
        assert np.any(np.isnan(ref)) and np.any(np.isinf(ref)) and np.any(np.isfinite(ref))
        got = _sddmm(gpu, d_rowptr, d_col, y16.to(gpu), g16.to(gpu), mean, written=False)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"k {k}, mean {mean}: NaN positions"
        inf = np.isinf(ref)
        assert np.array_equal(np.isinf(got), inf) and np.array_equal(np.sign(got[inf]), np.sign(ref[inf])), f"k {k}, mean {mean}: Inf positions and signs"
        fin = np.isfinite(ref)
        assert np.all(np.abs(got[fin].astype(np.float64) - ref[fin]) <= 1e-5 * mag[fin] + 1e-30), f"k {k}, mean {mean}: finite entries"


@DT
def test_ragged_k_does_not_turn_inf_into_nan(gpu, oracle_mod, dtype):
    """k = 66: y holds Inf in columns 58..63 -- the components the shifted last vector gathers a second time -- and g is positive
    there.  Every edge touching such a row is Inf of the row's sign, not NaN (Inf * 0) and not finite."""
    k = 66
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    y, g = cs.ragged_trap(m, k)
    y16, g16 = half_ref.to16(y, dtype), half_ref.to16(g, dtype)
    y32, g32 = half_ref.widen(y16), half_ref.widen(g16)
    d_rowptr, d_col = _on(gpu, rowptr, col)
    hot = np.isinf(y32).any(1)[col]
    want_sign = np.sign(y32[:, 58])[col]
    assert hot.any() and not hot.all()
    for mean in (False, True):
        ref = oracle_mod.sddmm(rowptr, col, y32, g32, mean=mean)
        assert np.array_equal(np.isinf(ref), hot) and not np.any(np.isnan(ref))
        got = _sddmm(gpu, d_rowptr, d_col, y16.to(gpu), g16.to(gpu), mean)
        assert not np.any(np.isnan(got)), f"mean {mean}: {np.count_nonzero(np.isnan(got))} edges are NaN"
        assert np.array_equal(np.isinf(got), hot) and np.array_equal(np.sign(got[hot]), want_sign[hot]), f"mean {mean}"
        mag = oracle_mod.sddmm(rowptr, col, np.abs(y32), np.abs(g32), mean=mean)
        _assert_within(got[~hot], ref[~hot], 1e-5 * mag[~hot] + 1e-30, rowptr, f"finite edges, mean {mean}")


@pytest.mark.parametrize("k", (66, 256))
def test_bf16_products_in_the_fp32_subnormal_range(gpu, oracle_mod, k):
    """Operands of magnitude ~1e-20: every product is an fp32 subnormal, and each of the at most k + 6 roundings may lose half a
    unit of 2^-149 -- the absolute term is k * 2^-149.  Nothing is flushed: the results are not all zero."""
    rowptr, col = cs.hub_graph()
    m = rowptr.size - 1
    y, g = cs.subnormal_operands(m, k)
    y16, g16 = half_ref.to16(y, torch.bfloat16), half_ref.to16(g, torch.bfloat16)
    y32, g32 = half_ref.widen(y16), half_ref.widen(g16)
    d_rowptr, d_col = _on(gpu, rowptr, col)
    ref = oracle_mod.sddmm(rowptr, col, y32, g32)
    assert np.any((ref != 0) & (np.abs(ref) < np.float32(2.0 ** -126)))
    got = _sddmm(gpu, d_rowptr, d_col, y16.to(gpu), g16.to(gpu), False)
    assert np.count_nonzero(got) > got.size // 2, "subnormal products were flushed"
    bound = 1e-5 * oracle_mod.sddmm(rowptr, col, np.abs(y32), np.abs(g32)).astype(np.float64) + k * 2.0 ** -149
    _assert_within(got, ref, bound, rowptr, f"subnormal, k {k}")


# ---- 7. refusals before any launch -----------------------------------------------------------------------------------------------

@DT
def test_entry_refuses_before_any_launch(gpu, dtype):
    """Each refused call returns ISPLIB_FAIL, leaves the NaN-filled dval as it was, and isplib_hip_last_error names the entry."""
    from isplib_amd import cabi
    rowptr, col = cases.random_csr(150, 120, 9.0, 21, empty_rows=(4,), hub=(9, 700), duplicates=True)
    m, n, k = 150, 120, 64
    d_rowptr, d_col = _on(gpu, rowptr, col)
    y = torch.ones((n, k), dtype=dtype, device=gpu)
    g = torch.ones((m, k), dtype=dtype, device=gpu)
    wide_y = torch.ones((n, 1032), dtype=dtype, device=gpu)
    wide_g = torch.ones((m, 1032), dtype=dtype, device=gpu)
    flat_y = torch.ones(n * k + 2, dtype=dtype, device=gpu)
    flat_g = torch.ones(m * k + 2, dtype=dtype, device=gpu)
    dv = "dval"
    calls = (
        ("isplib_sddmm_rows16_serves", y, g, dv, {"k": 63}),                                     # odd k
        ("isplib_sddmm_rows16_serves", y, g, dv, {"k": 6}),                                      # k < 8
        ("isplib_sddmm_rows16_serves", wide_y, wide_g, dv, {"k": 1026}),                         # k > 1024
        ("leading dimension", y, g, dv, {"ldy": 62}),
        ("leading dimension", y, g, dv, {"ldg": 62}),
        ("isplib_sddmm_rows16_serves", wide_y, g, dv, {"k": 64, "ldy": 1031}),                   # odd ldy
        ("isplib_sddmm_rows16_serves", y, wide_g, dv, {"k": 64, "ldg": 1031}),                   # odd ldg
        ("dtype", y, g, dv, {"dtype": 0}),                                                       # what an fp32 tensor maps to
        ("null operand", None, g, dv, {}),
        ("null operand", y, None, dv, {}),
        ("null operand", y, g, None, {}),
        ("4-byte aligned", flat_y[1:1 + n * k].view(n, k), g, dv, {}),                           # a base at 2 bytes mod 4
        ("4-byte aligned", y, flat_g[1:1 + m * k].view(m, k), dv, {}),
    )
    for cause, yy, gg, dd, extra in calls:
        dval = torch.full((col.size + PAD,), float("nan"), dtype=torch.float32, device=gpu)
        st = cabi.isplib_sddmm_csr_rows16_hip(d_rowptr, d_col, None, yy, gg, dval if dd is not None else None, check=False, **extra)
        torch.cuda.synchronize()
        assert st == cabi.FAIL and cause in cabi.last_error(), (cause, extra, st, cabi.last_error())
        assert "isplib_sddmm_csr_rows16_hip" in cabi.last_error()
        assert bool(torch.isnan(dval).all()), (cause, extra)
    # nothing to do is a success
    empty_rp = torch.zeros(1, dtype=torch.int64, device=gpu)
    assert cabi.isplib_sddmm_csr_rows16_hip(empty_rp, d_col[:0], None, y, g[:0], torch.empty(0, dtype=torch.float32, device=gpu), check=False) == cabi.SUCCESS
    # the wrapper raises before the call
    with pytest.raises(ValueError):
        cabi.sddmm_rows16(d_rowptr, d_col, y, g[:-1])                      # one row of g per row of the graph
    with pytest.raises(ValueError):
        cabi.sddmm_rows16(d_rowptr, d_col, y, g[:, :62])
    with pytest.raises(ValueError):
        cabi.sddmm_rows16(d_rowptr, d_col, y[:100], g)                     # column ids beyond n
    with pytest.raises(ValueError):
        cabi.sddmm_rows16(d_rowptr, d_col, y[:, :6], g[:, :6])
    with pytest.raises(ValueError):
        cabi.sddmm_rows16(d_rowptr, d_col, wide_y[:, :1026], wide_g[:, :1026])
    with pytest.raises(TypeError):
        cabi.sddmm_rows16(d_rowptr, d_col, y.to(torch.float32), g)
    with pytest.raises(TypeError):
        cabi.sddmm_rows16(d_rowptr, d_col, y, g.to(torch.float32))


# ---- 8. operator and autograd, through matmul ------------------------------------------------------------------------------------

M_OP, K_OP = 2000, 64
FP32_COPY = M_OP * K_OP * 4


def _peak_during(fn):
    from tests.test_gpu_rows16_colscale import _peak_during as peak
    return peak(fn)


@pytest.fixture(scope="module")
def op_graph():
    return cases.random_csr(M_OP, M_OP, 8.0, 51, empty_rows=(0, 1999), hub=(11, 1500), duplicates=True)


@pytest.fixture(scope="module")
def op_refs(oracle_mod, op_graph):
    """Per dtype: (x16, g16, the oracle's dA for sum, for mean, the mean's magnitude) -- computed once."""
    rowptr, col = op_graph
    out = {}
    for dtype in half_ref.DTYPES.values():
        x16, g16 = half_ref.to16(cases.dense(M_OP, K_OP, 3, "integer"), dtype), half_ref.to16(cases.dense(M_OP, K_OP, 5, "integer"), dtype)
        x32, g32 = half_ref.widen(x16), half_ref.widen(g16)
        out[dtype] = (x16, g16, oracle_mod.sddmm(rowptr, col, x32, g32), oracle_mod.sddmm(rowptr, col, x32, g32, mean=True),
                      oracle_mod.sddmm(rowptr, col, np.abs(x32), np.abs(g32), mean=True))
    return out


def _weights(nnz):
    return torch.from_numpy(cases.weights(nnz, 13, "signed_int"))


def _setenv(monkeypatch, da, half="native"):
    monkeypatch.setenv("ISPLIB_STREAM", "0")
    monkeypatch.setenv("ISPLIB_HALF", half)
    if da is None:
        monkeypatch.delenv("ISPLIB_HALF_DA", raising=False)
    else:
        monkeypatch.setenv("ISPLIB_HALF_DA", da)


def _grads(gpu, op_graph, x16, g16, red, x_grad=False, view=False):
    """(value.grad, x.grad or None, peak allocation of the backward, the forward's schedule) of matmul(adj, x, red).backward(g);
    `view`: x as an odd-pitch column view and g non-contiguous."""
    import isplib_amd
    rowptr, col = op_graph
    value = _weights(col.size).to(gpu).requires_grad_(True)
    adj = isplib_amd.SparseTensor.from_csr(torch.from_numpy(rowptr).to(gpu), torch.from_numpy(col).to(gpu), value, (M_OP, M_OP))
    x, g = x16.to(gpu), g16.to(gpu)
    if view:
        wide = torch.zeros((M_OP, K_OP + 3), dtype=x.dtype, device=gpu)
        wide[:, 1:1 + K_OP] = x
        x = wide[:, 1:1 + K_OP]                                            # pitch 67, base 2 bytes off a 4-byte boundary
        g = g.t().contiguous().t()                                         # column-major
        assert x.stride(0) == K_OP + 3 and not g.is_contiguous()
    x = x.detach().requires_grad_(x_grad)
    out = isplib_amd.matmul(adj, x, red)
    schedule = adj.storage._last_schedule
    peak, _ = _peak_during(lambda: out.backward(g))
    return value.grad.detach(), (x.grad.detach() if x_grad else None), peak, schedule


@DT
@pytest.mark.parametrize("red", ("sum", "mean"))
def test_native_value_gradient_through_matmul(gpu, op_graph, op_refs, monkeypatch, red, dtype):
    """ISPLIB_HALF_DA=native: value.grad is fp32, for sum the oracle's bits, for mean within 1e-6 * mag, and the backward allocates
    less than ONE fp32 copy of X (512,000 B; dval is about 70 KB) -- the conversion route makes two."""
    x16, g16, ref_sum, ref_mean, mag = op_refs[dtype]
    rowptr, _ = op_graph
    _setenv(monkeypatch, "native")
    grad, _, peak, schedule = _grads(gpu, op_graph, x16, g16, red)
    assert schedule == ("rows16",), schedule
    assert grad.dtype == torch.float32
    print(f"peak of the backward, {red}: {peak} B; an fp32 copy of X is {FP32_COPY} B")
    got = grad.cpu().numpy()
    if red == "sum":
        _assert_exact(got, ref_sum, rowptr, "value.grad, sum")
    else:
        _assert_within(got, ref_mean, 1e-6 * mag + 1e-30, rowptr, "value.grad, mean")
    assert peak < FP32_COPY, f"the backward allocated {peak} bytes: an fp32 copy of X is {FP32_COPY}"


@DT
@pytest.mark.parametrize("red", ("sum", "mean"))
def test_default_is_unchanged(gpu, op_graph, op_refs, monkeypatch, red, dtype):
    """The variable unset or `convert`: the fp32 copies are still made (the peak shows it) and the bits are convert's; the native
    route has those bits too on integer data (sum); ISPLIB_HALF=convert wins over ISPLIB_HALF_DA=native."""
    x16, g16, ref_sum, ref_mean, mag = op_refs[dtype]
    rowptr, _ = op_graph
    _setenv(monkeypatch, None)
    unset, _, peak, schedule = _grads(gpu, op_graph, x16, g16, red)
    assert schedule == ("rows16",) and unset.dtype == torch.float32
    print(f"peak of the backward, {red}: default {peak} B; an fp32 copy of X is {FP32_COPY} B")
    assert peak >= FP32_COPY, f"the default backward allocated {peak} bytes only: no fp32 copy of {FP32_COPY}?"
    _setenv(monkeypatch, "convert")
    conv, _, conv_peak, _ = _grads(gpu, op_graph, x16, g16, red)
    assert torch.equal(unset.view(torch.int32), conv.view(torch.int32)) and conv_peak >= FP32_COPY
    if red == "sum":
        _assert_exact(conv.cpu().numpy(), ref_sum, rowptr, "convert, sum")
    else:
        _assert_within(conv.cpu().numpy(), ref_mean, 1e-6 * mag + 1e-30, rowptr, "convert, mean")
    _setenv(monkeypatch, "native", half="convert")
    both, _, both_peak, schedule = _grads(gpu, op_graph, x16, g16, red)
    assert schedule[0] == "convert", schedule
    assert torch.equal(both.view(torch.int32), conv.view(torch.int32)) and both_peak >= FP32_COPY


@DT
def test_x_grad_views_and_the_direct_operator_call(gpu, op_graph, op_refs, monkeypatch, dtype):
    """With x requiring grad too, x.grad has the bits it has without the variable; x as an odd-pitch view and a non-contiguous dY
    give the same value.grad and raise nothing; torch.ops.isplib.fusedmm_spmm_planned carrying the marked plan gives it as well, and
    the unmarked plan today's."""
    import isplib_amd
    x16, g16, ref_sum, _, _ = op_refs[dtype]
    rowptr, col = op_graph
    _setenv(monkeypatch, None)
    _, dx_default, _, _ = _grads(gpu, op_graph, x16, g16, "sum", x_grad=True)
    _setenv(monkeypatch, "native")
    dv, dx, _, schedule = _grads(gpu, op_graph, x16, g16, "sum", x_grad=True)
    assert schedule == ("rows16",)
    _assert_exact(dv.cpu().numpy(), ref_sum, rowptr, "value.grad with x.grad")
    assert dx.dtype == dtype and np.array_equal(half_ref.bits(dx), half_ref.bits(dx_default)), "x.grad"
    dv_view, _, _, _ = _grads(gpu, op_graph, x16, g16, "sum", view=True)
    _assert_exact(dv_view.cpu().numpy(), ref_sum, rowptr, "value.grad, odd-pitch x and column-major dY")

    d_rowptr, d_col = _on(gpu, rowptr, col)
    row_plan = [torch.empty(0, dtype=torch.int32, device=gpu), torch.tensor([16], dtype=torch.int32)]
    marked = row_plan + [torch.tensor([0xDA], dtype=torch.int32)]

    def run(plan):
        value = _weights(col.size).to(gpu).requires_grad_(True)
        out = torch.ops.isplib.fusedmm_spmm_planned(d_rowptr, d_col, value, None, x16.to(gpu), None, None, plan, [])
        g = g16.to(gpu)
        peak, _ = _peak_during(lambda: out.backward(g))
        return out.detach(), value.grad.detach(), peak

    out3, dv3, peak3 = run(marked)
    out2, dv2, peak2 = run(row_plan)
    print(f"peak of the backward: marked plan {peak3} B, unmarked {peak2} B; an fp32 copy of X is {FP32_COPY} B")
    assert np.array_equal(half_ref.bits(out3), half_ref.bits(out2)), "the forward does not read the marker"
    _assert_exact(dv3.cpu().numpy(), ref_sum, rowptr, "marked plan")
    _assert_exact(dv2.cpu().numpy(), ref_sum, rowptr, "unmarked plan")
    assert peak3 < FP32_COPY <= peak2, (peak3, peak2, FP32_COPY)
