"""The 16-bit row kernel with an epilogue (fusedMM_csr_rows16_epilogue_hip),

    z[i,c] = round16( act( rs_i * ( sum_e cs[col[e]] * y[col[e],c] + ss_i * y[i,c] ) + bias[c] ) ),

the backward's 16-bit prologue (isplib_masked_colsum16_hip) and the fused GCN layer of bf16 / fp16 features that runs on them
(gcn_norm_matmul under ISPLIB_HALF_GCN), through the C ABI, the torch operator and the plug-in.

Without an epilogue the contract is EQUALITY OF BITS with the kernels already held to the oracle (fusedMM_csr_rows16_colscale_hip,
fusedMM_csr_rows16_hip); with one, integer data has the bits of the rounded fp64 formula and real-valued data meets the project's
1e-5 parity rule plus one rounding to 16 bits.  Every output is prefilled with NaN so an unwritten element shows, and every launch
runs twice to equal bits."""
import numpy as np
import pytest
import torch

from tests import cases, half_ref
from tests import rows16_gcn_cases as gc
from tests.test_gpu_rows16_colscale import K_OP, M_OP, _adj, _assert_same_bits, _nan_filled, _on, _peak_during, _twice, op_graph  # noqa: F401

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", tuple(half_ref.DTYPES.values()), ids=tuple(half_ref.DTYPES))
N = gc.N_HUB
# half the spacing of bf16's subnormals: a result below 2^-126 is rounded to a multiple of 2^-133 (fp16: rounding_bound's own 2^-25)
BF16_SUBNORMAL_HALF_SPACING = 2.0 ** -134


def _epilogue(gpu, rowptr, col, x16, col_scale=None, self_scale=None, row_scale=None, bias=None, act=False, order=None):
    """cabi.spmm_rows16_epilogue launched twice into NaN-filled outputs: equal bits, returned once."""
    from isplib_amd import cabi
    d_rowptr, d_col, d_cs, d_ss, d_rs, d_b = _on(gpu, rowptr, col, col_scale, self_scale, row_scale, bias)
    d_x = x16.to(gpu)
    d_o = None if order is None else torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(gpu)
    return _twice(lambda o: cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_cs, d_x, d_rs, d_ss, d_b, act, order=d_o, out=o), rowptr.size - 1,
                  x16.size(1), d_x)


def _tolerance(oracle, rowptr, col, x32, col_scale, self_scale, row_scale, bias):
    """1e-5 * ( |rs_i| * ( sum_e |cs x| + |ss_i x_i| ) + |b| ): the sum part from cases.sum_tolerance, the rest added."""
    w = np.ones(col.size, np.float32) if col_scale is None else col_scale[col]
    with np.errstate(invalid="ignore", over="ignore"):
        tol = cases.sum_tolerance(oracle, rowptr, col, w, x32).astype(np.float64)
        if self_scale is not None:
            tol = tol + 1e-5 * np.abs(self_scale.astype(np.float64)[:, None] * x32[:rowptr.size - 1])
        if row_scale is not None:
            tol = tol * np.abs(row_scale.astype(np.float64))[:, None]
        if bias is not None:
            tol = tol + 1e-5 * np.abs(bias.astype(np.float64))
    return tol


def _assert_within_bound(got16, ref, tol, dtype, what):
    """|got - ref| <= half_ref.rounding_bound(ref, tol, dtype) where ref is finite; NaN where ref is NaN, ref itself where it is Inf."""
    got = got16.cpu().to(torch.float32).numpy().astype(np.float64)
    nan, inf = np.isnan(ref), np.isinf(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN exactly where the formula has one"
    assert np.array_equal(got[inf], ref[inf]), f"{what}: Inf where the formula has one"
    fin = ~(nan | inf)
    tol = np.where(np.isfinite(tol), tol, 0.0)              # (a ReLU of NaN / -Inf is exactly +0.0: no tolerance to take from them)
    bound = half_ref.rounding_bound(ref[fin], tol[fin], dtype) + (BF16_SUBNORMAL_HALF_SPACING if dtype == torch.bfloat16 else 0.0)
    err = np.abs(got[fin] - ref[fin])
    print(f"{what}: max err / bound = {np.max(err / bound) if err.size else 0.0:.4f}")
    assert np.all(err <= bound), f"{what}: max err / bound = {np.max(err / bound)}"


# ---- 1. no epilogue: the bits of the kernels already verified --------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (8, 10, 64, 66, 128, 130, 256, 258, 512, 514, 1024, 1026))
def test_no_epilogue_gives_the_bits_of_the_plain_kernels(gpu, k, dtype):
    """ep == NULL, and separately a struct with every member NULL / 0: with a column table the bits of cabi.spmm_rows16_colscale, without
    one those of cabi.spmm_rows16(..., None, ...) -- the summation order is the verified kernels'."""
    from isplib_amd import cabi
    rowptr, col = gc.hub_graph()
    assert np.max(np.diff(rowptr)) > gc.LONG_ROW
    d_rowptr, d_col, d_s = _on(gpu, rowptr, col, gc.scale_table(N))
    d_x = half_ref.to16(cases.dense(N, k, 3, "uniform"), dtype).to(gpu)
    for table, want in ((d_s, cabi.spmm_rows16_colscale(d_rowptr, d_col, d_s, d_x, "sum")), (None, cabi.spmm_rows16(d_rowptr, d_col, None, d_x, "sum"))):
        for null in (True, False):
            got = _twice(lambda o: cabi.fusedMM_csr_rows16_epilogue_hip(d_rowptr, d_col, table, None, d_x, o, null_epilogue=null), N, k, d_x)
            _assert_same_bits(got, want, f"k {k}, table {table is not None}, ep NULL {null}")


# ---- 2. integer data: the bits of the rounded fp64 formula -----------------------------------------------------------------------

@DT
@pytest.mark.parametrize("act", (False, True), ids=("linear", "relu"))
@pytest.mark.parametrize("k", (10, 64, 256, 1026))
def test_integer_data_has_the_bits_of_the_rounded_formula(gpu, k, act, dtype):
    """x in [-3, 3], integer col / self scales in [-5, 5], row scales in {+-0.5, +-1, +-2}, integer bias: every fp32 intermediate is
    exact (tests/test_rows16_gcn_host.py: below 2^24), so the output is round16 of the fp64 formula bit for bit -- all members on and
    each absent in turn, on the hub graph and on the graph of loop-edge lengths."""
    for name, (rowptr, col) in (("hub", gc.hub_graph()), ("lengths", gc.length_graph())):
        m = rowptr.size - 1
        x16 = half_ref.to16(cases.dense(m, k, 3, "integer"), dtype)
        for which in gc.MEMBER_SETS:
            mem = gc.integer_members(which, m, k)
            ref, _ = gc.formula64(rowptr, col, half_ref.widen(x16), mem["col_scale"], mem["self_scale"], mem["row_scale"], mem["bias"], act)
            got = _epilogue(gpu, rowptr, col, x16, mem["col_scale"], mem["self_scale"], mem["row_scale"], mem["bias"], act)
            _assert_same_bits(got, half_ref.round16(ref, dtype), f"{name}, k {k}, {which}")


# ---- 3 / 4. real-valued data against the fp64 formula; row lengths ---------------------------------------------------------------

def _real_valued(gpu, oracle, rowptr, col, k, dtype, what):
    m = rowptr.size - 1
    x16 = half_ref.to16(cases.dense(m, k, 3, "uniform"), dtype)
    x32 = half_ref.widen(x16)
    c, s, r, b = gc.scale_table(m), gc.scale_table(m, 61), gc.scale_table(m, 67) * np.float32(4), gc.real_bias(k)
    for act in (False, True):
        ref, _ = gc.formula64(rowptr, col, x32, c, s, r, b, act)
        got = _epilogue(gpu, rowptr, col, x16, c, s, r, b, act)
        _assert_within_bound(got, ref, _tolerance(oracle, rowptr, col, x32, c, s, r, b), dtype, f"{what}, relu {act}")


@DT
@pytest.mark.parametrize("k", (8, 10, 64, 66, 256, 258, 1024, 1026))
def test_real_valued_data_meets_the_parity_bound(gpu, oracle_mod, k, dtype):
    """All members on: |got - ref| <= rounding_bound(ref, 1e-5 * (|rs_i| (sum_e |cs x| + |ss_i x_i|) + |b|)) -- the project's 1e-5 parity
    rule (the epilogue's three extra fp32 roundings are ~2e-7 of that magnitude) and one rounding to 16 bits."""
    rowptr, col = gc.hub_graph()
    _real_valued(gpu, oracle_mod, rowptr, col, k, dtype, f"hub, k {k}")


@DT
@pytest.mark.parametrize("k", (64, 256))
def test_row_lengths_around_every_loop_edge(gpu, oracle_mod, k, dtype):
    rowptr, col = gc.length_graph()
    _real_valued(gpu, oracle_mod, rowptr, col, k, dtype, f"lengths, k {k}")


# ---- 5. row order ----------------------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (64, 256))
def test_any_row_order_gives_the_bits_of_index_order(gpu, k, dtype):
    rowptr, col = gc.hub_graph()
    x16 = half_ref.to16(cases.dense(N, k, 3, "uniform"), dtype)
    members = (gc.scale_table(N), gc.scale_table(N, 61), gc.scale_table(N, 67), gc.real_bias(k), True)
    base = _epilogue(gpu, rowptr, col, x16, *members)
    for order in (np.random.default_rng(5).permutation(N), np.arange(N)[::-1].copy()):
        _assert_same_bits(_epilogue(gpu, rowptr, col, x16, *members, order=order), base, f"k {k}")


# ---- 6. ReLU edge cases ----------------------------------------------------------------------------------------------------------

@DT
def test_relu_and_empty_rows(gpu, dtype):
    """The ReLU is v > 0 ? v : 0 in fp32 (gc.relu: the fp32 epilogue's), so a row whose value before it is exactly -0.0 stores +0.0 --
    and -0.0 without ReLU.  An empty row gives act(rs_i * ss_i * x_i + b), an empty row without a self term act(b)."""
    rowptr, col = gc.hub_graph()
    k = 64
    x16 = half_ref.to16(cases.dense(N, k, 3, "integer"), dtype)
    x32 = half_ref.widen(x16)
    empty = [0, 150, 299]
    rs = gc.row_scale_table(N)
    rs[0], rs[150] = -1.0, 2.0
    ss, b = gc.integer_scale(N, 31), gc.integer_bias(k)
    # rs_0 * (+0.0) = -0.0: no bias, no self term
    lin = half_ref.bits(_epilogue(gpu, rowptr, col, x16, None, None, rs, None, False))
    act = half_ref.bits(_epilogue(gpu, rowptr, col, x16, None, None, rs, None, True))
    assert np.all(lin[0].view(np.uint16) == 0x8000) and np.all(act[0] == 0), "-0.0 without ReLU, +0.0 with it"
    assert np.all(lin[150] == 0) and np.all(act[150] == 0)
    for relu in (False, True):
        # an empty row: act(rs_i * ss_i * x_i + b)
        got = _epilogue(gpu, rowptr, col, x16, gc.integer_scale(N), ss, rs, b, relu)
        want = gc.epilogue_emulation(np.zeros((N, k), np.float32), x32, ss, rs, b, relu)
        assert np.array_equal(half_ref.bits(got)[empty], half_ref.bits(half_ref.round16(want, dtype))[empty])
        # ... and without a self term: act(b)
        got = _epilogue(gpu, rowptr, col, x16, gc.integer_scale(N), None, rs, b, relu)
        want = np.broadcast_to(gc.relu(b) if relu else b, (N, k))
        assert np.array_equal(half_ref.bits(got)[empty], half_ref.bits(half_ref.round16(want, dtype))[empty])


# ---- 7. non-finite and small values ----------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("where", ("operand", "col_scale", "self_scale", "row_scale", "bias"))
@pytest.mark.parametrize("kind", ("nonfinite", "denormal"))
def test_nonfinite_and_small_values(gpu, oracle_mod, kind, where, dtype):
    """Inf / NaN / subnormals in x and in each table: NaN exactly where the fp64 formula has one (without ReLU; with it NaN becomes +0.0
    as gc.relu says), Inf where it has one, the bound elsewhere.  K = 66: the last vector is shifted back over six columns of its
    neighbour, so a special value there must show in its own column only."""
    n, k = 97, 66
    rowptr, col = cases.random_csr(n, n, 3.0, 41, empty_rows=(5,))
    x16 = half_ref.to16(cases.dense(n, k, 3, kind if where == "operand" else "uniform"), dtype)
    x32 = half_ref.widen(x16)
    mem = {"col_scale": gc.scale_table(n), "self_scale": gc.scale_table(n, 61), "row_scale": gc.scale_table(n, 67), "bias": gc.real_bias(k)}
    if where != "operand":
        mem[where] = gc.special_scale(kind, k if where == "bias" else n)
    for act in (False, True):
        ref, _ = gc.formula64(rowptr, col, x32, mem["col_scale"], mem["self_scale"], mem["row_scale"], mem["bias"], act)
        if kind == "nonfinite" and not act:
            assert np.any(np.isnan(ref)) and np.any(np.isinf(ref)), "the case must hold NaN and Inf results"
        got = _epilogue(gpu, rowptr, col, x16, mem["col_scale"], mem["self_scale"], mem["row_scale"], mem["bias"], act)
        tol = _tolerance(oracle_mod, rowptr, col, x32, mem["col_scale"], mem["self_scale"], mem["row_scale"], mem["bias"])
        _assert_within_bound(got, ref, tol, dtype, f"{kind} in the {where}, relu {act}")


# ---- 8. views and pitches --------------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("k", (64, 10, 66))
def test_column_view_and_output_pitch(gpu, k, dtype):
    """y a [n, k] column view of a wider tensor whose neighbouring columns hold Inf (ragged K: the shifted last vector overlaps its
    neighbour INSIDE the view only), z a view at a wider pitch prefilled with NaN: the bits of the packed call, the padding untouched."""
    from isplib_amd import cabi
    rowptr, col = gc.hub_graph()
    wide = cases.dense(N, 192, 5, "uniform")
    wide[:, :64], wide[:, 64 + k:] = np.inf, np.inf
    d_wide = half_ref.to16(wide, dtype).to(gpu)
    d_view = d_wide[:, 64:64 + k]
    assert d_view.stride(0) == 192
    d_rowptr, d_col, d_c, d_s, d_r, d_b = _on(gpu, rowptr, col, gc.scale_table(N), gc.scale_table(N, 61), gc.scale_table(N, 67), gc.real_bias(k))
    big = _nan_filled(N, k + 66, dtype, gpu)
    out = cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_c, d_view, d_r, d_s, d_b, True, out=big[:, :k])
    torch.cuda.synchronize()
    assert out.data_ptr() == big.data_ptr() and out.stride(0) == k + 66
    want = cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_c, d_view.contiguous(), d_r, d_s, d_b, True)
    assert bool(torch.isfinite(want.float()).all()), "no Inf of the neighbouring columns may leak"
    _assert_same_bits(out.contiguous(), want, f"column view, k {k}")
    assert bool(torch.isnan(big[:, k:]).all()), "columns beyond k must not be touched"


@DT
@pytest.mark.parametrize("k", (10, 66))
def test_ragged_k_keeps_inf_in_its_own_column(gpu, oracle_mod, k, dtype):
    """Inf in the columns the shifted last vector re-reads (k-8 .. the slot's end) of x and of the bias: each stays in its own column."""
    rowptr, col = gc.hub_graph()
    x = cases.dense(N, k, 3, "uniform")
    x[::7, k - 8:k - 2] = np.inf
    x16 = half_ref.to16(x, dtype)
    x32 = half_ref.widen(x16)
    b = gc.real_bias(k)
    b[k - 3] = -np.inf
    c, s, r = np.abs(gc.scale_table(N)) + np.float32(0.25), np.abs(gc.scale_table(N, 61)) + np.float32(0.25), np.abs(gc.scale_table(N, 67)) + np.float32(0.25)
    ref, _ = gc.formula64(rowptr, col, x32, c, s, r, b, False)
    assert np.all(np.isfinite(ref[:, k - 2:])) and np.any(np.isinf(ref[:, k - 8:k - 2]))
    got = _epilogue(gpu, rowptr, col, x16, c, s, r, b, False)
    _assert_within_bound(got, ref, _tolerance(oracle_mod, rowptr, col, x32, c, s, r, b), dtype, f"ragged k {k}")


# ---- 9. refusals before any launch -----------------------------------------------------------------------------------------------

@DT
def test_entry_refuses_before_any_launch(gpu, dtype):
    """Each refused call returns ISPLIB_FAIL, leaves the output as it was, and isplib_hip_last_error names the entry and the cause."""
    from isplib_amd import cabi
    rowptr, col = cases.random_csr(120, 120, 9.0, 21, empty_rows=(4,), hub=(9, 700), duplicates=True)
    n, k = 120, 64
    d_rowptr, d_col, d_s = _on(gpu, rowptr, col, gc.scale_table(n))
    y = torch.ones((n, k), dtype=dtype, device=gpu)
    flat = torch.ones(n * k + 2, dtype=dtype, device=gpu)
    order = torch.arange(n, dtype=torch.int32, device=gpu)
    calls = (
        ("dtype", y, {"dtype": 0}),                                                  # what an fp32 tensor maps to
        ("isplib_rows16_serves", y, {"k": 63}),                                      # odd k
        ("isplib_rows16_serves", y, {"k": 6}),                                       # k < 8
        ("leading dimension", y, {"ldy": k - 2}),
        ("self_scale needs m == n", y, {"m": n - 1, "self_scale": d_s}),
        ("4-byte aligned", flat[1:1 + n * k].view(n, k), {}),                        # a base at 2 bytes mod 4
        ("m must be < 2^31", y, {"m": 2 ** 31, "order": order}),                     # sizes only: refused before anything is read
    )
    for cause, yy, extra in calls:
        z = _nan_filled(n, 66, dtype, gpu)
        o = extra.pop("order", None)
        st = cabi.fusedMM_csr_rows16_epilogue_hip(d_rowptr, d_col, d_s, o, yy, z[:, :k], check=False, **extra)
        torch.cuda.synchronize()
        assert st == cabi.FAIL and cause in cabi.last_error(), (cause, st, cabi.last_error())
        assert "fusedMM_csr_rows16_epilogue_hip" in cabi.last_error()
        assert bool(torch.isnan(z).all()), cause
    # nothing to do is a success: m = 0, k = 0
    empty_rp = torch.zeros(1, dtype=torch.int64, device=gpu)
    assert cabi.fusedMM_csr_rows16_epilogue_hip(empty_rp, d_col[:0], None, None, y, torch.empty((0, k), dtype=dtype, device=gpu), check=False) == cabi.SUCCESS
    z = _nan_filled(n, k, dtype, gpu)
    assert cabi.fusedMM_csr_rows16_epilogue_hip(d_rowptr, d_col, d_s, None, y, z, check=False, k=0) == cabi.SUCCESS
    torch.cuda.synchronize()
    assert bool(torch.isnan(z).all())
    # the wrapper raises before the call
    with pytest.raises(ValueError):
        cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_s[:-1], y)                       # one factor per column
    with pytest.raises(ValueError):
        cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_s, y, row_scale=d_s[:-1])
    with pytest.raises(ValueError):
        cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_s, y, bias=d_s[:k - 1])
    with pytest.raises(ValueError):
        cabi.spmm_rows16_epilogue(d_rowptr[:-1], d_col[:int(rowptr[-2])], d_s, y, self_scale=d_s[:-1])     # a self term, m != n
    with pytest.raises(ValueError):
        cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_s, y[:, :6])
    with pytest.raises(ValueError):
        cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_s[:100], y[:100])                # column ids beyond n
    with pytest.raises(TypeError):
        cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_s, y.to(torch.float32))
    with pytest.raises(TypeError):
        cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_s, y, row_scale=d_s.to(torch.float64))
    with pytest.raises(RuntimeError):
        cabi.spmm_rows16_epilogue(d_rowptr, d_col, d_s, y, bias=torch.zeros(k))      # a host table


@DT
def test_no_edges_still_runs_the_epilogue(gpu, dtype):
    """nnz == 0 launches: every row gets act(rs_i * ss_i * x_i + b)."""
    n, k = 37, 10
    rowptr, col = np.zeros(n + 1, np.int64), np.zeros(0, np.int64)
    x16 = half_ref.to16(cases.dense(n, k, 3, "integer"), dtype)
    ss, rs, b = gc.integer_scale(n, 31), gc.row_scale_table(n), gc.integer_bias(k)
    got = _epilogue(gpu, rowptr, col, x16, None, ss, rs, b, True)
    want = gc.epilogue_emulation(np.zeros((n, k), np.float32), half_ref.widen(x16), ss, rs, b, True)
    _assert_same_bits(got, half_ref.round16(want, dtype), "no edges")


# ---- 10. the backward's prologue -------------------------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("n,k,pitch", ((1000, 42, 48), (513, 8, None), (700, 300, None), (3, 64, None), (2049, 32, None)))
def test_masked_colsum16_matches_torch(gpu, n, k, pitch, dtype):
    """g has the bits of torch.where(out > 0, dz, 0); grad_bias is within 1e-5 * sum |g| of the fp64 column sum and has equal bits on
    two runs; each optional operand absent in turn."""
    from isplib_amd import cabi
    ld = pitch or k
    dz = half_ref.to16(cases.dense(n, ld, 3, "uniform"), dtype).to(gpu)[:, :k]
    out = half_ref.to16(cases.dense(n, ld, 5, "signed_zero"), dtype).to(gpu)[:, :k]
    assert dz.stride(0) == ld
    for use_out in (True, False):
        want = torch.where(out > 0, dz, torch.zeros((), dtype=dtype, device=gpu)) if use_out else dz
        g, gb = cabi.masked_colsum16(dz, out if use_out else None)
        g2, gb2 = cabi.masked_colsum16(dz, out if use_out else None)
        torch.cuda.synchronize()
        assert g.dtype == dtype and gb.dtype == torch.float32
        _assert_same_bits(g, want.contiguous(), f"g, mask {use_out}")
        assert torch.equal(gb.view(torch.int32), gb2.view(torch.int32)) and np.array_equal(half_ref.bits(g), half_ref.bits(g2)), "two runs: equal bits"
        w64 = want.cpu().to(torch.float64).numpy()
        err = np.abs(gb.cpu().numpy().astype(np.float64) - w64.sum(0))
        assert np.all(err <= 1e-5 * np.abs(w64).sum(0) + 1e-30), float(np.max(err))
        only_g, none = cabi.masked_colsum16(dz, out if use_out else None, want_bias=False)
        none2, only_b = cabi.masked_colsum16(dz, out if use_out else None, want_g=False)
        assert none is None and none2 is None
        _assert_same_bits(only_g, want.contiguous(), "g alone")
        assert torch.equal(only_b.view(torch.int32), gb.view(torch.int32)), "grad_bias alone"
    with pytest.raises(TypeError):
        cabi.masked_colsum16(dz.float(), None)
    with pytest.raises(ValueError):
        cabi.masked_colsum16(dz, out[:-1])


# ---- 11-14. operator and autograd, through gcn_norm_matmul -----------------------------------------------------------------------

FP32_COPY = M_OP * K_OP * 4


def _setenv(monkeypatch, gcn, half=None):
    monkeypatch.setenv("ISPLIB_STREAM", "0")
    for name, value in (("ISPLIB_HALF_GCN", gcn), ("ISPLIB_HALF", half)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)


def _layer(gpu, adj, x16, g16, bias=None, relu=False):
    """(out, x.grad, bias.grad, peak of the forward, peak of the backward, schedule) of gcn_norm_matmul(adj, x, bias, relu).backward(g)."""
    import isplib_amd
    x = x16.to(gpu).requires_grad_(True)
    b = None if bias is None else bias.to(gpu).requires_grad_(True)
    fw_peak, out = _peak_during(lambda: isplib_amd.gcn_norm_matmul(adj, x, b, relu))
    schedule = adj.storage._last_schedule
    g = g16.to(gpu)
    bw_peak, _ = _peak_during(lambda: out.backward(g))
    return out.detach(), x.grad.detach(), None if b is None else b.grad.detach(), fw_peak, bw_peak, schedule


def _layer_operands(dtype, k=K_OP):
    return half_ref.to16(cases.dense(M_OP, k, 3, "uniform"), dtype), half_ref.to16(cases.dense(M_OP, k, 5, "uniform"), dtype)


def _assert_layer(oracle, op_graph, dinv, out, xgrad, bgrad, x16, g16, bias, relu, dtype, what):
    """out against relu(D^-1/2 (A + I) D^-1/2 x + b) and x.grad against D (A^T + I) D (g . [out16 > 0]), both in fp64 on the widened
    operands under the bound of the C ABI tests; the mask is the RETURNED output's.  bias.grad within 1e-5 * sum |g| (+ one unit
    roundoff of a 16-bit bias)."""
    rowptr, col = op_graph
    x32, g32 = half_ref.widen(x16), half_ref.widen(g16)
    b32 = None if bias is None else bias.to(torch.float32).numpy()
    ref, _ = gc.formula64(rowptr, col, x32, dinv, dinv, dinv, b32, relu)
    _assert_within_bound(out, ref, _tolerance(oracle, rowptr, col, x32, dinv, dinv, dinv, b32), dtype, f"{what}: out")
    gm = g32 * (out.cpu().to(torch.float32).numpy() > 0) if relu else g32
    colptr, row_t = gc.transpose_csr(rowptr, col, M_OP)
    gref, _ = gc.formula64(colptr, row_t, gm, dinv, dinv, dinv, None, False)
    _assert_within_bound(xgrad, gref, _tolerance(oracle, colptr, row_t, gm.astype(np.float32), dinv, dinv, dinv, None), dtype, f"{what}: x.grad")
    if bias is not None:
        want = gm.astype(np.float64).sum(0)
        slack = 1e-5 * np.abs(gm).astype(np.float64).sum(0) + 1e-30
        if bias.dtype != torch.float32:
            slack = slack + half_ref.UNIT_ROUNDOFF[bias.dtype] * (np.abs(want) + slack)
        err = np.abs(bgrad.cpu().to(torch.float64).numpy() - want)
        assert np.all(err <= slack), f"{what}: bias.grad, max err / bound = {np.max(err / slack)}"


@DT
@pytest.mark.parametrize("bias_kind,relu", ((None, False), ("fp32", True), ("half", True)), ids=("plain", "fp32_bias_relu", "half_bias_relu"))
def test_gcn_norm_matmul_runs_in_16_bits(gpu, oracle_mod, op_graph, monkeypatch, bias_kind, relu, dtype):
    _setenv(monkeypatch, "native")
    adj = _adj(gpu, op_graph, None)
    x16, g16 = _layer_operands(dtype)
    bias = None if bias_kind is None else torch.from_numpy(gc.real_bias(K_OP)).to(torch.float32 if bias_kind == "fp32" else dtype)
    out, xgrad, bgrad, _, _, schedule = _layer(gpu, adj, x16, g16, bias, relu)
    assert schedule[0] == "rows16gcn", schedule
    assert out.dtype == dtype and xgrad.dtype == dtype and (bias is None or bgrad.dtype == bias.dtype)
    dinv = adj.storage.gcn_dinv().cpu().numpy()
    _assert_layer(oracle_mod, op_graph, dinv, out, xgrad, bgrad, x16, g16, bias, relu, dtype, f"bias {bias_kind}, relu {relu}")


@DT
def test_native_route_allocates_no_fp32_copy(gpu, op_graph, monkeypatch, dtype):
    """The native forward allocates less than one fp32 copy of X (it needs `out`, n k 2 bytes), the native backward with ReLU less than
    two (g and dX, n k 2 bytes each, and a workspace of a few KB); the conversion route's backward holds dz.float() and the scaled
    gradient together, at least two."""
    adj = _adj(gpu, op_graph, None)
    x16, g16 = _layer_operands(dtype)
    bias = torch.from_numpy(gc.real_bias(K_OP))
    _setenv(monkeypatch, "native")
    _layer(gpu, adj, x16, g16, bias, True)                                            # builds the transpose and the plans
    _, _, _, fw, bw, schedule = _layer(gpu, adj, x16, g16, bias, True)
    assert schedule[0] == "rows16gcn"
    _setenv(monkeypatch, "convert")
    _layer(gpu, adj, x16, g16, bias, True)
    _, _, _, cfw, cbw, cschedule = _layer(gpu, adj, x16, g16, bias, True)
    assert cschedule[0] == "convert"
    print(f"peak forward / backward: native {fw} / {bw}, convert {cfw} / {cbw}; an fp32 copy of X is {FP32_COPY}")
    assert fw < FP32_COPY, (fw, FP32_COPY)
    assert bw < 2 * FP32_COPY, (bw, 2 * FP32_COPY)
    assert cbw >= 2 * FP32_COPY, (cbw, 2 * FP32_COPY)


@DT
def test_route_is_opt_in(gpu, oracle_mod, op_graph, monkeypatch, dtype):
    import isplib_amd
    adj = _adj(gpu, op_graph, None)
    x16, g16 = _layer_operands(dtype)
    bias = torch.from_numpy(gc.real_bias(K_OP))
    dinv = adj.storage.gcn_dinv().cpu().numpy()
    # unset: the refusal as it always was
    _setenv(monkeypatch, None)
    with pytest.raises(RuntimeError, match="needs a float32 GPU matrix"):
        isplib_amd.gcn_norm_matmul(adj, x16.to(gpu))
    fp32_unset = _layer(gpu, adj, x16.float(), g16.float(), bias, True)
    # convert: the bits of the same thing written by hand
    _setenv(monkeypatch, "convert")
    out, xgrad, bgrad, _, _, schedule = _layer(gpu, adj, x16, g16, bias, True)
    assert schedule[0] == "convert" and out.dtype == dtype and xgrad.dtype == dtype and bgrad.dtype == torch.float32
    by_hand = isplib_amd.gcn_norm_matmul(adj, x16.to(gpu).float(), bias.to(gpu), True).to(dtype)
    _assert_same_bits(out, by_hand, "convert against x.float() -> gcn_norm_matmul -> .to(dtype)")
    # ISPLIB_HALF=convert wins over ISPLIB_HALF_GCN=native
    _setenv(monkeypatch, "native", "convert")
    out2, _, _, _, _, schedule = _layer(gpu, adj, x16, g16, bias, True)
    assert schedule[0] != "rows16gcn", schedule
    _assert_same_bits(out2, out, "ISPLIB_HALF=convert")
    # native outside the domain: no raise, the result within the bound
    _setenv(monkeypatch, "native")
    for k in (7, 6):
        xk, gk = _layer_operands(dtype, k)
        bk = torch.from_numpy(gc.real_bias(k))
        o, xg, bg, _, _, schedule = _layer(gpu, adj, xk, gk, bk, True)
        assert schedule[0] == "convert" and o.dtype == dtype and xg.dtype == dtype
        _assert_layer(oracle_mod, op_graph, dinv, o, xg, bg, xk, gk, bk, True, dtype, f"k {k}")
    # fp32 calls do not read the variable
    fp32_set = _layer(gpu, adj, x16.float(), g16.float(), bias, True)
    for a, b in zip(fp32_unset[:3], fp32_set[:3]):
        assert a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@DT
def test_direct_operator_call_outside_the_domain_converts(gpu, oracle_mod, op_graph, dtype):
    """torch.ops.isplib.gcn_norm_spmm with a 16-bit row plan and a 16-bit `mat` the family does not take (K = 7): the conversion route,
    nothing raises; without such a plan a 16-bit `mat` is refused as it always was."""
    adj = _adj(gpu, op_graph, None)
    s = adj.storage
    x16, _ = _layer_operands(dtype, 7)
    row_plan = [torch.empty(0, dtype=torch.int32, device=gpu), torch.tensor([16], dtype=torch.int32)]
    out = torch.ops.isplib.gcn_norm_spmm(s._rowptr, s._col, x16.to(gpu), s.gcn_dinv(), None, None, row_plan, [], None, True)
    assert out.dtype == dtype
    dinv = s.gcn_dinv().cpu().numpy()
    x32 = half_ref.widen(x16)
    ref, _ = gc.formula64(op_graph[0], op_graph[1], x32, dinv, dinv, dinv, None, True)
    _assert_within_bound(out, ref, _tolerance(oracle_mod, op_graph[0], op_graph[1], x32, dinv, dinv, dinv, None), dtype, "k 7")
    with pytest.raises(RuntimeError):
        torch.ops.isplib.gcn_norm_spmm(s._rowptr, s._col, x16.to(gpu), s.gcn_dinv(), None, None, [], [], None, True)


@DT
def test_community_order_gives_the_bits_of_index_order(gpu, op_graph, monkeypatch, dtype):
    """A row order on both sides (forced: the graph is far too small for the search to be asked): ("rows16gcn", "ordered"), and the
    forward and the backward have the bits of the call in index order."""
    _setenv(monkeypatch, "native")
    x16, g16 = _layer_operands(dtype)
    bias = torch.from_numpy(gc.real_bias(K_OP))
    base = _layer(gpu, _adj(gpu, op_graph, None), x16, g16, bias, True)
    assert base[5] == ("rows16gcn",)
    adj = _adj(gpu, op_graph, None)
    rng = np.random.default_rng(9)
    orders = {side: torch.from_numpy(rng.permutation(M_OP).astype(np.int32)).to(gpu) for side in (False, True)}
    seen = []

    def forced(transposed, k, itemsize=4):
        seen.append((transposed, itemsize))
        return [orders[bool(transposed)]]

    monkeypatch.setattr(adj.storage, "row_order", forced, raising=False)
    got = _layer(gpu, adj, x16, g16, bias, True)
    assert got[5] == ("rows16gcn", "ordered") and (False, 2) in seen and (True, 2) in seen, (got[5], seen)
    for a, b, what in zip(base[:3], got[:3], ("out", "x.grad", "bias.grad")):
        assert a.dtype == b.dtype
        assert torch.equal(a.view(torch.int16) if a.dtype != torch.float32 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype != torch.float32 else b.view(torch.int32)), what
