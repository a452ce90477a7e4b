"""The 16-bit attention operator on the GPU (isplib_amd/csrc/attention16.hip): the C ABI wrappers, torch.ops.isplib.attention_spmm16 with
its autograd backward, and the plug-in's opt-in route, each held to the per-element bounds of tests/attention16_ref.py against the
fp64 reference on the widened operands (inputs, references and bounds: tests/attention16_cases.py, computed once per case).  The
largest error / bound seen per output is printed before every assertion; DESIGN.md 4.6c records it.
"""
import numpy as np
import pytest
import torch

from tests import attention16_cases as c16
from tests import half_ref

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
BOTH = pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)


def dev(a, gpu):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).to(gpu)


def dev_graph(case, gpu):
    return dev(case.rowptr, gpu), dev(case.col, gpu)


_transposed = {}


def transposed(case, gpu):
    """colptr / row_t as SparseStorage caches them (the library's own csr2csc), once per graph."""
    import isplib_amd
    key = (case.rowptr.tobytes(), case.col.tobytes())
    if key not in _transposed:
        rowptr, col = dev_graph(case, gpu)
        st = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.y.shape[0])).storage
        _transposed[key] = (st.colptr(), st.row_t())
    return _transposed[key]


def held(case, got, names=("z", "lse", "dx", "dy", "D")):
    frac = c16.fractions(case, got, names)
    print(f"attention16 error/bound {case.name}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def run_cabi(case, gpu, x=None, y=None, g=None):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    x = dev(case.x16, gpu) if x is None else x
    y = dev(case.y16, gpu) if y is None else y
    g = dev(case.g16, gpu) if g is None else g
    z, lse = cabi.attention16(rowptr, col, x, y, case.p)
    dx, D = cabi.attention16_bw_rows(rowptr, col, x, y, g, lse, case.p)
    colptr, row_t = transposed(case, gpu)
    dy = cabi.attention16_bw_cols(colptr, row_t, x, y, g, lse, D, case.p)
    return dict(z=z, lse=lse, dx=dx, dy=dy, D=D)


@BOTH
@pytest.mark.parametrize("k", c16.WIDTHS)
def test_cabi_entries_at_every_width(gpu, k, dtype):
    """First, last and a ragged width of every slot, on both graphs: every row length and column in-degree on a loop edge."""
    for graph in ("g1", "g2"):
        case = c16.width_case(k, dtype, graph)
        got = run_cabi(case, gpu)
        assert got["z"].dtype == got["dx"].dtype == got["dy"].dtype == dtype and got["lse"].dtype == got["D"].dtype == torch.float32
        held(case, got)
        empty = ~case.live
        assert empty.any() and not got["z"].cpu()[empty].any() and not got["dx"].cpu()[empty].any()
        unreferenced = np.bincount(case.col, minlength=case.y.shape[0]) == 0
        assert unreferenced.any() and not got["dy"].cpu()[unreferenced].any()


@BOTH
@pytest.mark.parametrize("k", c16.WIDTHS)
def test_operator_and_autograd_at_every_width(gpu, k, dtype):
    """torch.ops.isplib.attention_spmm16 with y distinct; only x asking (the columns kernel does not run) and only y asking give the
    same bits."""
    case = c16.width_case(k, dtype, "g2" if k <= 32 else "g1")
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    g = dev(case.g16, gpu)
    x, y = dev(case.x16, gpu).requires_grad_(True), dev(case.y16, gpu).requires_grad_(True)
    z = torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, x, y, case.p)
    z.backward(g)
    assert z.dtype == x.grad.dtype == y.grad.dtype == dtype
    held(case, dict(z=z, dx=x.grad, dy=y.grad), ("z", "dx", "dy"))
    x2, y2 = dev(case.x16, gpu).requires_grad_(True), dev(case.y16, gpu)
    torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, x2, y2, case.p).backward(g.float())      # a grad of another dtype is cast
    assert y2.grad is None and torch.equal(x2.grad, x.grad)
    x3, y3 = dev(case.x16, gpu), dev(case.y16, gpu).requires_grad_(True)
    torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, x3, y3, case.p).backward(g)
    assert x3.grad is None and torch.equal(y3.grad, y.grad)


_self_cases = {}


def self_case(k, dtype):
    if (k, dtype) not in _self_cases:
        base = c16.width_case(k, dtype)
        case = c16.Case16(f"self{k}", base.rowptr, base.col, np.array(base.x), np.array(base.x), np.array(base.g), base.p, dtype)
        assert case.bound["rho"].max() <= 1e-3
        _self_cases[(k, dtype)] = case
    return _self_cases[(k, dtype)]


@BOTH
@pytest.mark.parametrize("k", (16, 130))
def test_shared_operand(gpu, k, dtype):
    """y = x: x.grad receives both contributions, each rounded once to the dtype and then added by autograd in the dtype."""
    case = self_case(k, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    x = dev(case.x16, gpu).requires_grad_(True)
    z = torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, x, x, case.p)
    z.backward(dev(case.g16, gpu))
    held(case, dict(z=z), ("z",))
    want = case.ref["dx"] + case.ref["dy"]
    u = half_ref.UNIT_ROUNDOFF[dtype]
    bound = case.bound["dx"] + case.bound["dy"] + u * (np.abs(want) + case.bound["dx"] + case.bound["dy"])      # autograd's one more rounding
    frac = c16.worst(c16.as_array(x.grad), want, bound)
    print(f"attention16 error/bound {case.name}: dx+dy={frac:.4f}")
    assert frac <= 1.0


@BOTH
def test_one_entry_rows_return_y_bit_for_bit(gpu, dtype):
    case = c16.single_case(dtype)
    got = run_cabi(case, gpu)
    live = case.live
    want = torch.zeros_like(case.y16[:case.m])
    want[torch.from_numpy(live)] = case.y16[torch.from_numpy(case.col)]
    assert np.array_equal(half_ref.bits(got["z"]), half_ref.bits(want))
    held(case, got, ("lse", "dx", "dy", "D"))


@BOTH
def test_scores_spread_over_200(gpu, dtype):
    case = c16.large_case(dtype)
    got = run_cabi(case, gpu)
    for name in ("z", "dx", "dy", "D"):
        assert torch.isfinite(got[name].float()).all(), name
    held(case, got)


@BOTH
@pytest.mark.parametrize("k", (10, 130, 512))
def test_outputs_are_write_only_and_launches_repeat(gpu, k, dtype):
    """NaN-filled, pitched (ld = K + 6), over-allocated outputs, launched twice: every element of every row is written, nothing between
    the rows or past the end, equal bits."""
    from isplib_amd import cabi
    case = c16.width_case(k, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    x, y, g = dev(case.x16, gpu), dev(case.y16, gpu), dev(case.g16, gpu)
    m, n, pad, ld = case.m, case.y.shape[0], 64, k + 6

    def fresh(rows, cols=None):
        if cols is None:
            buf = torch.full((rows + pad,), float("nan"), device=gpu)
            return buf, buf[:rows]
        buf = torch.full((rows * ld + pad,), float("nan"), device=gpu, dtype=dtype)
        return buf, buf[:rows * ld].view(rows, ld)[:, :cols]

    runs = []
    for _ in range(2):
        bufs = {name: fresh(*shape) for name, shape in (("z", (m, k)), ("lse", (m,)), ("dx", (m, k)), ("D", (m,)), ("dy", (n, k)))}
        cabi.attention16(rowptr, col, x, y, case.p, out=(bufs["z"][1], bufs["lse"][1]), check=False)
        cabi.attention16_bw_rows(rowptr, col, x, y, g, bufs["lse"][1], case.p, out=(bufs["dx"][1], bufs["D"][1]), check=False)
        cabi.attention16_bw_cols(colptr, row_t, x, y, g, bufs["lse"][1], bufs["D"][1], case.p, out=bufs["dy"][1], check=False)
        for name, (buf, view) in bufs.items():
            assert not torch.isnan(view).any(), name
            if view.dim() == 2:
                rest = buf[:view.size(0) * ld].view(view.size(0), ld)[:, k:]
                assert torch.isnan(rest).all() and torch.isnan(buf[view.size(0) * ld:]).all(), name
            else:
                assert torch.isnan(buf[view.numel():]).all(), name
        runs.append({name: view.clone() for name, (_, view) in bufs.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    held(case, runs[0])


@BOTH
@pytest.mark.parametrize("d", (10, 24))
def test_heads_between_nan_and_inf_neighbours(gpu, d, dtype):
    """Heads as column views of one [N, 3 d] tensor: the middle head is computed while its neighbours hold NaN and Inf, and equals the
    same head from packed copies bit for bit -- an over-read column in a dot product, or Inf * 0, would show."""
    case = c16.width_case(d, dtype) if d in c16.WIDTHS else None
    if case is None:
        raise AssertionError("head widths must be widths of the cases")
    packed = run_cabi(case, gpu)
    wide = {}
    for name, a in (("x", case.x16), ("y", case.y16), ("g", case.g16)):
        t = torch.empty(case.m, 3 * d, device=gpu, dtype=dtype)
        t[:, :d] = float("nan")
        t[:, 2 * d:] = float("inf")
        t[:, d:2 * d] = dev(a, gpu)
        wide[name] = t[:, d:2 * d]
        assert not wide[name].is_contiguous() and wide[name].stride(0) == 3 * d
    got = run_cabi(case, gpu, wide["x"], wide["y"], wide["g"])
    for name in ("z", "lse", "dx", "dy", "D"):
        assert torch.equal(got[name], packed[name]), name
    # the same through the operator: the views go in as they lie
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    xw = wide["x"]._base.clone().requires_grad_(True)
    yw = wide["y"]._base.clone().requires_grad_(True)
    z = torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, xw[:, d:2 * d], yw[:, d:2 * d], case.p)
    z.backward(dev(case.g16, gpu))
    assert torch.equal(z.detach(), packed["z"]) and torch.equal(xw.grad[:, d:2 * d], packed["dx"]) and torch.equal(yw.grad[:, d:2 * d], packed["dy"])
    assert not xw.grad[:, :d].any() and not yw.grad[:, 2 * d:].any()


@BOTH
def test_a_nan_row_of_y_poisons_exactly_the_rows_that_reference_it(gpu, dtype):
    case = c16.width_case(34, dtype)
    j = int(case.col[case.rowptr[2]])                     # a column some rows reference
    y = case.y16.clone()
    y[j, 5] = float("nan")
    got = run_cabi(case, gpu, y=dev(y, gpu))
    hit = np.zeros(case.m, bool)
    hit[case.ref["row"][case.col == j]] = True
    assert hit.any() and (~hit & case.live).any()
    z, lse, dx = (c16.as_array(got[name]) for name in ("z", "lse", "dx"))
    assert np.all(np.isnan(z[hit])) and np.all(np.isnan(lse[hit])) and np.all(np.isnan(dx[hit]))
    assert not np.isnan(z[~hit]).any() and not np.isnan(dx[~hit]).any() and not np.isnan(lse[~hit]).any()
    for name, v in (("z", z), ("dx", dx)):
        frac = c16.worst(v[~hit], case.ref[name][~hit], case.bound[name][~hit])
        print(f"attention16 error/bound nan-row others {c16.dtype_name(dtype)}: {name}={frac:.4f}")
        assert frac <= 1.0
    keep = ~hit & case.live
    assert c16.worst(lse[keep], case.ref["lse"][keep], case.bound["lse"][keep]) <= 1.0


def test_refusals_return_the_documented_codes_and_leave_the_outputs_untouched(gpu):
    from isplib_amd import cabi
    L = cabi.lib()
    case = c16.width_case(16, BF)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    m, nnz = case.m, col.numel()
    wide = torch.zeros(m, 520, device=gpu, dtype=BF)
    outs = {name: torch.full((m, 520), float("nan"), device=gpu, dtype=BF) for name in ("z", "dx", "dy")}
    vec = {name: torch.full((m,), float("nan"), device=gpu) for name in ("lse", "D")}
    lse_in, d_in = torch.zeros(m, device=gpu), torch.zeros(m, device=gpu)
    rp, cp = rowptr.data_ptr(), colptr.data_ptr()

    def call(code=cabi.DTYPE_BF16, k=16, ld=520, ldo=520, off=0):
        x = wide.data_ptr() + 2 * off
        fw = L.isplib_attention16_csr_hip(code, m, m, k, nnz, col.data_ptr(), rp, rp + 8, x, ld, x, ld, 1.0, outs["z"].data_ptr(), ldo,
                                          vec["lse"].data_ptr(), None)
        e_fw = cabi.last_error()
        rows = L.isplib_attention16_bw_rows_hip(code, m, m, k, nnz, col.data_ptr(), rp, rp + 8, x, ld, x, ld, 1.0, x, ld, lse_in.data_ptr(),
                                                outs["dx"].data_ptr(), ldo, vec["D"].data_ptr(), None)
        cols = L.isplib_attention16_bw_cols_hip(code, m, m, k, nnz, row_t.data_ptr(), cp, cp + 8, x, ld, x, ld, 1.0, x, ld, lse_in.data_ptr(),
                                                d_in.data_ptr(), outs["dy"].data_ptr(), ldo, None)
        return (fw, rows, cols), e_fw

    for what, kwargs, want in (("odd K", dict(k=15), cabi.NO_OPT_IMPL), ("K = 6", dict(k=6), cabi.NO_OPT_IMPL),
                               ("K = 514", dict(k=514), cabi.NO_OPT_IMPL), ("odd pitch", dict(ld=519), cabi.NO_OPT_IMPL),
                               ("odd output pitch", dict(ldo=519), cabi.NO_OPT_IMPL), ("a base offset by one element", dict(off=1), cabi.FAIL),
                               ("the fp32 dtype code", dict(code=0), cabi.FAIL), ("a pitch below K", dict(k=16, ldo=14), cabi.FAIL)):
        codes, message = call(**kwargs)
        assert codes == (want,) * 3, (what, codes)
        assert ("isplib_attention16_serves" in message) == (want == cabi.NO_OPT_IMPL), (what, message)
    torch.cuda.synchronize()
    for t in list(outs.values()) + list(vec.values()):
        assert torch.isnan(t).all()
    # nothing to do succeeds without a launch; a negative dimension and a null operand fail
    x = wide.data_ptr()
    args = lambda mm, k, xp: (cabi.DTYPE_BF16, mm, m, k, nnz, col.data_ptr(), rp, rp + 8, xp, 520, x, 520, 1.0, outs["z"].data_ptr(), 520,  # noqa: E731
                              vec["lse"].data_ptr(), None)
    assert L.isplib_attention16_csr_hip(*args(0, 16, None)) == cabi.SUCCESS and L.isplib_attention16_csr_hip(*args(m, 0, None)) == cabi.SUCCESS
    assert L.isplib_attention16_csr_hip(*args(-1, 16, x)) == cabi.FAIL
    assert L.isplib_attention16_csr_hip(*args(m, 16, None)) == cabi.FAIL and "null" in cabi.last_error()
    with pytest.raises(RuntimeError, match="attention_spmm16"):
        torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, wide[:, :16], wide[:, :16].to(FP), 1.0)
    with pytest.raises(RuntimeError, match="attention_spmm16"):
        torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, wide[:, :16].float(), wide[:, :16].float(), 1.0)
    with pytest.raises(RuntimeError, match="attention_spmm16"):
        torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, wide[:, :15], wide[:, :15], 1.0)
    torch.cuda.synchronize()
    assert torch.isnan(outs["z"]).all()


@BOTH
def test_plugin_routes(gpu, dtype, monkeypatch):
    """unset -> TypeError; convert -> the bits of the hand-written conversion; native -> the bits of the operator called directly, the
    gradients in the operands' dtype; native at odd K -> the conversion route's bits; mixed dtypes -> TypeError."""
    import isplib_amd
    case = c16.width_case(30, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    g = dev(case.g16, gpu)

    def leaves(cols=None):
        x, y = dev(case.x16, gpu), dev(case.y16, gpu)
        if cols is not None:
            x, y = x[:, :cols].contiguous(), y[:, :cols].contiguous()
        return x.requires_grad_(True), y.requires_grad_(True)

    def by_hand(x, y, gg, scale):
        z = isplib_amd.attention_matmul(adj, x.float(), y.float(), scale).to(dtype)
        z.backward(gg)
        return z.detach(), x.grad, y.grad

    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_ATTENTION", raising=False)
    x, y = leaves()
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.attention_matmul(adj, x, y)
    want = by_hand(*leaves(), g, case.p)

    monkeypatch.setenv("ISPLIB_HALF_ATTENTION", "convert")
    x, y = leaves()
    z = adj.attention_matmul(x, y, scale=case.p)
    z.backward(g)
    assert z.dtype == x.grad.dtype == y.grad.dtype == dtype
    assert torch.equal(z.detach(), want[0]) and torch.equal(x.grad, want[1]) and torch.equal(y.grad, want[2])

    monkeypatch.setenv("ISPLIB_HALF_ATTENTION", "native")
    xd, yd = leaves()
    zd = torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, xd, yd, case.p)
    zd.backward(g)
    x, y = leaves()
    z = adj.attention_matmul(x, y, scale=case.p)
    z.backward(g)
    assert z.dtype == x.grad.dtype == y.grad.dtype == dtype
    assert torch.equal(z.detach(), zd.detach()) and torch.equal(x.grad, xd.grad) and torch.equal(y.grad, yd.grad)
    held(case, dict(z=z, dx=x.grad, dy=y.grad), ("z", "dx", "dy"))
    with pytest.raises(TypeError, match="one dtype"):
        adj.attention_matmul(x.detach(), y.detach().to(FP if dtype == BF else BF))
    # ISPLIB_HALF=convert wins over native
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    x, y = leaves()
    assert torch.equal(adj.attention_matmul(x, y, scale=case.p).detach(), want[0])
    monkeypatch.delenv("ISPLIB_HALF")
    # odd K: outside the 16-bit domain, the conversion route's bits
    want_odd = by_hand(*leaves(29), g[:, :29].contiguous(), 0.2)
    x, y = leaves(29)
    z = adj.attention_matmul(x, y, scale=0.2)
    z.backward(g[:, :29].contiguous())
    assert torch.equal(z.detach(), want_odd[0]) and torch.equal(x.grad, want_odd[1]) and torch.equal(y.grad, want_odd[2])
    # y=None on the native route: x.grad receives both contributions
    x, _ = leaves()
    adj.attention_matmul(x, scale=case.p).backward(g)
    xs = dev(case.x16, gpu).requires_grad_(True)
    torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, xs, xs, case.p).backward(g)
    assert torch.equal(x.grad, xs.grad)
