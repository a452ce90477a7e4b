"""Row-softmax attention aggregation on the GPU (isplib_amd/csrc/attention.hip): the C ABI wrappers, torch.ops.isplib.attention_spmm
with its autograd backward, and the plug-in surface, each held to the per-element bounds of tests/attention_ref.py against the fp64
reference (inputs, references and bounds: tests/attention_cases.py, computed once per case).  The largest error / bound seen per
output is printed before every assertion; DESIGN.md 4.6b records it.
"""
import numpy as np
import pytest
import torch

from tests import attention_cases as cases
from tests import attention_ref as ref

pytestmark = pytest.mark.gpu


def dev_graph(case, gpu):
    return torch.from_numpy(np.array(case.rowptr)).to(gpu), torch.from_numpy(np.array(case.col)).to(gpu)


def dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def transposed(case, gpu):
    """colptr / row_t as SparseStorage caches them (the library's own csr2csc)."""
    import isplib_amd
    rowptr, col = dev_graph(case, gpu)
    st = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.y.shape[0])).storage
    return st.colptr(), st.row_t()


def held(case, got, names):
    """Print and assert error / bound <= 1 for the named outputs (tensors or arrays); returns the fractions."""
    live, frac = case.live, {}
    for name in names:
        v = got[name].detach().cpu().numpy() if isinstance(got[name], torch.Tensor) else np.asarray(got[name])
        if name == "lse":
            assert np.all(np.isneginf(v[~live])), "an empty row must have lse = -inf"
            frac[name] = ref.worst(v[live], case.ref["lse"][live], case.bound["lse"][live])
        elif name == "D":
            continue
        else:
            frac[name] = ref.worst(v, case.ref[name], case.bound[name])
    print(f"attention error/bound {case.name}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def run_cabi(case, gpu, x=None, y=None, g=None):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    x = dev(case.x, gpu) if x is None else x
    y = dev(case.y, gpu) if y is None else y
    g = dev(case.g, gpu) if g is None else g
    z, lse = cabi.attention(rowptr, col, x, y, case.p)
    dx, D = cabi.attention_bw_rows(rowptr, col, x, y, g, z, lse, case.p)
    colptr, row_t = transposed(case, gpu)
    dy = cabi.attention_bw_cols(colptr, row_t, x, y, g, lse, D, case.p)
    return dict(z=z, lse=lse, dx=dx, dy=dy, D=D)


@pytest.mark.parametrize("k", cases.WIDTHS)
def test_cabi_entries_at_every_width(gpu, k):
    """First, last and ragged width of every instantiation; the graph holds every row length and column in-degree on a loop edge,
    duplicates and unsorted rows."""
    case = cases.width_case(k)
    got = run_cabi(case, gpu)
    held(case, got, ("z", "lse", "dx", "dy"))
    empty = ~case.live
    assert np.all(got["z"].cpu().numpy()[empty] == 0) and np.all(got["dx"].cpu().numpy()[empty] == 0) and np.all(got["D"].cpu().numpy()[empty] == 0)
    unreferenced = np.bincount(case.col, minlength=case.y.shape[0]) == 0
    assert unreferenced.any() and np.all(got["dy"].cpu().numpy()[unreferenced] == 0)


@pytest.mark.parametrize("k", cases.WIDTHS)
def test_operator_and_autograd_at_every_width(gpu, k):
    case = cases.width_case(k)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    x, y = dev(case.x, gpu).requires_grad_(True), dev(case.y, gpu).requires_grad_(True)
    z = torch.ops.isplib.attention_spmm(rowptr, col, colptr, row_t, x, y, case.p)
    z.backward(dev(case.g, gpu))
    held(case, dict(z=z, dx=x.grad, dy=y.grad), ("z", "dx", "dy"))


@pytest.mark.parametrize("k", cases.WIDTHS)
def test_plugin_surface(gpu, k):
    """attention_matmul and SparseTensor.attention_matmul; scale=None is 1 / sqrt(K); a weighted storage gives the bits of the
    unweighted one (stored values are not read); only the requested gradients are computed."""
    import isplib_amd
    case = cases.width_case(k)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    w = torch.rand(col.numel(), device=gpu) + 0.5
    adj_w = isplib_amd.SparseTensor.from_csr(rowptr, col, w, (case.m, case.m))
    x, y = dev(case.x, gpu).requires_grad_(True), dev(case.y, gpu).requires_grad_(True)
    z = isplib_amd.attention_matmul(adj, x, y)
    z.backward(dev(case.g, gpu))
    held(case, dict(z=z, dx=x.grad, dy=y.grad), ("z", "dx", "dy"))
    zw = adj_w.attention_matmul(x.detach(), y.detach(), scale=case.p)
    assert torch.equal(zw, z.detach()) and not zw.requires_grad
    # only x asks: y.grad stays None and the result for x is the same bits
    x2, y2 = dev(case.x, gpu).requires_grad_(True), dev(case.y, gpu)
    isplib_amd.attention_matmul(adj, x2, y2).backward(dev(case.g, gpu))
    assert y2.grad is None and torch.equal(x2.grad, x.grad)
    x3, y3 = dev(case.x, gpu), dev(case.y, gpu).requires_grad_(True)
    isplib_amd.attention_matmul(adj, x3, y3).backward(dev(case.g, gpu))
    assert x3.grad is None and torch.equal(y3.grad, y.grad)


@pytest.mark.parametrize("k", (4, 129))
def test_self_attention_form(gpu, k):
    """y=None means y = x: x.grad receives both contributions."""
    import isplib_amd
    base = cases.width_case(k)
    case = self_case(k)
    rowptr, col = dev_graph(base, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (base.m, base.m))
    x = dev(case.x, gpu).requires_grad_(True)
    z = adj.attention_matmul(x)
    z.backward(dev(case.g, gpu))
    got, want, bound = x.grad.cpu().numpy(), case.ref["dx"] + case.ref["dy"], case.bound["dx"] + case.bound["dy"]
    frac = ref.worst(got, want, bound)
    print(f"attention error/bound self{k}: z={ref.worst(z.detach().cpu().numpy(), case.ref['z'], case.bound['z']):.4f} dx+dy={frac:.4f}")
    assert ref.worst(z.detach().cpu().numpy(), case.ref["z"], case.bound["z"]) <= 1.0 and frac <= 1.0


_self_cases = {}


def self_case(k):
    if k not in _self_cases:
        base = cases.width_case(k)
        _self_cases[k] = cases.Case(f"self{k}", base.rowptr, base.col, np.array(base.x), np.array(base.x), np.array(base.g), base.p)
        assert _self_cases[k].bound["rho"].max() <= ref.RHO_MAX
    return _self_cases[k]


def test_one_entry_rows_return_y_bit_for_bit(gpu):
    """Whatever the score, |s| near 1e4 included: exp of the raw score would be Inf or 0 there."""
    case = cases.single_case()
    got = run_cabi(case, gpu)
    z, lse = got["z"].cpu().numpy(), got["lse"].cpu().numpy()
    live = case.live
    want = np.zeros_like(case.y)
    want[live] = case.y[case.col]
    assert np.array_equal(z.view(np.uint32), want.view(np.uint32))
    assert np.all(np.isneginf(lse[~live])) and np.all(np.abs(lse[live] - case.ref["s"]) <= 1e-5 * np.abs(case.ref["s"]) + 1e-30)
    # a = 1 and t = D exactly in exact arithmetic: both gradients are rounding noise of t - D, far inside the bounds
    held(case, got, ("dx", "dy"))


def test_scores_spread_over_200(gpu):
    case = cases.large_case()
    got = run_cabi(case, gpu)
    for name in ("z", "lse", "dx", "dy"):
        v = got[name].cpu().numpy()
        assert np.all(np.isfinite(v[case.live] if v.ndim == 1 and name == "lse" else v)), name
    held(case, got, ("z", "lse", "dx", "dy"))


def test_zero_queries_give_the_unit_weight_mean(gpu):
    from isplib_amd import cabi
    case = cases.width_case(65)
    rowptr, col = dev_graph(case, gpu)
    y = dev(case.y, gpu)
    z, lse = cabi.attention(rowptr, col, torch.zeros_like(dev(case.x, gpu)), y, case.p)
    mean, _ = cabi.spmm(rowptr, col, None, y, "mean")
    zero = cases.Case("zero65", case.rowptr, case.col, np.zeros_like(case.x), np.array(case.y), np.array(case.g), case.p)
    frac = ref.worst(z.cpu().numpy(), mean.cpu().numpy().astype(np.float64), zero.bound["z"])
    print(f"attention error/bound zero-x vs mean: z={frac:.4f}")
    assert frac <= 1.0
    live = zero.live
    assert np.allclose(zero.ref["lse"][live], np.log(np.diff(case.rowptr)[live]), rtol=1e-12)          # lse_i = log deg_i
    assert ref.worst(lse.cpu().numpy()[live], zero.ref["lse"][live], zero.bound["lse"][live]) <= 1.0


@pytest.mark.parametrize("k", (33, 64))
def test_pitched_offset_and_head_views(gpu, k):
    """Operands with ld > k, a base offset by one float, and heads of one [N, H*d] tensor go in without a copy and give the bits of
    the packed operands."""
    case = cases.width_case(k)
    packed = run_cabi(case, gpu)

    def pitched(a, pad, off):
        buf = torch.full((a.shape[0] * (k + pad) + off + 8,), float("nan"), device=gpu)
        view = buf[off:off + a.shape[0] * (k + pad)].view(a.shape[0], k + pad)[:, :k]
        view.copy_(dev(a, gpu))
        assert view.stride(0) == k + pad and view.data_ptr() % 16 == (4 * off) % 16
        return view

    got = run_cabi(case, gpu, pitched(case.x, 3, 1), pitched(case.y, 5, 1), pitched(case.g, 1, 1))
    for name in ("z", "lse", "dx", "dy"):
        assert torch.equal(got[name], packed[name]), name
    # heads: three heads of width k in one tensor; head 1 and the last head (its last row ends with the allocation)
    heads = 3
    wide = {n: torch.randn(case.m, heads * k, device=gpu) for n in "xyg"}
    for h in (1, heads - 1):
        for n, a in (("x", case.x), ("y", case.y), ("g", case.g)):
            wide[n][:, h * k:(h + 1) * k] = dev(a, gpu)
        view = {n: wide[n][:, h * k:(h + 1) * k] for n in "xyg"}
        assert not view["y"].is_contiguous()
        got = run_cabi(case, gpu, view["x"], view["y"], view["g"])
        for name in ("z", "lse", "dx", "dy"):
            assert torch.equal(got[name], packed[name]), (h, name)
    import isplib_amd
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    xw, yw = wide["x"].clone().requires_grad_(True), wide["y"].clone().requires_grad_(True)
    h = heads - 1
    z = adj.attention_matmul(xw[:, h * k:(h + 1) * k], yw[:, h * k:(h + 1) * k], scale=case.p)
    z.backward(dev(case.g, gpu))
    assert torch.equal(z.detach(), packed["z"]) and torch.equal(xw.grad[:, h * k:(h + 1) * k], packed["dx"])
    assert torch.equal(yw.grad[:, h * k:(h + 1) * k], packed["dy"]) and not xw.grad[:, :h * k].any()


@pytest.mark.parametrize("k", (3, 129, 512))
def test_outputs_are_write_only_and_launches_repeat(gpu, k):
    """NaN-filled, over-allocated outputs, launched twice: every element is written, nothing past the end, equal bits."""
    from isplib_amd import cabi
    case = cases.width_case(k)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    x, y, g = dev(case.x, gpu), dev(case.y, gpu), dev(case.g, gpu)
    m, n, pad = case.m, case.y.shape[0], 64

    def fresh(rows, cols=None):
        count = rows * (cols or 1)
        buf = torch.full((count + pad,), float("nan"), device=gpu)
        return buf, (buf[:count].view(rows, cols) if cols else buf[:count])

    runs = []
    for _ in range(2):
        bufs = {name: fresh(*shape) for name, shape in (("z", (m, k)), ("lse", (m,)), ("dx", (m, k)), ("D", (m,)), ("dy", (n, k)))}
        cabi.attention(rowptr, col, x, y, case.p, out=(bufs["z"][1], bufs["lse"][1]), check=False)
        cabi.attention_bw_rows(rowptr, col, x, y, g, bufs["z"][1], bufs["lse"][1], case.p, out=(bufs["dx"][1], bufs["D"][1]), check=False)
        cabi.attention_bw_cols(colptr, row_t, x, y, g, bufs["lse"][1], bufs["D"][1], case.p, out=bufs["dy"][1], check=False)
        for name, (buf, view) in bufs.items():
            assert not torch.isnan(view).any(), name
            assert torch.isnan(buf[view.numel():]).all(), name
        runs.append({name: view.clone() for name, (_, view) in bufs.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    # pitched outputs: nothing is written between the rows
    buf = torch.full((m, k + 3), float("nan"), device=gpu)
    lse = torch.empty(m, device=gpu)
    cabi.attention(rowptr, col, x, y, case.p, out=(buf[:, :k], lse))
    assert torch.equal(buf[:, :k], runs[0]["z"]) and torch.isnan(buf[:, k:]).all()


def test_a_nan_row_of_y_poisons_exactly_the_rows_that_reference_it(gpu):
    case = cases.width_case(33)
    j = int(case.col[case.rowptr[2]])                     # a column some rows reference
    y = np.array(case.y)
    y[j, 5] = np.nan
    got = run_cabi(case, gpu, y=dev(y, gpu))
    row = case.ref["row"]
    hit = np.zeros(case.m, bool)
    hit[row[case.col == j]] = True
    assert hit.any() and (~hit & case.live).any()
    z, lse, dx = got["z"].cpu().numpy(), got["lse"].cpu().numpy(), got["dx"].cpu().numpy()
    assert np.all(np.isnan(z[hit])) and np.all(np.isnan(lse[hit])) and np.all(np.isnan(dx[hit]))
    for name, v in (("z", z), ("dx", dx)):
        frac = ref.worst(v[~hit], case.ref[name][~hit], case.bound[name][~hit])
        print(f"attention error/bound nan-row others: {name}={frac:.4f}")
        assert frac <= 1.0
    assert ref.worst(lse[~hit & case.live], case.ref["lse"][~hit & case.live], case.bound["lse"][~hit & case.live]) <= 1.0
    # an infinite score does the same: +inf in one row of x
    x = np.array(case.x)
    i = int(np.argmax(np.diff(case.rowptr) == 9))
    x[i, 0] = np.inf
    z = run_cabi(case, gpu, x=dev(x, gpu))["z"].cpu().numpy()
    others = np.arange(case.m) != i
    assert np.all(np.isnan(z[i])) and ref.worst(z[others], case.ref["z"][others], case.bound["z"][others]) <= 1.0


def test_error_paths_raise_before_a_launch(gpu):
    import isplib_amd
    from isplib_amd import cabi
    case = cases.width_case(4)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    x, y = dev(case.x, gpu), dev(case.y, gpu)
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.attention_matmul(x.cpu(), y)
    with pytest.raises(ValueError, match="2-D"):
        adj.attention_matmul(x[0], y)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32"):
            adj.attention_matmul(x.to(dt), y.to(dt))
    with pytest.raises(ValueError, match="one row per row"):
        adj.attention_matmul(x[:-1], y)
    with pytest.raises(ValueError, match="one row per column"):
        adj.attention_matmul(x, y[:-1])
    with pytest.raises(ValueError, match="512"):
        adj.attention_matmul(torch.zeros(case.m, 513, device=gpu), torch.zeros(case.m, 513, device=gpu))
    rect = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m + 1))
    with pytest.raises(ValueError, match="square"):
        rect.attention_matmul(x)
    # the wrappers: structure checks that read the device
    with pytest.raises(ValueError, match="ascend"):
        cabi.attention(torch.flip(rowptr, (0,)), col, x, y)
    bad = col.clone()
    bad[3] = case.m
    with pytest.raises(ValueError, match=r"lie in \[0, 200\)"):
        cabi.attention(rowptr, bad, x, y)
    with pytest.raises(RuntimeError, match="attention_spmm"):
        torch.ops.isplib.attention_spmm(rowptr, col, rowptr, col, x[:-1], y, 1.0)
    # the entries themselves: outside the domain NO_OPT_IMPL, bad arguments FAIL, nothing to do SUCCESS -- all without a launch
    L = cabi.lib()
    rp, z, lse = rowptr.data_ptr(), torch.empty_like(x), torch.empty(case.m, device=gpu)
    args = lambda m, k, ldy, xp: (m, case.m, k, col.numel(), col.data_ptr(), rp, rp + 8, xp, max(k, 4), y.data_ptr(), ldy, 1.0,  # noqa: E731
                                  z.data_ptr(), max(k, 4), lse.data_ptr(), None)
    assert L.isplib_attention_csr_hip(*args(case.m, 513, 513, x.data_ptr())) == cabi.NO_OPT_IMPL and "isplib_attention_serves" in cabi.last_error()
    assert L.isplib_attention_csr_hip(*args(case.m, 4, 3, x.data_ptr())) == cabi.NO_OPT_IMPL
    assert L.isplib_attention_csr_hip(*args(-1, 4, 4, x.data_ptr())) == cabi.FAIL
    assert L.isplib_attention_csr_hip(*args(case.m, 4, 4, None)) == cabi.FAIL and "null" in cabi.last_error()
    assert L.isplib_attention_csr_hip(*args(0, 4, 4, None)) == cabi.SUCCESS and L.isplib_attention_csr_hip(*args(case.m, 0, 4, None)) == cabi.SUCCESS
    torch.cuda.synchronize()
