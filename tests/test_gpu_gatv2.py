"""GATv2 attention aggregation on the GPU (isplib_amd/csrc/gatv2.hip): the C ABI wrappers, torch.ops.isplib.gatv2_spmm with its
autograd backward, and the plug-in surface, each held to the per-element bounds of tests/gatv2_ref.py against the fp64 reference
(inputs, references and bounds: tests/gatv2_cases.py, computed once per case).  The largest error / bound seen per output is printed
before every assertion; DESIGN.md 4.6f records it.
"""
import numpy as np
import pytest
import torch

from tests import gatv2_cases as cases
from tests import gatv2_ref as ref

pytestmark = pytest.mark.gpu

CABI_OUTPUTS = ("z", "lse", "dx", "D", "datt", "dy")
IDS = [f"h{h}d{d}" for h, d in cases.CONFIGS]


def dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def dev_graph(case, gpu):
    return dev(case.rowptr, gpu), dev(case.col, gpu)


def transposed(case, gpu):
    """colptr / row_t as SparseStorage caches them (the library's own csr2csc)."""
    import isplib_amd
    rowptr, col = dev_graph(case, gpu)
    st = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n)).storage
    return st.colptr(), st.row_t()


def held(case, got, names, what=""):
    """Print and assert error / bound <= 1 for the named outputs (tensors or arrays); returns the fractions."""
    live, frac = case.live, {}
    for name in names:
        v = got[name].detach().cpu().numpy() if isinstance(got[name], torch.Tensor) else np.asarray(got[name])
        if name == "lse":
            assert np.all(np.isneginf(v[~live])), "an empty row must have lse = -inf"
            frac[name] = ref.worst(v[live], case.ref["lse"][live], case.bound["lse"][live])
        else:
            frac[name] = ref.worst(v, case.ref[name], case.bound[name])
    print(f"gatv2 error/bound {case.name}{what}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def run_cabi(case, gpu, x=None, y=None, g=None, want_datt=True):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    x = dev(case.x, gpu) if x is None else x
    y = dev(case.y, gpu) if y is None else y
    g = dev(case.g, gpu) if g is None else g
    att = dev(case.att, gpu)
    z, lse = cabi.gatv2(rowptr, col, x, y, att, case.heads, case.ns)
    dx, D, datt = cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, z, lse, case.heads, case.ns, want_datt=want_datt)
    colptr, row_t = transposed(case, gpu)
    dy = cabi.gatv2_bw_cols(colptr, row_t, x, y, att, g, lse, D, case.heads, case.ns)
    return dict(z=z, lse=lse, dx=dx, D=D, datt=datt, dy=dy)


def check_cabi(case, gpu):
    got = run_cabi(case, gpu)
    held(case, got, CABI_OUTPUTS)
    empty = ~case.live
    for name in ("z", "dx", "D"):
        assert np.all(got[name].cpu().numpy()[empty] == 0), name
    unreferenced = np.bincount(case.col, minlength=case.n) == 0
    assert unreferenced.any() and np.all(got["dy"].cpu().numpy()[unreferenced] == 0)
    return got


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_cabi_entries_at_every_configuration(gpu, heads, d):
    """Every LPR instantiation, first, last and ragged; heads of one lane up to a whole chunk; both chunks in one head and in two."""
    check_cabi(cases.config_case(heads, d), gpu)


@pytest.mark.parametrize("case", cases.slope_cases(), ids=lambda c: c.name)
def test_cabi_entries_at_every_slope(gpu, case):
    check_cabi(case, gpu)


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_operator_and_plugin_under_autograd(gpu, heads, d):
    """torch.ops.isplib.gatv2_spmm and gatv2_matmul / SparseTensor.gatv2_matmul give the same bits; a weighted storage too (stored
    values are not read); only the requested gradients are computed."""
    import isplib_amd
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    g = dev(case.g, gpu)
    x, y, att = (dev(a, gpu).requires_grad_(True) for a in (case.x, case.y, case.att))
    z = torch.ops.isplib.gatv2_spmm(rowptr, col, colptr, row_t, x, y, att, heads, case.ns)
    z.backward(g)
    held(case, dict(z=z, dx=x.grad, dy=y.grad, datt=att.grad), ("z", "dx", "dy", "datt"), " op")
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, torch.rand(col.numel(), device=gpu) + 0.5, (case.m, case.n))
    x2, y2, a2 = (dev(a, gpu).requires_grad_(True) for a in (case.x, case.y, case.att))
    z2 = isplib_amd.gatv2_matmul(adj, x2, a2, y2, heads=heads, negative_slope=case.ns)
    z2.backward(g)
    for a, b in ((z2, z), (x2.grad, x.grad), (y2.grad, y.grad), (a2.grad, att.grad)):
        assert torch.equal(a.detach(), b.detach())
    # only x asks: neither the datt instantiation nor the columns kernel runs, the others stay None
    x3, y3, a3 = dev(case.x, gpu).requires_grad_(True), dev(case.y, gpu), dev(case.att, gpu)
    adj.gatv2_matmul(x3, a3, y3, heads, case.ns).backward(g)
    assert y3.grad is None and a3.grad is None and torch.equal(x3.grad, x.grad)
    x4, y4, a4 = dev(case.x, gpu), dev(case.y, gpu).requires_grad_(True), dev(case.att, gpu)
    adj.gatv2_matmul(x4, a4, y4, heads, case.ns).backward(g)
    assert x4.grad is None and a4.grad is None and torch.equal(y4.grad, y.grad)
    if heads == 1:                                                          # att may be [d]
        a5 = dev(case.att[0], gpu).requires_grad_(True)
        z5 = adj.gatv2_matmul(dev(case.x, gpu), a5, dev(case.y, gpu))
        z5.backward(g)
        assert torch.equal(z5.detach(), z.detach()) and torch.equal(a5.grad, att.grad[0])


_shared = {}


def shared_case(heads, d):
    if (heads, d) not in _shared:
        base = cases.config_case(heads, d)
        _shared[heads, d] = cases.Case(f"shared-h{heads}d{d}", base.rowptr, base.col, np.array(base.x), np.array(base.x), np.array(base.att),
                                       np.array(base.g), heads, base.ns)
    return _shared[heads, d]


@pytest.mark.parametrize("heads,d", ((1, 47), (8, 16)))
def test_y_none_shares_one_tensor(gpu, heads, d):
    """y=None (share_weights): the one tensor's gradient receives dx and dy through ordinary autograd."""
    import isplib_amd
    case = shared_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    x, att = dev(case.x, gpu).requires_grad_(True), dev(case.att, gpu).requires_grad_(True)
    z = adj.gatv2_matmul(x, att, heads=heads, negative_slope=case.ns)
    z.backward(dev(case.g, gpu))
    held(case, dict(z=z, datt=att.grad), ("z", "datt"))
    frac = ref.worst(x.grad.cpu().numpy(), case.ref["dx"] + case.ref["dy"], case.bound["dx"] + case.bound["dy"])
    print(f"gatv2 error/bound {case.name}: dx+dy={frac:.4f}")
    assert frac <= 1.0


@pytest.mark.parametrize("heads,d", ((1, 47), (8, 8), (3, 128), (8, 64)))
def test_att_without_gradient_gives_the_same_bits(gpu, heads, d):
    """datt == NULL selects the instantiation without the LDS fold and the barrier: dx, D and dy are the same bits."""
    case = cases.config_case(heads, d)
    with_datt, without = run_cabi(case, gpu), run_cabi(case, gpu, want_datt=False)
    assert without["datt"] is None
    for name in ("dx", "D", "dy"):
        assert torch.equal(with_datt[name], without[name]), name
    x, y = dev(case.x, gpu).requires_grad_(True), dev(case.y, gpu).requires_grad_(True)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    torch.ops.isplib.gatv2_spmm(rowptr, col, colptr, row_t, x, y, dev(case.att, gpu), heads, case.ns).backward(dev(case.g, gpu))
    assert torch.equal(x.grad, with_datt["dx"]) and torch.equal(y.grad, with_datt["dy"])


def test_one_entry_rows_return_y_bit_for_bit(gpu):
    case = cases.single_case()
    got = run_cabi(case, gpu)
    z, lse = got["z"].cpu().numpy(), got["lse"].cpu().numpy()
    live = case.live
    want = np.zeros_like(case.y)
    want[live] = case.y[case.col]
    assert np.array_equal(z.view(np.uint32), want.view(np.uint32))
    # lse is the score: within delta s_e + 2 eps |s_e| of fp64
    s = case.ref["s"]
    slack = ref.ACC * (np.abs(case.att.astype(np.float64))[None] * np.abs(case.ref["v"])).sum(2) + 2.0 * ref.EPS * np.abs(s)
    assert np.all(np.isneginf(lse[~live])) and np.all(np.abs(lse[live] - s) <= slack)
    held(case, got, CABI_OUTPUTS)


def test_scores_spread_beyond_150(gpu):
    case = cases.large_case()
    got = run_cabi(case, gpu)
    for name in CABI_OUTPUTS:
        v = got[name].cpu().numpy()
        assert np.all(np.isfinite(v[case.live] if name == "lse" else v)), name
    held(case, got, CABI_OUTPUTS)


@pytest.mark.parametrize("heads,d", ((1, 41), (8, 8)))
def test_zero_att_gives_the_unit_weight_mean(gpu, heads, d):
    from isplib_amd import cabi
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    x, y = dev(case.x, gpu), dev(case.y, gpu)
    z, lse = cabi.gatv2(rowptr, col, x, y, torch.zeros(heads, d, device=gpu), heads, case.ns)
    mean, _ = cabi.spmm(rowptr, col, None, y, "mean")
    zero = cases.Case(f"zero-h{heads}d{d}", case.rowptr, case.col, np.array(case.x), np.array(case.y), np.zeros_like(case.att),
                      np.array(case.g), heads, case.ns)
    frac = ref.worst(z.cpu().numpy(), mean.cpu().numpy().astype(np.float64), zero.bound["z"])
    print(f"gatv2 error/bound zero att vs mean h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    live = zero.live
    assert np.allclose(zero.ref["lse"][live], np.log(np.diff(case.rowptr)[live])[:, None], rtol=1e-12)   # lse = log deg
    assert ref.worst(lse.cpu().numpy()[live], zero.ref["lse"][live], zero.bound["lse"][live]) <= 1.0


@pytest.mark.parametrize("heads,d", ((1, 41), (8, 8), (3, 128)))
def test_pitched_offset_and_column_block_views(gpu, heads, d):
    """x, y and g with ld > K and a base offset by one float, and as the LAST column block of a wider tensor (its last row ends with
    the allocation: the descriptor's extent), go in without a copy and give the bits of the packed operands."""
    import isplib_amd
    case = cases.config_case(heads, d)
    k = case.k
    packed = run_cabi(case, gpu)

    def pitched(a, pad, off):
        buf = torch.full((a.shape[0] * (k + pad) + off + 8,), float("nan"), device=gpu)
        view = buf[off:off + a.shape[0] * (k + pad)].view(a.shape[0], k + pad)[:, :k]
        view.copy_(dev(a, gpu))
        assert view.stride(0) == k + pad and view.data_ptr() % 16 == (4 * off) % 16
        return view

    got = run_cabi(case, gpu, x=pitched(case.x, 3, 1), y=pitched(case.y, 5, 1), g=pitched(case.g, 1, 1))
    for name in CABI_OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    blocks = 3
    wide = {n: torch.randn(case.m, blocks * k, device=gpu) for n in "xyg"}
    for b in (1, blocks - 1):
        for n, a in (("x", case.x), ("y", case.y), ("g", case.g)):
            wide[n][:, b * k:(b + 1) * k] = dev(a, gpu)
        view = {n: wide[n][:, b * k:(b + 1) * k] for n in "xyg"}
        assert not view["y"].is_contiguous()
        got = run_cabi(case, gpu, x=view["x"], y=view["y"], g=view["g"])
        for name in CABI_OUTPUTS:
            assert torch.equal(got[name], packed[name]), (b, name)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    xw, yw = wide["x"].clone().requires_grad_(True), wide["y"].clone().requires_grad_(True)
    b = blocks - 1
    z = adj.gatv2_matmul(xw[:, b * k:(b + 1) * k], dev(case.att, gpu), yw[:, b * k:(b + 1) * k], heads, case.ns)
    z.backward(wide["g"][:, b * k:(b + 1) * k])
    assert torch.equal(z.detach(), packed["z"]) and torch.equal(yw.grad[:, b * k:(b + 1) * k], packed["dy"]) and not yw.grad[:, :b * k].any()
    assert torch.equal(xw.grad[:, b * k:(b + 1) * k], packed["dx"]) and not xw.grad[:, :b * k].any()


@pytest.mark.parametrize("heads,d", ((1, 3), (5, 8), (1, 512), (8, 64)))
def test_outputs_are_write_only_and_launches_repeat(gpu, heads, d):
    """NaN-filled, over-allocated outputs and workspace, launched twice: every element is written, nothing past the end, equal bits --
    datt included."""
    from isplib_amd import cabi
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    x, y, att, g = dev(case.x, gpu), dev(case.y, gpu), dev(case.att, gpu), dev(case.g, gpu)
    m, n, k, pad, H, ns = case.m, case.n, case.k, 64, heads, case.ns

    def fresh(rows, cols):
        buf = torch.full((rows * cols + pad,), float("nan"), device=gpu)
        return buf, buf[:rows * cols].view(rows, cols)

    need = cabi.gatv2_bw_rows_workspace_bytes(m, k)
    runs = []
    for _ in range(2):
        b = {name: fresh(*shape) for name, shape in (("z", (m, k)), ("lse", (m, H)), ("dx", (m, k)), ("D", (m, H)), ("datt", (H, d)),
                                                     ("dy", (n, k)))}
        work = torch.full((need // 4 + pad,), float("nan"), device=gpu).view(torch.uint8)
        cabi.gatv2(rowptr, col, x, y, att, H, ns, out=(b["z"][1], b["lse"][1]), check=False)
        cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, b["z"][1], b["lse"][1], H, ns, out=(b["dx"][1], b["D"][1], b["datt"][1]),
                           workspace=work[:need], check=False)
        cabi.gatv2_bw_cols(colptr, row_t, x, y, att, g, b["lse"][1], b["D"][1], H, ns, out=b["dy"][1], check=False)
        for name, (buf, view) in b.items():
            assert not torch.isnan(view).any(), name
            assert torch.isnan(buf[view.numel():]).all(), name
        assert torch.isnan(work[need:].view(torch.float32)).all()           # nothing past the queried size
        runs.append({name: view.clone() for name, (_, view) in b.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    # pitched outputs: nothing is written between the rows
    buf = torch.full((m, k + 3), float("nan"), device=gpu)
    lse = torch.empty(m, H, device=gpu)
    cabi.gatv2(rowptr, col, x, y, att, H, ns, out=(buf[:, :k], lse))
    assert torch.equal(buf[:, :k], runs[0]["z"]) and torch.isnan(buf[:, k:]).all()
    buf = torch.full((m, k + 3), float("nan"), device=gpu)
    cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, runs[0]["z"], runs[0]["lse"], H, ns, want_datt=False, out=(buf[:, :k], torch.empty(m, H, device=gpu), None))
    assert torch.equal(buf[:, :k], runs[0]["dx"]) and torch.isnan(buf[:, k:]).all()
    buf = torch.full((n, k + 3), float("nan"), device=gpu)
    cabi.gatv2_bw_cols(colptr, row_t, x, y, att, g, runs[0]["lse"], runs[0]["D"], H, ns, out=buf[:, :k])
    assert torch.equal(buf[:, :k], runs[0]["dy"]) and torch.isnan(buf[:, k:]).all()


@pytest.mark.parametrize("heads,d", ((8, 8), (2, 256), (1, 47)))
def test_a_nan_in_y_poisons_exactly_its_head_of_the_rows_that_reference_it(gpu, heads, d):
    """Forward only: y[j, c] = NaN makes the head of c NaN in z and lse of the rows referencing j, and nothing else."""
    from isplib_amd import cabi
    case = cases.config_case(heads, d)
    j = int(case.col[case.rowptr[2]])                     # a column some rows reference
    hit = np.zeros(case.m, bool)
    hit[case.ref["row"][case.col == j]] = True
    assert hit.any() and (~hit & case.live).any()
    h = heads - 1
    y = np.array(case.y)
    y[j, h * d + d // 2] = np.nan
    rowptr, col = dev_graph(case, gpu)
    z, lse = cabi.gatv2(rowptr, col, dev(case.x, gpu), dev(y, gpu), dev(case.att, gpu), heads, case.ns)
    z, lse = ref.per_head(z.cpu().numpy(), heads), lse.cpu().numpy()
    want, bound = ref.per_head(case.ref["z"], heads), ref.per_head(case.bound["z"], heads)
    assert np.all(np.isnan(z[hit, h])) and np.all(np.isnan(lse[hit, h]))
    clean = np.ones((case.m, heads), bool)
    clean[hit, h] = False
    frac = ref.worst(z[clean], want[clean], bound[clean])
    print(f"gatv2 error/bound nan in y, everything else h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    ok = clean & case.live[:, None]
    assert ref.worst(lse[ok], case.ref["lse"][ok], case.bound["lse"][ok]) <= 1.0


_prefix = {}


def prefix_case(rows, heads, d):
    """The first `rows` rows of the graph (all columns kept): M no multiple of the rows kernel's WAVES, or smaller than it."""
    if (rows, heads, d) not in _prefix:
        base = cases.config_case(heads, d)
        rowptr = np.array(base.rowptr[:rows + 1])
        col = np.array(base.col[:rowptr[-1]])
        _prefix[rows, heads, d] = cases.Case(f"first{rows}-h{heads}d{d}", rowptr, col, np.array(base.x[:rows]), np.array(base.y), np.array(base.att),
                                             np.array(base.g[:rows]), heads, base.ns)
    return _prefix[rows, heads, d]


@pytest.mark.parametrize("rows", (1, 3, 5, 7, 13, 99))
@pytest.mark.parametrize("heads,d", ((1, 47), (8, 64)))
def test_rows_that_meet_the_barrier_with_nothing_to_do(gpu, rows, heads, d):
    """M smaller than the block's WAVES and M no multiple of it, with datt asked: the waves past M contribute zeros."""
    case = prefix_case(rows, heads, d)
    assert case.m == rows and case.n == cases.N
    got = run_cabi(case, gpu)
    held(case, got, CABI_OUTPUTS)
    again = run_cabi(case, gpu)
    assert torch.equal(got["datt"], again["datt"])


def test_error_paths_raise_before_a_launch(gpu):
    import isplib_amd
    from isplib_amd import cabi
    case = cases.config_case(2, 4)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    x, y, att = dev(case.x, gpu), dev(case.y, gpu), dev(case.att, gpu)
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gatv2_matmul(x.cpu(), att, y, 2)
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gatv2_matmul(x, att.cpu(), y, 2)
    with pytest.raises(ValueError, match="2-D"):
        adj.gatv2_matmul(x[0], att, y, 2)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32"):
            adj.gatv2_matmul(x.to(dt), att.to(dt), y.to(dt), 2)
    with pytest.raises(ValueError, match="one row per column"):
        adj.gatv2_matmul(x, att, y[:-1], 2)
    with pytest.raises(ValueError, match="one row per row"):
        adj.gatv2_matmul(x[:-1], att, y, 2)
    with pytest.raises(ValueError, match=r"`att` must be \[2, 4\]"):
        adj.gatv2_matmul(x, att[:, :2], y, 2)
    with pytest.raises(ValueError, match="power of two"):
        adj.gatv2_matmul(torch.zeros(case.m, 12, device=gpu), torch.zeros(2, 6, device=gpu), torch.zeros(case.m, 12, device=gpu), 2)
    with pytest.raises(ValueError, match="512"):
        adj.gatv2_matmul(torch.zeros(case.m, 1024, device=gpu), torch.zeros(2, 512, device=gpu), torch.zeros(case.m, 1024, device=gpu), 2)
    # the wrappers: structure checks that read the device
    with pytest.raises(ValueError, match="ascend"):
        cabi.gatv2(torch.flip(rowptr, (0,)), col, x, y, att, 2)
    bad = col.clone()
    bad[3] = case.m
    with pytest.raises(ValueError, match=r"lie in \[0, 200\)"):
        cabi.gatv2(rowptr, bad, x, y, att, 2)
    with pytest.raises(ValueError, match="workspace"):
        z, lse = cabi.gatv2(rowptr, col, x, y, att, 2)
        cabi.gatv2_bw_rows(rowptr, col, x, y, att, x, z, lse, 2, workspace=torch.empty(256, dtype=torch.uint8, device=gpu))
    # the operator: every shape before a launch
    for args in ((x, y[:-1], att, 2), (x[:-1], y, att, 2), (x, y, att[:, :2], 2), (x, y, att, 3),
                 (torch.zeros(case.m, 12, device=gpu), torch.zeros(case.m, 12, device=gpu), torch.zeros(2, 6, device=gpu), 2), (x, y, att.cpu(), 2)):
        with pytest.raises(RuntimeError, match="gatv2_spmm|GPU tensor"):
            torch.ops.isplib.gatv2_spmm(rowptr, col, rowptr, col, *args, 0.2)
    with pytest.raises(RuntimeError, match="gatv2_spmm"):
        torch.ops.isplib.gatv2_spmm(rowptr[:-1], col, rowptr, col, x, y, att, 2, 0.2)
    # the entries themselves: outside the domain NO_OPT_IMPL, bad arguments FAIL, nothing to do SUCCESS -- all without a launch
    L = cabi.lib()
    rp, z, lse = rowptr.data_ptr(), torch.empty(case.m, 1024, device=gpu), torch.empty(case.m, 128, device=gpu)
    big = torch.zeros(case.m, 1024, device=gpu)
    args = lambda m, k, ldy, heads, xp: (m, case.m, k, col.numel(), col.data_ptr(), rp, rp + 8, xp, 1024, big.data_ptr(), ldy, big.data_ptr(),  # noqa: E731
                                         heads, 0.2, z.data_ptr(), 1024, lse.data_ptr(), None)
    xp = big.data_ptr()
    assert L.isplib_gatv2_csr_hip(*args(case.m, 516, 516, 1, xp)) == cabi.NO_OPT_IMPL and "isplib_gatv2_serves" in cabi.last_error()
    assert L.isplib_gatv2_csr_hip(*args(case.m, 12, 12, 2, xp)) == cabi.NO_OPT_IMPL                # d = 6
    assert L.isplib_gatv2_csr_hip(*args(case.m, 4, 4, 2, xp)) == cabi.NO_OPT_IMPL                  # d = 2
    assert L.isplib_gatv2_csr_hip(*args(case.m, 8, 7, 2, xp)) == cabi.NO_OPT_IMPL                  # ldy < k
    assert L.isplib_gatv2_csr_hip(*args(case.m, 8, 8, 0, xp)) == cabi.NO_OPT_IMPL
    assert L.isplib_gatv2_csr_hip(*args(case.m, 9, 9, 2, xp)) == cabi.FAIL                         # k is no multiple of heads
    assert L.isplib_gatv2_csr_hip(*args(-1, 8, 8, 2, xp)) == cabi.FAIL
    assert L.isplib_gatv2_csr_hip(*args(case.m, 8, 8, 2, None)) == cabi.FAIL and "null" in cabi.last_error()
    assert L.isplib_gatv2_csr_hip(*args(0, 8, 8, 2, None)) == cabi.SUCCESS and L.isplib_gatv2_csr_hip(*args(case.m, 0, 8, 2, None)) == cabi.SUCCESS
    # the rows entry: datt without a workspace is refused, datt == NULL needs none
    g, D, dx, datt = big, torch.empty(case.m, 2, device=gpu), torch.empty(case.m, 8, device=gpu), torch.empty(8, device=gpu)
    rows = lambda dp, wp, wb: (case.m, case.m, 8, col.numel(), col.data_ptr(), rp, rp + 8, xp, 1024, big.data_ptr(), 1024, big.data_ptr(), 2, 0.2,  # noqa: E731
                               g.data_ptr(), 1024, z.data_ptr(), 1024, lse.data_ptr(), dx.data_ptr(), 8, D.data_ptr(), dp, wp, wb, None)
    assert L.isplib_gatv2_bw_rows_hip(*rows(datt.data_ptr(), None, 0)) == cabi.NOT_ENOUGH_MEM
    work = torch.empty(cabi.gatv2_bw_rows_workspace_bytes(case.m, 8), dtype=torch.uint8, device=gpu)
    assert L.isplib_gatv2_bw_rows_hip(*rows(datt.data_ptr(), work.data_ptr(), work.numel() - 1)) == cabi.NOT_ENOUGH_MEM
    torch.cuda.synchronize()
