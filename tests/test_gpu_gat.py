"""GAT attention aggregation on the GPU (isplib_amd/csrc/gat.hip): the C ABI wrappers, torch.ops.isplib.gat_spmm with its autograd
backward, and the plug-in surface, each held to the per-element bounds of tests/gat_ref.py against the fp64 reference (inputs,
references and bounds: tests/gat_cases.py, computed once per case).  The largest error / bound seen per output is printed before every
assertion; DESIGN.md 4.6d records it.
"""
import numpy as np
import pytest
import torch

from tests import gat_cases as cases
from tests import gat_ref as ref

pytestmark = pytest.mark.gpu

CABI_OUTPUTS = ("z", "lse", "dadst", "D", "dy", "dasrc")
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
    print(f"gat error/bound {case.name}{what}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def run_cabi(case, gpu, y=None, a_dst=None, a_src=None, g=None):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    y = dev(case.y, gpu) if y is None else y
    a_dst = dev(case.a_dst, gpu) if a_dst is None else a_dst
    a_src = dev(case.a_src, gpu) if a_src is None else a_src
    g = dev(case.g, gpu) if g is None else g
    z, lse = cabi.gat(rowptr, col, y, a_dst, a_src, case.heads, case.ns)
    dadst, D = cabi.gat_bw_rows(rowptr, col, y, a_dst, a_src, g, z, lse, case.heads, case.ns)
    colptr, row_t = transposed(case, gpu)
    dy, dasrc = cabi.gat_bw_cols(colptr, row_t, y, a_dst, a_src, g, lse, D, case.heads, case.ns)
    return dict(z=z, lse=lse, dadst=dadst, D=D, dy=dy, dasrc=dasrc)


def check_cabi(case, gpu):
    got = run_cabi(case, gpu)
    held(case, got, CABI_OUTPUTS)
    empty = ~case.live
    for name in ("z", "dadst", "D"):
        assert np.all(got[name].cpu().numpy()[empty] == 0), name
    unreferenced = np.bincount(case.col, minlength=case.n) == 0
    assert unreferenced.any() and np.all(got["dy"].cpu().numpy()[unreferenced] == 0) and np.all(got["dasrc"].cpu().numpy()[unreferenced] == 0)


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_cabi_entries_at_every_configuration(gpu, heads, d):
    """Every LPR instantiation, first, last and ragged; heads of one lane up to a whole chunk; both chunks in one head and in two."""
    check_cabi(cases.config_case(heads, d), gpu)


@pytest.mark.parametrize("case", cases.slope_cases(), ids=lambda c: c.name)
def test_cabi_entries_at_every_slope(gpu, case):
    check_cabi(case, gpu)


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_operator_and_plugin_under_autograd(gpu, heads, d):
    """torch.ops.isplib.gat_spmm and gat_matmul / SparseTensor.gat_matmul give the same bits; a weighted storage too (stored values are
    not read); only the requested gradients are computed."""
    import isplib_amd
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    g = dev(case.g, gpu)
    y, a_dst, a_src = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src))
    z = torch.ops.isplib.gat_spmm(rowptr, col, colptr, row_t, y, a_dst, a_src, heads, case.ns)
    z.backward(g)
    held(case, dict(z=z, dy=y.grad, dadst=a_dst.grad, dasrc=a_src.grad), ("z", "dy", "dadst", "dasrc"), " op")
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, torch.rand(col.numel(), device=gpu) + 0.5, (case.m, case.n))
    y2, d2, s2 = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src))
    z2 = isplib_amd.gat_matmul(adj, y2, d2, s2, heads=heads, negative_slope=case.ns)
    z2.backward(g)
    for a, b in ((z2, z), (y2.grad, y.grad), (d2.grad, a_dst.grad), (s2.grad, a_src.grad)):
        assert torch.equal(a.detach(), b.detach())
    # only a_dst asks: the columns kernel does not run, the others stay None
    y3, d3, s3 = dev(case.y, gpu), dev(case.a_dst, gpu).requires_grad_(True), dev(case.a_src, gpu)
    adj.gat_matmul(y3, d3, s3, heads, case.ns).backward(g)
    assert y3.grad is None and s3.grad is None and torch.equal(d3.grad, a_dst.grad)
    y4, d4, s4 = dev(case.y, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu).requires_grad_(True)
    adj.gat_matmul(y4, d4, s4, heads, case.ns).backward(g)
    assert y4.grad is None and d4.grad is None and torch.equal(s4.grad, a_src.grad)
    if heads == 1:                                                          # the scores may be [rows]
        d5, s5 = dev(case.a_dst[:, 0], gpu).requires_grad_(True), dev(case.a_src[:, 0], gpu).requires_grad_(True)
        z5 = adj.gat_matmul(dev(case.y, gpu), d5, s5)
        z5.backward(g)
        assert torch.equal(z5.detach(), z.detach()) and torch.equal(d5.grad, a_dst.grad[:, 0]) and torch.equal(s5.grad, a_src.grad[:, 0])


_shared = {}


def shared_case(heads, d):
    if (heads, d) not in _shared:
        base = cases.config_case(heads, d)
        _shared[heads, d] = cases.Case(f"shared-h{heads}d{d}", base.rowptr, base.col, np.array(base.y), np.array(base.a_dst), np.array(base.a_dst),
                                       np.array(base.g), heads, base.ns)
    return _shared[heads, d]


@pytest.mark.parametrize("heads,d", ((1, 47), (8, 16)))
def test_one_score_tensor_for_both_sides(gpu, heads, d):
    """The same tensor as a_dst and a_src on a square graph: its gradient receives both parts through ordinary autograd."""
    import isplib_amd
    case = shared_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    y, a = dev(case.y, gpu).requires_grad_(True), dev(case.a_dst, gpu).requires_grad_(True)
    z = adj.gat_matmul(y, a, a, heads=heads, negative_slope=case.ns)
    z.backward(dev(case.g, gpu))
    held(case, dict(z=z, dy=y.grad), ("z", "dy"))
    frac = ref.worst(a.grad.cpu().numpy(), case.ref["dadst"] + case.ref["dasrc"], case.bound["dadst"] + case.bound["dasrc"])
    print(f"gat error/bound {case.name}: dadst+dasrc={frac:.4f}")
    assert frac <= 1.0


def test_one_entry_rows_return_y_bit_for_bit(gpu):
    """Whatever the score, |u| of thousands included: exp of the raw score would be Inf or 0 there."""
    case = cases.single_case()
    got = run_cabi(case, gpu)
    z, lse = got["z"].cpu().numpy(), got["lse"].cpu().numpy()
    live = case.live
    want = np.zeros_like(case.y)
    want[live] = case.y[case.col]
    assert np.array_equal(z.view(np.uint32), want.view(np.uint32))
    u32 = (case.a_dst[case.ref["row"]] + case.a_src[case.col]).astype(np.float32)           # ONE fp32 add, then the slope
    s32 = np.where(u32 > 0, u32, (np.float32(case.ns) * u32).astype(np.float32)).astype(np.float32)
    assert np.all(np.isneginf(lse[~live])) and np.array_equal(lse[live].view(np.uint32), s32.view(np.uint32))
    # a = 1 and t = D in exact arithmetic: the gradients of the scores are rounding noise of t - D, inside the bounds
    held(case, got, CABI_OUTPUTS)


def test_scores_spread_over_200(gpu):
    case = cases.large_case()
    got = run_cabi(case, gpu)
    for name in CABI_OUTPUTS:
        v = got[name].cpu().numpy()
        assert np.all(np.isfinite(v[case.live] if name == "lse" else v)), name
    held(case, got, CABI_OUTPUTS)


@pytest.mark.parametrize("heads,d", ((1, 41), (8, 8)))
def test_zero_scores_give_the_unit_weight_mean(gpu, heads, d):
    from isplib_amd import cabi
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    y = dev(case.y, gpu)
    zeros_m, zeros_n = torch.zeros(case.m, heads, device=gpu), torch.zeros(case.n, heads, device=gpu)
    z, lse = cabi.gat(rowptr, col, y, zeros_m, zeros_n, heads, case.ns)
    mean, _ = cabi.spmm(rowptr, col, None, y, "mean")
    zero = cases.Case(f"zero-h{heads}d{d}", case.rowptr, case.col, np.array(case.y), np.zeros_like(case.a_dst), np.zeros_like(case.a_src),
                      np.array(case.g), heads, case.ns)
    frac = ref.worst(z.cpu().numpy(), mean.cpu().numpy().astype(np.float64), zero.bound["z"])
    print(f"gat error/bound zero scores vs mean h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    live = zero.live
    assert np.allclose(zero.ref["lse"][live], np.log(np.diff(case.rowptr)[live])[:, None], rtol=1e-12)   # lse = log deg
    assert ref.worst(lse.cpu().numpy()[live], zero.ref["lse"][live], zero.bound["lse"][live]) <= 1.0


@pytest.mark.parametrize("heads,d", ((1, 41), (8, 8), (3, 128)))
def test_pitched_offset_and_column_block_views(gpu, heads, d):
    """y and g with ld > K and a base offset by one float, and as the LAST column block of a wider tensor (its last row ends with the
    allocation: the descriptor's extent), go in without a copy and give the bits of the packed operands."""
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

    got = run_cabi(case, gpu, y=pitched(case.y, 5, 1), g=pitched(case.g, 1, 1))
    for name in CABI_OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    blocks = 3
    wide = {n: torch.randn(case.m, blocks * k, device=gpu) for n in "yg"}
    for b in (1, blocks - 1):
        for n, a in (("y", case.y), ("g", case.g)):
            wide[n][:, b * k:(b + 1) * k] = dev(a, gpu)
        view = {n: wide[n][:, b * k:(b + 1) * k] for n in "yg"}
        assert not view["y"].is_contiguous()
        got = run_cabi(case, gpu, y=view["y"], g=view["g"])
        for name in CABI_OUTPUTS:
            assert torch.equal(got[name], packed[name]), (b, name)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    yw = wide["y"].clone().requires_grad_(True)
    b = blocks - 1
    z = adj.gat_matmul(yw[:, b * k:(b + 1) * k], dev(case.a_dst, gpu), dev(case.a_src, gpu), heads, case.ns)
    z.backward(wide["g"][:, b * k:(b + 1) * k])
    assert torch.equal(z.detach(), packed["z"]) and torch.equal(yw.grad[:, b * k:(b + 1) * k], packed["dy"]) and not yw.grad[:, :b * k].any()


@pytest.mark.parametrize("heads,d", ((1, 3), (5, 8), (1, 512), (8, 64)))
def test_outputs_are_write_only_and_launches_repeat(gpu, heads, d):
    """NaN-filled, over-allocated outputs, launched twice: every element is written, nothing past the end, equal bits."""
    from isplib_amd import cabi
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    y, a_dst, a_src, g = dev(case.y, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu), dev(case.g, gpu)
    m, n, k, pad, H, ns = case.m, case.n, case.k, 64, heads, case.ns

    def fresh(rows, cols):
        buf = torch.full((rows * cols + pad,), float("nan"), device=gpu)
        return buf, buf[:rows * cols].view(rows, cols)

    runs = []
    for _ in range(2):
        b = {name: fresh(*shape) for name, shape in (("z", (m, k)), ("lse", (m, H)), ("dadst", (m, H)), ("D", (m, H)), ("dy", (n, k)),
                                                     ("dasrc", (n, H)))}
        cabi.gat(rowptr, col, y, a_dst, a_src, H, ns, out=(b["z"][1], b["lse"][1]), check=False)
        cabi.gat_bw_rows(rowptr, col, y, a_dst, a_src, g, b["z"][1], b["lse"][1], H, ns, out=(b["dadst"][1], b["D"][1]), check=False)
        cabi.gat_bw_cols(colptr, row_t, y, a_dst, a_src, g, b["lse"][1], b["D"][1], H, ns, out=(b["dy"][1], b["dasrc"][1]), check=False)
        for name, (buf, view) in b.items():
            assert not torch.isnan(view).any(), name
            assert torch.isnan(buf[view.numel():]).all(), name
        runs.append({name: view.clone() for name, (_, view) in b.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    # pitched outputs: nothing is written between the rows
    buf = torch.full((m, k + 3), float("nan"), device=gpu)
    lse = torch.empty(m, H, device=gpu)
    cabi.gat(rowptr, col, y, a_dst, a_src, H, ns, out=(buf[:, :k], lse))
    assert torch.equal(buf[:, :k], runs[0]["z"]) and torch.isnan(buf[:, k:]).all()
    buf = torch.full((n, k + 3), float("nan"), device=gpu)
    dasrc = torch.empty(n, H, device=gpu)
    cabi.gat_bw_cols(colptr, row_t, y, a_dst, a_src, g, runs[0]["lse"], runs[0]["D"], H, ns, out=(buf[:, :k], dasrc))
    assert torch.equal(buf[:, :k], runs[0]["dy"]) and torch.isnan(buf[:, k:]).all()


@pytest.mark.parametrize("heads,d", ((8, 8), (2, 256)))
def test_nans_poison_exactly_what_references_them(gpu, heads, d):
    """A NaN row of y: exactly the rows that reference it.  A NaN in a_src[j, h]: exactly head h of those rows."""
    case = cases.config_case(heads, d)
    j = int(case.col[case.rowptr[2]])                     # a column some rows reference
    hit = np.zeros(case.m, bool)
    hit[case.ref["row"][case.col == j]] = True
    assert hit.any() and (~hit & case.live).any()
    y = np.array(case.y)
    y[j, :] = np.nan
    got = run_cabi(case, gpu, y=dev(y, gpu))
    z, lse = got["z"].cpu().numpy(), got["lse"].cpu().numpy()
    assert np.all(np.isnan(z[hit])) and ref.worst(z[~hit], case.ref["z"][~hit], case.bound["z"][~hit]) <= 1.0
    live = case.live
    assert ref.worst(lse[live], case.ref["lse"][live], case.bound["lse"][live]) <= 1.0          # y does not enter the scores
    h = heads - 1
    a_src = np.array(case.a_src)
    a_src[j, h] = np.nan
    got = run_cabi(case, gpu, a_src=dev(a_src, gpu))
    z, lse = ref.per_head(got["z"].cpu().numpy(), heads), got["lse"].cpu().numpy()
    want, bound = ref.per_head(case.ref["z"], heads), ref.per_head(case.bound["z"], heads)
    assert np.all(np.isnan(z[hit, h])) and np.all(np.isnan(lse[hit, h]))
    clean = np.ones((case.m, heads), bool)
    clean[hit, h] = False
    frac = ref.worst(z[clean], want[clean], bound[clean])
    print(f"gat error/bound nan a_src, everything else h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    ok = clean & live[:, None]
    assert ref.worst(lse[ok], case.ref["lse"][ok], case.bound["lse"][ok]) <= 1.0


def test_error_paths_raise_before_a_launch(gpu):
    import isplib_amd
    from isplib_amd import cabi
    case = cases.config_case(2, 4)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    y, a_dst, a_src = dev(case.y, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu)
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gat_matmul(y.cpu(), a_dst, a_src, 2)
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gat_matmul(y, a_dst, a_src.cpu(), 2)
    with pytest.raises(ValueError, match="2-D"):
        adj.gat_matmul(y[0], a_dst, a_src, 2)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32"):
            adj.gat_matmul(y.to(dt), a_dst.to(dt), a_src.to(dt), 2)
    with pytest.raises(ValueError, match="one row per column"):
        adj.gat_matmul(y[:-1], a_dst, a_src, 2)
    with pytest.raises(ValueError, match=r"`a_dst` must be \[200, 2\]"):
        adj.gat_matmul(y, a_dst[:-1], a_src, 2)
    with pytest.raises(ValueError, match=r"`a_src` must be \[200, 2\]"):
        adj.gat_matmul(y, a_dst, a_src[:, :1], 2)
    with pytest.raises(ValueError, match="power of two"):
        adj.gat_matmul(torch.zeros(case.m, 12, device=gpu), a_dst, a_src, 2)
    with pytest.raises(ValueError, match="512"):
        adj.gat_matmul(torch.zeros(case.m, 1024, device=gpu), a_dst, a_src, 2)
    # the wrappers: structure checks that read the device
    with pytest.raises(ValueError, match="ascend"):
        cabi.gat(torch.flip(rowptr, (0,)), col, y, a_dst, a_src, 2)
    bad = col.clone()
    bad[3] = case.m
    with pytest.raises(ValueError, match=r"lie in \[0, 200\)"):
        cabi.gat(rowptr, bad, y, a_dst, a_src, 2)
    # the operator: every shape before a launch
    for args in ((y[:-1], a_dst, a_src, 2), (y, a_dst[:-1], a_src, 2), (y, a_dst, a_src[:, :1], 2), (y, a_dst, a_src, 3),
                 (torch.zeros(case.m, 12, device=gpu), a_dst, a_src, 2), (y, a_dst, a_src.cpu(), 2)):
        with pytest.raises(RuntimeError, match="gat_spmm|GPU tensor"):
            torch.ops.isplib.gat_spmm(rowptr, col, rowptr, col, *args, 0.2)
    with pytest.raises(RuntimeError, match="gat_spmm"):
        torch.ops.isplib.gat_spmm(rowptr[:-1], col, rowptr, col, y, a_dst, a_src, 2, 0.2)
    # the entries themselves: outside the domain NO_OPT_IMPL, bad arguments FAIL, nothing to do SUCCESS -- all without a launch
    L = cabi.lib()
    rp, z, lse = rowptr.data_ptr(), torch.empty(case.m, 1024, device=gpu), torch.empty(case.m, 128, device=gpu)
    args = lambda m, k, ldy, heads, dp: (m, case.m, k, col.numel(), col.data_ptr(), rp, rp + 8, dp, y.data_ptr(), ldy, a_src.data_ptr(),  # noqa: E731
                                         heads, 0.2, z.data_ptr(), 1024, lse.data_ptr(), None)
    ad = a_dst.data_ptr()
    assert L.isplib_gat_csr_hip(*args(case.m, 516, 516, 1, ad)) == cabi.NO_OPT_IMPL and "isplib_gat_serves" in cabi.last_error()
    assert L.isplib_gat_csr_hip(*args(case.m, 12, 12, 2, ad)) == cabi.NO_OPT_IMPL                  # d = 6
    assert L.isplib_gat_csr_hip(*args(case.m, 4, 4, 2, ad)) == cabi.NO_OPT_IMPL                    # d = 2
    assert L.isplib_gat_csr_hip(*args(case.m, 8, 7, 2, ad)) == cabi.NO_OPT_IMPL                    # ldy < k
    assert L.isplib_gat_csr_hip(*args(case.m, 8, 8, 0, ad)) == cabi.NO_OPT_IMPL
    assert L.isplib_gat_csr_hip(*args(case.m, 9, 9, 2, ad)) == cabi.FAIL                           # k is no multiple of heads
    assert L.isplib_gat_csr_hip(*args(-1, 8, 8, 2, ad)) == cabi.FAIL
    assert L.isplib_gat_csr_hip(*args(case.m, 8, 8, 2, None)) == cabi.FAIL and "null" in cabi.last_error()
    assert L.isplib_gat_csr_hip(*args(0, 8, 8, 2, None)) == cabi.SUCCESS and L.isplib_gat_csr_hip(*args(case.m, 0, 8, 2, None)) == cabi.SUCCESS
    torch.cuda.synchronize()
