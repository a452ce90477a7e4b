"""GATv2 aggregation with attention dropout on the GPU (isplib_amd/csrc/gatv2.hip, DROP kernels): the C ABI wrappers,
torch.ops.isplib.gatv2_drop_spmm with its autograd backward, and gatv2_matmul(..., dropout=, training=, seed=), each held to the
per-element bounds of tests/gatv2_dropout_ref.py against the reference with the same mask (inputs, references and bounds:
tests/gatv2_dropout_cases.py, computed once per case).  The largest error / bound seen per output is printed before every assertion;
DESIGN.md 4.6j records it.
"""
import numpy as np
import pytest
import torch

from tests import gatv2_dropout_cases as cases
from tests import gatv2_dropout_ref as ref

pytestmark = pytest.mark.gpu

OUTPUTS = ("z", "lse", "dx", "D", "datt", "dy")
IDS = [f"h{h}d{d}" for h, d in cases.CONFIGS]


def dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def dev_graph(case, gpu):
    return dev(case.rowptr, gpu), dev(case.col, gpu)


def adjacency(case, gpu):
    import isplib_amd
    rowptr, col = dev_graph(case, gpu)
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))


def transposed(case, gpu):
    """colptr / row_t / csr2csc as SparseStorage caches them (the library's own csr2csc)."""
    st = adjacency(case, gpu).storage
    return st.colptr(), st.row_t(), st.csr2csc()


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
    print(f"gatv2_dropout error/bound {case.name}{what}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def poisoned(gpu, *shape):
    return torch.full(shape, float("nan"), device=gpu)


def run_cabi(case, gpu, threshold=None, scale=None, seed=None, want_datt=True):
    """The three entries on NaN-filled outputs, with the case's mask unless another (threshold, scale, seed) is given."""
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    x, y, att, g = dev(case.x, gpu), dev(case.y, gpu), dev(case.att, gpu), dev(case.g, gpu)
    T = case.threshold if threshold is None else threshold
    c = case.scale if scale is None else scale
    sd = case.seed if seed is None else seed
    m, n, k, H = case.m, case.n, case.k, case.heads
    z, lse = cabi.gatv2_drop(rowptr, col, x, y, att, T, c, sd, H, case.ns, out=(poisoned(gpu, m, k), poisoned(gpu, m, H)))
    dx, D, datt = cabi.gatv2_drop_bw_rows(rowptr, col, x, y, att, g, z, lse, T, c, sd, H, case.ns, want_datt=want_datt,
                                          out=(poisoned(gpu, m, k), poisoned(gpu, m, H), poisoned(gpu, H, k // H) if want_datt else None))
    colptr, row_t, csr2csc = transposed(case, gpu)
    dy = cabi.gatv2_drop_bw_cols(colptr, row_t, csr2csc, x, y, att, g, lse, D, T, c, sd, H, case.ns, out=poisoned(gpu, n, k))
    return dict(z=z, lse=lse, dx=dx, D=D, datt=datt, dy=dy)


def check_cabi(case, gpu):
    """Every output within its bound, element by element, on NaN-filled outputs, with and without datt (the same bits); an empty row
    and a (row, head) that lost every entry have z = 0 exactly, the latter with a finite lse."""
    got = run_cabi(case, gpu)
    held(case, got, OUTPUTS)
    for name in OUTPUTS:
        assert not np.isnan(got[name].cpu().numpy()).any(), name        # every element was written
    empty = ~case.live
    for name in ("z", "dx", "D"):
        assert np.all(got[name].cpu().numpy()[empty] == 0), name
    gone = case.all_dropped()
    assert np.all(ref.per_head(got["z"].cpu().numpy(), case.heads)[gone] == 0) and np.all(np.isfinite(got["lse"].cpu().numpy()[gone]))
    without = run_cabi(case, gpu, want_datt=False)
    assert without["datt"] is None
    for name in ("z", "lse", "dx", "D", "dy"):
        assert torch.equal(got[name], without[name]), name
    return got


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_cabi_entries_at_every_configuration(gpu, heads, d):
    check_cabi(cases.config_case(heads, d), gpu)


@pytest.mark.parametrize("case", cases.slope_cases(), ids=lambda c: c.name)
def test_cabi_entries_at_every_slope_with_light_and_heavy_dropout(gpu, case):
    assert case.p in (0.1, 0.9)
    if case.p == 0.9 and (case.heads, case.k) == (8, 64):
        assert case.all_dropped().any()
    check_cabi(case, gpu)


@pytest.mark.parametrize("heads,d", cases.WIDTH_CONFIGS)
def test_threshold_0_and_scale_1_give_the_bits_of_the_entries_without_dropout(gpu, heads, d):
    """Every entry is kept and c = 1: t * 1, z * 1 and a * 1 are exact and the kernels are one template, so all outputs are equal bit
    for bit at the five width instantiations."""
    from isplib_amd import cabi
    case = cases.config_case(heads, d)
    got = run_cabi(case, gpu, threshold=0, scale=1.0, seed=case.seed)
    rowptr, col = dev_graph(case, gpu)
    x, y, att, g = dev(case.x, gpu), dev(case.y, gpu), dev(case.att, gpu), dev(case.g, gpu)
    colptr, row_t, _ = transposed(case, gpu)
    z, lse = cabi.gatv2(rowptr, col, x, y, att, heads, case.ns)
    dx, D, datt = cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, z, lse, heads, case.ns)
    dy = cabi.gatv2_bw_cols(colptr, row_t, x, y, att, g, lse, D, heads, case.ns)
    for name, w in dict(z=z, lse=lse, dx=dx, D=D, datt=datt, dy=dy).items():
        assert torch.equal(got[name], w), name


@pytest.mark.parametrize("heads,d", ((8, 8), (2, 256)))
def test_one_mask_in_three_kernels(gpu, heads, d):
    """At one seed: z of the forward is the reference's under the mask, D of the rows kernel equals <g, z> of THAT z within bound (the
    rows kernel's t_e and the forward's z agree on the mask), and dy of the columns kernel matches."""
    case = cases.config_case(heads, d)
    got = run_cabi(case, gpu)
    held(case, got, ("z", "D", "dy", "dx", "datt"))
    gz = (ref.per_head(case.g.astype(np.float64), heads) * ref.per_head(got["z"].cpu().numpy().astype(np.float64), heads)).sum(2)
    assert np.all(np.abs(got["D"].cpu().numpy() - gz) <= case.bound["D"])
    other = ref.keep(case.seed + 1, case.nnz, heads, case.p)             # and another seed's mask is far away
    assert ref.worst(got["z"].cpu().numpy(), case.with_mask(other)["z"], case.bound["z"]) > 10.0


def test_one_entry_rows_are_exact(gpu):
    """One-entry rows: a_e = 1 and l = 1 exactly, so a kept (row, head) has z = float32(y_j c) bit for bit and a dropped one 0; lse does
    not see the mask; the value part of dy vanishes in a head whose incoming entries are all dropped: dy is then the r part alone."""
    case = cases.single_case()
    assert case.seed == 1
    got = run_cabi(case, gpu)
    H, d = case.heads, case.k // case.heads
    q, row = case.ref["q"], case.ref["row"]
    want = np.zeros((case.m, H, d), np.float32)
    yc = (ref.per_head(case.y, H)[case.col] * np.float32(case.scale)).astype(np.float32)
    want[row] = np.where(q[:, :, None], yc, np.float32(0.0))
    z = got["z"].cpu().numpy()
    assert np.array_equal(ref.per_head(z, H)[row][~q], np.zeros_like(yc)[~q])
    assert np.array_equal(np.abs(z).view(np.uint32), np.abs(want.reshape(case.m, case.k)).view(np.uint32))
    assert np.array_equal(np.signbit(ref.per_head(z, H)[row][q]), np.signbit(yc[q]))
    base = run_cabi(case, gpu, threshold=0, scale=1.0)
    assert torch.equal(got["lse"], base["lse"])
    held(case, got, OUTPUTS)
    # ds_e = a_e (t_e - D) = 0 in a one-entry row whatever the bit (D = t_e), up to rounding: dy is its value part, which is exactly 0
    # where no incoming entry is kept
    dy = ref.per_head(got["dy"].cpu().numpy(), H)
    none_kept = (case.kept_in == 0) & case.has_in[:, None]
    bound = ref.per_head(case.bound["dy"], H)
    assert none_kept.any() and np.all(np.abs(dy[none_kept]) <= bound[none_kept])
    value = np.abs(ref.per_head(case.ref["dy"], H))
    assert np.all(value[none_kept].max(1) <= bound[none_kept].max(1)) and np.all(value[(case.kept_in > 0)].max(1) > 0)


def test_duplicates_have_bits_of_their_own(gpu):
    """Two stored entries (i, j) with different keep bits in some head: z_i is the reference's, and far -- beyond eight bounds -- from
    what a mask per (i, j) would give."""
    case = cases.duplicate_case()
    assert case.seed == 1 and case.pairs[0] == (6, 7)
    got = check_cabi(case, gpu)
    e1, e2 = case.pairs[0]
    wrong = np.array(case.ref["q"])
    wrong[e2] = wrong[e1]
    H, i = case.heads, case.row
    z = ref.per_head(got["z"].cpu().numpy().astype(np.float64), H)[i]
    bound = ref.per_head(case.bound["z"], H)[i]
    assert np.all(np.abs(z - ref.per_head(case.ref["z"], H)[i]) <= bound)
    far = np.abs(z - ref.per_head(case.with_mask(wrong)["z"], H)[i]) > 8.0 * bound
    assert case.wide.any() and np.all(far.any(1)[case.wide])


def test_the_columns_kernel_hashes_the_csr_position(gpu):
    """dy under the mask of the CSR positions (through csr2csc) is the reference's; the mask indexed by the transposed position is far."""
    case = cases.position_case()
    got = run_cabi(case, gpu)
    held(case, got, ("dy",))
    wrong = np.empty_like(case.ref["q"])
    wrong[cases.transposed_positions(case.col)] = case.ref["q"]
    assert ref.worst(got["dy"].cpu().numpy(), case.with_mask(wrong)["dy"], case.bound["dy"]) > 8.0


def test_rectangular_graph(gpu):
    """M != N (67 x 233): through the entries and through the plug-in, which give the same bits."""
    case = cases.rect_case()
    got = check_cabi(case, gpu)
    adj = adjacency(case, gpu)
    x, y, att = (dev(a, gpu).requires_grad_(True) for a in (case.x, case.y, case.att))
    z = adj.gatv2_matmul(x, att, y, case.heads, case.ns, dropout=case.p, seed=case.seed)
    z.backward(dev(case.g, gpu))
    for name, a in (("z", z), ("dx", x.grad), ("dy", y.grad), ("datt", att.grad)):
        assert torch.equal(a.detach(), got[name]), name


@pytest.mark.parametrize("heads,d", ((8, 8), (1, 47), (2, 256)))
def test_operator_and_plugin_under_autograd(gpu, heads, d):
    """torch.ops.isplib.gatv2_drop_spmm and gatv2_matmul give the bits of the three entries, inside the bounds; gat_dropout_mask on the
    matrix's device is the mask the kernels used; y=None shares the one tensor, whose gradient receives both parts."""
    import isplib_amd
    case = cases.config_case(heads, d)
    want = run_cabi(case, gpu)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    g = dev(case.g, gpu)
    x, y, att = (dev(a, gpu).requires_grad_(True) for a in (case.x, case.y, case.att))
    z = torch.ops.isplib.gatv2_drop_spmm(rowptr, col, colptr, row_t, csr2csc, x, y, att, heads, case.ns, case.p, case.seed)
    z.backward(g)
    got = dict(z=z, dx=x.grad, dy=y.grad, datt=att.grad)
    held(case, got, tuple(got), " op")
    for name, v in got.items():
        assert torch.equal(v.detach(), want[name]), name
    adj = adjacency(case, gpu)
    x2, y2, a2 = (dev(a, gpu).requires_grad_(True) for a in (case.x, case.y, case.att))
    z2 = isplib_amd.gatv2_matmul(adj, x2, a2, y2, heads=heads, negative_slope=case.ns, dropout=case.p, training=True, seed=case.seed)
    z2.backward(g)
    for a, b in ((z2, z), (x2.grad, x.grad), (y2.grad, y.grad), (a2.grad, att.grad)):
        assert torch.equal(a.detach(), b.detach())
    mask = isplib_amd.gat_dropout_mask(adj, heads, case.p, case.seed)
    assert mask.device == z.device and np.array_equal(mask.cpu().numpy(), case.ref["q"])
    # y=None: the call with y = x, and dx + dy in the one gradient
    xs, ys, as_ = (dev(a, gpu).requires_grad_(True) for a in (case.x, case.x, case.att))
    zs = adj.gatv2_matmul(xs, as_, ys, heads, case.ns, dropout=case.p, seed=case.seed)
    zs.backward(g)
    x1, a1 = dev(case.x, gpu).requires_grad_(True), dev(case.att, gpu).requires_grad_(True)
    z1 = adj.gatv2_matmul(x1, a1, heads=heads, negative_slope=case.ns, dropout=case.p, seed=case.seed)
    z1.backward(g)
    assert torch.equal(z1.detach(), zs.detach()) and torch.equal(a1.grad, as_.grad) and torch.equal(x1.grad, xs.grad + ys.grad)


def test_determinism_and_seed_handling(gpu):
    case = cases.config_case(8, 8)
    adj = adjacency(case, gpu)
    x, y, att = dev(case.x, gpu), dev(case.y, gpu), dev(case.att, gpu)
    z1 = adj.gatv2_matmul(x, att, y, 8, case.ns, dropout=0.6, seed=11)
    z2 = adj.gatv2_matmul(x, att, y, 8, case.ns, dropout=0.6, seed=11)
    z3 = adj.gatv2_matmul(x, att, y, 8, case.ns, dropout=0.6, seed=12)
    assert torch.equal(z1, z2) and not torch.equal(z1, z3)
    torch.manual_seed(99)
    a = adj.gatv2_matmul(x, att, y, 8, case.ns, dropout=0.6)
    b = adj.gatv2_matmul(x, att, y, 8, case.ns, dropout=0.6)
    torch.manual_seed(99)
    c = adj.gatv2_matmul(x, att, y, 8, case.ns, dropout=0.6)
    assert torch.equal(a, c) and not torch.equal(a, b)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()


def test_partial_gradients(gpu):
    """Only x or only att asks: the columns kernel does not run -- the backward allocates nothing of y's size beside dx -- and the
    gradient has the bits of the full call; only y: dx and datt stay None; every subset gets the full call's bits."""
    case = cases.config_case(8, 64)
    adj = adjacency(case, gpu)
    g = dev(case.g, gpu)

    def run(need):
        ops = {name: dev(a, gpu).requires_grad_(name in need) for name, a in (("x", case.x), ("y", case.y), ("att", case.att))}
        z = adj.gatv2_matmul(ops["x"], ops["att"], ops["y"], case.heads, case.ns, dropout=case.p, seed=case.seed)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        z.backward(g)
        torch.cuda.synchronize()
        return z, {name: t.grad for name, t in ops.items()}, torch.cuda.max_memory_allocated() - before

    names = ("x", "y", "att")
    z, full, grew_full = run(names)
    assert all(full[name] is not None for name in names)
    assert grew_full >= (case.m + case.n) * case.k * 4                   # dx and dy
    for need in (("x",), ("att",), ("y",), ("x", "att"), ("y", "att")):
        z1, part, grew = run(need)
        assert torch.equal(z1, z)
        for name in names:
            assert (part[name] is None) if name not in need else torch.equal(part[name], full[name]), (need, name)
        if "y" not in need:
            assert grew < (case.m + case.n) * case.k * 4, (need, grew)   # dx, D, datt and its workspace: no dy, so no columns kernel


def test_eval_mode_and_zero_dropout_are_the_call_without_the_keywords(gpu):
    case = cases.config_case(8, 8)
    adj = adjacency(case, gpu)
    g = dev(case.g, gpu)

    def run(**kw):
        ops = [dev(a, gpu).requires_grad_(True) for a in (case.x, case.att, case.y)]
        z = adj.gatv2_matmul(ops[0], ops[1], ops[2], case.heads, case.ns, **kw)
        z.backward(g)
        return [z.detach()] + [t.grad for t in ops]

    plain = run()
    for kw in (dict(dropout=0.6, training=False), dict(dropout=0.6, training=False, seed=3), dict(dropout=0.0), dict(dropout=0, seed=3)):
        for a, b in zip(run(**kw), plain):
            assert torch.equal(a, b), kw
    assert not torch.equal(run(dropout=0.6, seed=3)[0], plain[0])


def test_16_bit_operands_convert_when_the_variable_is_set(gpu, monkeypatch):
    """There is no 16-bit dropout kernel: under ISPLIB_HALF_GATV2 (any value) bf16 operands go through the fp32 dropout operator on
    the widened operands, and come back rounded once; gradients return in their own dtypes."""
    case = cases.config_case(8, 8)
    adj = adjacency(case, gpu)
    g = dev(case.g, gpu)
    xb, yb = dev(case.x, gpu).bfloat16(), dev(case.y, gpu).bfloat16()
    att = dev(case.att, gpu)
    monkeypatch.delenv("ISPLIB_HALF_GATV2", raising=False)
    with pytest.raises(TypeError, match="float32"):
        adj.gatv2_matmul(xb, att, yb, 8, case.ns, dropout=0.6, seed=5)
    x32, y32, a32 = xb.float().requires_grad_(True), yb.float().requires_grad_(True), att.clone().requires_grad_(True)
    z32 = adj.gatv2_matmul(x32, a32, y32, 8, case.ns, dropout=0.6, seed=5)
    z32.backward(g.bfloat16().float())
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "native")
    x16, y16, a16 = xb.clone().requires_grad_(True), yb.clone().requires_grad_(True), att.clone().requires_grad_(True)
    z16 = adj.gatv2_matmul(x16, a16, y16, 8, case.ns, dropout=0.6, seed=5)
    assert z16.dtype == torch.bfloat16 and torch.equal(z16.detach(), z32.detach().bfloat16())
    z16.backward(g.bfloat16())
    assert x16.grad.dtype == y16.grad.dtype == torch.bfloat16 and a16.grad.dtype == torch.float32
    assert torch.equal(x16.grad, x32.grad.bfloat16()) and torch.equal(y16.grad, y32.grad.bfloat16()) and torch.equal(a16.grad, a32.grad)


def test_error_paths_raise_before_a_launch(gpu):
    from isplib_amd import cabi
    case = cases.config_case(2, 4)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    x, y, att, g = (dev(a, gpu) for a in (case.x, case.y, case.att, case.g))
    m, n, k, nnz = case.m, case.n, case.k, case.nnz
    z, lse = poisoned(gpu, m, k), poisoned(gpu, m, 2)
    for bad in (dict(threshold=-1), dict(threshold=2 ** 32), dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan")),
                dict(seed=-1), dict(seed=2 ** 63)):
        kw = dict(threshold=5, scale=2.5, seed=1)
        kw.update(bad)
        with pytest.raises(ValueError, match="`threshold`|`scale`|`seed`"):
            cabi.gatv2_drop(rowptr, col, x, y, att, kw["threshold"], kw["scale"], kw["seed"], 2, out=(z, lse))
    with pytest.raises(ValueError, match="`csr2csc` must be a 1-D tensor"):
        cabi.gatv2_drop_bw_cols(colptr, row_t, csr2csc[:-1], x, y, att, g, lse, lse, 5, 2.5, 1, 2)
    with pytest.raises(TypeError, match="`csr2csc` must be int64"):
        cabi.gatv2_drop_bw_cols(colptr, row_t, csr2csc.int(), x, y, att, g, lse, lse, 5, 2.5, 1, 2)
    L = cabi.lib()
    rp, cp = rowptr.data_ptr(), colptr.data_ptr()
    fw = lambda scale, heads=2, nz=nnz: (m, n, k, nz, col.data_ptr(), rp, rp + 8, x.data_ptr(), k, y.data_ptr(), k, att.data_ptr(), heads,  # noqa: E731
                                         0.2, z.data_ptr(), k, lse.data_ptr(), None, 5, scale, 1)
    assert L.isplib_gatv2_drop_csr_hip(*fw(0.0)) == cabi.FAIL and "scale" in cabi.last_error()
    assert L.isplib_gatv2_drop_csr_hip(*fw(float("nan"))) == cabi.FAIL
    assert L.isplib_gatv2_drop_csr_hip(*fw(float("inf"))) == cabi.FAIL
    assert L.isplib_gatv2_drop_csr_hip(*fw(2.5, nz=2 ** 31)) == cabi.FAIL and "2^31" in cabi.last_error()
    assert L.isplib_gatv2_drop_csr_hip(*fw(2.5, heads=0)) == cabi.NO_OPT_IMPL and "isplib_gatv2_serves" in cabi.last_error()
    dx, D, dy = poisoned(gpu, m, k), poisoned(gpu, m, 2), poisoned(gpu, n, k)
    rows = lambda scale, nz=nnz: (m, n, k, nz, col.data_ptr(), rp, rp + 8, x.data_ptr(), k, y.data_ptr(), k, att.data_ptr(), 2, 0.2,  # noqa: E731
                                  g.data_ptr(), k, g.data_ptr(), k, g.data_ptr(), dx.data_ptr(), k, D.data_ptr(), None, None, 0, None, 5, scale, 1)
    assert L.isplib_gatv2_drop_bw_rows_hip(*rows(-1.0)) == cabi.FAIL and "scale" in cabi.last_error()
    assert L.isplib_gatv2_drop_bw_rows_hip(*rows(2.5, 2 ** 31)) == cabi.FAIL
    cols = lambda perm, scale=2.5, nz=nnz: (m, n, k, nz, row_t.data_ptr(), cp, cp + 8, perm, x.data_ptr(), k, y.data_ptr(), k, att.data_ptr(),  # noqa: E731
                                            2, 0.2, g.data_ptr(), k, g.data_ptr(), g.data_ptr(), dy.data_ptr(), k, None, 5, scale, 1)
    assert L.isplib_gatv2_drop_bw_cols_hip(*cols(None)) == cabi.FAIL and "csr2csc" in cabi.last_error()
    assert L.isplib_gatv2_drop_bw_cols_hip(*cols(csr2csc.data_ptr(), 0.0)) == cabi.FAIL
    assert L.isplib_gatv2_drop_bw_cols_hip(*cols(csr2csc.data_ptr(), 2.5, 2 ** 31)) == cabi.FAIL
    torch.cuda.synchronize()
    for t in (z, lse, dx, D, dy):
        assert torch.isnan(t).all()
    with pytest.raises(RuntimeError, match="`p` must lie in"):
        torch.ops.isplib.gatv2_drop_spmm(rowptr, col, colptr, row_t, csr2csc, x, y, att, 2, 0.2, 1.0, 1)
    with pytest.raises(RuntimeError, match="`p` must lie in"):
        torch.ops.isplib.gatv2_drop_spmm(rowptr, col, colptr, row_t, csr2csc, x, y, att, 2, 0.2, 0.0, 1)
    with pytest.raises(RuntimeError, match="`seed` must be"):
        torch.ops.isplib.gatv2_drop_spmm(rowptr, col, colptr, row_t, csr2csc, x, y, att, 2, 0.2, 0.5, -1)
    with pytest.raises(RuntimeError, match="csr2csc"):
        torch.ops.isplib.gatv2_drop_spmm(rowptr, col, colptr, row_t, csr2csc[:-1], x, y, att, 2, 0.2, 0.5, 1)
