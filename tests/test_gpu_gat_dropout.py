"""GAT aggregation with attention dropout on the GPU (isplib_amd/csrc/gat.hip, DROP kernels): the C ABI wrappers,
torch.ops.isplib.gat_drop_spmm with its autograd backward, and gat_matmul(..., dropout=, training=, seed=), each held to the per-element
bounds of tests/gat_dropout_ref.py against the reference with the same mask (inputs, references and bounds: tests/gat_dropout_cases.py,
computed once per case).  The largest error / bound seen per output is printed before every assertion; DESIGN.md 4.6i records it.
"""
import numpy as np
import pytest
import torch

from tests import gat_dropout_cases as cases
from tests import gat_dropout_ref as ref

pytestmark = pytest.mark.gpu

OUTPUTS = ("z", "lse", "dadst", "D", "dy", "dasrc")
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


def names_of(case):
    return OUTPUTS + (("daedge",) if case.a_edge is not None else ())


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
    print(f"gat_dropout error/bound {case.name}{what}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def poisoned(gpu, *shape):
    return torch.full(shape, float("nan"), device=gpu)


def run_cabi(case, gpu, threshold=None, scale=None, seed=None, a_edge="case"):
    """The three entries on NaN-filled outputs, with the case's mask unless another (threshold, scale, seed) is given."""
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    y, a_dst, a_src, g = dev(case.y, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu), dev(case.g, gpu)
    if isinstance(a_edge, str):
        a_edge = dev(case.a_edge, gpu) if case.a_edge is not None else None
    T = case.threshold if threshold is None else threshold
    c = case.scale if scale is None else scale
    sd = case.seed if seed is None else seed
    m, n, k, H, nnz = case.m, case.n, case.k, case.heads, case.nnz
    z, lse = cabi.gat_drop(rowptr, col, y, a_dst, a_src, a_edge, T, c, sd, H, case.ns, out=(poisoned(gpu, m, k), poisoned(gpu, m, H)))
    dadst, D, daedge = cabi.gat_drop_bw_rows(rowptr, col, y, a_dst, a_src, a_edge, g, z, lse, T, c, sd, H, case.ns,
                                             out=(poisoned(gpu, m, H), poisoned(gpu, m, H), poisoned(gpu, nnz, H) if a_edge is not None else None))
    colptr, row_t, csr2csc = transposed(case, gpu)
    dy, dasrc = cabi.gat_drop_bw_cols(colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, g, lse, D, T, c, sd, H, case.ns,
                                      out=(poisoned(gpu, n, k), poisoned(gpu, n, H)))
    got = dict(z=z, lse=lse, dadst=dadst, D=D, dy=dy, dasrc=dasrc)
    if a_edge is not None:
        got["daedge"] = daedge
    return got


def all_dropped(case):
    """bool [m, H]: a live row whose entries are all dropped for the head"""
    kept = np.zeros((case.m, case.heads), np.int64)
    np.add.at(kept, case.ref["row"], case.ref["q"].astype(np.int64))
    return case.live[:, None] & (kept == 0)


def check_cabi(case, gpu):
    """Every output within its bound, element by element, on NaN-filled outputs; an empty row and a (row, head) that lost every entry
    have z = 0 exactly, the latter with a finite lse; a second launch gives the same bits."""
    got = run_cabi(case, gpu)
    names = names_of(case)
    held(case, got, names)
    for name in names:
        assert not np.isnan(got[name].cpu().numpy()).any(), name        # every element was written
    empty = ~case.live
    for name in ("z", "dadst", "D"):
        assert np.all(got[name].cpu().numpy()[empty] == 0), name
    gone = all_dropped(case)
    assert np.all(ref.per_head(got["z"].cpu().numpy(), case.heads)[gone] == 0) and np.all(np.isfinite(got["lse"].cpu().numpy()[gone]))
    again = run_cabi(case, gpu)
    for name in names:
        assert torch.equal(got[name], again[name]), name
    return got


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_cabi_entries_at_every_configuration(gpu, heads, d):
    check_cabi(cases.config_case(heads, d), gpu)


@pytest.mark.parametrize("case", cases.slope_cases(), ids=lambda c: c.name)
def test_cabi_entries_at_every_slope_with_light_and_heavy_dropout(gpu, case):
    assert case.p in (0.1, 0.9)
    check_cabi(case, gpu)


@pytest.mark.parametrize("heads,d", cases.EDGE_CONFIGS)
def test_cabi_entries_with_the_edge_term_too(gpu, heads, d):
    case = cases.edge_case(heads, d)
    got = check_cabi(case, gpu)
    assert "daedge" in got


@pytest.mark.parametrize("edge", (False, True), ids=("plain", "edge"))
@pytest.mark.parametrize("heads,d", cases.WIDTH_CONFIGS)
def test_threshold_0_and_scale_1_give_the_bits_of_the_entries_without_dropout(gpu, heads, d, edge):
    """Every entry is kept and c = 1: t * 1, z * 1 and dy * 1 are exact and the kernels are one template, so all outputs -- d a_edge
    included -- are equal bit for bit at the five width instantiations."""
    from isplib_amd import cabi
    case = cases.edge_case(heads, d) if edge else cases.config_case(heads, d)
    got = run_cabi(case, gpu, threshold=0, scale=1.0, seed=case.seed)
    rowptr, col = dev_graph(case, gpu)
    y, a_dst, a_src, g = dev(case.y, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu), dev(case.g, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    H = case.heads
    if edge:
        a_edge = dev(case.a_edge, gpu)
        z, lse = cabi.gat_edge(rowptr, col, y, a_dst, a_src, a_edge, H, case.ns)
        dadst, D, daedge = cabi.gat_edge_bw_rows(rowptr, col, y, a_dst, a_src, a_edge, g, z, lse, H, case.ns)
        dy, dasrc = cabi.gat_edge_bw_cols(colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, g, lse, D, H, case.ns)
        want = dict(z=z, lse=lse, dadst=dadst, D=D, dy=dy, dasrc=dasrc, daedge=daedge)
    else:
        z, lse = cabi.gat(rowptr, col, y, a_dst, a_src, H, case.ns)
        dadst, D = cabi.gat_bw_rows(rowptr, col, y, a_dst, a_src, g, z, lse, H, case.ns)
        dy, dasrc = cabi.gat_bw_cols(colptr, row_t, y, a_dst, a_src, g, lse, D, H, case.ns)
        want = dict(z=z, lse=lse, dadst=dadst, D=D, dy=dy, dasrc=dasrc)
    for name, w in want.items():
        assert torch.equal(got[name], w), name


def test_one_mask_in_three_kernels(gpu):
    """One-entry rows: a_e = 1 and l = 1 exactly, so a kept (row, head) has z = float32(y_j c) bit for bit and a dropped one 0; lse does
    not see the mask; dy of a column whose incoming entries are all dropped in a head is exactly 0 there, and of any other not."""
    case = cases.single_case()
    got = run_cabi(case, gpu)
    H, d = case.heads, case.k // case.heads
    q, row, live = case.ref["q"], case.ref["row"], case.live
    assert q.any() and not q.all()
    want = np.zeros((case.m, H, d), np.float32)
    yc = (ref.per_head(case.y, H)[case.col] * np.float32(case.scale)).astype(np.float32)
    want[row] = np.where(q[:, :, None], yc, np.float32(0.0))
    z = got["z"].cpu().numpy()
    assert np.array_equal(ref.per_head(z, H)[row][~q], np.zeros_like(yc)[~q])
    assert np.array_equal(np.abs(z).view(np.uint32), np.abs(want.reshape(case.m, case.k)).view(np.uint32))
    assert np.array_equal(np.signbit(ref.per_head(z, H)[row][q]), np.signbit(yc[q]))
    f32 = np.float32
    u32 = (case.a_dst[row] + case.a_src[case.col]).astype(f32)
    s32 = np.where(u32 > 0, u32, (f32(case.ns) * u32).astype(f32)).astype(f32)
    lse = got["lse"].cpu().numpy()
    assert np.all(np.isneginf(lse[~live])) and np.array_equal(lse[live].view(np.uint32), s32.view(np.uint32))
    dy = ref.per_head(got["dy"].cpu().numpy(), H)
    none_kept = case.kept_in == 0                                       # [n, H], columns without incoming entries included
    assert np.all(dy[none_kept] == 0)
    assert np.all(np.abs(dy[~none_kept]).max(1) > 0)
    held(case, got, OUTPUTS)


def test_duplicates_have_bits_of_their_own(gpu):
    """Two stored entries (i, j) with the SAME a_edge row and different keep bits in some head: their d a_edge differ there by what
    the reference says, far beyond both bounds -- a mask per (i, j) would give both the same."""
    case = cases.duplicate_case()
    got = check_cabi(case, gpu)
    e1, e2 = case.pairs[0]
    da = got["daedge"].cpu().numpy().astype(np.float64)
    for e in (e1, e2):
        assert np.all(np.abs(da[e] - case.ref["daedge"][e]) <= case.bound["daedge"][e]), e
    both = case.bound["daedge"][e1] + case.bound["daedge"][e2]
    assert case.wide.any() and np.all(np.abs(da[e1] - da[e2])[case.wide] > 8.0 * both[case.wide])
    same = ~case.differ                                                 # heads whose two bits agree: the two entries are indistinguishable
    assert np.array_equal(da[e1][same], da[e2][same])


def test_rectangular_graph(gpu):
    """M != N (67 x 233), with a_edge: through the entries and through the plug-in, which give the same bits."""
    case = cases.rect_case()
    got = check_cabi(case, gpu)
    adj = adjacency(case, gpu)
    y, a_dst, a_src, a_edge = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src, case.a_edge))
    z = adj.gat_matmul(y, a_dst, a_src, case.heads, case.ns, a_edge=a_edge, dropout=case.p, seed=case.seed)
    z.backward(dev(case.g, gpu))
    for name, a in (("z", z), ("dy", y.grad), ("dadst", a_dst.grad), ("dasrc", a_src.grad), ("daedge", a_edge.grad)):
        assert torch.equal(a.detach(), got[name]), name


@pytest.mark.parametrize("heads,d,edge", ((8, 8, False), (1, 47, False), (2, 256, True), (8, 4, True)))
def test_operator_and_plugin_under_autograd(gpu, heads, d, edge):
    """torch.ops.isplib.gat_drop_spmm and gat_matmul give the bits of the three entries, inside the bounds; gat_dropout_mask on the
    matrix's device is the mask the kernels used."""
    import isplib_amd
    case = cases.edge_case(heads, d) if edge else cases.config_case(heads, d)
    want = run_cabi(case, gpu)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    g = dev(case.g, gpu)
    y, a_dst, a_src = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src))
    a_edge = dev(case.a_edge, gpu).requires_grad_(True) if edge else None
    z = torch.ops.isplib.gat_drop_spmm(rowptr, col, colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, heads, case.ns, case.p, case.seed)
    z.backward(g)
    got = dict(z=z, dy=y.grad, dadst=a_dst.grad, dasrc=a_src.grad)
    if edge:
        got["daedge"] = a_edge.grad
    held(case, got, tuple(got), " op")
    for name, v in got.items():
        assert torch.equal(v.detach(), want[name]), name
    adj = adjacency(case, gpu)
    y2, d2, s2 = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src))
    e2 = dev(case.a_edge, gpu).requires_grad_(True) if edge else None
    z2 = isplib_amd.gat_matmul(adj, y2, d2, s2, heads=heads, negative_slope=case.ns, a_edge=e2, dropout=case.p, training=True, seed=case.seed)
    z2.backward(g)
    for a, b in ((z2, z), (y2.grad, y.grad), (d2.grad, a_dst.grad), (s2.grad, a_src.grad)) + (((e2.grad, a_edge.grad),) if edge else ()):
        assert torch.equal(a.detach(), b.detach())
    mask = isplib_amd.gat_dropout_mask(adj, heads, case.p, case.seed)
    assert mask.device == z.device and np.array_equal(mask.cpu().numpy(), case.ref["q"])


def test_determinism_and_seed_handling(gpu):
    case = cases.config_case(8, 8)
    adj = adjacency(case, gpu)
    y, a_dst, a_src = dev(case.y, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu)
    z1 = adj.gat_matmul(y, a_dst, a_src, 8, case.ns, dropout=0.6, seed=11)
    z2 = adj.gat_matmul(y, a_dst, a_src, 8, case.ns, dropout=0.6, seed=11)
    z3 = adj.gat_matmul(y, a_dst, a_src, 8, case.ns, dropout=0.6, seed=12)
    assert torch.equal(z1, z2) and not torch.equal(z1, z3)
    torch.manual_seed(99)
    a = adj.gat_matmul(y, a_dst, a_src, 8, case.ns, dropout=0.6)
    b = adj.gat_matmul(y, a_dst, a_src, 8, case.ns, dropout=0.6)
    torch.manual_seed(99)
    c = adj.gat_matmul(y, a_dst, a_src, 8, case.ns, dropout=0.6)
    assert torch.equal(a, c) and not torch.equal(a, b)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()


@pytest.mark.parametrize("edge", (False, True), ids=("plain", "edge"))
def test_partial_gradients(gpu, edge):
    """Only a_dst asks: the columns kernel does not run -- the backward allocates nothing of y's size (its dy would be [N, K]) -- and
    d a_dst has the bits of the full call; every other subset of the inputs gets the full call's bits too."""
    case = cases.edge_case(8, 32) if edge else cases.config_case(8, 64)
    adj = adjacency(case, gpu)
    g = dev(case.g, gpu)
    kw = dict(dropout=case.p, seed=case.seed)

    def run(need):
        ops = {name: dev(a, gpu).requires_grad_(name in need) for name, a in
               (("y", case.y), ("a_dst", case.a_dst), ("a_src", case.a_src)) + ((("a_edge", case.a_edge),) if edge else ())}
        z = adj.gat_matmul(ops["y"], ops["a_dst"], ops["a_src"], case.heads, case.ns, a_edge=ops.get("a_edge"), **kw)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        z.backward(g)
        torch.cuda.synchronize()
        return z, {name: t.grad for name, t in ops.items()}, torch.cuda.max_memory_allocated() - before

    names = ("y", "a_dst", "a_src") + (("a_edge",) if edge else ())
    z, full, _ = run(names)
    assert all(full[name] is not None for name in names)
    z1, only, grew = run(("a_dst",))
    assert torch.equal(z1, z) and torch.equal(only["a_dst"], full["a_dst"])
    assert all(only[name] is None for name in names if name != "a_dst")
    assert grew < case.n * case.k * 4, grew                             # d a_dst and D, [M, H] each: no dy, so no columns kernel
    for need in (("y",), ("a_src",), ("y", "a_dst")) + ((("a_edge",), ("a_edge", "a_src")) if edge else ()):
        _, part, _ = run(need)
        for name in names:
            assert (part[name] is None) if name not in need else torch.equal(part[name], full[name]), (need, name)


@pytest.mark.parametrize("edge", (False, True), ids=("plain", "edge"))
def test_eval_mode_is_the_call_without_dropout(gpu, edge):
    case = cases.edge_case(8, 8) if edge else cases.config_case(8, 8)
    adj = adjacency(case, gpu)
    g = dev(case.g, gpu)

    def run(**kw):
        ops = [dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src) + ((case.a_edge,) if edge else ())]
        z = adj.gat_matmul(ops[0], ops[1], ops[2], case.heads, case.ns, a_edge=ops[3] if edge else None, **kw)
        z.backward(g)
        return [z.detach()] + [t.grad for t in ops]

    plain = run()
    for kw in (dict(dropout=0.6, training=False), dict(dropout=0.6, training=False, seed=3), dict(dropout=0.0), dict(dropout=0, seed=3)):
        for a, b in zip(run(**kw), plain):
            assert torch.equal(a, b), kw
    assert not torch.equal(run(dropout=0.6, seed=3)[0], plain[0])


def test_error_paths_raise_before_a_launch(gpu):
    from isplib_amd import cabi
    case = cases.config_case(2, 4)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    y, a_dst, a_src, g = (dev(a, gpu) for a in (case.y, case.a_dst, case.a_src, case.g))
    m, n, k, nnz = case.m, case.n, case.k, case.nnz
    z, lse = poisoned(gpu, m, k), poisoned(gpu, m, 2)
    for bad in (dict(threshold=-1), dict(threshold=2 ** 32), dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan")),
                dict(seed=-1), dict(seed=2 ** 63)):
        kw = dict(threshold=5, scale=2.5, seed=1)
        kw.update(bad)
        with pytest.raises(ValueError, match="`threshold`|`scale`|`seed`"):
            cabi.gat_drop(rowptr, col, y, a_dst, a_src, None, kw["threshold"], kw["scale"], kw["seed"], 2, out=(z, lse))
    L = cabi.lib()
    rp, cp = rowptr.data_ptr(), colptr.data_ptr()
    fw = lambda scale, heads=2: (m, n, k, nnz, col.data_ptr(), rp, rp + 8, a_dst.data_ptr(), y.data_ptr(), k, a_src.data_ptr(), None, heads,  # noqa: E731
                                 0.2, z.data_ptr(), k, lse.data_ptr(), None, 5, scale, 1)
    assert L.isplib_gat_drop_csr_hip(*fw(0.0)) == cabi.FAIL and "scale" in cabi.last_error()
    assert L.isplib_gat_drop_csr_hip(*fw(float("nan"))) == cabi.FAIL
    assert L.isplib_gat_drop_csr_hip(*fw(2.5, heads=0)) == cabi.NO_OPT_IMPL and "isplib_gat_serves" in cabi.last_error()
    dy, dasrc = poisoned(gpu, n, k), poisoned(gpu, n, 2)
    cols = lambda perm: (m, n, k, nnz, row_t.data_ptr(), cp, cp + 8, perm, a_dst.data_ptr(), y.data_ptr(), k, a_src.data_ptr(), None, 2, 0.2,  # noqa: E731
                         g.data_ptr(), k, lse.data_ptr(), lse.data_ptr(), dy.data_ptr(), k, dasrc.data_ptr(), None, 5, 2.5, 1)
    assert L.isplib_gat_drop_bw_cols_hip(*cols(None)) == cabi.FAIL and "null" in cabi.last_error()      # csr2csc is required without a_edge too
    torch.cuda.synchronize()
    assert torch.isnan(z).all() and torch.isnan(lse).all() and torch.isnan(dy).all() and torch.isnan(dasrc).all()
    with pytest.raises(RuntimeError, match="`p` must lie in"):
        torch.ops.isplib.gat_drop_spmm(rowptr, col, colptr, row_t, csr2csc, y, a_dst, a_src, None, 2, 0.2, 1.0, 1)
    with pytest.raises(RuntimeError, match="`seed` must be"):
        torch.ops.isplib.gat_drop_spmm(rowptr, col, colptr, row_t, csr2csc, y, a_dst, a_src, None, 2, 0.2, 0.5, -1)
