"""GAT aggregation with a per-edge score term on the GPU (isplib_amd/csrc/gat.hip, EDGE kernels): the C ABI wrappers,
torch.ops.isplib.gat_edge_spmm with its autograd backward, and gat_matmul(..., a_edge=...), each held to the per-element bounds of
tests/gat_edge_ref.py against the fp64 reference (inputs, references and bounds: tests/gat_edge_cases.py, computed once per case).  The
largest error / bound seen per output is printed before every assertion; DESIGN.md 4.6h records it.
"""
import numpy as np
import pytest
import torch

from tests import gat_edge_cases as cases
from tests import gat_edge_ref as ref

pytestmark = pytest.mark.gpu

CABI_OUTPUTS = ("z", "lse", "dadst", "D", "dy", "dasrc", "daedge")
IDS = [f"h{h}d{d}" for h, d in cases.CONFIGS]


def dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def dev_graph(case, gpu):
    return dev(case.rowptr, gpu), dev(case.col, gpu)


def transposed(case, gpu):
    """colptr / row_t / csr2csc as SparseStorage caches them (the library's own csr2csc)."""
    import isplib_amd
    rowptr, col = dev_graph(case, gpu)
    st = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n)).storage
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
    print(f"gat_edge error/bound {case.name}{what}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def poisoned(gpu, *shape):
    return torch.full(shape, float("nan"), device=gpu)


def run_cabi(case, gpu, y=None, a_edge=None, g=None):
    """The three entries on NaN-filled outputs."""
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    y = dev(case.y, gpu) if y is None else y
    a_dst, a_src = dev(case.a_dst, gpu), dev(case.a_src, gpu)
    a_edge = dev(case.a_edge, gpu) if a_edge is None else a_edge
    g = dev(case.g, gpu) if g is None else g
    m, n, k, H, nnz = case.m, case.n, case.k, case.heads, case.nnz
    z, lse = cabi.gat_edge(rowptr, col, y, a_dst, a_src, a_edge, H, case.ns, out=(poisoned(gpu, m, k), poisoned(gpu, m, H)))
    dadst, D, daedge = cabi.gat_edge_bw_rows(rowptr, col, y, a_dst, a_src, a_edge, g, z, lse, H, case.ns,
                                             out=(poisoned(gpu, m, H), poisoned(gpu, m, H), poisoned(gpu, nnz, H)))
    colptr, row_t, csr2csc = transposed(case, gpu)
    dy, dasrc = cabi.gat_edge_bw_cols(colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, g, lse, D, H, case.ns,
                                      out=(poisoned(gpu, n, k), poisoned(gpu, n, H)))
    return dict(z=z, lse=lse, dadst=dadst, D=D, dy=dy, dasrc=dasrc, daedge=daedge)


def check_cabi(case, gpu):
    """Every output within its bound, element by element, on NaN-filled outputs; a second launch gives the same bits."""
    got = run_cabi(case, gpu)
    held(case, got, CABI_OUTPUTS)
    for name in CABI_OUTPUTS:
        v = got[name].cpu().numpy()
        assert not np.isnan(v).any(), name                              # every element was written
    empty = ~case.live
    for name in ("z", "dadst", "D"):
        assert np.all(got[name].cpu().numpy()[empty] == 0), name
    again = run_cabi(case, gpu)
    for name in CABI_OUTPUTS:
        assert torch.equal(got[name], again[name]), name
    return got


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_cabi_entries_at_every_configuration(gpu, heads, d):
    check_cabi(cases.config_case(heads, d), gpu)


@pytest.mark.parametrize("case", cases.slope_cases() + [cases.edge_only_case()], ids=lambda c: c.name)
def test_cabi_entries_at_every_slope_and_with_the_edge_term_alone(gpu, case):
    check_cabi(case, gpu)


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_operator_and_plugin_under_autograd(gpu, heads, d):
    """torch.ops.isplib.gat_edge_spmm and gat_matmul / SparseTensor.gat_matmul with a_edge give the same bits; a_edge without
    requires_grad gets None and leaves the other gradients bit for bit; a_edge alone asking still gets the right gradient."""
    import isplib_amd
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    g = dev(case.g, gpu)
    y, a_dst, a_src, a_edge = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src, case.a_edge))
    z = torch.ops.isplib.gat_edge_spmm(rowptr, col, colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, heads, case.ns)
    z.backward(g)
    held(case, dict(z=z, dy=y.grad, dadst=a_dst.grad, dasrc=a_src.grad, daedge=a_edge.grad), ("z", "dy", "dadst", "dasrc", "daedge"), " op")
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, torch.rand(col.numel(), device=gpu) + 0.5, (case.m, case.n))
    y2, d2, s2, e2 = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src, case.a_edge))
    z2 = isplib_amd.gat_matmul(adj, y2, d2, s2, heads=heads, negative_slope=case.ns, a_edge=e2)
    z2.backward(g)
    for a, b in ((z2, z), (y2.grad, y.grad), (d2.grad, a_dst.grad), (s2.grad, a_src.grad), (e2.grad, a_edge.grad)):
        assert torch.equal(a.detach(), b.detach())
    # a_edge does not ask: None for it, the others unchanged bit for bit
    y3, d3, s3, e3 = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src, case.a_edge))
    e3.requires_grad_(False)
    adj.gat_matmul(y3, d3, s3, heads, case.ns, e3).backward(g)
    assert e3.grad is None and torch.equal(y3.grad, y.grad) and torch.equal(d3.grad, a_dst.grad) and torch.equal(s3.grad, a_src.grad)
    # only a_edge asks: the columns kernel does not run, the others stay None
    y4, d4, s4, e4 = dev(case.y, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu), dev(case.a_edge, gpu).requires_grad_(True)
    adj.gat_matmul(y4, d4, s4, heads, case.ns, a_edge=e4).backward(g)
    assert y4.grad is None and d4.grad is None and s4.grad is None and torch.equal(e4.grad, a_edge.grad)
    if heads == 1:                                                          # the scores, a_edge included, may be 1-D
        d5, s5, e5 = (dev(a[:, 0], gpu).requires_grad_(True) for a in (case.a_dst, case.a_src, case.a_edge))
        z5 = adj.gat_matmul(dev(case.y, gpu), d5, s5, a_edge=e5)
        z5.backward(g)
        assert torch.equal(z5.detach(), z.detach()) and torch.equal(e5.grad, a_edge.grad[:, 0]) and torch.equal(d5.grad, a_dst.grad[:, 0])


@pytest.mark.parametrize("heads,d", ((1, 41), (8, 8), (3, 128), (1, 512), (2, 4), (4, 32), (1, 129)))
def test_zero_edge_term_gives_the_bits_of_the_operator_without_it(gpu, heads, d):
    """(a + b) + 0 is exact, and the kernels are one template: z and the gradients of y, a_dst and a_src are equal bit for bit.  The
    last three configurations complete the set of instantiations (LPR = 8, 32 and 64 with one chunk)."""
    import isplib_amd
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    g = dev(case.g, gpu)
    y0, d0, s0 = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src))
    z0 = adj.gat_matmul(y0, d0, s0, heads, case.ns)
    z0.backward(g)
    y1, d1, s1 = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src))
    e1 = torch.zeros(case.nnz, heads, device=gpu, requires_grad=True)
    z1 = adj.gat_matmul(y1, d1, s1, heads, case.ns, a_edge=e1)
    z1.backward(g)
    for name, a, b in (("z", z1, z0), ("dy", y1.grad, y0.grad), ("dadst", d1.grad, d0.grad), ("dasrc", s1.grad, s0.grad)):
        assert torch.equal(a.detach(), b.detach()), name
    assert e1.grad is not None and torch.isfinite(e1.grad).all()


def test_duplicates_are_entries_of_their_own(gpu):
    """Two stored entries (i, j) with different a_edge rows: each gets its own d a_edge, within its bound -- indexing per (i, j)
    would give both the same."""
    case = cases.duplicate_case()
    got = check_cabi(case, gpu)
    e1, e2 = case.pairs[0]
    da = got["daedge"].cpu().numpy().astype(np.float64)
    for e in (e1, e2):
        assert np.all(np.abs(da[e] - case.ref["daedge"][e]) <= case.bound["daedge"][e]), e
    assert np.any(da[e1] != da[e2])
    gap = np.abs(case.ref["daedge"][e1] - case.ref["daedge"][e2]) > 10.0 * (case.bound["daedge"][e1] + case.bound["daedge"][e2])
    assert gap.any() and np.all(np.abs(da[e1] - da[e2])[gap] > 8.0 * (case.bound["daedge"][e1] + case.bound["daedge"][e2])[gap])
    # swapping the two rows of a_edge swaps the two gradients: the pair shares i and j, so nothing else tells them apart
    swapped = np.array(case.a_edge)
    swapped[[e1, e2]] = swapped[[e2, e1]]
    other = run_cabi(case, gpu, a_edge=dev(swapped, gpu))["daedge"].cpu().numpy()
    assert np.all(np.abs(other[e1] - case.ref["daedge"][e2]) <= case.bound["daedge"][e2])
    assert np.all(np.abs(other[e2] - case.ref["daedge"][e1]) <= case.bound["daedge"][e1])


def test_one_entry_rows_return_y_bit_for_bit(gpu):
    """Whatever the score, |u| of thousands included; a_e = 1 and D = t_e bit for bit, so d a_edge is exactly 0."""
    case = cases.single_case()
    got = run_cabi(case, gpu)
    z = got["z"].cpu().numpy()
    live = case.live
    want = np.zeros_like(case.y)
    want[live] = case.y[case.col]
    assert np.array_equal(z.view(np.uint32), want.view(np.uint32))
    f32 = np.float32
    u32 = ((case.a_dst[case.ref["row"]] + case.a_src[case.col]).astype(f32) + case.a_edge).astype(f32)       # TWO fp32 adds, then the slope
    s32 = np.where(u32 > 0, u32, (f32(case.ns) * u32).astype(f32)).astype(f32)
    lse = got["lse"].cpu().numpy()
    assert np.all(np.isneginf(lse[~live])) and np.array_equal(lse[live].view(np.uint32), s32.view(np.uint32))
    da = got["daedge"].cpu().numpy()
    assert da.shape == (case.nnz, case.heads) and np.all(da == 0)
    held(case, got, CABI_OUTPUTS)


def test_edge_term_spread_over_200(gpu):
    case = cases.large_case()
    got = run_cabi(case, gpu)
    for name in CABI_OUTPUTS:
        v = got[name].cpu().numpy()
        assert np.all(np.isfinite(v[case.live] if name == "lse" else v)), name
    held(case, got, CABI_OUTPUTS)


def test_rectangular_graph(gpu):
    """M != N, with csr2csc of the rectangular structure; through the entries and through the plug-in."""
    import isplib_amd
    case = cases.rect_case()
    assert case.m != case.n
    got = check_cabi(case, gpu)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    y, a_dst, a_src, a_edge = (dev(a, gpu).requires_grad_(True) for a in (case.y, case.a_dst, case.a_src, case.a_edge))
    z = adj.gat_matmul(y, a_dst, a_src, case.heads, case.ns, a_edge=a_edge)
    z.backward(dev(case.g, gpu))
    for name, a in (("z", z), ("dy", y.grad), ("dadst", a_dst.grad), ("dasrc", a_src.grad), ("daedge", a_edge.grad)):
        assert torch.equal(a.detach(), got[name]), name


@pytest.mark.parametrize("heads,d", ((8, 8), (2, 256)))
def test_a_nan_in_the_edge_term_poisons_one_head_of_one_row(gpu, heads, d):
    case = cases.config_case(heads, d)
    i = int(np.argmax(np.diff(case.rowptr) == 9))
    e, h = int(case.rowptr[i]) + 4, heads - 1
    a_edge = np.array(case.a_edge)
    a_edge[e, h] = np.nan
    got = run_cabi(case, gpu, a_edge=dev(a_edge, gpu))
    z, lse = ref.per_head(got["z"].cpu().numpy(), heads), got["lse"].cpu().numpy()
    assert np.all(np.isnan(z[i, h])) and np.isnan(lse[i, h])
    clean = np.ones((case.m, heads), bool)
    clean[i, h] = False
    want, bound = ref.per_head(case.ref["z"], heads), ref.per_head(case.bound["z"], heads)
    frac = ref.worst(z[clean], want[clean], bound[clean])
    print(f"gat_edge error/bound nan a_edge, everything else h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    ok = clean & case.live[:, None]
    assert ref.worst(lse[ok], case.ref["lse"][ok], case.bound["lse"][ok]) <= 1.0


@pytest.mark.parametrize("heads,d", ((1, 41), (8, 8), (3, 128)))
def test_pitched_column_block_and_non_contiguous_views(gpu, heads, d):
    """A pitched y, a column-block view of y and a non-contiguous a_edge (which is copied) give the bits of the packed operands."""
    import isplib_amd
    case = cases.config_case(heads, d)
    k = case.k
    packed = run_cabi(case, gpu)
    buf = torch.full((case.n * (k + 5) + 9,), float("nan"), device=gpu)
    pitched = buf[1:1 + case.n * (k + 5)].view(case.n, k + 5)[:, :k]
    pitched.copy_(dev(case.y, gpu))
    assert pitched.stride(0) == k + 5
    got = run_cabi(case, gpu, y=pitched)
    for name in CABI_OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    wide = torch.randn(case.n, 3 * k, device=gpu)
    wide[:, 2 * k:] = dev(case.y, gpu)
    got = run_cabi(case, gpu, y=wide[:, 2 * k:])
    for name in CABI_OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    yw = wide.clone().requires_grad_(True)
    e_t = dev(case.a_edge, gpu).t().contiguous().requires_grad_(True)          # [heads, nnz]: its transpose is a_edge, non-contiguous
    a_edge = e_t.t() if heads > 1 else torch.stack([dev(case.a_edge, gpu), torch.zeros(case.nnz, 1, device=gpu)], 2)[:, :, 0]
    assert not a_edge.is_contiguous() and tuple(a_edge.shape) == (case.nnz, heads)
    a_dst, a_src = dev(case.a_dst, gpu).requires_grad_(True), dev(case.a_src, gpu).requires_grad_(True)
    z = adj.gat_matmul(yw[:, 2 * k:], a_dst, a_src, heads, case.ns, a_edge=a_edge)
    z.backward(dev(case.g, gpu))
    assert torch.equal(z.detach(), packed["z"]) and torch.equal(yw.grad[:, 2 * k:], packed["dy"]) and not yw.grad[:, :2 * k].any()
    assert torch.equal(a_dst.grad, packed["dadst"]) and torch.equal(a_src.grad, packed["dasrc"])
    if heads > 1:
        assert torch.equal(e_t.grad.t(), packed["daedge"])


FAR_HEADS_CHECKED = (0, 63, 64, 127)


def test_the_far_end_of_the_edge_table(gpu):
    """heads = 128, d = 4, N = M = 64, nnz the largest with nnz * 128 * 4 <= 3.5 GiB (a_edge and d a_edge: 3.5 GiB each, about 7.5 GiB
    with the structure), rows of equal length.  a_edge is zero but for seeded values on the entries of the first and last row; the last
    row's entries reference two columns no other row does.  Rows are independent, and so are heads: the first and last row of z, the
    last row's d a_edge and d a_src / dy of its private columns are checked against the fp64 reference of those rows alone, computed
    for the first and last head of each of a lane's two chunks (0, 63, 64, 127: the reference of one such row over all 128 heads is
    59 M elements per array, minutes of NumPy); the other heads of those rows are checked to be finite and written.  A row has
    deg = nnz / 64 = 114688 entries, so rho = 8 eps (R + deg + 4) is 0.055, not inside the first-order range the small cases are held
    to: the bound is used as it stands (its second-order part is rho^2 / 2, under 3 % of it)."""
    from isplib_amd import cabi
    heads, d, M = 128, 4, 64
    k, N, ns = heads * d, M, 0.2
    nnz = cabi.DENSE_BYTES_MAX // (4 * heads)
    assert cabi.gat_edge_serves(nnz, heads) and not cabi.gat_edge_serves(nnz + 1, heads) and nnz % M == 0
    per = nnz // M
    private = np.array([N - 2, N - 1])                                  # the last row's columns: no other row references them
    rowptr = torch.arange(0, M + 1, device=gpu, dtype=torch.int64) * per
    col = (torch.arange(nnz, device=gpu, dtype=torch.int64) * 7 + 3) % (N - 2)
    col[nnz - per:] = torch.arange(per, device=gpu, dtype=torch.int64) % 2 + (N - 2)
    y, g = cases.normal((N, k), 32), cases.normal((M, k), 33)
    a_dst, a_src = cases.normal((M, heads), 34), cases.normal((N, heads), 35)
    seeded = {0: cases.normal((per, heads), 36, 0.5), M - 1: cases.normal((per, heads), 37, 0.5)}
    a_edge = torch.zeros(nnz, heads, device=gpu)
    a_edge[:per] = dev(seeded[0], gpu)
    a_edge[nnz - per:] = dev(seeded[M - 1], gpu)
    colptr, perm, row_t, _ = cabi.csr2csc(rowptr, col, None, N, want_val=False)
    yd, gd, add, asd = dev(y, gpu), dev(g, gpu), dev(a_dst, gpu), dev(a_src, gpu)
    z, lse = cabi.gat_edge(rowptr, col, yd, add, asd, a_edge, heads, ns, check=False)
    daedge = poisoned(gpu, nnz, heads)
    dadst, D, _ = cabi.gat_edge_bw_rows(rowptr, col, yd, add, asd, a_edge, gd, z, lse, heads, ns, check=False,
                                        out=(poisoned(gpu, M, heads), poisoned(gpu, M, heads), daedge))
    dy, dasrc = cabi.gat_edge_bw_cols(colptr, row_t, perm, yd, add, asd, a_edge, gd, lse, D, heads, ns, check=False)
    torch.cuda.synchronize()
    for t in (z, lse, dadst, D, dy, dasrc):
        assert torch.isfinite(t).all()
    # every element of d a_edge was written: both ends whole, the 3.5 GiB between them on a strided sample of its rows
    assert torch.isfinite(daedge[:per]).all() and torch.isfinite(daedge[nnz - per:]).all() and torch.isfinite(daedge[::509]).all()
    hs = np.array(FAR_HEADS_CHECKED)
    cols = (hs[:, None] * d + np.arange(d)).ravel()
    col_cpu, zc = col.cpu().numpy(), z.cpu().numpy()
    rp = np.array([0, per], dtype=np.int64)
    for i in (0, M - 1):
        cl = col_cpu[i * per:(i + 1) * per]
        ops = (y[:, cols], a_dst[i:i + 1, hs], a_src[:, hs], seeded[i][:, hs])
        one = ref.gat_edge(rp, cl, *ops, hs.size, ns, g[i:i + 1, cols])
        bound = ref.bounds(rp, cl, *ops, hs.size, ns, one, g[i:i + 1, cols])
        assert float(bound["rho"].max()) <= 0.06, float(bound["rho"].max())
        frac = {"z": ref.worst(zc[i:i + 1, cols], one["z"], bound["z"])}
        if i == M - 1:
            frac["daedge"] = ref.worst(daedge[nnz - per:].cpu().numpy()[:, hs], one["daedge"], bound["daedge"])
            frac["dasrc"] = ref.worst(dasrc.cpu().numpy()[private][:, hs], one["dasrc"][private], bound["dasrc"][private])
            frac["dy"] = ref.worst(dy.cpu().numpy()[private][:, cols], one["dy"][private], bound["dy"][private])
        print(f"gat_edge error/bound far end, row {i}: " + " ".join(f"{k_}={v:.4f}" for k_, v in frac.items()))
        assert all(v <= 1.0 for v in frac.values()), (i, frac)


def test_error_paths_raise_before_a_launch(gpu):
    import isplib_amd
    from isplib_amd import cabi
    case = cases.config_case(2, 4)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    y, a_dst, a_src, a_edge, g = (dev(a, gpu) for a in (case.y, case.a_dst, case.a_src, case.a_edge, case.g))
    nnz, m, n, k = case.nnz, case.m, case.n, case.k
    z, lse = poisoned(gpu, m, k), poisoned(gpu, m, 2)

    def still_poisoned():
        torch.cuda.synchronize()
        return bool(torch.isnan(z).all()) and bool(torch.isnan(lse).all())

    # the plug-in
    with pytest.raises(ValueError, match=rf"`a_edge` must be \[{nnz}, 2\]"):
        adj.gat_matmul(y, a_dst, a_src, 2, a_edge=a_edge[:-1])
    with pytest.raises(ValueError, match=rf"`a_edge` must be \[{nnz}, 2\]"):
        adj.gat_matmul(y, a_dst, a_src, 2, a_edge=a_edge[:, :1])
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.gat_matmul(y, a_dst, a_src, 2, a_edge=a_edge.cpu())
    with pytest.raises(TypeError, match="float32"):
        adj.gat_matmul(y, a_dst, a_src, 2, a_edge=a_edge.double())
    # the wrappers, on poisoned outputs
    with pytest.raises(ValueError, match=rf"`a_edge` must be \[{nnz}, 2\]"):
        cabi.gat_edge(rowptr, col, y, a_dst, a_src, a_edge[:-1], 2, out=(z, lse))
    with pytest.raises(ValueError, match=rf"`a_edge` must be \[{nnz}, 2\]"):
        cabi.gat_edge(rowptr, col, y, a_dst, a_src, a_edge[:, :1], 2, out=(z, lse))
    with pytest.raises(ValueError, match="contiguous"):
        cabi.gat_edge(rowptr, col, y, a_dst, a_src, a_edge.t().contiguous().t(), 2, out=(z, lse))
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.gat_edge(rowptr, col, y, a_dst, a_src, a_edge.cpu(), 2, out=(z, lse))
    with pytest.raises(TypeError, match="float32"):
        cabi.gat_edge(rowptr, col, y, a_dst, a_src, a_edge.half(), 2, out=(z, lse))
    assert still_poisoned()
    dy, dasrc = poisoned(gpu, n, k), poisoned(gpu, n, 2)
    zz, ll = cabi.gat_edge(rowptr, col, y, a_dst, a_src, a_edge, 2)
    _, D, _ = cabi.gat_edge_bw_rows(rowptr, col, y, a_dst, a_src, a_edge, g, zz, ll, 2, want_edge=False)
    with pytest.raises(ValueError, match=rf"`csr2csc` must be a 1-D tensor of {nnz} entries"):
        cabi.gat_edge_bw_cols(colptr, row_t, csr2csc[:-1], y, a_dst, a_src, a_edge, g, ll, D, 2, out=(dy, dasrc))
    with pytest.raises(TypeError, match="int64"):
        cabi.gat_edge_bw_cols(colptr, row_t, csr2csc.int(), y, a_dst, a_src, a_edge, g, ll, D, 2, out=(dy, dasrc))
    bad = csr2csc.clone()
    bad[5] = nnz
    with pytest.raises(ValueError, match=rf"lie in \[0, {nnz}\)"):
        cabi.gat_edge_bw_cols(colptr, row_t, bad, y, a_dst, a_src, a_edge, g, ll, D, 2, out=(dy, dasrc))
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.gat_edge_bw_cols(colptr, row_t, csr2csc.cpu(), y, a_dst, a_src, a_edge, g, ll, D, 2, out=(dy, dasrc), check=False)
    torch.cuda.synchronize()
    assert torch.isnan(dy).all() and torch.isnan(dasrc).all()
    # the operator: every shape before a launch
    op = torch.ops.isplib.gat_edge_spmm
    for args in ((csr2csc, y, a_dst, a_src, a_edge[:-1]), (csr2csc, y, a_dst, a_src, a_edge[:, :1]), (csr2csc[:-1], y, a_dst, a_src, a_edge),
                 (csr2csc, y, a_dst, a_src, a_edge.cpu()), (csr2csc, y, a_dst, a_src, a_edge.double()), (csr2csc, y[:-1], a_dst, a_src, a_edge),
                 (csr2csc.int(), y, a_dst, a_src, a_edge)):
        with pytest.raises(RuntimeError, match="isplib: gat_(edge_)?spmm|GPU tensor|float32|int64"):      # y, a_dst, a_src: gat_spmm's own checks
            op(rowptr, col, colptr, row_t, *args, 2, 0.2)
    # the entries themselves: outside either domain NO_OPT_IMPL, bad arguments FAIL, nothing to do SUCCESS -- all without a launch
    L = cabi.lib()
    rp = rowptr.data_ptr()
    far = cabi.DENSE_BYTES_MAX // 8 + 1                                 # nnz * 2 heads * 4 bytes: the first refused

    def args(m_, k_, nnz_, heads, ep):
        return (m_, n, k_, nnz_, col.data_ptr(), rp, rp + 8, a_dst.data_ptr(), y.data_ptr(), k, a_src.data_ptr(), ep, heads, 0.2,
                z.data_ptr(), max(k, k_), lse.data_ptr(), None)              # every one of these calls is refused: nothing is written

    ep = a_edge.data_ptr()
    assert L.isplib_gat_edge_csr_hip(*args(m, k, far, 2, ep)) == cabi.NO_OPT_IMPL and "isplib_gat_edge_serves" in cabi.last_error()
    assert L.isplib_gat_edge_csr_hip(*args(m, k, 2 ** 31, 2, ep)) == cabi.NO_OPT_IMPL
    assert L.isplib_gat_edge_csr_hip(*args(m, 12, nnz, 2, ep)) == cabi.NO_OPT_IMPL and "isplib_gat_serves" in cabi.last_error()      # d = 6
    assert L.isplib_gat_edge_csr_hip(*args(m, k, nnz, 0, ep)) == cabi.NO_OPT_IMPL
    assert L.isplib_gat_edge_csr_hip(*args(m, k, nnz, 2, None)) == cabi.FAIL and "null" in cabi.last_error()
    assert L.isplib_gat_edge_csr_hip(*args(m, k, -1, 2, ep)) == cabi.FAIL
    assert L.isplib_gat_edge_csr_hip(*args(m, 9, nnz, 2, ep)) == cabi.FAIL                                   # k is no multiple of heads
    assert L.isplib_gat_edge_csr_hip(*args(0, k, nnz, 2, None)) == cabi.SUCCESS
    assert L.isplib_gat_edge_csr_hip(*args(m, 0, nnz, 2, None)) == cabi.SUCCESS
    cp = colptr.data_ptr()
    cols = lambda nnz_, perm, ep_: (m, n, k, nnz_, row_t.data_ptr(), cp, cp + 8, perm, a_dst.data_ptr(), y.data_ptr(), k, a_src.data_ptr(),  # noqa: E731
                                    ep_, 2, 0.2, g.data_ptr(), k, ll.data_ptr(), D.data_ptr(), dy.data_ptr(), k, dasrc.data_ptr(), None)
    assert L.isplib_gat_edge_bw_cols_hip(*cols(nnz, None, ep)) == cabi.FAIL and "null" in cabi.last_error()
    assert L.isplib_gat_edge_bw_cols_hip(*cols(far, csr2csc.data_ptr(), ep)) == cabi.NO_OPT_IMPL
    assert still_poisoned() and torch.isnan(dy).all() and torch.isnan(dasrc).all()
    # nnz == 0 launches with empty descriptors: every row is empty
    empty_ptr = torch.zeros(m + 1, dtype=torch.int64, device=gpu)
    none = torch.empty(0, dtype=torch.int64, device=gpu)
    z0, lse0 = cabi.gat_edge(empty_ptr, none, y, a_dst, a_src, torch.empty(0, 2, device=gpu), 2, out=(z, lse))
    assert not z0.any() and torch.isneginf(lse0).all()
