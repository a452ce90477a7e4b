"""The six attention families on rectangular graphs (M != N) on the GPU: attention.hip, gat.hip, gatv2.hip and their 16-bit twins, through
the C ABI wrappers of isplib_amd/cabi.py, the operators torch.ops.isplib.*_spmm{,16} under autograd and the plug-in surface
(attention_matmul, gat_matmul, gatv2_matmul).  Two shapes (tests/rect_cases.py): tall, M = 233 and N = 67, and wide, M = 67 and N = 233.
x, g, z, lse, D and a_dst have M rows; y, dy, a_src and dasrc have N rows.  The host entries take each gathered operand's extent from one
count and each launch grid from the other side's, so an m / n mix-up clips rows, over-reads a neighbour or leaves rows unwritten -- and
is invisible on the square graph every other attention test uses.  tests/test_rect_host.py shows on the CPU that each case here leaves its
bound under such a clip.

Nothing here has a tolerance of its own: every output is held to error / bound <= 1 by the family's own `held` helper, imported from
its GPU test file, against the fp64 reference and bounds of the family's *_ref.py.  The largest fraction per output is printed before
every assertion; DESIGN.md 4.6b-4.6g record them.
"""
import numpy as np
import pytest
import torch

from tests import rect_cases as rc
from tests import test_gpu_attention as t_att
from tests import test_gpu_attention16 as t_att16
from tests import test_gpu_gat as t_gat
from tests import test_gpu_gat16 as t_gat16
from tests import test_gpu_gatv2 as t_v2
from tests import test_gpu_gatv2_16 as t_v216

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
SHAPE = pytest.mark.parametrize("shape", tuple(rc.SHAPES))
SPEC_IDS = [f"h{h}d{d}-{rc.dtype_name(t)}" for h, d, t in rc.GAT16_SPECS]


def dev(a, gpu):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).to(gpu)


def leaf(a, gpu):
    return dev(a, gpu).requires_grad_(True)


def array(t):
    return t.detach().float().cpu().numpy()


def shaped(got, want):
    for name, shape in want.items():
        assert tuple(got[name].shape) == shape, (name, tuple(got[name].shape), shape)


def exact_edges(case, n, got, row_side, col_side):
    """An empty row's outputs and the unreferenced column's outputs are exactly 0 (lse = -inf is the helpers' own assertion)."""
    empty = ~case.live
    unreferenced = np.bincount(case.col, minlength=n) == 0
    assert empty.any() and unreferenced.any()
    for name in row_side:
        assert np.all(array(got[name])[empty] == 0), name
    for name in col_side:
        assert np.all(array(got[name])[unreferenced] == 0), name
    assert np.all(np.isneginf(array(got["lse"])[empty]))


def grads_match_operands(*leaves):
    for t in leaves:
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype


def weighted(case, n, gpu):
    """The structure as a SparseTensor [M, N] with random stored values: they are not read, so they must not matter."""
    import isplib_amd
    rowptr, col = dev(case.rowptr, gpu), dev(case.col, gpu)
    m = case.rowptr.size - 1
    return isplib_amd.SparseTensor.from_csr(rowptr, col, torch.rand(col.numel(), device=gpu) + 0.5, (m, n))


# ---- the C ABI wrappers: forward, bw_rows, bw_cols on colptr / row_t of a storage with sparse_sizes = (M, N) --------------------------

@SHAPE
@pytest.mark.parametrize("k", rc.ATTENTION_WIDTHS)
def test_attention_cabi(gpu, shape, k):
    case, (m, n) = rc.attention_case(shape, k), rc.SHAPES[shape]
    got = t_att.run_cabi(case, gpu)
    shaped(got, dict(z=(m, k), lse=(m,), dx=(m, k), D=(m,), dy=(n, k)))
    t_att.held(case, got, ("z", "lse", "dx", "D", "dy"))       # the fp32 family states no bound for D: it is held through dy, which reads it
    exact_edges(case, n, got, ("z", "dx", "D"), ("dy",))


@SHAPE
@pytest.mark.parametrize("dtype", (BF, FP), ids=rc.dtype_name)
@pytest.mark.parametrize("k", rc.ATTENTION16_WIDTHS)
def test_attention16_cabi(gpu, shape, k, dtype):
    case, (m, n) = rc.attention16_case(shape, k, dtype), rc.SHAPES[shape]
    got = t_att16.run_cabi(case, gpu)
    shaped(got, dict(z=(m, k), lse=(m,), dx=(m, k), D=(m,), dy=(n, k)))
    assert got["z"].dtype == got["dx"].dtype == got["dy"].dtype == dtype and got["lse"].dtype == got["D"].dtype == torch.float32
    t_att16.held(case, got)
    exact_edges(case, n, got, ("z", "dx", "D"), ("dy",))


@SHAPE
@pytest.mark.parametrize("heads,d", rc.GAT_CONFIGS)
def test_gat_cabi(gpu, shape, heads, d):
    case, (m, n), k = rc.gat_case(shape, heads, d), rc.SHAPES[shape], heads * d
    got = t_gat.run_cabi(case, gpu)
    shaped(got, dict(z=(m, k), lse=(m, heads), dadst=(m, heads), D=(m, heads), dy=(n, k), dasrc=(n, heads)))
    t_gat.held(case, got, t_gat.CABI_OUTPUTS)
    exact_edges(case, n, got, ("z", "dadst", "D"), ("dy", "dasrc"))


@SHAPE
@pytest.mark.parametrize("heads,d,dtype", rc.GAT16_SPECS, ids=SPEC_IDS)
def test_gat16_cabi_and_operator_bits(gpu, shape, heads, d, dtype):
    """check_case of tests/test_gpu_gat16.py: every output of the wrappers, then the operator's autograd gives the wrappers' bits."""
    case, (m, n), k = rc.gat16_case(shape, heads, d, dtype), rc.SHAPES[shape], heads * d
    got = t_gat16.check_case(case, gpu)
    shaped(got, dict(z=(m, k), lse=(m, heads), dadst=(m, heads), D=(m, heads), dy=(n, k), dasrc=(n, heads)))
    exact_edges(case, n, got, ("z", "dadst", "D"), ("dy", "dasrc"))


@SHAPE
@pytest.mark.parametrize("heads,d", rc.GAT_CONFIGS)
def test_gatv2_cabi(gpu, shape, heads, d):
    case, (m, n), k = rc.gatv2_case(shape, heads, d), rc.SHAPES[shape], heads * d
    got = t_v2.run_cabi(case, gpu)
    shaped(got, dict(z=(m, k), lse=(m, heads), dx=(m, k), D=(m, heads), datt=(heads, d), dy=(n, k)))
    t_v2.held(case, got, t_v2.CABI_OUTPUTS)
    exact_edges(case, n, got, ("z", "dx", "D"), ("dy",))
    assert torch.equal(t_v2.run_cabi(case, gpu)["datt"], got["datt"])              # the fold of att.grad repeats its bits


@SHAPE
@pytest.mark.parametrize("heads,d,dtype", rc.GAT16_SPECS, ids=SPEC_IDS)
def test_gatv2_16_cabi_and_operator_bits(gpu, shape, heads, d, dtype):
    """check_case of tests/test_gpu_gatv2_16.py: every output of the wrappers, then the operator's autograd gives the wrappers' bits."""
    case, (m, n), k = rc.gatv2_16_case(shape, heads, d, dtype), rc.SHAPES[shape], heads * d
    got = t_v216.check_case(case, gpu)
    shaped(got, dict(z=(m, k), lse=(m, heads), dx=(m, k), D=(m, heads), datt=(heads, d), dy=(n, k)))
    exact_edges(case, n, got, ("z", "dx", "D"), ("dy",))


# ---- the operators under autograd (every dense operand asks) and the plug-in surface on a weighted [M, N] SparseTensor -----------------

@SHAPE
@pytest.mark.parametrize("k", (33, 257))
def test_attention_operator_and_plugin(gpu, shape, k):
    import isplib_amd
    case, (m, n) = rc.attention_case(shape, k), rc.SHAPES[shape]
    rowptr, col = t_att.dev_graph(case, gpu)
    colptr, row_t = t_att.transposed(case, gpu)
    assert colptr.numel() == n + 1 and rowptr.numel() == m + 1
    g = dev(case.g, gpu)
    x, y = leaf(case.x, gpu), leaf(case.y, gpu)
    z = torch.ops.isplib.attention_spmm(rowptr, col, colptr, row_t, x, y, case.p)
    z.backward(g)
    assert tuple(z.shape) == (m, k) and z.dtype == torch.float32
    grads_match_operands(x, y)
    t_att.held(case, dict(z=z, dx=x.grad, dy=y.grad), ("z", "dx", "dy"))
    adj = weighted(case, n, gpu)
    x2, y2 = leaf(case.x, gpu), leaf(case.y, gpu)
    z2 = isplib_amd.attention_matmul(adj, x2, y2, case.p)
    z2.backward(g)
    assert torch.equal(z2.detach(), z.detach()) and torch.equal(x2.grad, x.grad) and torch.equal(y2.grad, y.grad)


@SHAPE
@pytest.mark.parametrize("k,dtype", ((34, BF), (512, FP)), ids=("k34-bf16", "k512-fp16"))
def test_attention16_operator_and_plugin(gpu, shape, k, dtype, monkeypatch):
    import isplib_amd
    case, (m, n) = rc.attention16_case(shape, k, dtype), rc.SHAPES[shape]
    rowptr, col = t_att16.dev_graph(case, gpu)
    colptr, row_t = t_att16.transposed(case, gpu)
    g = dev(case.g16, gpu)
    x, y = leaf(case.x16, gpu), leaf(case.y16, gpu)
    z = torch.ops.isplib.attention_spmm16(rowptr, col, colptr, row_t, x, y, case.p)
    z.backward(g)
    assert tuple(z.shape) == (m, k) and z.dtype == dtype
    grads_match_operands(x, y)
    t_att16.held(case, dict(z=z, dx=x.grad, dy=y.grad), ("z", "dx", "dy"))
    adj = weighted(case, n, gpu)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.setenv("ISPLIB_HALF_ATTENTION", "native")
    x2, y2 = leaf(case.x16, gpu), leaf(case.y16, gpu)
    z2 = isplib_amd.attention_matmul(adj, x2, y2, case.p)
    z2.backward(g)
    assert torch.equal(z2.detach(), z.detach()) and torch.equal(x2.grad, x.grad) and torch.equal(y2.grad, y.grad)
    monkeypatch.setenv("ISPLIB_HALF_ATTENTION", "convert")
    x3, y3 = leaf(case.x16, gpu), leaf(case.y16, gpu)
    z3 = isplib_amd.attention_matmul(adj, x3, y3, case.p)
    z3.backward(g)
    xh, yh = leaf(case.x16, gpu), leaf(case.y16, gpu)
    zh = isplib_amd.attention_matmul(adj, xh.float(), yh.float(), case.p).to(dtype)
    zh.backward(g)
    assert z3.dtype == dtype and torch.equal(z3.detach(), zh.detach()) and torch.equal(x3.grad, xh.grad) and torch.equal(y3.grad, yh.grad)
    grads_match_operands(x3, y3)


@SHAPE
@pytest.mark.parametrize("heads,d", ((1, 47), (8, 8)))
def test_gat_operator_and_plugin(gpu, shape, heads, d):
    import isplib_amd
    case, (m, n), k = rc.gat_case(shape, heads, d), rc.SHAPES[shape], heads * d
    rowptr, col = t_gat.dev_graph(case, gpu)
    colptr, row_t = t_gat.transposed(case, gpu)
    g = dev(case.g, gpu)
    y, a_dst, a_src = leaf(case.y, gpu), leaf(case.a_dst, gpu), leaf(case.a_src, gpu)
    z = torch.ops.isplib.gat_spmm(rowptr, col, colptr, row_t, y, a_dst, a_src, heads, case.ns)
    z.backward(g)
    assert tuple(z.shape) == (m, k) and tuple(a_dst.shape) == (m, heads) and tuple(a_src.shape) == (n, heads)
    grads_match_operands(y, a_dst, a_src)
    t_gat.held(case, dict(z=z, dy=y.grad, dadst=a_dst.grad, dasrc=a_src.grad), ("z", "dy", "dadst", "dasrc"), " op")
    adj = weighted(case, n, gpu)
    y2, d2, s2 = leaf(case.y, gpu), leaf(case.a_dst, gpu), leaf(case.a_src, gpu)
    z2 = isplib_amd.gat_matmul(adj, y2, d2, s2, heads=heads, negative_slope=case.ns)
    z2.backward(g)
    for a, b in ((z2, z), (y2.grad, y.grad), (d2.grad, a_dst.grad), (s2.grad, a_src.grad)):
        assert torch.equal(a.detach(), b.detach())


@SHAPE
@pytest.mark.parametrize("heads,d,dtype", ((1, 46, BF), (8, 8, FP)), ids=("h1d46-bf16", "h8d8-fp16"))
def test_gat16_operator_and_plugin(gpu, shape, heads, d, dtype, monkeypatch):
    import isplib_amd
    case, (m, n), k = rc.gat16_case(shape, heads, d, dtype), rc.SHAPES[shape], heads * d
    z, y, a_dst, a_src = t_gat16.run_op(case, gpu)
    assert tuple(z.shape) == (m, k) and z.dtype == dtype and tuple(a_dst.shape) == (m, heads) and tuple(a_src.shape) == (n, heads)
    grads_match_operands(y, a_dst, a_src)
    t_gat16.held(case, dict(z=z, dy=y.grad, dadst=a_dst.grad, dasrc=a_src.grad), ("z", "dy", "dadst", "dasrc"), "gat_spmm16")
    adj, g = weighted(case, n, gpu), dev(case.g16, gpu)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.setenv("ISPLIB_HALF_GAT", "native")
    y2, d2, s2 = leaf(case.y16, gpu), leaf(case.a_dst, gpu), leaf(case.a_src, gpu)
    z2 = isplib_amd.gat_matmul(adj, y2, d2, s2, heads, case.ns)
    z2.backward(g)
    for a, b in ((z2, z), (y2.grad, y.grad), (d2.grad, a_dst.grad), (s2.grad, a_src.grad)):
        assert torch.equal(a.detach(), b.detach())
    monkeypatch.setenv("ISPLIB_HALF_GAT", "convert")
    y3, d3, s3 = leaf(case.y16, gpu), leaf(case.a_dst, gpu), leaf(case.a_src, gpu)
    z3 = isplib_amd.gat_matmul(adj, y3, d3, s3, heads, case.ns)
    z3.backward(g)
    yh, dh, sh = leaf(case.y16, gpu), leaf(case.a_dst, gpu), leaf(case.a_src, gpu)
    zh = isplib_amd.gat_matmul(adj, yh.float(), dh, sh, heads, case.ns).to(dtype)
    zh.backward(g)
    assert z3.dtype == dtype
    for a, b in ((z3, zh), (y3.grad, yh.grad), (d3.grad, dh.grad), (s3.grad, sh.grad)):
        assert torch.equal(a.detach(), b.detach())
    grads_match_operands(y3, d3, s3)


@SHAPE
@pytest.mark.parametrize("heads,d", ((1, 47), (8, 8)))
def test_gatv2_operator_and_plugin(gpu, shape, heads, d):
    import isplib_amd
    case, (m, n), k = rc.gatv2_case(shape, heads, d), rc.SHAPES[shape], heads * d
    rowptr, col = t_v2.dev_graph(case, gpu)
    colptr, row_t = t_v2.transposed(case, gpu)
    g = dev(case.g, gpu)
    x, y, att = leaf(case.x, gpu), leaf(case.y, gpu), leaf(case.att, gpu)
    z = torch.ops.isplib.gatv2_spmm(rowptr, col, colptr, row_t, x, y, att, heads, case.ns)
    z.backward(g)
    assert tuple(z.shape) == (m, k) and tuple(x.shape) == (m, k) and tuple(y.shape) == (n, k)
    grads_match_operands(x, y, att)
    t_v2.held(case, dict(z=z, dx=x.grad, dy=y.grad, datt=att.grad), ("z", "dx", "dy", "datt"), " op")
    adj = weighted(case, n, gpu)
    x2, y2, a2 = leaf(case.x, gpu), leaf(case.y, gpu), leaf(case.att, gpu)
    z2 = isplib_amd.gatv2_matmul(adj, x2, a2, y2, heads=heads, negative_slope=case.ns)
    z2.backward(g)
    for a, b in ((z2, z), (x2.grad, x.grad), (y2.grad, y.grad), (a2.grad, att.grad)):
        assert torch.equal(a.detach(), b.detach())


@SHAPE
@pytest.mark.parametrize("heads,d,dtype", ((1, 46, BF), (8, 8, FP)), ids=("h1d46-bf16", "h8d8-fp16"))
def test_gatv2_16_operator_and_plugin(gpu, shape, heads, d, dtype, monkeypatch):
    import isplib_amd
    case, (m, n), k = rc.gatv2_16_case(shape, heads, d, dtype), rc.SHAPES[shape], heads * d
    z, x, y, att = t_v216.run_op(case, gpu)
    assert tuple(z.shape) == (m, k) and z.dtype == dtype and tuple(x.shape) == (m, k) and tuple(y.shape) == (n, k)
    grads_match_operands(x, y, att)
    t_v216.held(case, dict(z=z, dx=x.grad, dy=y.grad, datt=att.grad), t_v216.OP_OUTPUTS, "gatv2_spmm16")
    adj, g = weighted(case, n, gpu), dev(case.g16, gpu)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "native")
    x2, y2, a2 = leaf(case.x16, gpu), leaf(case.y16, gpu), leaf(case.att, gpu)
    z2 = isplib_amd.gatv2_matmul(adj, x2, a2, y2, heads, case.ns)
    z2.backward(g)
    for a, b in ((z2, z), (x2.grad, x.grad), (y2.grad, y.grad), (a2.grad, att.grad)):
        assert torch.equal(a.detach(), b.detach())
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "convert")
    x3, y3, a3 = leaf(case.x16, gpu), leaf(case.y16, gpu), leaf(case.att, gpu)
    z3 = isplib_amd.gatv2_matmul(adj, x3, a3, y3, heads, case.ns)
    z3.backward(g)
    xh, yh, ah = leaf(case.x16, gpu), leaf(case.y16, gpu), leaf(case.att, gpu)
    zh = isplib_amd.gatv2_matmul(adj, xh.float(), ah, yh.float(), heads, case.ns).to(dtype)
    zh.backward(g)
    assert z3.dtype == dtype
    for a, b in ((z3, zh), (x3.grad, xh.grad), (y3.grad, yh.grad), (a3.grad, ah.grad)):
        assert torch.equal(a.detach(), b.detach())
    grads_match_operands(x3, y3, a3)


# ---- refusals on a rectangular matrix: raised by the plug-in's own checks, before any launch --------------------------------------------

@SHAPE
def test_the_plugin_refuses_what_only_a_square_matrix_admits(gpu, shape):
    import isplib_amd
    m, n = rc.SHAPES[shape]
    case = rc.attention_case(shape, 3)
    adj = weighted(case, n, gpu)
    x, y = dev(case.x, gpu), dev(case.y, gpu)
    x_n, y_m = torch.zeros(n, 3, device=gpu), torch.zeros(m, 3, device=gpu)            # the two row counts swapped
    with pytest.raises(ValueError, match="square"):
        isplib_amd.attention_matmul(adj, x)
    with pytest.raises(ValueError, match="one row per row"):
        isplib_amd.attention_matmul(adj, x_n, y_m)
    with pytest.raises(ValueError, match="one row per row"):
        isplib_amd.attention_matmul(adj, x_n, y)
    with pytest.raises(ValueError, match="one row per column"):
        isplib_amd.attention_matmul(adj, x, y_m)

    v2 = rc.gatv2_case(shape, 8, 8)
    x, y, att = dev(v2.x, gpu), dev(v2.y, gpu), dev(v2.att, gpu)
    x_n, y_m = torch.zeros(n, 64, device=gpu), torch.zeros(m, 64, device=gpu)
    with pytest.raises(ValueError, match="square"):
        isplib_amd.gatv2_matmul(adj, x, att, heads=8)
    with pytest.raises(ValueError, match="one row per row"):
        isplib_amd.gatv2_matmul(adj, x_n, att, y_m, heads=8)
    with pytest.raises(ValueError, match="one row per row"):
        isplib_amd.gatv2_matmul(adj, x_n, att, y, heads=8)
    with pytest.raises(ValueError, match="one row per column"):
        isplib_amd.gatv2_matmul(adj, x, att, y_m, heads=8)

    gat = rc.gat_case(shape, 8, 8)
    y, a_dst, a_src = dev(gat.y, gpu), dev(gat.a_dst, gpu), dev(gat.a_src, gpu)
    with pytest.raises(ValueError, match="one row per column"):
        isplib_amd.gat_matmul(adj, y_m, a_dst, a_src, 8)
    with pytest.raises(ValueError, match=rf"`a_dst` must be \[{m}, 8\]"):
        isplib_amd.gat_matmul(adj, y, torch.zeros(n, 8, device=gpu), a_src, 8)
    with pytest.raises(ValueError, match=rf"`a_src` must be \[{n}, 8\]"):
        isplib_amd.gat_matmul(adj, y, a_dst, torch.zeros(m, 8, device=gpu), 8)
    with pytest.raises(ValueError, match=rf"`a_src` must be \[{n}, 8\]"):
        isplib_amd.gat_matmul(adj, y, a_dst, a_dst, 8)                                 # one tensor for both scores
    with pytest.raises(ValueError, match=rf"`a_dst` must be \[{m}, 8\]"):
        isplib_amd.gat_matmul(adj, y, a_src, a_src, 8)
    torch.cuda.synchronize()


# ---- write-only outputs and scratch: NaN-filled wider buffers, launched twice ----------------------------------------------------------

PAD = 64


def nan_view(gpu, rows, cols=None, dtype=torch.float32, ld=None):
    """-> (buffer, view): [rows, cols] at pitch ld (cols when None), or [rows], at the start of a NaN-filled buffer PAD elements longer."""
    if cols is None:
        buf = torch.full((rows + PAD,), float("nan"), device=gpu, dtype=dtype)
        return buf, buf[:rows]
    ld = cols if ld is None else ld
    buf = torch.full((rows * ld + PAD,), float("nan"), device=gpu, dtype=dtype)
    return buf, buf[:rows * ld].view(rows, ld)[:, :cols]


def written_and_nothing_else(name, buf, view):
    assert not torch.isnan(view).any(), f"{name}: an element was not written"
    if view.dim() == 2:
        rows, cols, ld = view.size(0), view.size(1), view.stride(0)
        assert torch.isnan(buf[:rows * ld].view(rows, ld)[:, cols:]).all(), f"{name}: written between the rows"
        assert torch.isnan(buf[rows * ld:]).all(), f"{name}: written past the end"
    else:
        assert torch.isnan(buf[view.numel():]).all(), f"{name}: written past the end"


def twice(gpu, specs, launch):
    """Run `launch(views)` twice on fresh NaN-filled buffers built from specs = {name: nan_view arguments}: every element of every output
    is written, the padding keeps its fill, and the second launch gives the first one's bits.  Returns the first run's outputs."""
    runs = []
    for _ in range(2):
        bufs = {name: nan_view(gpu, *args) for name, args in specs.items()}
        launch({name: view for name, (_, view) in bufs.items()})
        for name, (buf, view) in bufs.items():
            written_and_nothing_else(name, buf, view)
        runs.append({name: view.clone() for name, (_, view) in bufs.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    return runs[0]


@SHAPE
def test_attention_outputs_are_write_only(gpu, shape):
    from isplib_amd import cabi
    k = 33
    case, (m, n) = rc.attention_case(shape, k), rc.SHAPES[shape]
    rowptr, col = t_att.dev_graph(case, gpu)
    colptr, row_t = t_att.transposed(case, gpu)
    x, y, g = dev(case.x, gpu), dev(case.y, gpu), dev(case.g, gpu)

    def launch(o):
        cabi.attention(rowptr, col, x, y, case.p, out=(o["z"], o["lse"]), check=False)
        cabi.attention_bw_rows(rowptr, col, x, y, g, o["z"], o["lse"], case.p, out=(o["dx"], o["D"]), check=False)
        cabi.attention_bw_cols(colptr, row_t, x, y, g, o["lse"], o["D"], case.p, out=o["dy"], check=False)

    got = twice(gpu, dict(z=(m, k), lse=(m,), dx=(m, k), D=(m,), dy=(n, k)), launch)
    t_att.held(case, got, ("z", "lse", "dx", "dy"))


@SHAPE
def test_attention16_outputs_are_write_only(gpu, shape):
    from isplib_amd import cabi
    k, dtype = 34, BF
    case, (m, n) = rc.attention16_case(shape, k, dtype), rc.SHAPES[shape]
    rowptr, col = t_att16.dev_graph(case, gpu)
    colptr, row_t = t_att16.transposed(case, gpu)
    x, y, g = dev(case.x16, gpu), dev(case.y16, gpu), dev(case.g16, gpu)

    def launch(o):
        cabi.attention16(rowptr, col, x, y, case.p, out=(o["z"], o["lse"]), check=False)
        cabi.attention16_bw_rows(rowptr, col, x, y, g, o["lse"], case.p, out=(o["dx"], o["D"]), check=False)
        cabi.attention16_bw_cols(colptr, row_t, x, y, g, o["lse"], o["D"], case.p, out=o["dy"], check=False)

    got = twice(gpu, dict(z=(m, k, dtype, k + 6), lse=(m,), dx=(m, k, dtype, k + 6), D=(m,), dy=(n, k, dtype, k + 6)), launch)
    t_att16.held(case, got)


@SHAPE
def test_gat_outputs_are_write_only(gpu, shape):
    from isplib_amd import cabi
    H, d = 3, 128
    case, (m, n), k = rc.gat_case(shape, H, d), rc.SHAPES[shape], H * d
    rowptr, col = t_gat.dev_graph(case, gpu)
    colptr, row_t = t_gat.transposed(case, gpu)
    y, a_dst, a_src, g, ns = dev(case.y, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu), dev(case.g, gpu), case.ns

    def launch(o):
        cabi.gat(rowptr, col, y, a_dst, a_src, H, ns, out=(o["z"], o["lse"]), check=False)
        cabi.gat_bw_rows(rowptr, col, y, a_dst, a_src, g, o["z"], o["lse"], H, ns, out=(o["dadst"], o["D"]), check=False)
        cabi.gat_bw_cols(colptr, row_t, y, a_dst, a_src, g, o["lse"], o["D"], H, ns, out=(o["dy"], o["dasrc"]), check=False)

    got = twice(gpu, dict(z=(m, k), lse=(m, H), dadst=(m, H), D=(m, H), dy=(n, k), dasrc=(n, H)), launch)
    t_gat.held(case, got, t_gat.CABI_OUTPUTS)


@SHAPE
def test_gat16_outputs_are_write_only(gpu, shape):
    from isplib_amd import cabi
    H, d, dtype = 8, 8, BF
    case, (m, n), k = rc.gat16_case(shape, H, d, dtype), rc.SHAPES[shape], H * d
    rowptr, col = t_gat16.dev_graph(case, gpu)
    colptr, row_t = t_gat16.transposed(case, gpu)
    y, g, a_dst, a_src, ns = dev(case.y16, gpu), dev(case.g16, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu), case.ns

    def launch(o):
        cabi.gat16_forward(rowptr, col, y, a_dst, a_src, H, ns, out=(o["z"], o["lse"]), check=False)
        cabi.gat16_backward_rows(rowptr, col, y, a_dst, a_src, g, o["lse"], H, ns, out=(o["dadst"], o["D"]), check=False)
        cabi.gat16_backward_cols(colptr, row_t, y, a_dst, a_src, g, o["lse"], o["D"], H, ns, out=(o["dy"], o["dasrc"]), check=False)

    got = twice(gpu, dict(z=(m, k, dtype, k + 6), lse=(m, H), dadst=(m, H), D=(m, H), dy=(n, k, dtype, k + 6), dasrc=(n, H)), launch)
    t_gat16.held(case, got)


def scratch(gpu, need):
    """A workspace of `need` bytes inside a buffer of 0xFF bytes (0xFFFFFFFF: a NaN in every float) 256 bytes longer."""
    return torch.full((need + 256,), 0xFF, device=gpu, dtype=torch.uint8)


@SHAPE
def test_gatv2_outputs_and_workspace_are_write_only(gpu, shape):
    from isplib_amd import cabi
    H, d = 3, 128
    case, (m, n), k = rc.gatv2_case(shape, H, d), rc.SHAPES[shape], H * d
    rowptr, col = t_v2.dev_graph(case, gpu)
    colptr, row_t = t_v2.transposed(case, gpu)
    x, y, att, g, ns = dev(case.x, gpu), dev(case.y, gpu), dev(case.att, gpu), dev(case.g, gpu), case.ns
    need = cabi.gatv2_bw_rows_workspace_bytes(m, k)

    def launch(o):
        work = scratch(gpu, need)
        cabi.gatv2(rowptr, col, x, y, att, H, ns, out=(o["z"], o["lse"]), check=False)
        cabi.gatv2_bw_rows(rowptr, col, x, y, att, g, o["z"], o["lse"], H, ns, out=(o["dx"], o["D"], o["datt"]), workspace=work[:need],
                           check=False)
        cabi.gatv2_bw_cols(colptr, row_t, x, y, att, g, o["lse"], o["D"], H, ns, out=o["dy"], check=False)
        assert (work[need:] == 0xFF).all(), "the rows kernel wrote past its workspace"

    got = twice(gpu, dict(z=(m, k), lse=(m, H), dx=(m, k), D=(m, H), datt=(H, d), dy=(n, k)), launch)
    t_v2.held(case, got, t_v2.CABI_OUTPUTS)


@SHAPE
def test_gatv2_16_outputs_and_workspace_are_write_only(gpu, shape):
    from isplib_amd import cabi
    H, d, dtype = 8, 8, BF
    case, (m, n), k = rc.gatv2_16_case(shape, H, d, dtype), rc.SHAPES[shape], H * d
    rowptr, col = t_v216.dev_graph(case, gpu)
    colptr, row_t = t_v216.transposed(case, gpu)
    x, y, g, att, ns = dev(case.x16, gpu), dev(case.y16, gpu), dev(case.g16, gpu), dev(case.att, gpu), case.ns
    need = cabi.gatv2_16_bw_rows_workspace_bytes(m, k)

    def launch(o):
        work = scratch(gpu, need)
        cabi.gatv2_16_forward(rowptr, col, x, y, att, H, ns, out=(o["z"], o["lse"]), check=False)
        cabi.gatv2_16_backward_rows(rowptr, col, x, y, att, g, o["lse"], H, ns, out=(o["dx"], o["D"], o["datt"]), workspace=work[:need],
                                    check=False)
        cabi.gatv2_16_backward_cols(colptr, row_t, x, y, att, g, o["lse"], o["D"], H, ns, out=o["dy"], check=False)
        assert (work[need:] == 0xFF).all(), "the rows kernel wrote past its workspace"

    got = twice(gpu, dict(z=(m, k, dtype, k + 6), lse=(m, H), dx=(m, k, dtype, k + 6), D=(m, H), datt=(H, d), dy=(n, k, dtype, k + 6)), launch)
    t_v216.held(case, got)
