"""Sparse multi-head dot-product attention with separate keys and values on the GPU (isplib_amd/csrc/mha.hip): the C ABI wrappers,
torch.ops.isplib.mha_spmm with its autograd backward, and the plug-in surface, each held to the per-element bounds of tests/mha_ref.py
against the fp64 reference (inputs, references and bounds: tests/mha_cases.py, computed once per case).  The largest error / bound seen
per output is printed before every assertion; DESIGN.md 4.6k records it.
"""
import numpy as np
import pytest
import torch

from tests import attention_ref
from tests import mha_cases as cases
from tests import mha_ref as ref
from tests import rect_cases

pytestmark = pytest.mark.gpu

CABI_OUTPUTS = ("z", "lse", "dq", "D", "dk", "dv")
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
    print(f"mha error/bound {case.name}{what}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def run_cabi(case, gpu, q=None, k=None, v=None, g=None):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    q = dev(case.q, gpu) if q is None else q
    k = dev(case.k, gpu) if k is None else k
    v = dev(case.v, gpu) if v is None else v
    g = dev(case.g, gpu) if g is None else g
    z, lse = cabi.mha(rowptr, col, q, k, v, case.heads, case.p)
    dq, D = cabi.mha_bw_rows(rowptr, col, q, k, v, g, z, lse, case.heads, case.p)
    colptr, row_t = transposed(case, gpu)
    dk, dv = cabi.mha_bw_cols(colptr, row_t, q, k, v, g, lse, D, case.heads, case.p)
    return dict(z=z, lse=lse, dq=dq, D=D, dk=dk, dv=dv)


def check_cabi(case, gpu):
    got = run_cabi(case, gpu)
    held(case, got, CABI_OUTPUTS)
    empty = ~case.live
    assert empty.any()
    for name in ("z", "dq", "D"):
        assert np.all(got[name].cpu().numpy()[empty] == 0), name                # exact zeros; lse = -inf is asserted by held()
    unreferenced = np.bincount(case.col, minlength=case.n) == 0
    assert unreferenced.any()
    for name in ("dk", "dv"):
        assert np.all(got[name].cpu().numpy()[unreferenced] == 0), name
    return got


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_cabi_entries_at_every_configuration(gpu, heads, d):
    """Every LPR instantiation, first, last and ragged; heads of one lane up to a whole chunk; both chunks in one head and in two."""
    check_cabi(cases.config_case(heads, d), gpu)


@pytest.mark.parametrize("case", cases.scale_cases(), ids=lambda c: c.name)
def test_cabi_entries_with_an_explicit_scale(gpu, case):
    """A scale other than 1 / sqrt(d), and a negative one, through the wrappers and through the plug-in."""
    import isplib_amd
    got = check_cabi(case, gpu)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    q, k, v = (dev(a, gpu).requires_grad_(True) for a in (case.q, case.k, case.v))
    z = adj.mha_matmul(q, k, v, case.heads, case.p)
    z.backward(dev(case.g, gpu))
    for a, b in ((z, "z"), (q.grad, "dq"), (k.grad, "dk"), (v.grad, "dv")):
        assert torch.equal(a.detach(), got[b]), b
    default = adj.mha_matmul(q.detach(), k.detach(), v.detach(), case.heads)
    assert not torch.equal(default, got["z"])


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_operator_and_plugin_under_autograd(gpu, heads, d):
    """torch.ops.isplib.mha_spmm and mha_matmul / SparseTensor.mha_matmul give the bits of the C ABI path; a weighted storage too
    (stored values are not read); only the requested gradients are computed."""
    import isplib_amd
    case = cases.config_case(heads, d)
    want = run_cabi(case, gpu)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    g = dev(case.g, gpu)
    q, k, v = (dev(a, gpu).requires_grad_(True) for a in (case.q, case.k, case.v))
    z = torch.ops.isplib.mha_spmm(rowptr, col, colptr, row_t, q, k, v, heads, case.p)
    z.backward(g)
    for a, b in ((z, "z"), (q.grad, "dq"), (k.grad, "dk"), (v.grad, "dv")):
        assert torch.equal(a.detach(), want[b]), b
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, torch.rand(col.numel(), device=gpu) + 0.5, (case.m, case.n))
    q2, k2, v2 = (dev(a, gpu).requires_grad_(True) for a in (case.q, case.k, case.v))
    z2 = isplib_amd.mha_matmul(adj, q2, k2, v2, heads=heads)                   # scale=None: 1 / sqrt(d)
    z2.backward(g)
    for a, b in ((z2, "z"), (q2.grad, "dq"), (k2.grad, "dk"), (v2.grad, "dv")):
        assert torch.equal(a.detach(), want[b]), b
    # one operand asks at a time: the others stay None
    for pos, name in enumerate(("dq", "dk", "dv")):
        ops = [dev(a, gpu) for a in (case.q, case.k, case.v)]
        ops[pos].requires_grad_(True)
        adj.mha_matmul(*ops, heads).backward(g)
        assert torch.equal(ops[pos].grad, want[name]), name
        assert all(t.grad is None for i, t in enumerate(ops) if i != pos), name


@pytest.mark.parametrize("heads,d", ((1, 47), (8, 8)))
def test_k_is_v_adds_both_parts_and_meets_attention_matmul(gpu, heads, d):
    """k is v: the one tensor's gradient is dk + dv, held to the sum of the two bounds.  The same call spelled with attention_matmul
    (one call at H = 1, one per head on column views at (8, 8)) lies within its own bounds of the same fp64 reference, so the two
    results differ by at most the sum of both bounds."""
    import isplib_amd
    case = cases.shared_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    g = dev(case.g, gpu)
    q, k = dev(case.q, gpu).requires_grad_(True), dev(case.k, gpu).requires_grad_(True)
    z = adj.mha_matmul(q, k, k, heads)
    z.backward(g)
    held(case, dict(z=z, dq=q.grad), ("z", "dq"), " k is v")
    frac = ref.worst(k.grad.cpu().numpy(), case.ref["dk"] + case.ref["dv"], case.bound["dk"] + case.bound["dv"])
    print(f"mha error/bound {case.name}: dk+dv={frac:.4f}")
    assert frac <= 1.0
    # attention_matmul, head by head, with its own reference bounds
    qa, ka = dev(case.q, gpu).requires_grad_(True), dev(case.k, gpu).requires_grad_(True)
    za = torch.cat([adj.attention_matmul(qa[:, h * d:(h + 1) * d], ka[:, h * d:(h + 1) * d], case.p) for h in range(heads)], 1)
    za.backward(g)
    zb, dxb, dyb = [], [], []
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        r = attention_ref.attention(case.rowptr, case.col, case.q[:, sl], case.k[:, sl], case.p, case.g[:, sl])
        b = attention_ref.bounds(case.rowptr, case.col, case.q[:, sl], case.k[:, sl], case.p, r, case.g[:, sl])
        zb.append(b["z"]), dxb.append(b["dx"]), dyb.append(b["dy"])
    both = dict(z=case.bound["z"] + np.concatenate(zb, 1), dq=case.bound["dq"] + np.concatenate(dxb, 1),
                dkv=case.bound["dk"] + case.bound["dv"] + np.concatenate(dyb, 1))
    fr = dict(z=ref.worst(z.detach().cpu().numpy(), za.detach().cpu().numpy().astype(np.float64), both["z"]),
              dq=ref.worst(q.grad.cpu().numpy(), qa.grad.cpu().numpy().astype(np.float64), both["dq"]),
              dkv=ref.worst(k.grad.cpu().numpy(), ka.grad.cpu().numpy().astype(np.float64), both["dkv"]))
    print(f"mha vs attention_matmul, difference / sum of both bounds {case.name}: " + " ".join(f"{n}={x:.4f}" for n, x in fr.items()))
    assert all(x <= 1.0 for x in fr.values()), fr


@pytest.mark.parametrize("heads,d", cases.FUSED_CONFIGS)
def test_views_of_one_fused_projection(gpu, heads, d):
    """q, k, v as the three column blocks of one [N, 3K] tensor: the bits of contiguous copies, and the fused tensor's gradient is the
    concatenation of the three."""
    import isplib_amd
    case = cases.config_case(heads, d)
    K = case.width
    want = run_cabi(case, gpu)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    fused = torch.cat([dev(case.q, gpu), dev(case.k, gpu), dev(case.v, gpu)], 1).requires_grad_(True)
    q, k, v = fused[:, :K], fused[:, K:2 * K], fused[:, 2 * K:]
    assert not k.is_contiguous() and k.stride(0) == 3 * K
    z = adj.mha_matmul(q, k, v, heads)
    z.backward(dev(case.g, gpu))
    assert torch.equal(z.detach(), want["z"])
    assert torch.equal(fused.grad, torch.cat([want["dq"], want["dk"], want["dv"]], 1))
    got = run_cabi(case, gpu, q=q.detach(), k=k.detach(), v=v.detach())         # the wrappers take the views at their pitch too
    for name in CABI_OUTPUTS:
        assert torch.equal(got[name], want[name]), name


def test_one_entry_rows_return_v_bit_for_bit(gpu):
    case = cases.single_case()
    got = run_cabi(case, gpu)
    z, lse = got["z"].cpu().numpy(), got["lse"].cpu().numpy()
    live = case.live
    want = np.zeros_like(case.v)
    want[live] = case.v[case.col]
    assert np.array_equal(z.view(np.uint32), want.view(np.uint32))
    # lse is the score: within delta s_e + 2 eps |s_e| of fp64
    s = case.ref["s"]
    qe = np.abs(ref.per_head(case.q.astype(np.float64), case.heads))[case.ref["row"]]
    ke = np.abs(ref.per_head(case.k.astype(np.float64), case.heads))[case.col]
    slack = ref.ACC * abs(case.p) * (qe * ke).sum(2) + 2.0 * ref.EPS * np.abs(s)
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
def test_zero_q_gives_the_unit_weight_mean_of_v(gpu, heads, d):
    from isplib_amd import cabi
    case = cases.zero_q_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    v = dev(case.v, gpu)
    z, lse = cabi.mha(rowptr, col, dev(case.q, gpu), dev(case.k, gpu), v, heads)
    mean, _ = cabi.spmm(rowptr, col, None, v, "mean")
    frac = ref.worst(z.cpu().numpy(), mean.cpu().numpy().astype(np.float64), case.bound["z"])
    print(f"mha error/bound zero q vs mean h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    live = case.live
    assert np.allclose(case.ref["lse"][live], np.log(np.diff(case.rowptr)[live])[:, None], rtol=1e-12)   # lse = log deg
    frac = ref.worst(lse.cpu().numpy()[live], case.ref["lse"][live], case.bound["lse"][live])
    print(f"mha error/bound zero q h{heads}d{d}: lse={frac:.4f}")
    assert frac <= 1.0 and np.all(np.isneginf(lse.cpu().numpy()[~live]))


@pytest.mark.parametrize("heads,d", cases.RECT_CONFIGS)
@pytest.mark.parametrize("shape", tuple(rect_cases.SHAPES))
def test_rectangular_graphs(gpu, shape, heads, d):
    """M != N: q, g, z, lse, D and dq have M rows, k, v, dk and dv have N rows; through the C ABI and the plug-in."""
    import isplib_amd
    case = cases.rect_case(shape, heads, d)
    assert (case.m, case.n) == rect_cases.SHAPES[shape]
    got = check_cabi(case, gpu)
    assert got["dq"].shape == (case.m, case.width) and got["dk"].shape == got["dv"].shape == (case.n, case.width)
    assert got["lse"].shape == got["D"].shape == (case.m, heads)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    q, k, v = (dev(a, gpu).requires_grad_(True) for a in (case.q, case.k, case.v))
    z = adj.mha_matmul(q, k, v, heads)
    z.backward(dev(case.g, gpu))
    assert q.grad.shape == q.shape and k.grad.shape == k.shape and v.grad.shape == v.shape
    for a, b in ((z, "z"), (q.grad, "dq"), (k.grad, "dk"), (v.grad, "dv")):
        assert torch.equal(a.detach(), got[b]), b


@pytest.mark.parametrize("heads,d", ((1, 3), (5, 8), (1, 512), (8, 64)))
def test_outputs_are_write_only_and_launches_repeat(gpu, heads, d):
    """NaN-filled, over-allocated outputs, launched twice: every element is written, nothing past the end, equal bits; pitched outputs
    with a NaN pad come back fully written with the pad untouched."""
    from isplib_amd import cabi
    case = cases.config_case(heads, d)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    q, k, v, g = (dev(a, gpu) for a in (case.q, case.k, case.v, case.g))
    m, n, K, pad, H, p = case.m, case.n, case.width, 64, heads, case.p

    def fresh(rows, cols):
        buf = torch.full((rows * cols + pad,), float("nan"), device=gpu)
        return buf, buf[:rows * cols].view(rows, cols)

    runs = []
    for _ in range(2):
        b = {name: fresh(*shape) for name, shape in (("z", (m, K)), ("lse", (m, H)), ("dq", (m, K)), ("D", (m, H)), ("dk", (n, K)),
                                                     ("dv", (n, K)))}
        cabi.mha(rowptr, col, q, k, v, H, p, out=(b["z"][1], b["lse"][1]), check=False)
        cabi.mha_bw_rows(rowptr, col, q, k, v, g, b["z"][1], b["lse"][1], H, p, out=(b["dq"][1], b["D"][1]), check=False)
        cabi.mha_bw_cols(colptr, row_t, q, k, v, g, b["lse"][1], b["D"][1], H, p, out=(b["dk"][1], b["dv"][1]), check=False)
        for name, (buf, view) in b.items():
            assert not torch.isnan(view).any(), name
            assert torch.isnan(buf[view.numel():]).all(), name
        runs.append({name: view.clone() for name, (_, view) in b.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    # pitched outputs: nothing is written between the rows
    buf = torch.full((m, K + 3), float("nan"), device=gpu)
    cabi.mha(rowptr, col, q, k, v, H, p, out=(buf[:, :K], torch.empty(m, H, device=gpu)))
    assert torch.equal(buf[:, :K], runs[0]["z"]) and torch.isnan(buf[:, K:]).all()
    buf = torch.full((m, K + 3), float("nan"), device=gpu)
    cabi.mha_bw_rows(rowptr, col, q, k, v, g, runs[0]["z"], runs[0]["lse"], H, p, out=(buf[:, :K], torch.empty(m, H, device=gpu)))
    assert torch.equal(buf[:, :K], runs[0]["dq"]) and torch.isnan(buf[:, K:]).all()
    bk, bv = torch.full((n, K + 3), float("nan"), device=gpu), torch.full((n, K + 5), float("nan"), device=gpu)
    cabi.mha_bw_cols(colptr, row_t, q, k, v, g, runs[0]["lse"], runs[0]["D"], H, p, out=(bk[:, :K], bv[:, :K]))
    assert torch.equal(bk[:, :K], runs[0]["dk"]) and torch.isnan(bk[:, K:]).all()
    assert torch.equal(bv[:, :K], runs[0]["dv"]) and torch.isnan(bv[:, K:]).all()


def test_error_paths_raise_before_a_launch(gpu):
    import isplib_amd
    from isplib_amd import cabi
    case = cases.config_case(2, 4)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    q, k, v = dev(case.q, gpu), dev(case.k, gpu), dev(case.v, gpu)
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.mha_matmul(q.cpu(), k, v, 2)
    with pytest.raises(TypeError, match="GPU tensor"):
        adj.mha_matmul(q, k, v.cpu(), 2)
    with pytest.raises(ValueError, match="2-D"):
        adj.mha_matmul(q[0], k, v, 2)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32"):
            adj.mha_matmul(q.to(dt), k.to(dt), v.to(dt), 2)
    with pytest.raises(ValueError, match="one row per column"):
        adj.mha_matmul(q, k[:-1], v, 2)
    with pytest.raises(ValueError, match="one row per column"):
        adj.mha_matmul(q, k, v[:-1], 2)
    with pytest.raises(ValueError, match="one row per row"):
        adj.mha_matmul(q[:-1], k, v, 2)
    with pytest.raises(ValueError, match="power of two"):
        adj.mha_matmul(*(torch.zeros(case.m, 12, device=gpu) for _ in range(3)), 2)
    with pytest.raises(ValueError, match="512"):
        adj.mha_matmul(*(torch.zeros(case.m, 1024, device=gpu) for _ in range(3)), 2)
    with pytest.raises(ValueError, match="`scale`"):
        adj.mha_matmul(q, k, v, 2, float("inf"))
    # the wrappers: structure checks that read the device
    with pytest.raises(ValueError, match="ascend"):
        cabi.mha(torch.flip(rowptr, (0,)), col, q, k, v, 2)
    bad = col.clone()
    bad[3] = case.m
    with pytest.raises(ValueError, match=r"lie in \[0, 200\)"):
        cabi.mha(rowptr, bad, q, k, v, 2)
    # the operator: every shape before a launch
    z12 = torch.zeros(case.m, 12, device=gpu)
    for args in ((q, k[:-1], v, 2, 0.5), (q, k, v[:-1], 2, 0.5), (q[:-1], k, v, 2, 0.5), (q, k, v, 3, 0.5), (z12, z12, z12, 2, 0.5),
                 (q, k, v.cpu(), 2, 0.5), (q, k, v, 2, float("nan"))):
        with pytest.raises(RuntimeError, match="mha_spmm|GPU tensor"):
            torch.ops.isplib.mha_spmm(rowptr, col, rowptr, col, *args)
    with pytest.raises(RuntimeError, match="mha_spmm"):
        torch.ops.isplib.mha_spmm(rowptr[:-1], col, rowptr, col, q, k, v, 2, 0.5)
    # the entries themselves: outside the domain NO_OPT_IMPL, bad arguments FAIL, nothing to do SUCCESS -- all without a launch, on
    # outputs that stay poisoned
    L = cabi.lib()
    m, rp = case.m, rowptr.data_ptr()
    big = torch.zeros(m, 1024, device=gpu)
    z, lse = torch.full((m, 1024), float("nan"), device=gpu), torch.full((m, 128), float("nan"), device=gpu)
    dk, dv = torch.full((m, 1024), float("nan"), device=gpu), torch.full((m, 1024), float("nan"), device=gpu)
    bp = big.data_ptr()

    def fw(mm, kk, ldk, ldv, heads, qp, scale=0.5):
        return L.isplib_mha_csr_hip(mm, m, kk, col.numel(), col.data_ptr(), rp, rp + 8, heads, scale, qp, 1024, bp, ldk, bp, ldv,
                                    z.data_ptr(), 1024, lse.data_ptr(), None)

    assert fw(m, 516, 516, 516, 1, bp) == cabi.NO_OPT_IMPL and "isplib_mha_serves" in cabi.last_error()
    assert fw(m, 12, 12, 12, 2, bp) == cabi.NO_OPT_IMPL                # d = 6
    assert fw(m, 4, 4, 4, 2, bp) == cabi.NO_OPT_IMPL                   # d = 2
    assert fw(m, 8, 7, 8, 2, bp) == cabi.NO_OPT_IMPL                   # ldk < k: each gathered operand at its own pitch
    assert fw(m, 8, 8, 7, 2, bp) == cabi.NO_OPT_IMPL                   # ldv < k
    assert fw(m, 8, 8, 8, 0, bp) == cabi.NO_OPT_IMPL
    assert fw(m, 9, 9, 9, 2, bp) == cabi.FAIL                          # k is no multiple of heads
    assert fw(-1, 8, 8, 8, 2, bp) == cabi.FAIL
    assert fw(m, 8, 8, 8, 2, bp, float("nan")) == cabi.FAIL and "scale" in cabi.last_error()
    assert fw(m, 8, 8, 8, 2, None) == cabi.FAIL and "null" in cabi.last_error()
    assert fw(0, 8, 8, 8, 2, None) == cabi.SUCCESS and fw(m, 0, 8, 8, 2, None) == cabi.SUCCESS

    def rows(ldk, ldv, lddq):
        return L.isplib_mha_bw_rows_hip(m, m, 8, col.numel(), col.data_ptr(), rp, rp + 8, 2, 0.5, bp, 1024, bp, ldk, bp, ldv, bp, 1024,
                                        bp, 1024, bp, z.data_ptr(), lddq, lse.data_ptr(), None)

    assert rows(7, 8, 1024) == cabi.NO_OPT_IMPL and rows(8, 7, 1024) == cabi.NO_OPT_IMPL and rows(8, 8, 7) == cabi.FAIL

    def cols(ldq, ldg, lddk, lddv):
        return L.isplib_mha_bw_cols_hip(m, m, 8, col.numel(), col.data_ptr(), rp, rp + 8, 2, 0.5, bp, ldq, bp, ldg, bp, bp, bp, 1024, bp,
                                        1024, dk.data_ptr(), lddk, dv.data_ptr(), lddv, None)

    assert cols(7, 8, 1024, 1024) == cabi.NO_OPT_IMPL and cols(8, 7, 1024, 1024) == cabi.NO_OPT_IMPL
    assert cols(8, 8, 7, 1024) == cabi.FAIL and cols(8, 8, 1024, 7) == cabi.FAIL
    torch.cuda.synchronize()
    for t in (z, lse, dk, dv):
        assert torch.isnan(t).all()                                     # nothing was launched: the outputs stay poisoned
