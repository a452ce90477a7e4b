"""Sparse multi-head attention (q, k, v) with attention dropout on the GPU (isplib_amd/csrc/mha.hip, DROP kernels): the C ABI wrappers,
torch.ops.isplib.mha_drop_spmm with its autograd backward, and mha_matmul(..., dropout=, training=, seed=), each held to the
per-element bounds of tests/mha_dropout_ref.py against the reference with the same mask (inputs, references and bounds:
tests/mha_dropout_cases.py, computed once per case).  The largest error / bound seen per output is printed before every assertion;
DESIGN.md 4.6m records it.
"""
import numpy as np
import pytest
import torch

from tests import mha_dropout_cases as cases
from tests import mha_dropout_ref as ref

pytestmark = pytest.mark.gpu

OUTPUTS = ("z", "lse", "dq", "D", "dk", "dv")
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
    print(f"mha_dropout error/bound {case.name}{what}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def poisoned(gpu, *shape):
    return torch.full(shape, float("nan"), device=gpu)


def run_cabi(case, gpu, threshold=None, scale=None, seed=None, operands=None):
    """The three entries on NaN-filled outputs, with the case's mask unless another (threshold, keep scale, seed) is given.
    `operands`: (q, k, v) device tensors to use in place of the case's packed ones (views at a pitch of their own)."""
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    q, k, v = operands if operands is not None else (dev(case.q, gpu), dev(case.k, gpu), dev(case.v, gpu))
    g = dev(case.g, gpu)
    T = case.threshold if threshold is None else threshold
    c = case.scale if scale is None else scale
    sd = case.seed if seed is None else seed
    m, n, K, H = case.m, case.n, case.width, case.heads
    z, lse = cabi.mha_drop(rowptr, col, q, k, v, T, c, sd, H, case.ps, out=(poisoned(gpu, m, K), poisoned(gpu, m, H)))
    dq, D = cabi.mha_drop_bw_rows(rowptr, col, q, k, v, g, z, lse, T, c, sd, H, case.ps, out=(poisoned(gpu, m, K), poisoned(gpu, m, H)))
    colptr, row_t, csr2csc = transposed(case, gpu)
    dk, dv = cabi.mha_drop_bw_cols(colptr, row_t, csr2csc, q, k, v, g, lse, D, T, c, sd, H, case.ps,
                                   out=(poisoned(gpu, n, K), poisoned(gpu, n, K)))
    return dict(z=z, lse=lse, dq=dq, D=D, dk=dk, dv=dv)


def check_cabi(case, gpu):
    """Every output within its bound, element by element, on NaN-filled outputs; an empty row and a (row, head) that lost every entry
    have z = 0 exactly, the latter with a finite lse."""
    got = run_cabi(case, gpu)
    held(case, got, OUTPUTS)
    for name in OUTPUTS:
        assert not np.isnan(got[name].cpu().numpy()).any(), name        # every element was written
    empty = ~case.live
    for name in ("z", "dq", "D"):
        assert np.all(got[name].cpu().numpy()[empty] == 0), name
    gone = case.all_dropped()
    assert np.all(ref.per_head(got["z"].cpu().numpy(), case.heads)[gone] == 0) and np.all(np.isfinite(got["lse"].cpu().numpy()[gone]))
    return got


@pytest.mark.parametrize("heads,d", cases.CONFIGS, ids=IDS)
def test_cabi_entries_at_every_configuration(gpu, heads, d):
    case = cases.config_case(heads, d)
    if (heads, d) == (8, 8):
        assert case.all_dropped().sum() == 82
    check_cabi(case, gpu)


@pytest.mark.parametrize("case", cases.scale_cases(), ids=lambda c: c.name)
def test_cabi_entries_at_every_scale_with_light_and_heavy_dropout(gpu, case):
    assert case.p in (0.1, 0.9)
    if (case.heads, case.width) == (8, 64):
        assert case.all_dropped().any()
    check_cabi(case, gpu)


def plain_cabi(case, gpu):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    q, k, v, g = dev(case.q, gpu), dev(case.k, gpu), dev(case.v, gpu), dev(case.g, gpu)
    colptr, row_t, _ = transposed(case, gpu)
    z, lse = cabi.mha(rowptr, col, q, k, v, case.heads, case.ps)
    dq, D = cabi.mha_bw_rows(rowptr, col, q, k, v, g, z, lse, case.heads, case.ps)
    dk, dv = cabi.mha_bw_cols(colptr, row_t, q, k, v, g, lse, D, case.heads, case.ps)
    return dict(z=z, lse=lse, dq=dq, D=D, dk=dk, dv=dv)


@pytest.mark.parametrize("heads,d", cases.WIDTH_CONFIGS)
def test_threshold_0_and_keep_scale_1_give_the_bits_of_the_entries_without_dropout(gpu, heads, d):
    """Every entry is kept and c = 1: t * 1, z * 1 and a * 1 are exact and the kernels are one template, so all outputs are equal bit
    for bit at the five width instantiations."""
    case = cases.config_case(heads, d)
    got = run_cabi(case, gpu, threshold=0, scale=1.0, seed=case.seed)
    for name, w in plain_cabi(case, gpu).items():
        assert torch.equal(got[name], w), name


@pytest.mark.parametrize("heads,d", ((8, 8), (2, 256)))
def test_one_mask_in_three_kernels(gpu, heads, d):
    """At one seed: z of the forward is the reference's under the mask, D of the rows kernel equals <g, z> of THAT z within bound (the
    rows kernel's t_e and the forward's z agree on the mask), and dk, dv of the columns kernel match."""
    case = cases.config_case(heads, d)
    got = run_cabi(case, gpu)
    held(case, got, ("z", "D", "dq", "dk", "dv"))
    gz = (ref.per_head(case.g.astype(np.float64), heads) * ref.per_head(got["z"].cpu().numpy().astype(np.float64), heads)).sum(2)
    assert np.all(np.abs(got["D"].cpu().numpy() - gz) <= case.bound["D"])
    other = case.with_mask(ref.keep(case.seed + 1, case.nnz, heads, case.p))       # and another seed's reference is far away
    for name in ("z", "dq", "dv"):
        assert ref.worst(got[name].cpu().numpy(), other[name], case.bound[name]) > 10.0, name


def test_one_entry_rows_are_exact(gpu):
    """One-entry rows: a_e = 1 and l = 1 exactly, so a kept (row, head) has z = float32(v_j c) bit for bit and a dropped one 0; lse is
    that of the call without dropout; dv vanishes in a head whose incoming entries are all dropped."""
    case = cases.single_case()
    got = run_cabi(case, gpu)
    H = case.heads
    mask, row = case.ref["q"], case.ref["row"]
    want = np.zeros((case.m, H, case.width // H), np.float32)
    vc = (ref.per_head(case.v, H)[case.col] * np.float32(case.scale)).astype(np.float32)
    want[row] = np.where(mask[:, :, None], vc, np.float32(0.0))
    z = got["z"].cpu().numpy()
    assert np.array_equal(ref.per_head(z, H)[row][~mask], np.zeros_like(vc)[~mask])
    assert np.array_equal(np.abs(z).view(np.uint32), np.abs(want.reshape(case.m, case.width)).view(np.uint32))
    assert np.array_equal(np.signbit(ref.per_head(z, H)[row][mask]), np.signbit(vc[mask]))
    assert torch.equal(got["lse"], plain_cabi(case, gpu)["lse"])
    held(case, got, OUTPUTS)
    dv = ref.per_head(got["dv"].cpu().numpy(), H)
    none_kept = (case.kept_in == 0) & case.has_in[:, None]
    assert none_kept.any() and np.all(dv[none_kept] == 0)
    assert np.all(np.abs(ref.per_head(case.ref["dv"], H))[case.kept_in > 0].max(1) > 0)


def test_duplicates_have_bits_of_their_own(gpu):
    """Two stored entries (i, j) with different keep bits in some head: z_i is the reference's, and far -- beyond eight bounds -- from
    what a mask per (i, j) would give."""
    case = cases.duplicate_case()
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
    """dk and dv under the mask of the CSR positions (through csr2csc) are the reference's; the mask indexed by the transposed position
    is far."""
    case = cases.position_case()
    got = run_cabi(case, gpu)
    held(case, got, ("dk", "dv"))
    wrong = np.empty_like(case.ref["q"])
    wrong[cases.transposed_positions(case.col)] = case.ref["q"]
    assert ref.worst(got["dv"].cpu().numpy(), case.with_mask(wrong)["dv"], case.bound["dv"]) > 8.0


def test_rectangular_graph(gpu):
    """M != N (67 x 233): through the entries and through the plug-in, which give the same bits."""
    case = cases.rect_case()
    got = check_cabi(case, gpu)
    adj = adjacency(case, gpu)
    q, k, v = (dev(a, gpu).requires_grad_(True) for a in (case.q, case.k, case.v))
    z = adj.mha_matmul(q, k, v, case.heads, case.ps, dropout=case.p, seed=case.seed)
    z.backward(dev(case.g, gpu))
    for name, a in (("z", z), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert torch.equal(a.detach(), got[name]), name


def test_k_is_v_receives_both_parts(gpu):
    """One tensor as keys and values: the entries hold the bounds with v = k, and under autograd its gradient is dk + dv."""
    case = cases.shared_case()
    got = check_cabi(case, gpu)
    adj = adjacency(case, gpu)
    q, kv = dev(case.q, gpu).requires_grad_(True), dev(case.k, gpu).requires_grad_(True)
    z = adj.mha_matmul(q, kv, kv, case.heads, dropout=case.p, seed=case.seed)
    z.backward(dev(case.g, gpu))
    assert torch.equal(z.detach(), got["z"]) and torch.equal(q.grad, got["dq"]) and torch.equal(kv.grad, got["dk"] + got["dv"])


@pytest.mark.parametrize("heads,d", cases.FUSED_CONFIGS)
def test_fused_projection_views_go_in_at_their_own_pitch(gpu, heads, d):
    """q, k, v as column views of one [N, 3K] tensor: the entries and the operator read them at a pitch of 3K, give the bits of the packed
    operands, and the fused tensor's gradient holds dq | dk | dv."""
    case = cases.fused_case(heads, d)
    K = case.width
    fused = dev(case.fused, gpu)
    views = (fused[:, :K], fused[:, K:2 * K], fused[:, 2 * K:])
    assert all(t.stride(0) == 3 * K and not t.is_contiguous() for t in views)
    got = run_cabi(case, gpu, operands=views)
    held(case, got, OUTPUTS, " fused")
    packed = run_cabi(case, gpu)
    for name in OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    adj = adjacency(case, gpu)
    leaf = dev(case.fused, gpu).requires_grad_(True)
    z = adj.mha_matmul(leaf[:, :K], leaf[:, K:2 * K], leaf[:, 2 * K:], heads, dropout=case.p, seed=case.seed)
    z.backward(dev(case.g, gpu))
    assert torch.equal(z.detach(), got["z"])
    assert torch.equal(leaf.grad, torch.cat([got["dq"], got["dk"], got["dv"]], dim=1))


@pytest.mark.parametrize("heads,d", ((8, 8), (1, 47), (2, 256)))
def test_operator_and_plugin_under_autograd(gpu, heads, d):
    """torch.ops.isplib.mha_drop_spmm and mha_matmul give the bits of the three entries, inside the bounds; gat_dropout_mask on the
    matrix's device is the mask the kernels used."""
    import isplib_amd
    case = cases.config_case(heads, d)
    want = run_cabi(case, gpu)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    g = dev(case.g, gpu)
    q, k, v = (dev(a, gpu).requires_grad_(True) for a in (case.q, case.k, case.v))
    z = torch.ops.isplib.mha_drop_spmm(rowptr, col, colptr, row_t, csr2csc, q, k, v, heads, case.ps, case.p, case.seed)
    z.backward(g)
    got = dict(z=z, dq=q.grad, dk=k.grad, dv=v.grad)
    held(case, got, tuple(got), " op")
    for name, t in got.items():
        assert torch.equal(t.detach(), want[name]), name
    adj = adjacency(case, gpu)
    q2, k2, v2 = (dev(a, gpu).requires_grad_(True) for a in (case.q, case.k, case.v))
    z2 = isplib_amd.mha_matmul(adj, q2, k2, v2, heads=heads, dropout=case.p, training=True, seed=case.seed)     # scale None: 1 / sqrt(d)
    z2.backward(g)
    for a, b in ((z2, z), (q2.grad, q.grad), (k2.grad, k.grad), (v2.grad, v.grad)):
        assert torch.equal(a.detach(), b.detach())
    mask = isplib_amd.gat_dropout_mask(adj, heads, case.p, case.seed)
    assert mask.device == z.device and np.array_equal(mask.cpu().numpy(), case.ref["q"])


def test_determinism_and_seed_handling(gpu):
    case = cases.config_case(8, 8)
    adj = adjacency(case, gpu)
    q, k, v = dev(case.q, gpu), dev(case.k, gpu), dev(case.v, gpu)
    z1 = adj.mha_matmul(q, k, v, 8, dropout=0.6, seed=11)
    z2 = adj.mha_matmul(q, k, v, 8, dropout=0.6, seed=11)
    z3 = adj.mha_matmul(q, k, v, 8, dropout=0.6, seed=12)
    assert torch.equal(z1, z2) and not torch.equal(z1, z3)
    torch.manual_seed(99)
    a = adj.mha_matmul(q, k, v, 8, dropout=0.6)
    b = adj.mha_matmul(q, k, v, 8, dropout=0.6)
    torch.manual_seed(99)
    c = adj.mha_matmul(q, k, v, 8, dropout=0.6)
    assert torch.equal(a, c) and not torch.equal(a, b)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()


def test_partial_gradients(gpu):
    """Only q asks: the columns kernel does not run -- the backward allocates nothing of k's size beside dq -- and the gradient has the
    bits of the full call; only v, or k and v: the gradients not asked for stay None; every subset gets the full call's bits."""
    case = cases.config_case(8, 64)
    adj = adjacency(case, gpu)
    g = dev(case.g, gpu)

    def run(need):
        ops = {name: dev(a, gpu).requires_grad_(name in need) for name, a in (("q", case.q), ("k", case.k), ("v", case.v))}
        z = adj.mha_matmul(ops["q"], ops["k"], ops["v"], case.heads, dropout=case.p, seed=case.seed)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        z.backward(g)
        torch.cuda.synchronize()
        return z, {name: t.grad for name, t in ops.items()}, torch.cuda.max_memory_allocated() - before

    names = ("q", "k", "v")
    z, full, grew_full = run(names)
    assert all(full[name] is not None for name in names)
    assert grew_full >= (case.m + 2 * case.n) * case.width * 4           # dq, dk and dv
    for need in (("q",), ("v",), ("k", "v"), ("k",), ("q", "v")):
        z1, part, grew = run(need)
        assert torch.equal(z1, z)
        for name in names:
            assert (part[name] is None) if name not in need else torch.equal(part[name], full[name]), (need, name)
        if need == ("q",):
            assert grew < (case.m + case.n) * case.width * 4, (need, grew)   # dq and D: no dk, dv, so no columns kernel


def test_eval_mode_and_zero_dropout_are_the_call_without_the_keywords(gpu):
    case = cases.config_case(8, 8)
    adj = adjacency(case, gpu)
    g = dev(case.g, gpu)

    def run(**kw):
        ops = [dev(a, gpu).requires_grad_(True) for a in (case.q, case.k, case.v)]
        z = adj.mha_matmul(ops[0], ops[1], ops[2], case.heads, case.ps, **kw)
        z.backward(g)
        return [z.detach()] + [t.grad for t in ops]

    plain = run()
    for kw in (dict(dropout=0.6, training=False), dict(dropout=0.6, training=False, seed=3), dict(dropout=0.0), dict(dropout=0, seed=3)):
        for a, b in zip(run(**kw), plain):
            assert torch.equal(a, b), kw
    assert not torch.equal(run(dropout=0.6, seed=3)[0], plain[0])


def test_16_bit_operands_convert_when_the_variable_is_set(gpu, monkeypatch):
    """There is no 16-bit dropout kernel: under ISPLIB_HALF_MHA (any value) bf16 operands go through the fp32 dropout operator on the
    widened operands, and come back rounded once; gradients return in their own dtypes; k is v is preserved."""
    case = cases.config_case(8, 8)
    adj = adjacency(case, gpu)
    g = dev(case.g, gpu)
    qb, kb, vb = (dev(a, gpu).bfloat16() for a in (case.q, case.k, case.v))
    monkeypatch.delenv("ISPLIB_HALF_MHA", raising=False)
    with pytest.raises(TypeError, match="float32"):
        adj.mha_matmul(qb, kb, vb, 8, dropout=0.6, seed=5)
    q32, k32, v32 = (t.float().requires_grad_(True) for t in (qb, kb, vb))
    z32 = adj.mha_matmul(q32, k32, v32, 8, dropout=0.6, seed=5)
    z32.backward(g.bfloat16().float())
    for value in ("native", "convert", "anything"):
        monkeypatch.setenv("ISPLIB_HALF_MHA", value)
        q16, k16, v16 = (t.clone().requires_grad_(True) for t in (qb, kb, vb))
        z16 = adj.mha_matmul(q16, k16, v16, 8, dropout=0.6, seed=5)
        assert z16.dtype == torch.bfloat16 and torch.equal(z16.detach(), z32.detach().bfloat16()), value
        z16.backward(g.bfloat16())
        for a, b in ((q16, q32), (k16, k32), (v16, v32)):
            assert a.grad.dtype == torch.bfloat16 and torch.equal(a.grad, b.grad.bfloat16()), value
    # k is v: one widened tensor on the fp32 side, one gradient with both parts
    s32 = kb.float().requires_grad_(True)
    qs = qb.float()
    zs = adj.mha_matmul(qs, s32, s32, 8, dropout=0.6, seed=5)
    zs.backward(g.bfloat16().float())
    s16 = kb.clone().requires_grad_(True)
    zh = adj.mha_matmul(qb, s16, s16, 8, dropout=0.6, seed=5)
    zh.backward(g.bfloat16())
    assert torch.equal(zh.detach(), zs.detach().bfloat16()) and torch.equal(s16.grad, s32.grad.bfloat16())


def test_error_paths_raise_before_a_launch(gpu):
    from isplib_amd import cabi
    case = cases.config_case(2, 4)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    q, k, v, g = (dev(a, gpu) for a in (case.q, case.k, case.v, case.g))
    m, n, K, nnz = case.m, case.n, case.width, case.nnz
    z, lse = poisoned(gpu, m, K), poisoned(gpu, m, 2)
    for bad in (dict(threshold=-1), dict(threshold=2 ** 32), dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan")),
                dict(seed=-1), dict(seed=2 ** 63)):
        kw = dict(threshold=5, scale=2.5, seed=1)
        kw.update(bad)
        with pytest.raises(ValueError, match="`threshold`|`keep_scale`|`seed`"):
            cabi.mha_drop(rowptr, col, q, k, v, kw["threshold"], kw["scale"], kw["seed"], 2, out=(z, lse))
    with pytest.raises(ValueError, match="`csr2csc` must be a 1-D tensor"):
        cabi.mha_drop_bw_cols(colptr, row_t, csr2csc[:-1], q, k, v, g, lse, lse, 5, 2.5, 1, 2)
    with pytest.raises(TypeError, match="`csr2csc` must be int64"):
        cabi.mha_drop_bw_cols(colptr, row_t, csr2csc.int(), q, k, v, g, lse, lse, 5, 2.5, 1, 2)
    L = cabi.lib()
    rp, cp = rowptr.data_ptr(), colptr.data_ptr()
    fw = lambda c, heads=2, nz=nnz, seed=1, ps=0.5: (m, n, K, nz, col.data_ptr(), rp, rp + 8, heads, ps, q.data_ptr(), K, k.data_ptr(), K,  # noqa: E731
                                                     v.data_ptr(), K, z.data_ptr(), K, lse.data_ptr(), None, 5, c, seed)
    assert L.isplib_qkv_drop_csr_hip(*fw(0.0)) == cabi.FAIL and "keep_scale" in cabi.last_error()
    assert L.isplib_qkv_drop_csr_hip(*fw(float("nan"))) == cabi.FAIL
    assert L.isplib_qkv_drop_csr_hip(*fw(float("inf"))) == cabi.FAIL
    assert L.isplib_qkv_drop_csr_hip(*fw(2.5, nz=2 ** 31)) == cabi.FAIL and "2^31" in cabi.last_error()
    assert L.isplib_qkv_drop_csr_hip(*fw(2.5, seed=2 ** 63)) == cabi.FAIL and "2^63" in cabi.last_error()
    assert L.isplib_qkv_drop_csr_hip(*fw(2.5, ps=float("nan"))) == cabi.FAIL and "scale" in cabi.last_error()
    assert L.isplib_qkv_drop_csr_hip(*fw(2.5, heads=0)) == cabi.NO_OPT_IMPL and "isplib_mha_serves" in cabi.last_error()
    dq, D, dk, dv = poisoned(gpu, m, K), poisoned(gpu, m, 2), poisoned(gpu, n, K), poisoned(gpu, n, K)
    rows = lambda c, nz=nnz, seed=1: (m, n, K, nz, col.data_ptr(), rp, rp + 8, 2, 0.5, q.data_ptr(), K, k.data_ptr(), K, v.data_ptr(), K,  # noqa: E731
                                      g.data_ptr(), K, g.data_ptr(), K, g.data_ptr(), dq.data_ptr(), K, D.data_ptr(), None, 5, c, seed)
    assert L.isplib_qkv_drop_bw_rows_hip(*rows(-1.0)) == cabi.FAIL and "keep_scale" in cabi.last_error()
    assert L.isplib_qkv_drop_bw_rows_hip(*rows(2.5, 2 ** 31)) == cabi.FAIL
    assert L.isplib_qkv_drop_bw_rows_hip(*rows(2.5, seed=2 ** 63)) == cabi.FAIL
    cols = lambda perm, c=2.5, nz=nnz, seed=1: (m, n, K, nz, row_t.data_ptr(), cp, cp + 8, perm, 2, 0.5, q.data_ptr(), K, g.data_ptr(), K,  # noqa: E731
                                                g.data_ptr(), g.data_ptr(), k.data_ptr(), K, v.data_ptr(), K, dk.data_ptr(), K,
                                                dv.data_ptr(), K, None, 5, c, seed)
    assert L.isplib_qkv_drop_bw_cols_hip(*cols(None)) == cabi.FAIL and "csr2csc" in cabi.last_error()
    assert L.isplib_qkv_drop_bw_cols_hip(*cols(csr2csc.data_ptr(), 0.0)) == cabi.FAIL
    assert L.isplib_qkv_drop_bw_cols_hip(*cols(csr2csc.data_ptr(), 2.5, 2 ** 31)) == cabi.FAIL
    assert L.isplib_qkv_drop_bw_cols_hip(*cols(csr2csc.data_ptr(), 2.5, seed=2 ** 63)) == cabi.FAIL
    torch.cuda.synchronize()
    for t in (z, lse, dq, D, dk, dv):
        assert torch.isnan(t).all()
    with pytest.raises(RuntimeError, match="`p` must lie in"):
        torch.ops.isplib.mha_drop_spmm(rowptr, col, colptr, row_t, csr2csc, q, k, v, 2, 0.5, 1.0, 1)
    with pytest.raises(RuntimeError, match="`p` must lie in"):
        torch.ops.isplib.mha_drop_spmm(rowptr, col, colptr, row_t, csr2csc, q, k, v, 2, 0.5, 0.0, 1)
    with pytest.raises(RuntimeError, match="`seed` must be"):
        torch.ops.isplib.mha_drop_spmm(rowptr, col, colptr, row_t, csr2csc, q, k, v, 2, 0.5, 0.5, -1)
    with pytest.raises(RuntimeError, match="csr2csc"):
        torch.ops.isplib.mha_drop_spmm(rowptr, col, colptr, row_t, csr2csc[:-1], q, k, v, 2, 0.5, 0.5, 1)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="`dropout` must lie in"):
            adjacency(case, gpu).mha_matmul(q, k, v, 2, dropout=bad)
