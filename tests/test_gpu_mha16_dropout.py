"""The 16-bit multi-head attention operator (q, k, v) with attention dropout on the GPU (isplib_amd/csrc/mha16.hip, DROP kernels): the
three C entries (isplib_qkv_half_drop_*_hip) on NaN-filled outputs, torch.ops.isplib.mha_drop_spmm16 with its autograd backward, and
the plug-in's opt-in route (ISPLIB_HALF_MHA with ISPLIB_HALF_MHA_DROP), each held to the per-element bounds of
tests/mha16_dropout_ref.py against the fp64 reference on the widened operands (inputs, references and bounds:
tests/mha16_dropout_cases.py, computed once per case).  The largest error / bound per output is printed before every assertion;
DESIGN.md 4.6o records the largest.
"""
import numpy as np
import pytest
import torch

from tests import half_ref
from tests import mha16_dropout_cases as cases
from tests import mha_dropout_ref as ref
from tests import rect_cases
from tests.gat_ref import per_head
from tests.test_gpu_mha16 import dev, dev_graph

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
OP_OUTPUTS = ("z", "dq", "dk", "dv")

_transposed = {}


def transposed(case, gpu):
    """colptr / row_t / csr2csc as SparseStorage caches them (the library's own csr2csc), once per graph."""
    import isplib_amd
    key = (case.rowptr.tobytes(), case.col.tobytes(), case.n)
    if key not in _transposed:
        rowptr, col = dev_graph(case, gpu)
        st = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n)).storage
        _transposed[key] = (st.colptr(), st.row_t(), st.csr2csc())
    return _transposed[key]


def held(case, got, names=cases.OUTPUTS, what="mha16 dropout"):
    frac = cases.fractions(case, got, names)
    print(f"{what} error/bound {case.name}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def nan_outputs(case, gpu):
    """NaN-filled outputs: an element the kernels do not write stays NaN and misses every bound."""
    wide = lambda rows: torch.full((rows, case.width), float("nan"), device=gpu, dtype=case.dtype)      # noqa: E731
    table = lambda: torch.full((case.m, case.heads), float("nan"), device=gpu)                          # noqa: E731
    return dict(z=wide(case.m), lse=table(), dq=wide(case.m), D=table(), dk=wide(case.n), dv=wide(case.n))


def run_cabi(case, gpu, q=None, k=None, v=None, threshold=None, keep_scale=None, seed=None, positions=None):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    q = dev(case.q16, gpu) if q is None else q
    k = dev(case.k16, gpu) if k is None else k
    v = (k if case.shared else dev(case.v16, gpu)) if v is None else v
    g = dev(case.g16, gpu)
    drop = (case.threshold if threshold is None else threshold, case.scale if keep_scale is None else keep_scale,
            case.seed if seed is None else seed)
    o = nan_outputs(case, gpu)
    cabi.mha16_drop_forward(rowptr, col, q, k, v, *drop, case.heads, case.ps, out=(o["z"], o["lse"]))
    cabi.mha16_drop_backward_rows(rowptr, col, q, k, v, g, o["lse"], *drop, case.heads, case.ps, out=(o["dq"], o["D"]))
    cabi.mha16_drop_backward_cols(colptr, row_t, csr2csc if positions is None else positions, q, k, v, g, o["lse"], o["D"], *drop,
                                  case.heads, case.ps, out=(o["dk"], o["dv"]))
    return o


def run_plain(case, gpu):
    """The entries without dropout (isplib_qkv16_*_hip) on the same operands."""
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, _ = transposed(case, gpu)
    q, k, g = dev(case.q16, gpu), dev(case.k16, gpu), dev(case.g16, gpu)
    v = k if case.shared else dev(case.v16, gpu)
    z, lse = cabi.mha16_forward(rowptr, col, q, k, v, case.heads, case.ps)
    dq, D = cabi.mha16_backward_rows(rowptr, col, q, k, v, g, lse, case.heads, case.ps)
    dk, dv = cabi.mha16_backward_cols(colptr, row_t, q, k, v, g, lse, D, case.heads, case.ps)
    return dict(z=z, lse=lse, dq=dq, D=D, dk=dk, dv=dv)


def run_op(case, gpu, need=(True, True, True), ops=None):
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    q, k, v = ops if ops is not None else (dev(t, gpu).requires_grad_(n) for t, n in zip((case.q16, case.k16, case.v16), need))
    z = torch.ops.isplib.mha_drop_spmm16(rowptr, col, colptr, row_t, csr2csc, q, k, v, case.heads, case.ps, case.p, case.seed)
    if any(need):
        z.backward(dev(case.g16, gpu))
    return z.detach(), q, k, v


def check_case(case, gpu):
    """The three C entries on NaN-filled outputs, every element (cases.fractions also holds the empty rows and the unreferenced
    columns to exact zeros and -inf); then the operator's forward and gradients have the entries' bits."""
    got = run_cabi(case, gpu)
    held(case, got)
    z, q, k, v = run_op(case, gpu)
    assert z.dtype == q.grad.dtype == k.grad.dtype == v.grad.dtype == case.dtype
    for name, t in (("z", z), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert torch.equal(t, got[name]), name
    return got


@pytest.mark.parametrize("spec", cases.config_specs(), ids=cases.case_id)
def test_every_configuration(gpu, spec):
    check_case(cases.config_case(*spec), gpu)


@pytest.mark.parametrize("spec", cases.p_specs(), ids=lambda s: f"h{s[0]}d{s[1]}-p{s[2]}")
def test_every_p(gpu, spec):
    """p = 0.1, 0.6, 0.9 per head form; a live (row, head) with every entry dropped has z = 0 exactly and a finite lse."""
    h, d, p = spec
    case = cases.config_case(h, d, BF, "g1", p)
    got = check_case(case, gpu)
    gone = case.all_dropped()
    if (h, d) == (8, 8):
        assert gone.any()
    assert np.all(per_head(cases.as_array(got["z"]), h)[gone] == 0) and np.all(np.isfinite(cases.as_array(got["lse"])[gone]))


@pytest.mark.parametrize("dtype", (BF, FP), ids=("bf16", "fp16"))
def test_scores_spread_beyond_150(gpu, dtype):
    case = cases.large_case(dtype)
    got = check_case(case, gpu)
    for name in cases.OUTPUTS:
        v = cases.as_array(got[name])
        assert np.all(np.isfinite(v[case.live] if name == "lse" else v)), name


@pytest.mark.parametrize("spec", ((8, 8, BF), (1, 46, BF), (3, 128, BF), (8, 16, FP)), ids=lambda s: f"h{s[0]}d{s[1]}")
def test_every_bit_kept_and_scale_one_is_the_call_without_dropout(gpu, spec):
    """threshold = 0, keep_scale = 1: the bits of isplib_qkv16_*_hip for all six outputs."""
    case = cases.config_case(*spec)
    got, want = run_cabi(case, gpu, threshold=0, keep_scale=1.0), run_plain(case, gpu)
    for name in cases.OUTPUTS:
        assert torch.equal(got[name], want[name]), name


def test_launches_repeat_and_the_seed_matters(gpu):
    case = cases.config_case(8, 8)
    a, b = run_cabi(case, gpu), run_cabi(case, gpu)
    for name in cases.OUTPUTS:
        assert torch.equal(a[name], b[name]), name
    other = run_cabi(case, gpu, seed=case.seed + 1)
    assert not torch.equal(other["z"], a["z"]) and torch.equal(other["lse"], a["lse"])        # lse does not see the mask


@pytest.mark.parametrize("dtype", (BF, FP), ids=("bf16", "fp16"))
def test_single_entry_rows_are_exact_and_the_zero_pattern_is_the_mask(gpu, dtype):
    """a_e = 1: a kept (row, head) is round16(float32(v_j c)), a dropped one 0, exactly; the zero pattern of z is
    isplib_amd.gat_dropout_mask's and that of the fp32 dropout operator under the same seed."""
    import isplib_amd
    case = cases.single_case(dtype)
    got = check_case(case, gpu)
    row, H = case.ref["row"], case.heads
    want = np.zeros((case.m, H, case.d), np.float32)
    want[row] = np.where(case.ref["q"][:, :, None], (per_head(case.v, H)[case.col] * np.float32(case.scale)).astype(np.float32), np.float32(0))
    want16 = half_ref.round16(want.reshape(case.m, case.width), dtype)
    assert np.array_equal(half_ref.bits(got["z"]), half_ref.bits(want16))
    mask = isplib_amd.gat_dropout_mask(case.nnz, H, case.p, case.seed).numpy()
    assert np.array_equal(mask, case.ref["q"])
    kept = np.zeros((case.m, H), bool)
    kept[row] = mask
    nonzero_v = np.zeros((case.m, H), bool)
    nonzero_v[row] = (per_head(case.v, H)[case.col] != 0).all(2)
    z3 = per_head(cases.as_array(got["z"]), H)
    assert nonzero_v[row].all()                                          # so a zero of z is a dropped entry, not a zero of v
    assert np.array_equal((z3 != 0).all(2), kept) and np.array_equal((z3 == 0).all(2), ~kept)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    z32 = adj.mha_matmul(dev(case.q, gpu), dev(case.k, gpu), dev(case.v, gpu), H, case.ps, case.p, True, case.seed)
    assert np.array_equal((per_head(z32.cpu().numpy(), H) != 0).all(2), kept)
    # a column that lost every incoming entry in a head has dv = 0 there
    dv3 = per_head(cases.as_array(got["dv"]), H)
    lost = case.has_in[:, None] & (case.kept_in == 0)
    assert lost.any() and np.all(dv3[lost] == 0)


def test_duplicates_have_their_own_bits(gpu):
    case = cases.duplicate_case()
    got = check_case(case, gpu)
    keyed = case.with_mask(cases.pair_mask(case))                        # what a mask keyed by (i, j) would give: far outside the bound
    assert ref.worst(cases.as_array(got["z"]), keyed["z"], case.bound["z"]) > 10.0


def test_the_columns_kernel_hashes_the_csr_position(gpu):
    case = cases.position_case()
    got = check_case(case, gpu)
    assert ref.worst(cases.as_array(got["dv"]), case.wrong["dv"], case.bound["dv"]) > 10.0
    # and it is csr2csc it reads: handed the identity, it computes the transposed-position mask's dv
    wrong = run_cabi(case, gpu, positions=torch.arange(case.nnz, device=gpu))
    frac = ref.worst(cases.as_array(wrong["dv"]), case.wrong["dv"], case.bound_of(case.wrong, ref.bounds(
        case.rowptr, case.col, case.q, case.k, case.v, case.heads, case.ps, case.wrong, case.g))["dv"])
    print(f"mha16 dropout error/bound {case.name} under the transposed-position mask: dv={frac:.4f}")
    assert frac <= 1.0


@pytest.mark.parametrize("shape", tuple(rect_cases.SHAPES))
@pytest.mark.parametrize("heads,d", cases.RECT_CONFIGS)
def test_rectangular_shapes(gpu, shape, heads, d):
    check_case(cases.rect_case(shape, heads, d), gpu)


def test_one_tensor_as_key_and_value(gpu):
    """k is v: through the entries dk and dv apart, each to its own bound; through the operator the one tensor's gradient is dk + dv,
    each rounded once and added in the operands' dtype."""
    case = cases.shared_case()
    got = check_case(case, gpu)
    q, k = dev(case.q16, gpu).requires_grad_(True), dev(case.k16, gpu).requires_grad_(True)
    z, _, _, _ = run_op(case, gpu, ops=(q, k, k))
    assert torch.equal(z, got["z"]) and torch.equal(q.grad, got["dq"]) and torch.equal(k.grad, got["dk"] + got["dv"])


@pytest.mark.parametrize("heads,d", cases.FUSED_CONFIGS)
def test_views_of_one_fused_projection(gpu, heads, d):
    """q, k, v as the column blocks of one 16-bit [N, 3 K] tensor go in at their own pitch and give the bits of contiguous copies."""
    case = cases.fused_case(heads, d)
    kk = case.width
    packed = run_cabi(case, gpu)
    held(case, packed)
    fused = dev(case.fused, gpu)
    views = [fused[:, i * kk:(i + 1) * kk] for i in range(3)]
    assert all(not t.is_contiguous() and t.stride(0) == 3 * kk for t in views)
    got = run_cabi(case, gpu, q=views[0], k=views[1], v=views[2])
    for name in cases.OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    leaf = fused.clone().requires_grad_(True)
    z, _, _, _ = run_op(case, gpu, ops=(leaf[:, :kk], leaf[:, kk:2 * kk], leaf[:, 2 * kk:]))
    assert torch.equal(z, packed["z"])
    assert torch.equal(leaf.grad, torch.cat([packed["dq"], packed["dk"], packed["dv"]], 1))


def test_gradient_flags(gpu):
    """With only q requiring a gradient, k.grad and v.grad stay None (the columns kernel does not run); the others keep their bits."""
    case = cases.config_case(8, 8)
    z, q, k, v = run_op(case, gpu)
    z1, q1, k1, v1 = run_op(case, gpu, need=(True, False, False))
    assert k1.grad is None and v1.grad is None and torch.equal(q1.grad, q.grad) and torch.equal(z1, z)
    _, q2, k2, v2 = run_op(case, gpu, need=(False, True, True))
    assert q2.grad is None and torch.equal(k2.grad, k.grad) and torch.equal(v2.grad, v.grad)
    z3, q3, k3, v3 = run_op(case, gpu, need=(False, False, False))
    assert q3.grad is None and k3.grad is None and v3.grad is None and torch.equal(z3, z) and not z3.requires_grad


def test_the_operator_refuses_before_a_launch(gpu):
    case = cases.config_case(8, 8)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t, csr2csc = transposed(case, gpu)
    q, k, v = (dev(t, gpu) for t in (case.q16, case.k16, case.v16))
    op = torch.ops.isplib.mha_drop_spmm16
    for p in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(RuntimeError, match="must lie in"):
            op(rowptr, col, colptr, row_t, csr2csc, q, k, v, 8, 0.25, p, 1)
    with pytest.raises(RuntimeError, match="non-negative"):
        op(rowptr, col, colptr, row_t, csr2csc, q, k, v, 8, 0.25, 0.5, -1)
    with pytest.raises(RuntimeError, match="mha_drop_spmm16"):
        op(rowptr, col, colptr, row_t, csr2csc, q.float(), k, v, 8, 0.25, 0.5, 1)
    with pytest.raises(RuntimeError, match="mha_drop_spmm16"):
        op(rowptr, col, colptr, row_t, csr2csc[:-1], q, k, v, 8, 0.25, 0.5, 1)
    with pytest.raises(RuntimeError, match="mha_drop_spmm16"):
        op(rowptr, col, colptr, row_t, csr2csc, q, k, v, 16, 0.25, 0.5, 1)           # d = 4: outside the 16-bit domain


@pytest.mark.parametrize("dtype", (BF, FP), ids=("bf16", "fp16"))
def test_plugin_routes(gpu, dtype, monkeypatch):
    """Both variables native -> the operator's bits; ISPLIB_HALF_MHA_DROP unset or convert -> the conversion route's bits; so with
    ISPLIB_HALF=convert; odd K and (heads, d) = (2, 4) convert and nothing raises; training=False -> mha_spmm16's bits; auto follows
    the measured rule, whatever it says."""
    import isplib_amd
    from isplib_amd import cabi
    case = cases.config_case(8, 8, dtype)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    g = dev(case.g16, gpu)

    def leaves(k=None):
        ops = [dev(t, gpu) for t in (case.q16, case.k16, case.v16)]
        if k is not None:
            ops = [t[:, :k].contiguous() for t in ops]
        return [t.requires_grad_(True) for t in ops]

    def by_hand(q, k, v, gg, heads):
        z = isplib_amd.mha_matmul(adj, q.float(), k.float(), v.float(), heads, None, case.p, True, case.seed).to(dtype)
        z.backward(gg)
        return z.detach(), q.grad, k.grad, v.grad

    def through(q, k, v, gg, heads, training=True):
        z = adj.mha_matmul(q, k, v, heads, None, case.p, training, case.seed)
        z.backward(gg)
        assert z.dtype == q.grad.dtype == k.grad.dtype == v.grad.dtype == dtype
        return z.detach(), q.grad, k.grad, v.grad

    def same(a, b):
        return all(torch.equal(u, v) for u, v in zip(a, b))

    for name in ("ISPLIB_HALF", "ISPLIB_HALF_MHA", "ISPLIB_HALF_MHA_DROP"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("ISPLIB_HALF_MHA_DROP", "native")
    with pytest.raises(TypeError, match="float32"):                      # ISPLIB_HALF_MHA unset: the TypeError it always raised
        adj.mha_matmul(*[t.detach() for t in leaves()], 8, None, case.p, True, case.seed)
    monkeypatch.delenv("ISPLIB_HALF_MHA_DROP")
    want = by_hand(*leaves(), g, 8)
    abi = run_cabi(case, gpu)
    native = tuple(abi[n] for n in OP_OUTPUTS)
    assert not same(native, want)

    monkeypatch.setenv("ISPLIB_HALF_MHA", "native")
    assert same(through(*leaves(), g, 8), want)                          # ISPLIB_HALF_MHA_DROP unset: convert
    monkeypatch.setenv("ISPLIB_HALF_MHA_DROP", "convert")
    assert same(through(*leaves(), g, 8), want)
    monkeypatch.setenv("ISPLIB_HALF_MHA_DROP", "native")
    got = through(*leaves(), g, 8)
    assert same(got, native)
    held(case, dict(zip(OP_OUTPUTS, got)), OP_OUTPUTS, "mha_matmul native dropout")
    # outside the 16-bit domain: the conversion route's bits, nothing raised
    for k, heads in ((29, 1), (8, 2)):
        gg = g[:, :k].contiguous()
        assert same(through(*leaves(k), gg, heads), by_hand(*leaves(k), gg, heads)), (k, heads)
    # training=False does not reach any of this: mha_spmm16's bits
    plain = run_plain(case, gpu)
    assert same(through(*leaves(), g, 8, training=False), tuple(plain[n] for n in OP_OUTPUTS))
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert same(through(*leaves(), g, 8), want)
    monkeypatch.delenv("ISPLIB_HALF")
    monkeypatch.setenv("ISPLIB_HALF_MHA", "convert")
    assert same(through(*leaves(), g, 8), want)
    monkeypatch.setenv("ISPLIB_HALF_MHA", "auto")
    assert same(through(*leaves(), g, 8), native)                        # mha16_native_pays: both classes pay
    monkeypatch.setenv("ISPLIB_HALF_MHA_DROP", "auto")
    assert same(through(*leaves(), g, 8), native if cabi.mha16_drop_native_pays(case.n, case.width) else want)
    for pays in (True, False):
        with monkeypatch.context() as mp:
            mp.setattr(cabi, "mha16_drop_native_pays", lambda rows, ld, pays=pays: pays)
            assert same(through(*leaves(), g, 8), native if pays else want)
