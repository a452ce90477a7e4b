"""The 16-bit multi-head attention operator (q, k, v) on the GPU (isplib_amd/csrc/mha16.hip): the C ABI wrappers,
torch.ops.isplib.mha_spmm16 with its autograd backward, and the plug-in's opt-in route (ISPLIB_HALF_MHA), each held to the per-element
bounds of tests/mha16_ref.py against the fp64 reference on the widened operands (inputs, references and bounds: tests/mha16_cases.py,
computed once per case).  The largest error / bound seen per output is printed before every assertion; DESIGN.md 4.6l records it.
"""
import numpy as np
import pytest
import torch

from tests import half_ref
from tests import mha16_cases as c16
from tests import mha_ref as ref
from tests import rect_cases
from tests.gat_ref import per_head

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
OP_OUTPUTS = ("z", "dq", "dk", "dv")


def dev(a, gpu):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).to(gpu)


def dev_graph(case, gpu):
    return dev(case.rowptr, gpu), dev(case.col, gpu)


_transposed = {}


def transposed(case, gpu):
    """colptr / row_t as SparseStorage caches them (the library's own csr2csc), once per graph."""
    import isplib_amd
    key = (case.rowptr.tobytes(), case.col.tobytes(), case.n)
    if key not in _transposed:
        rowptr, col = dev_graph(case, gpu)
        st = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n)).storage
        _transposed[key] = (st.colptr(), st.row_t())
    return _transposed[key]


def held(case, got, names=c16.OUTPUTS, what="mha16"):
    frac = c16.fractions(case, got, names)
    print(f"{what} error/bound {case.name}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def run_cabi(case, gpu, q=None, k=None, v=None, g=None):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    q = dev(case.q16, gpu) if q is None else q
    k = dev(case.k16, gpu) if k is None else k
    v = (k if case.shared else dev(case.v16, gpu)) if v is None else v
    g = dev(case.g16, gpu) if g is None else g
    z, lse = cabi.mha16_forward(rowptr, col, q, k, v, case.heads, case.p)
    dq, D = cabi.mha16_backward_rows(rowptr, col, q, k, v, g, lse, case.heads, case.p)
    dk, dv = cabi.mha16_backward_cols(colptr, row_t, q, k, v, g, lse, D, case.heads, case.p)
    return dict(z=z, lse=lse, dq=dq, D=D, dk=dk, dv=dv)


def run_op(case, gpu, need=(True, True, True)):
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    q, k, v = (dev(t, gpu).requires_grad_(n) for t, n in zip((case.q16, case.k16, case.v16), need))
    z = torch.ops.isplib.mha_spmm16(rowptr, col, colptr, row_t, q, k, v, case.heads, case.p)
    if any(need):
        z.backward(dev(case.g16, gpu))
    return z.detach(), q, k, v


def check_case(case, gpu):
    """Both surfaces on one case: every output of the wrappers, elementwise (c16.fractions also holds the empty rows and the
    unreferenced columns to exact zeros and -inf); then the operator's autograd gives the wrappers' bits."""
    got = run_cabi(case, gpu)
    assert got["z"].dtype == got["dq"].dtype == got["dk"].dtype == got["dv"].dtype == case.dtype
    assert got["lse"].dtype == got["D"].dtype == torch.float32
    held(case, got)
    z, q, k, v = run_op(case, gpu)
    assert z.dtype == q.grad.dtype == k.grad.dtype == v.grad.dtype == case.dtype
    for name, t in (("z", z), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert torch.equal(t, got[name]), name
    return got


@pytest.mark.parametrize("spec", c16.config_cases(), ids=c16.case_id)
def test_every_configuration(gpu, spec):
    """First, last and a ragged width of every LPR, heads of one lane up to half a slot, head counts that are no power of two; bf16
    everywhere, fp16 once per LPR; (8, 8) and (1, 34) also on the graph whose row lengths sit at the edges of G and of a step."""
    check_case(c16.config_case(spec[0], spec[1], spec[2], graph=spec[3]), gpu)


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
def test_scores_spread_beyond_150(gpu, dtype):
    case = c16.large_case(dtype)
    got = check_case(case, gpu)
    for name in c16.OUTPUTS:
        v = c16.as_array(got[name])
        assert np.all(np.isfinite(v[case.live] if name == "lse" else v)), name


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
def test_one_entry_rows_return_v_bit_for_bit(gpu, dtype):
    """z equals v_j's 16 bits whatever the score; an empty row writes 0, -inf and 0."""
    case = c16.single_case(dtype)
    got = check_case(case, gpu)
    live = case.live
    want = torch.zeros_like(case.q16)
    want[torch.from_numpy(live)] = case.v16[torch.from_numpy(case.col)]
    assert np.array_equal(half_ref.bits(got["z"]), half_ref.bits(want))
    lse = got["lse"].cpu().numpy()
    assert (~live).any() and np.all(np.isneginf(lse[~live])) and np.all(np.isfinite(lse[live]))
    assert not got["z"].cpu()[~live].any() and not got["dq"].cpu()[~live].any() and not got["D"].cpu()[~live].any()


def test_one_tensor_as_key_and_value(gpu):
    """k is v through the wrappers (the same device tensor behind both arguments): dk and dv apart, each held to its own bound."""
    check_case(c16.shared_case(8, 8), gpu)


def test_zero_q(gpu):
    """q = 0: every score is 0, the weights are 1 / deg, lse = log deg."""
    check_case(c16.zero_q_case(8, 8), gpu)


@pytest.mark.parametrize("shape", tuple(rect_cases.SHAPES))
@pytest.mark.parametrize("heads,d", c16.RECT_CONFIGS)
def test_rectangular_shapes(gpu, shape, heads, d):
    """233 x 67 and 67 x 233: q and g have M rows, k and v have N; the columns kernel gathers from the M-row tables."""
    case = c16.rect_case(shape, heads, d)
    assert (case.m, case.n) == rect_cases.SHAPES[shape]
    check_case(case, gpu)


@pytest.mark.parametrize("heads,d,dtype", ((1, 10, BF), (5, 8, BF), (1, 510, FP), (8, 64, BF)))
def test_outputs_are_write_only_and_launches_repeat(gpu, heads, d, dtype):
    """NaN-filled, pitched (ld = K + 6), over-allocated outputs, launched twice: every element of every row is written, nothing
    between the rows or past the end, equal bits."""
    from isplib_amd import cabi
    case = c16.config_case(heads, d, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    q, k, v, g = dev(case.q16, gpu), dev(case.k16, gpu), dev(case.v16, gpu), dev(case.g16, gpu)
    m, n, kk, H, p, pad, ld = case.m, case.n, case.width, heads, case.p, 64, case.width + 6

    def wide(rows):
        buf = torch.full((rows * ld + pad,), float("nan"), device=gpu, dtype=dtype)
        return buf, buf[:rows * ld].view(rows, ld)[:, :kk]

    def table(rows, cols):
        buf = torch.full((rows * cols + pad,), float("nan"), device=gpu)
        return buf, buf[:rows * cols].view(rows, cols)

    runs = []
    for _ in range(2):
        b = dict(z=wide(m), lse=table(m, H), dq=wide(m), D=table(m, H), dk=wide(n), dv=wide(n))
        cabi.mha16_forward(rowptr, col, q, k, v, H, p, out=(b["z"][1], b["lse"][1]), check=False)
        cabi.mha16_backward_rows(rowptr, col, q, k, v, g, b["lse"][1], H, p, out=(b["dq"][1], b["D"][1]), check=False)
        cabi.mha16_backward_cols(colptr, row_t, q, k, v, g, b["lse"][1], b["D"][1], H, p, out=(b["dk"][1], b["dv"][1]), check=False)
        for name, (buf, view) in b.items():
            assert not torch.isnan(view).any(), name
            if name in c16.OUT16:
                rest = buf[:view.size(0) * ld].view(view.size(0), ld)[:, kk:]
                assert torch.isnan(rest).all() and torch.isnan(buf[view.size(0) * ld:]).all(), name
            else:
                assert torch.isnan(buf[view.numel():]).all(), name
        runs.append({name: view.clone() for name, (_, view) in b.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    held(case, runs[0])


@pytest.mark.parametrize("heads,d", c16.FUSED_CONFIGS)
def test_views_of_one_fused_projection(gpu, heads, d):
    """q, k, v as the three column blocks of one 16-bit [N, 3 K] tensor go in without a copy and give the bits of contiguous copies,
    through the wrappers and the operator; the fused tensor's gradient is the concatenation of the three."""
    case = c16.config_case(heads, d)
    kk = case.width
    packed = run_cabi(case, gpu)
    fused = torch.cat([dev(case.q16, gpu), dev(case.k16, gpu), dev(case.v16, gpu)], 1)
    views = [fused[:, i * kk:(i + 1) * kk] for i in range(3)]
    assert all(not t.is_contiguous() and t.stride(0) == 3 * kk for t in views)
    got = run_cabi(case, gpu, q=views[0], k=views[1], v=views[2])
    for name in c16.OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    leaf = fused.clone().requires_grad_(True)
    z = torch.ops.isplib.mha_spmm16(rowptr, col, colptr, row_t, leaf[:, :kk], leaf[:, kk:2 * kk], leaf[:, 2 * kk:], heads, case.p)
    z.backward(dev(case.g16, gpu))
    assert torch.equal(z.detach(), packed["z"])
    assert torch.equal(leaf.grad, torch.cat([packed["dq"], packed["dk"], packed["dv"]], 1))


@pytest.mark.parametrize("heads,d", ((8, 8), (2, 256), (1, 46)))
def test_a_nan_poisons_exactly_what_reads_it(gpu, heads, d):
    """Forward only: key[j, c] = NaN makes the head of c NaN in z and lse of the rows referencing j; v[j, c] = NaN makes column c of
    z NaN in those rows; nothing else moves out of its bound."""
    from isplib_amd import cabi
    case = c16.config_case(heads, d)
    j = int(case.col[case.rowptr[2]])                     # a column some rows reference
    hit = np.zeros(case.m, bool)
    hit[case.ref["row"][case.col == j]] = True
    assert hit.any() and (~hit & case.live).any()
    h = heads - 1
    c = h * d + d // 2
    rowptr, col = dev_graph(case, gpu)
    want, bound = case.ref["z"], case.bound["z"]
    # a NaN in the key
    k = case.k16.clone()
    k[j, c] = float("nan")
    z, lse = cabi.mha16_forward(rowptr, col, dev(case.q16, gpu), dev(k, gpu), dev(case.v16, gpu), heads, case.p)
    z3, lse = per_head(c16.as_array(z), heads), c16.as_array(lse)
    assert np.all(np.isnan(z3[hit, h])) and np.all(np.isnan(lse[hit, h]))
    clean = np.ones((case.m, heads), bool)
    clean[hit, h] = False
    frac = ref.worst(z3[clean], per_head(want, heads)[clean], per_head(bound, heads)[clean])
    print(f"mha16 error/bound nan in key, everything else h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    ok = clean & case.live[:, None]
    assert ref.worst(lse[ok], case.ref["lse"][ok], case.bound["lse"][ok]) <= 1.0
    # a NaN in the value
    v = case.v16.clone()
    v[j, c] = float("nan")
    z, lse = cabi.mha16_forward(rowptr, col, dev(case.q16, gpu), dev(case.k16, gpu), dev(v, gpu), heads, case.p)
    z, lse = c16.as_array(z), c16.as_array(lse)
    assert np.all(np.isnan(z[hit, c]))
    clean = np.ones((case.m, case.width), bool)
    clean[hit, c] = False
    frac = ref.worst(z[clean], want[clean], bound[clean])
    print(f"mha16 error/bound nan in v, everything else h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    live = case.live
    assert ref.worst(lse[live], case.ref["lse"][live], case.bound["lse"][live]) <= 1.0      # lse does not read v


def test_gradient_flags(gpu):
    """Only q, only k, only v, none: a gradient that is not asked for stays None, the others keep their bits."""
    case = c16.config_case(8, 8)
    z, q, k, v = run_op(case, gpu)
    z1, q1, k1, v1 = run_op(case, gpu, need=(True, False, False))
    assert k1.grad is None and v1.grad is None and torch.equal(q1.grad, q.grad) and torch.equal(z1, z)
    _, q2, k2, v2 = run_op(case, gpu, need=(False, True, False))
    assert q2.grad is None and v2.grad is None and torch.equal(k2.grad, k.grad)
    _, q3, k3, v3 = run_op(case, gpu, need=(False, False, True))
    assert q3.grad is None and k3.grad is None and torch.equal(v3.grad, v.grad)
    z4, q4, k4, v4 = run_op(case, gpu, need=(False, False, False))
    assert q4.grad is None and k4.grad is None and v4.grad is None and torch.equal(z4, z) and not z4.requires_grad


@pytest.mark.parametrize("mode", ("native", "convert"))
@pytest.mark.parametrize("heads,d,dtype", ((8, 8, BF), (1, 46, FP)))
def test_k_is_v_shares_one_tensor(gpu, heads, d, dtype, mode, monkeypatch):
    """k is v, both routes: the one tensor's gradient receives dk + dv -- each rounded once, then one add in the operands' dtype, so
    the summed bound carries one more unit roundoff of the sum."""
    import isplib_amd
    case = c16.shared_case(heads, d, dtype)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.setenv("ISPLIB_HALF_MHA", mode)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    q, k = dev(case.q16, gpu).requires_grad_(True), dev(case.k16, gpu).requires_grad_(True)
    z = adj.mha_matmul(q, k, k, heads)
    z.backward(dev(case.g16, gpu))
    assert z.dtype == q.grad.dtype == k.grad.dtype == dtype
    held(case, dict(z=z, dq=q.grad), ("z", "dq"), f"mha_matmul {mode}")
    want = case.ref["dk"] + case.ref["dv"]
    bound = case.bound["dk"] + case.bound["dv"]
    bound = bound + half_ref.UNIT_ROUNDOFF[dtype] * np.abs(want)
    frac = ref.worst(c16.as_array(k.grad), want, bound)
    print(f"mha_matmul {mode} error/bound {case.name}: dk+dv={frac:.4f}")
    assert frac <= 1.0


_prefix = {}


def prefix_case(rows, heads, d):
    """The first `rows` rows of the graph (all columns kept): the last block of every kernel's rows launch is not full."""
    if (rows, heads, d) not in _prefix:
        base = c16.config_case(heads, d)
        rowptr = np.array(base.rowptr[:rows + 1])
        col = np.array(base.col[:rowptr[-1]])
        _prefix[rows, heads, d] = c16.Case16(f"first{rows}-h{heads}d{d}", rowptr, col, np.array(base.q[:rows]), np.array(base.k),
                                             np.array(base.v), np.array(base.g[:rows]), heads, base.p, BF)
    return _prefix[rows, heads, d]


@pytest.mark.parametrize("rows", (1, 3, 5))
@pytest.mark.parametrize("heads,d", ((1, 46), (8, 64)))
def test_short_graphs(gpu, rows, heads, d):
    case = prefix_case(rows, heads, d)
    assert case.m == rows and case.n == c16.N
    held(case, run_cabi(case, gpu))


def test_refusals_return_the_documented_codes_in_order_and_leave_the_outputs_untouched(gpu):
    from isplib_amd import cabi
    L = cabi.lib()
    case = c16.config_case(2, 8)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    m, nnz = case.m, col.numel()
    wide = torch.zeros(m, 520, device=gpu, dtype=BF)
    outs = {name: torch.full((m, 520), float("nan"), device=gpu, dtype=BF) for name in ("z", "dq", "dk", "dv")}
    tabs = {name: torch.full((m, 64), float("nan"), device=gpu) for name in ("lse", "D")}
    t_in = torch.zeros(m, 64, device=gpu)
    rp, cp = rowptr.data_ptr(), colptr.data_ptr()

    def call(code=cabi.DTYPE_BF16, mm=m, k=16, heads=2, scale=0.25, ld=520, ldo=520, off=0, null=False):
        w, t = wide.data_ptr() + 2 * off, t_in.data_ptr()
        own = None if null else w
        fw = L.isplib_qkv16_csr_hip(code, mm, m, k, nnz, col.data_ptr(), rp, rp + 8, heads, scale, own, min(ld, ldo), w, ld, w, ld,
                                    outs["z"].data_ptr(), ldo, tabs["lse"].data_ptr(), None)
        e_fw = cabi.last_error()
        rows = L.isplib_qkv16_bw_rows_hip(code, mm, m, k, nnz, col.data_ptr(), rp, rp + 8, heads, scale, own, min(ld, ldo), w, ld, w, ld, w,
                                          min(ld, ldo), t, outs["dq"].data_ptr(), ldo, tabs["D"].data_ptr(), None)
        e_rows = cabi.last_error()
        cols = L.isplib_qkv16_bw_cols_hip(code, mm, m, k, nnz, row_t.data_ptr(), cp, cp + 8, heads, scale, w, ld, w, ld, t, t, own,
                                          min(ld, ldo), w, min(ld, ldo), outs["dk"].data_ptr(), ldo, outs["dv"].data_ptr(), ldo, None)
        return (fw, rows, cols), (e_fw, e_rows, cabi.last_error())

    F, N_ = cabi.FAIL, cabi.NO_OPT_IMPL
    # (what, arguments, the three codes, a word of every message): each row adds one fault to the right of the previous one's kind, so the
    # earlier refusal must win
    for what, kwargs, want, word in (
            ("the fp32 dtype code", dict(code=0), (F, F, F), "dtype"),
            ("dtype before a negative dimension", dict(code=0, mm=-1), (F, F, F), "dtype"),
            ("a negative dimension before a pitch below K", dict(mm=-1, ldo=14), (F, F, F), "negative"),
            ("a pitch below K before k % heads", dict(k=18, heads=4, ldo=16), (F, F, F), "leading dimension"),
            ("k % heads before the scale", dict(k=18, heads=4, scale=float("nan")), (F, F, F), "multiple of heads"),
            ("the scale before the domain", dict(k=16, heads=4, scale=float("inf")), (F, F, F), "finite"),
            ("odd K", dict(k=15, heads=1), (N_, N_, N_), "isplib_qkv16_serves"),
            ("K = 6", dict(k=6, heads=1), (N_, N_, N_), "isplib_qkv16_serves"),
            ("K = 514", dict(k=514, heads=1), (N_, N_, N_), "isplib_qkv16_serves"),
            ("d = 4", dict(k=16, heads=4), (N_, N_, N_), "isplib_qkv16_serves"),
            ("d = 12", dict(k=24, heads=2), (N_, N_, N_), "isplib_qkv16_serves"),
            ("heads = 0", dict(heads=0), (N_, N_, N_), "isplib_qkv16_serves"),
            ("odd pitch", dict(ld=519), (N_, N_, N_), "isplib_qkv16_serves"),
            ("odd output pitch", dict(ldo=519), (N_, N_, N_), "isplib_qkv16_serves"),
            ("the domain before a null operand", dict(k=16, heads=4, null=True), (N_, N_, N_), "isplib_qkv16_serves"),
            ("a null operand before alignment", dict(null=True, off=1), (F, F, F), "null"),
            ("a base offset by one element", dict(off=1), (F, F, F), "4-byte aligned")):
        codes, messages = call(**kwargs)
        assert codes == want, (what, codes, messages)
        assert all(word in msg for msg in messages), (what, messages)
    torch.cuda.synchronize()
    for t in list(outs.values()) + list(tabs.values()):
        assert torch.isnan(t).all()
    # nothing to do comes before everything but dtype and a negative dimension: success without a launch, whatever else is wrong
    codes, _ = call(mm=0, ldo=14, null=True)
    assert codes[:2] == (cabi.SUCCESS, cabi.SUCCESS)
    codes, _ = call(k=0, heads=0, null=True, scale=float("nan"))
    assert codes == (cabi.SUCCESS,) * 3
    q16 = wide[:, :16]
    for qq, kk, vv, heads in ((q16.float(), q16, q16, 2), (q16, q16.to(FP), q16, 2), (q16, q16, q16.float(), 2),
                              (wide[:, :15], wide[:, :15], wide[:, :15], 1), (q16, q16, q16, 4), (q16[:-1], q16, q16, 2), (q16, q16, q16, 3),
                              (q16, q16, q16.cpu(), 2)):
        with pytest.raises(RuntimeError, match="mha_spmm16"):
            torch.ops.isplib.mha_spmm16(rowptr, col, colptr, row_t, qq, kk, vv, heads, 0.25)
    with pytest.raises(RuntimeError, match="finite"):
        torch.ops.isplib.mha_spmm16(rowptr, col, colptr, row_t, q16, q16, q16, 2, float("nan"))
    torch.cuda.synchronize()
    assert torch.isnan(outs["z"]).all()


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
def test_plugin_routes(gpu, dtype, monkeypatch):
    """unset -> the existing TypeError; convert -> the bits of the hand-written conversion, within the 16-bit bound; native inside the
    domain -> the operator's bits (the C ABI path's), within the bound; native at K = 6, at odd K and at (H, d) = (2, 4) -> the
    conversion route's bits, nothing raised; auto follows native_pays; ISPLIB_HALF=convert wins; mixed dtypes -> TypeError; fp32 calls
    are unaffected by any setting."""
    import isplib_amd
    from isplib_amd import cabi
    case = c16.config_case(8, 8, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n))
    g = dev(case.g16, gpu)

    def leaves(k=None):
        ops = [dev(t, gpu) for t in (case.q16, case.k16, case.v16)]
        if k is not None:
            ops = [t[:, :k].contiguous() for t in ops]
        return [t.requires_grad_(True) for t in ops]

    def by_hand(q, k, v, gg, heads):
        z = isplib_amd.mha_matmul(adj, q.float(), k.float(), v.float(), heads).to(dtype)
        z.backward(gg)
        return z.detach(), q.grad, k.grad, v.grad

    def through(q, k, v, gg, heads):
        z = adj.mha_matmul(q, k, v, heads)
        z.backward(gg)
        assert z.dtype == q.grad.dtype == k.grad.dtype == v.grad.dtype == dtype
        return z.detach(), q.grad, k.grad, v.grad

    def same(a, b):
        return all(torch.equal(u, v) for u, v in zip(a, b))

    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_MHA", raising=False)
    q0, k0, v0 = (t.detach() for t in leaves())
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.mha_matmul(adj, q0, k0, v0, 8)
    want = by_hand(*leaves(), g, 8)
    fp32 = isplib_amd.mha_matmul(adj, q0.float(), k0.float(), v0.float(), 8)

    monkeypatch.setenv("ISPLIB_HALF_MHA", "convert")
    got = through(*leaves(), g, 8)
    assert same(got, want)
    held(case, dict(zip(OP_OUTPUTS, got)), OP_OUTPUTS, "mha_matmul convert")
    assert torch.equal(isplib_amd.mha_matmul(adj, q0.float(), k0.float(), v0.float(), 8), fp32)

    monkeypatch.setenv("ISPLIB_HALF_MHA", "native")
    abi = run_cabi(case, gpu)
    native = tuple(abi[n] for n in OP_OUTPUTS)
    got = through(*leaves(), g, 8)
    assert same(got, native)
    held(case, dict(zip(OP_OUTPUTS, got)), OP_OUTPUTS, "mha_matmul native")
    assert torch.equal(isplib_amd.mha_matmul(adj, q0.float(), k0.float(), v0.float(), 8), fp32)
    other = FP if dtype == BF else BF
    for ops in ((q0, k0.to(other), v0), (q0, k0, v0.float()), (q0.float(), k0, v0)):
        with pytest.raises(TypeError, match="share one 16-bit dtype"):
            adj.mha_matmul(*ops, 8)
    # native at K = 6, at odd K and at (H, d) = (2, 4): outside the 16-bit domain, the conversion route's bits, nothing raised
    for k, heads in ((6, 1), (29, 1), (8, 2)):
        gg = g[:, :k].contiguous()
        assert same(through(*leaves(k), gg, heads), by_hand(*leaves(k), gg, heads)), (k, heads)
    # ISPLIB_HALF=convert wins over native
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert same(through(*leaves(), g, 8), want)
    monkeypatch.delenv("ISPLIB_HALF")
    # auto: whatever the measured rule says for this class, and whatever it could say
    monkeypatch.setenv("ISPLIB_HALF_MHA", "auto")
    assert same(through(*leaves(), g, 8), native if cabi.mha16_native_pays(case.n, case.width) else want)
    for pays in (True, False):
        with monkeypatch.context() as mp:
            mp.setattr(cabi, "mha16_native_pays", lambda rows, ld, pays=pays: pays)
            assert same(through(*leaves(), g, 8), native if pays else want)
