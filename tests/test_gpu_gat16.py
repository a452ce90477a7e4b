"""The 16-bit GAT operator on the GPU (isplib_amd/csrc/gat16.hip): the C ABI wrappers, torch.ops.isplib.gat_spmm16 with its autograd
backward, and the plug-in's opt-in route (ISPLIB_HALF_GAT), each held to the per-element bounds of tests/gat16_ref.py against the fp64
reference on the widened operands (inputs, references and bounds: tests/gat16_cases.py, computed once per case).  The largest
error / bound seen per output is printed before every assertion; DESIGN.md 4.6e records it.
"""
import numpy as np
import pytest
import torch

from tests import gat16_cases as c16
from tests import gat_ref as ref
from tests import half_ref

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16


def dev(a, gpu):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a))).to(gpu)


def dev_graph(case, gpu):
    return dev(case.rowptr, gpu), dev(case.col, gpu)


_transposed = {}


def transposed(case, gpu):
    """colptr / row_t as SparseStorage caches them (the library's own csr2csc), once per graph."""
    import isplib_amd
    key = (case.rowptr.tobytes(), case.col.tobytes())
    if key not in _transposed:
        rowptr, col = dev_graph(case, gpu)
        st = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.n)).storage
        _transposed[key] = (st.colptr(), st.row_t())
    return _transposed[key]


def held(case, got, names=c16.OUTPUTS, what="gat16"):
    frac = c16.fractions(case, got, names)
    print(f"{what} error/bound {case.name}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def run_cabi(case, gpu, y=None, a_src=None, g=None):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    y = dev(case.y16, gpu) if y is None else y
    g = dev(case.g16, gpu) if g is None else g
    a_dst, a_src = dev(case.a_dst, gpu), dev(case.a_src, gpu) if a_src is None else a_src
    z, lse = cabi.gat16_forward(rowptr, col, y, a_dst, a_src, case.heads, case.ns)
    dadst, D = cabi.gat16_backward_rows(rowptr, col, y, a_dst, a_src, g, lse, case.heads, case.ns)
    dy, dasrc = cabi.gat16_backward_cols(colptr, row_t, y, a_dst, a_src, g, lse, D, case.heads, case.ns)
    return dict(z=z, lse=lse, dadst=dadst, D=D, dy=dy, dasrc=dasrc)


def run_op(case, gpu, need=(True, True, True)):
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    y = dev(case.y16, gpu).requires_grad_(need[0])
    a_dst, a_src = dev(case.a_dst, gpu).requires_grad_(need[1]), dev(case.a_src, gpu).requires_grad_(need[2])
    z = torch.ops.isplib.gat_spmm16(rowptr, col, colptr, row_t, y, a_dst, a_src, case.heads, case.ns)
    z.backward(dev(case.g16, gpu))
    return z.detach(), y, a_dst, a_src


def check_case(case, gpu):
    """Both surfaces on one case: every output of the wrappers, elementwise; then the operator's autograd gives the wrappers' bits."""
    got = run_cabi(case, gpu)
    assert got["z"].dtype == got["dy"].dtype == case.dtype
    assert all(got[n].dtype == torch.float32 for n in ("lse", "dadst", "D", "dasrc"))
    held(case, got)
    empty = ~case.live
    if empty.any():
        assert not got["z"].cpu()[empty].any() and not got["dadst"].cpu()[empty].any() and not got["D"].cpu()[empty].any()
    unreferenced = np.bincount(case.col, minlength=case.n) == 0
    if unreferenced.any():
        assert not got["dy"].cpu()[unreferenced].any() and not got["dasrc"].cpu()[unreferenced].any()
    z, y, a_dst, a_src = run_op(case, gpu)
    assert z.dtype == y.grad.dtype == case.dtype and a_dst.grad.dtype == a_src.grad.dtype == torch.float32
    held(case, dict(z=z, dy=y.grad, dadst=a_dst.grad, dasrc=a_src.grad), ("z", "dy", "dadst", "dasrc"), "gat_spmm16")
    for name, v in (("z", z), ("dy", y.grad), ("dadst", a_dst.grad), ("dasrc", a_src.grad)):
        assert torch.equal(v, got[name]), name
    return got


@pytest.mark.parametrize("spec", c16.config_cases(), ids=c16.case_id)
def test_every_configuration(gpu, spec):
    """First, last and a ragged width of every LPR, heads of one lane up to half a slot, head counts that are no power of two; bf16
    everywhere, fp16 once per LPR; (8, 8) and (1, 34) also on the graph whose row lengths sit at the edges of G and of a step."""
    check_case(c16.config_case(spec[0], spec[1], spec[2], graph=spec[3]), gpu)


@pytest.mark.parametrize("case", c16.slope_cases(), ids=lambda c: c.name)
def test_slopes_zero_and_one(gpu, case):
    check_case(case, gpu)


def test_scores_spread_over_200(gpu):
    case = c16.large_case()
    got = check_case(case, gpu)
    for name in c16.OUTPUTS:
        v = c16.as_array(got[name])
        assert np.all(np.isfinite(v[case.live] if name == "lse" else v)), name


def test_one_entry_rows_return_y_bit_for_bit(gpu):
    """z equals y_j's 16 bits whatever the score (|u| to 8e3) and lse equals the fp32 s_e; an empty row writes 0 and -inf."""
    case = c16.single_case()
    got = check_case(case, gpu)
    live = case.live
    want = torch.zeros_like(case.y16[:case.m])
    want[torch.from_numpy(live)] = case.y16[torch.from_numpy(case.col)]
    assert np.array_equal(half_ref.bits(got["z"]), half_ref.bits(want))
    u32 = (case.a_dst[case.ref["row"]] + case.a_src[case.col]).astype(np.float32)           # ONE fp32 add, then the slope
    s32 = np.where(u32 > 0, u32, (np.float32(case.ns) * u32).astype(np.float32)).astype(np.float32)
    lse = got["lse"].cpu().numpy()
    assert np.all(np.isneginf(lse[~live])) and np.array_equal(lse[live].view(np.uint32), s32.view(np.uint32))
    assert (~live).any() and not got["z"].cpu()[~live].any()


@pytest.mark.parametrize("heads,d,dtype", ((1, 10, BF), (5, 8, BF), (1, 510, FP), (8, 64, BF)))
def test_outputs_are_write_only_and_launches_repeat(gpu, heads, d, dtype):
    """NaN-filled, pitched (ld = K + 6), over-allocated outputs, launched twice: every element of every row is written, nothing between
    the rows or past the end, equal bits."""
    from isplib_amd import cabi
    case = c16.config_case(heads, d, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    y, g, a_dst, a_src = dev(case.y16, gpu), dev(case.g16, gpu), dev(case.a_dst, gpu), dev(case.a_src, gpu)
    m, n, k, H, ns, pad, ld = case.m, case.n, case.k, heads, case.ns, 64, case.k + 6

    def wide(rows):
        buf = torch.full((rows * ld + pad,), float("nan"), device=gpu, dtype=dtype)
        return buf, buf[:rows * ld].view(rows, ld)[:, :k]

    def table(rows):
        buf = torch.full((rows * H + pad,), float("nan"), device=gpu)
        return buf, buf[:rows * H].view(rows, H)

    runs = []
    for _ in range(2):
        b = dict(z=wide(m), lse=table(m), dadst=table(m), D=table(m), dy=wide(n), dasrc=table(n))
        cabi.gat16_forward(rowptr, col, y, a_dst, a_src, H, ns, out=(b["z"][1], b["lse"][1]), check=False)
        cabi.gat16_backward_rows(rowptr, col, y, a_dst, a_src, g, b["lse"][1], H, ns, out=(b["dadst"][1], b["D"][1]), check=False)
        cabi.gat16_backward_cols(colptr, row_t, y, a_dst, a_src, g, b["lse"][1], b["D"][1], H, ns, out=(b["dy"][1], b["dasrc"][1]), check=False)
        for name, (buf, view) in b.items():
            assert not torch.isnan(view).any(), name
            if name in ("z", "dy"):
                rest = buf[:view.size(0) * ld].view(view.size(0), ld)[:, k:]
                assert torch.isnan(rest).all() and torch.isnan(buf[view.size(0) * ld:]).all(), name
            else:
                assert torch.isnan(buf[view.numel():]).all(), name
        runs.append({name: view.clone() for name, (_, view) in b.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    held(case, runs[0])


@pytest.mark.parametrize("heads,d", ((1, 10), (8, 8), (3, 128)))
def test_column_views_keep_their_pitch(gpu, heads, d):
    """y and g as the middle column block of a [N, 3 K] tensor whose neighbours hold NaN and Inf go in without a copy and give the bits
    of the packed operands -- an over-read column in a dot product, or Inf * 0, would show -- through the wrappers and the operator."""
    case = c16.config_case(heads, d)
    k = case.k
    packed = run_cabi(case, gpu)
    view = {}
    for name, a in (("y", case.y16), ("g", case.g16)):
        t = torch.empty(case.m, 3 * k, device=gpu, dtype=case.dtype)
        t[:, :k] = float("nan")
        t[:, 2 * k:] = float("inf")
        t[:, k:2 * k] = dev(a, gpu)
        view[name] = t[:, k:2 * k]
        assert not view[name].is_contiguous() and view[name].stride(0) == 3 * k
    got = run_cabi(case, gpu, y=view["y"], g=view["g"])
    for name in c16.OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    yw = view["y"]._base.clone().requires_grad_(True)
    a_dst, a_src = dev(case.a_dst, gpu).requires_grad_(True), dev(case.a_src, gpu).requires_grad_(True)
    z = torch.ops.isplib.gat_spmm16(rowptr, col, colptr, row_t, yw[:, k:2 * k], a_dst, a_src, heads, case.ns)
    z.backward(view["g"])
    assert torch.equal(z.detach(), packed["z"]) and torch.equal(yw.grad[:, k:2 * k], packed["dy"])
    assert torch.equal(a_dst.grad, packed["dadst"]) and torch.equal(a_src.grad, packed["dasrc"])
    assert not yw.grad[:, :k].any() and not yw.grad[:, 2 * k:].any()


@pytest.mark.parametrize("heads,d", ((8, 8), (2, 256)))
def test_a_nan_score_poisons_exactly_its_head(gpu, heads, d):
    """A NaN in a_src[j, h]: exactly head h of the rows that reference j, in z and lse; everything else inside the bound."""
    case = c16.config_case(heads, d)
    j = int(case.col[case.rowptr[2]])                     # a column some rows reference
    hit = np.zeros(case.m, bool)
    hit[case.ref["row"][case.col == j]] = True
    assert hit.any() and (~hit & case.live).any()
    h = heads - 1
    a_src = np.array(case.a_src)
    a_src[j, h] = np.nan
    got = run_cabi(case, gpu, a_src=dev(a_src, gpu))
    z, lse = ref.per_head(c16.as_array(got["z"]), heads), c16.as_array(got["lse"])
    want, bound = ref.per_head(case.ref["z"], heads), ref.per_head(case.bound["z"], heads)
    assert np.all(np.isnan(z[hit, h])) and np.all(np.isnan(lse[hit, h]))
    clean = np.ones((case.m, heads), bool)
    clean[hit, h] = False
    frac = ref.worst(z[clean], want[clean], bound[clean])
    print(f"gat16 error/bound nan a_src, everything else h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    ok = clean & case.live[:, None]
    assert ref.worst(lse[ok], case.ref["lse"][ok], case.bound["lse"][ok]) <= 1.0


def test_gradient_flags_and_one_tensor_for_both_scores(gpu):
    """Only a_dst asking: the columns kernel does not run (y.grad and a_src.grad stay None) and d a_dst has the same bits.  One tensor
    for both scores on the square graph: its gradient is the sum of both parts."""
    case = c16.config_case(8, 8)
    z, y, a_dst, a_src = run_op(case, gpu)
    z1, y1, a_dst1, a_src1 = run_op(case, gpu, need=(False, True, False))
    assert y1.grad is None and a_src1.grad is None and torch.equal(a_dst1.grad, a_dst.grad) and torch.equal(z1, z)
    _, y2, a_dst2, a_src2 = run_op(case, gpu, need=(True, False, False))
    assert a_dst2.grad is None and a_src2.grad is None and torch.equal(y2.grad, y.grad)
    _, y3, a_dst3, a_src3 = run_op(case, gpu, need=(False, False, True))
    assert y3.grad is None and a_dst3.grad is None and torch.equal(a_src3.grad, a_src.grad)
    # one tensor for both scores
    both = c16.Case16("h8d8-one-score", case.rowptr, case.col, np.array(case.y), case.a_dst, case.a_dst, np.array(case.g), 8, case.ns, BF)
    rowptr, col = dev_graph(both, gpu)
    colptr, row_t = transposed(both, gpu)
    a = dev(both.a_dst, gpu).requires_grad_(True)
    z = torch.ops.isplib.gat_spmm16(rowptr, col, colptr, row_t, dev(both.y16, gpu), a, a, 8, both.ns)
    z.backward(dev(both.g16, gpu))
    held(both, dict(z=z), ("z",), "gat_spmm16")
    want = both.ref["dadst"] + both.ref["dasrc"]
    bound = both.bound["dadst"] + both.bound["dasrc"]
    bound = bound + 2.0 ** -24 * (np.abs(want) + bound)                                  # autograd's one fp32 add of the two parts
    frac = ref.worst(c16.as_array(a.grad), want, bound)
    print(f"gat_spmm16 error/bound {both.name}: dadst+dasrc={frac:.4f}")
    assert frac <= 1.0


def test_refusals_return_the_documented_codes_and_leave_the_outputs_untouched(gpu):
    from isplib_amd import cabi
    L = cabi.lib()
    case = c16.config_case(2, 8)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    m, nnz = case.m, col.numel()
    wide = torch.zeros(m, 520, device=gpu, dtype=BF)
    outs = {name: torch.full((m, 520), float("nan"), device=gpu, dtype=BF) for name in ("z", "dy")}
    tabs = {name: torch.full((m, 64), float("nan"), device=gpu) for name in ("lse", "dadst", "D", "dasrc")}
    t_in = torch.zeros(m, 64, device=gpu)
    rp, cp = rowptr.data_ptr(), colptr.data_ptr()

    def call(code=cabi.DTYPE_BF16, k=16, heads=2, ld=520, ldo=520, off=0):
        y, t = wide.data_ptr() + 2 * off, t_in.data_ptr()
        fw = L.isplib_gat16_csr_hip(code, m, m, k, nnz, col.data_ptr(), rp, rp + 8, t, y, ld, t, heads, 0.2, outs["z"].data_ptr(), ldo,
                                    tabs["lse"].data_ptr(), None)
        e_fw = cabi.last_error()
        rows = L.isplib_gat16_bw_rows_hip(code, m, m, k, nnz, col.data_ptr(), rp, rp + 8, t, y, ld, t, heads, 0.2, y, min(ld, ldo), t,
                                          tabs["dadst"].data_ptr(), tabs["D"].data_ptr(), None)
        cols = L.isplib_gat16_bw_cols_hip(code, m, m, k, nnz, row_t.data_ptr(), cp, cp + 8, t, y, min(ld, ldo), t, heads, 0.2, y, ld, t, t,
                                          outs["dy"].data_ptr(), ldo, tabs["dasrc"].data_ptr(), None)
        return (fw, rows, cols), e_fw

    for what, kwargs, want in (("odd K", dict(k=15, heads=1), cabi.NO_OPT_IMPL), ("K = 6", dict(k=6, heads=1), cabi.NO_OPT_IMPL),
                               ("K = 514", dict(k=514, heads=1), cabi.NO_OPT_IMPL), ("d = 4", dict(k=16, heads=4), cabi.NO_OPT_IMPL),
                               ("d = 12", dict(k=24, heads=2), cabi.NO_OPT_IMPL), ("heads = 0", dict(heads=0), cabi.NO_OPT_IMPL),
                               ("odd pitch", dict(ld=519), cabi.NO_OPT_IMPL), ("odd output pitch", dict(ldo=519), cabi.NO_OPT_IMPL),
                               ("a base offset by one element", dict(off=1), cabi.FAIL), ("the fp32 dtype code", dict(code=0), cabi.FAIL),
                               ("k no multiple of heads", dict(k=18, heads=4), cabi.FAIL), ("a pitch below K", dict(k=16, ldo=14), cabi.FAIL)):
        codes, message = call(**kwargs)
        assert codes == (want,) * 3, (what, codes)
        assert ("isplib_gat16_serves" in message) == (want == cabi.NO_OPT_IMPL), (what, message)
    torch.cuda.synchronize()
    for t in list(outs.values()) + list(tabs.values()):
        assert torch.isnan(t).all()
    y, t = wide.data_ptr(), t_in.data_ptr()
    args = lambda mm, k, yp: (cabi.DTYPE_BF16, mm, m, k, nnz, col.data_ptr(), rp, rp + 8, t, yp, 520, t, 2, 0.2, outs["z"].data_ptr(), 520,  # noqa: E731
                              tabs["lse"].data_ptr(), None)
    assert L.isplib_gat16_csr_hip(*args(0, 16, None)) == cabi.SUCCESS and L.isplib_gat16_csr_hip(*args(m, 0, None)) == cabi.SUCCESS
    assert L.isplib_gat16_csr_hip(*args(-1, 16, y)) == cabi.FAIL
    assert L.isplib_gat16_csr_hip(*args(m, 16, None)) == cabi.FAIL and "null" in cabi.last_error()
    a_dst, a_src = t_in[:, :2].contiguous(), t_in[:, :2].contiguous()
    for yy, ad, heads in ((wide[:, :16].float(), a_dst, 2), (wide[:, :16], a_dst.to(BF), 2), (wide[:, :15], a_dst[:, :1].contiguous(), 1),
                          (wide[:, :16], a_dst, 4), (wide[:, :16], a_dst[:-1], 2), (wide[:, :16], a_dst, 3)):
        with pytest.raises(RuntimeError, match="gat_spmm16"):
            torch.ops.isplib.gat_spmm16(rowptr, col, colptr, row_t, yy, ad, a_src if heads == 2 else a_src[:, :1].contiguous(), heads, 0.2)
    torch.cuda.synchronize()
    assert torch.isnan(outs["z"]).all()


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
def test_plugin_routes(gpu, dtype, monkeypatch):
    """unset -> the existing TypeError; convert -> the bits of the hand-written conversion; native inside the domain -> the operator's
    bits, within the bound; native at (8, 4) and at odd K -> the conversion route's bits, nothing raised; ISPLIB_HALF=convert wins;
    mixed dtypes -> TypeError; fp32 calls are unaffected by any setting."""
    import isplib_amd
    case = c16.config_case(8, 8, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    g = dev(case.g16, gpu)

    def leaves(k=None, heads=None):
        y = dev(case.y16, gpu)
        a_dst, a_src = dev(case.a_dst, gpu), dev(case.a_src, gpu)
        if k is not None:
            y, a_dst, a_src = y[:, :k].contiguous(), a_dst[:, :heads].contiguous(), a_src[:, :heads].contiguous()
        return y.requires_grad_(True), a_dst.requires_grad_(True), a_src.requires_grad_(True)

    def by_hand(y, a_dst, a_src, gg, heads):
        z = isplib_amd.gat_matmul(adj, y.float(), a_dst, a_src, heads, case.ns).to(dtype)
        z.backward(gg)
        return z.detach(), y.grad, a_dst.grad, a_src.grad

    def through(y, a_dst, a_src, gg, heads):
        z = adj.gat_matmul(y, a_dst, a_src, heads, case.ns)
        z.backward(gg)
        assert z.dtype == y.grad.dtype == dtype and a_dst.grad.dtype == a_src.grad.dtype == torch.float32
        return z.detach(), y.grad, a_dst.grad, a_src.grad

    def same(a, b):
        return all(torch.equal(u, v) for u, v in zip(a, b))

    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_GAT", raising=False)
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.gat_matmul(adj, *leaves(), 8, case.ns)
    want = by_hand(*leaves(), g, 8)
    y32, ad32, as32 = leaves()
    fp32 = isplib_amd.gat_matmul(adj, y32.detach().float(), ad32.detach(), as32.detach(), 8, case.ns)

    monkeypatch.setenv("ISPLIB_HALF_GAT", "convert")
    assert same(through(*leaves(), g, 8), want)
    assert torch.equal(isplib_amd.gat_matmul(adj, y32.detach().float(), ad32.detach(), as32.detach(), 8, case.ns), fp32)

    monkeypatch.setenv("ISPLIB_HALF_GAT", "native")
    yd, add, asd = leaves()
    zd = torch.ops.isplib.gat_spmm16(rowptr, col, colptr, row_t, yd, add, asd, 8, case.ns)
    zd.backward(g)
    got = through(*leaves(), g, 8)
    assert same(got, (zd.detach(), yd.grad, add.grad, asd.grad))
    held(case, dict(z=got[0], dy=got[1], dadst=got[2], dasrc=got[3]), ("z", "dy", "dadst", "dasrc"), "gat_matmul")
    assert torch.equal(isplib_amd.gat_matmul(adj, y32.detach().float(), ad32.detach(), as32.detach(), 8, case.ns), fp32)
    other = FP if dtype == BF else BF
    with pytest.raises(TypeError, match="`y`'s dtype"):
        adj.gat_matmul(yd.detach(), add.detach().to(other), asd.detach(), 8, case.ns)
    with pytest.raises(TypeError, match="float32"):
        adj.gat_matmul(yd.detach().float(), add.detach().to(dtype), asd.detach(), 8, case.ns)
    # native at (8, 4) and at odd K: outside the 16-bit domain, the conversion route's bits, nothing raised
    for k, heads in ((32, 8), (29, 1)):
        gg = g[:, :k].contiguous()
        assert same(through(*leaves(k, heads), gg, heads), by_hand(*leaves(k, heads), gg, heads)), (k, heads)
    # ISPLIB_HALF=convert wins over native
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert same(through(*leaves(), g, 8), want)
    monkeypatch.delenv("ISPLIB_HALF")
    # auto: whatever the measured rule says for this class, one of the two routes' bits
    monkeypatch.setenv("ISPLIB_HALF_GAT", "auto")
    from isplib_amd import cabi
    pays = cabi.gat16_native_pays(case.n, case.k)
    assert same(through(*leaves(), g, 8), (zd.detach(), yd.grad, add.grad, asd.grad) if pays else want)


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
def test_scores_in_the_operand_dtype(gpu, dtype, monkeypatch):
    """16-bit scores through gat_matmul give the bits of the same call with the scores widened by hand; their gradients have the scores'
    dtype: the fp32 gradient rounded once by the cast."""
    import isplib_amd
    case = c16.config_case(8, 8, dtype)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    g = dev(case.g16, gpu)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    for mode in ("native", "convert"):
        monkeypatch.setenv("ISPLIB_HALF_GAT", mode)
        y = dev(case.y16, gpu).requires_grad_(True)
        a_dst, a_src = dev(case.a_dst, gpu).to(dtype).requires_grad_(True), dev(case.a_src, gpu).to(dtype).requires_grad_(True)
        z = adj.gat_matmul(y, a_dst, a_src, 8, case.ns)
        z.backward(g)
        yh = dev(case.y16, gpu).requires_grad_(True)
        ad_h, as_h = a_dst.detach().float().requires_grad_(True), a_src.detach().float().requires_grad_(True)
        zh = adj.gat_matmul(yh, ad_h, as_h, 8, case.ns)
        zh.backward(g)
        assert a_dst.grad.dtype == a_src.grad.dtype == dtype and z.dtype == y.grad.dtype == dtype
        assert torch.equal(z, zh) and torch.equal(y.grad, yh.grad), mode
        assert torch.equal(a_dst.grad, ad_h.grad.to(dtype)) and torch.equal(a_src.grad, as_h.grad.to(dtype)), mode
        # one score in each dtype is admitted too
        z2 = adj.gat_matmul(y.detach(), a_dst.detach(), as_h.detach(), 8, case.ns)
        assert torch.equal(z2, z.detach()), mode
