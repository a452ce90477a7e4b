"""The 16-bit GATv2 operator on the GPU (isplib_amd/csrc/gatv2_16.hip): the C ABI wrappers, torch.ops.isplib.gatv2_spmm16 with its
autograd backward, and the plug-in's opt-in route (ISPLIB_HALF_GATV2), each held to the per-element bounds of tests/gatv2_16_ref.py
against the fp64 reference on the widened operands (inputs, references and bounds: tests/gatv2_16_cases.py, computed once per case).
The largest error / bound seen per output is printed before every assertion; DESIGN.md 4.6g records it.
"""
import numpy as np
import pytest
import torch

from tests import gatv2_16_cases as c16
from tests import gatv2_ref as ref
from tests import half_ref
from tests.gat_ref import per_head

pytestmark = pytest.mark.gpu

BF, FP = torch.bfloat16, torch.float16
OP_OUTPUTS = ("z", "dx", "dy", "datt")


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


def held(case, got, names=c16.OUTPUTS, what="gatv2_16"):
    frac = c16.fractions(case, got, names)
    print(f"{what} error/bound {case.name}: " + " ".join(f"{k}={v:.4f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (case.name, frac)
    return frac


def run_cabi(case, gpu, x=None, y=None, g=None, want_datt=True):
    from isplib_amd import cabi
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    x = dev(case.x16, gpu) if x is None else x
    y = dev(case.y16, gpu) if y is None else y
    g = dev(case.g16, gpu) if g is None else g
    att = dev(case.att, gpu)
    z, lse = cabi.gatv2_16_forward(rowptr, col, x, y, att, case.heads, case.ns)
    dx, D, datt = cabi.gatv2_16_backward_rows(rowptr, col, x, y, att, g, lse, case.heads, case.ns, want_datt=want_datt)
    dy = cabi.gatv2_16_backward_cols(colptr, row_t, x, y, att, g, lse, D, case.heads, case.ns)
    return dict(z=z, lse=lse, dx=dx, D=D, dy=dy, datt=datt)


def run_op(case, gpu, need=(True, True, True)):
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    x, y = dev(case.x16, gpu).requires_grad_(need[0]), dev(case.y16, gpu).requires_grad_(need[1])
    att = dev(case.att, gpu).requires_grad_(need[2])
    z = torch.ops.isplib.gatv2_spmm16(rowptr, col, colptr, row_t, x, y, att, case.heads, case.ns)
    if any(need):
        z.backward(dev(case.g16, gpu))
    return z.detach(), x, y, att


def check_case(case, gpu):
    """Both surfaces on one case: every output of the wrappers, elementwise; then the operator's autograd gives the wrappers' bits."""
    got = run_cabi(case, gpu)
    assert got["z"].dtype == got["dx"].dtype == got["dy"].dtype == case.dtype
    assert all(got[n].dtype == torch.float32 for n in ("lse", "D", "datt"))
    held(case, got)
    empty = ~case.live
    if empty.any():
        assert not got["z"].cpu()[empty].any() and not got["dx"].cpu()[empty].any() and not got["D"].cpu()[empty].any()
    unreferenced = np.bincount(case.col, minlength=case.n) == 0
    if unreferenced.any():
        assert not got["dy"].cpu()[unreferenced].any()
    z, x, y, att = run_op(case, gpu)
    assert z.dtype == x.grad.dtype == y.grad.dtype == case.dtype and att.grad.dtype == torch.float32
    held(case, dict(z=z, dx=x.grad, dy=y.grad, datt=att.grad), OP_OUTPUTS, "gatv2_spmm16")
    for name, v in (("z", z), ("dx", x.grad), ("dy", y.grad), ("datt", att.grad)):
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


def test_scores_spread_beyond_150(gpu):
    case = c16.large_case()
    got = check_case(case, gpu)
    for name in c16.OUTPUTS:
        v = c16.as_array(got[name])
        assert np.all(np.isfinite(v[case.live] if name == "lse" else v)), name


def test_one_entry_rows_return_y_bit_for_bit(gpu):
    """z equals y_j's 16 bits whatever the score; dx of a one-entry row is exactly 0 or within the bound (check_case holds it to the
    bound); an empty row writes 0, -inf and 0."""
    case = c16.single_case()
    got = check_case(case, gpu)
    live = case.live
    want = torch.zeros_like(case.y16[:case.m])
    want[torch.from_numpy(live)] = case.y16[torch.from_numpy(case.col)]
    assert np.array_equal(half_ref.bits(got["z"]), half_ref.bits(want))
    lse = got["lse"].cpu().numpy()
    assert (~live).any() and np.all(np.isneginf(lse[~live])) and np.all(np.isfinite(lse[live]))
    assert not got["z"].cpu()[~live].any() and not got["dx"].cpu()[~live].any() and not got["D"].cpu()[~live].any()
    dx = c16.as_array(got["dx"])
    print(f"gatv2_16 one-entry rows: dx exactly 0 in {int((dx[live] == 0).all(1).sum())} of {int(live.sum())} rows")


@pytest.mark.parametrize("heads,d,dtype", ((1, 10, BF), (5, 8, BF), (1, 510, FP), (8, 64, BF)))
def test_outputs_are_write_only_and_launches_repeat(gpu, heads, d, dtype):
    """NaN-filled, pitched (ld = K + 6), over-allocated outputs and a NaN-filled workspace, launched twice with datt: every element of
    every row is written, nothing between the rows or past the end, equal bits -- datt included."""
    from isplib_amd import cabi
    case = c16.config_case(heads, d, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    x, y, g, att = dev(case.x16, gpu), dev(case.y16, gpu), dev(case.g16, gpu), dev(case.att, gpu)
    m, n, k, H, ns, pad, ld = case.m, case.n, case.k, heads, case.ns, 64, case.k + 6
    need = cabi.gatv2_16_bw_rows_workspace_bytes(m, k)

    def wide(rows):
        buf = torch.full((rows * ld + pad,), float("nan"), device=gpu, dtype=dtype)
        return buf, buf[:rows * ld].view(rows, ld)[:, :k]

    def table(rows, cols):
        buf = torch.full((rows * cols + pad,), float("nan"), device=gpu)
        return buf, buf[:rows * cols].view(rows, cols)

    runs = []
    for _ in range(2):
        b = dict(z=wide(m), lse=table(m, H), dx=wide(m), D=table(m, H), dy=wide(n), datt=table(H, d))
        work = torch.full((need + 256,), 0xFF, device=gpu, dtype=torch.uint8)             # 0xFFFFFFFF: a NaN in every float
        cabi.gatv2_16_forward(rowptr, col, x, y, att, H, ns, out=(b["z"][1], b["lse"][1]), check=False)
        cabi.gatv2_16_backward_rows(rowptr, col, x, y, att, g, b["lse"][1], H, ns, out=(b["dx"][1], b["D"][1], b["datt"][1]),
                                    workspace=work[:need], check=False)
        cabi.gatv2_16_backward_cols(colptr, row_t, x, y, att, g, b["lse"][1], b["D"][1], H, ns, out=b["dy"][1], check=False)
        assert (work[need:] == 0xFF).all(), "the rows kernel wrote past its workspace"
        for name, (buf, view) in b.items():
            assert not torch.isnan(view).any(), name
            if name in ("z", "dx", "dy"):
                rest = buf[:view.size(0) * ld].view(view.size(0), ld)[:, k:]
                assert torch.isnan(rest).all() and torch.isnan(buf[view.size(0) * ld:]).all(), name
            else:
                assert torch.isnan(buf[view.numel():]).all(), name
        runs.append({name: view.clone() for name, (_, view) in b.items()})
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name
    held(case, runs[0])


@pytest.mark.parametrize("heads,d,dtype", ((1, 46, BF), (8, 8, BF), (3, 128, FP), (8, 64, BF)))
def test_datt_null_gives_the_same_dx_and_d_bits(gpu, heads, d, dtype):
    case = c16.config_case(heads, d, dtype)
    with_datt, without = run_cabi(case, gpu), run_cabi(case, gpu, want_datt=False)
    assert without["datt"] is None and with_datt["datt"] is not None
    for name in ("dx", "D", "dy"):
        assert torch.equal(with_datt[name], without[name]), name


@pytest.mark.parametrize("heads,d", ((1, 10), (8, 8), (3, 128)))
def test_column_views_keep_their_pitch(gpu, heads, d):
    """x, y and g as the middle column block of a [N, 3 K] tensor whose neighbours hold NaN and Inf go in without a copy and give the
    bits of the packed operands -- an over-read column in a dot product, or Inf * 0, would show -- through the wrappers and the
    operator."""
    case = c16.config_case(heads, d)
    k = case.k
    packed = run_cabi(case, gpu)
    view = {}
    for name, a in (("x", case.x16), ("y", case.y16), ("g", case.g16)):
        t = torch.empty(case.m, 3 * k, device=gpu, dtype=case.dtype)
        t[:, :k] = float("nan")
        t[:, 2 * k:] = float("inf")
        t[:, k:2 * k] = dev(a, gpu)
        view[name] = t[:, k:2 * k]
        assert not view[name].is_contiguous() and view[name].stride(0) == 3 * k
    got = run_cabi(case, gpu, x=view["x"], y=view["y"], g=view["g"])
    for name in c16.OUTPUTS:
        assert torch.equal(got[name], packed[name]), name
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    xw, yw = view["x"]._base.clone().requires_grad_(True), view["y"]._base.clone().requires_grad_(True)
    att = dev(case.att, gpu).requires_grad_(True)
    z = torch.ops.isplib.gatv2_spmm16(rowptr, col, colptr, row_t, xw[:, k:2 * k], yw[:, k:2 * k], att, heads, case.ns)
    z.backward(view["g"])
    assert torch.equal(z.detach(), packed["z"]) and torch.equal(xw.grad[:, k:2 * k], packed["dx"])
    assert torch.equal(yw.grad[:, k:2 * k], packed["dy"]) and torch.equal(att.grad, packed["datt"])
    for w in (xw, yw):
        assert not w.grad[:, :k].any() and not w.grad[:, 2 * k:].any()


@pytest.mark.parametrize("heads,d", ((8, 8), (2, 256), (1, 46)))
def test_a_nan_in_y_poisons_exactly_its_head_of_the_rows_that_reference_it(gpu, heads, d):
    """Forward only: y[j, c] = NaN makes the head of c NaN in z and lse of the rows referencing j, and nothing else."""
    from isplib_amd import cabi
    case = c16.config_case(heads, d)
    j = int(case.col[case.rowptr[2]])                     # a column some rows reference
    hit = np.zeros(case.m, bool)
    hit[case.ref["row"][case.col == j]] = True
    assert hit.any() and (~hit & case.live).any()
    h = heads - 1
    y = case.y16.clone()
    y[j, h * d + d // 2] = float("nan")
    rowptr, col = dev_graph(case, gpu)
    z, lse = cabi.gatv2_16_forward(rowptr, col, dev(case.x16, gpu), dev(y, gpu), dev(case.att, gpu), heads, case.ns)
    z, lse = per_head(c16.as_array(z), heads), c16.as_array(lse)
    want, bound = per_head(case.ref["z"], heads), per_head(case.bound["z"], heads)
    assert np.all(np.isnan(z[hit, h])) and np.all(np.isnan(lse[hit, h]))
    clean = np.ones((case.m, heads), bool)
    clean[hit, h] = False
    frac = ref.worst(z[clean], want[clean], bound[clean])
    print(f"gatv2_16 error/bound nan in y, everything else h{heads}d{d}: z={frac:.4f}")
    assert frac <= 1.0
    ok = clean & case.live[:, None]
    assert ref.worst(lse[ok], case.ref["lse"][ok], case.bound["lse"][ok]) <= 1.0


def test_gradient_flags(gpu):
    """Only x, only y, only att, none: a gradient that is not asked for stays None, the others keep their bits."""
    case = c16.config_case(8, 8)
    z, x, y, att = run_op(case, gpu)
    z1, x1, y1, att1 = run_op(case, gpu, need=(True, False, False))
    assert y1.grad is None and att1.grad is None and torch.equal(x1.grad, x.grad) and torch.equal(z1, z)
    _, x2, y2, att2 = run_op(case, gpu, need=(False, True, False))
    assert x2.grad is None and att2.grad is None and torch.equal(y2.grad, y.grad)
    _, x3, y3, att3 = run_op(case, gpu, need=(False, False, True))
    assert x3.grad is None and y3.grad is None and torch.equal(att3.grad, att.grad)
    z4, x4, y4, att4 = run_op(case, gpu, need=(False, False, False))
    assert x4.grad is None and y4.grad is None and att4.grad is None and torch.equal(z4, z) and not z4.requires_grad


_shared = {}


def shared_case(heads, d, dtype):
    if (heads, d, dtype) not in _shared:
        base = c16.config_case(heads, d, dtype)
        _shared[heads, d, dtype] = c16.Case16(f"shared-h{heads}d{d}", base.rowptr, base.col, np.array(base.x), np.array(base.x),
                                              np.array(base.att), np.array(base.g), heads, base.ns, dtype)
    return _shared[heads, d, dtype]


@pytest.mark.parametrize("mode", ("native", "convert"))
@pytest.mark.parametrize("heads,d,dtype", ((1, 46, BF), (8, 16, FP)))
def test_y_none_shares_one_tensor(gpu, heads, d, dtype, mode, monkeypatch):
    """y=None (share_weights) on the square graph, both routes: the one tensor's gradient receives dx + dy -- each rounded once, then
    one add in the operands' dtype, so the summed bound carries one more unit roundoff of the sum."""
    import isplib_amd
    case = shared_case(heads, d, dtype)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.setenv("ISPLIB_HALF_GATV2", mode)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    x, att = dev(case.x16, gpu).requires_grad_(True), dev(case.att, gpu).requires_grad_(True)
    z = adj.gatv2_matmul(x, att, heads=heads, negative_slope=case.ns)
    z.backward(dev(case.g16, gpu))
    assert z.dtype == x.grad.dtype == dtype and att.grad.dtype == torch.float32
    if mode == "native":
        held(case, dict(z=z, datt=att.grad), ("z", "datt"), "gatv2_matmul")
        want = case.ref["dx"] + case.ref["dy"]
        bound = case.bound["dx"] + case.bound["dy"]
        bound = bound + half_ref.UNIT_ROUNDOFF[dtype] * (np.abs(want) + bound)
        frac = ref.worst(c16.as_array(x.grad), want, bound)
        print(f"gatv2_matmul error/bound {case.name}: dx+dy={frac:.4f}")
        assert frac <= 1.0
    else:
        xh, ah = dev(case.x16, gpu).requires_grad_(True), dev(case.att, gpu).requires_grad_(True)
        zh = adj.gatv2_matmul(xh.float(), ah, heads=heads, negative_slope=case.ns).to(dtype)
        zh.backward(dev(case.g16, gpu))
        assert torch.equal(z, zh) and torch.equal(x.grad, xh.grad) and torch.equal(att.grad, ah.grad)


_prefix = {}


def prefix_case(rows, heads, d):
    """The first `rows` rows of the graph (all columns kept): M at the block edges of the 8-row datt fold."""
    if (rows, heads, d) not in _prefix:
        base = c16.config_case(heads, d)
        rowptr = np.array(base.rowptr[:rows + 1])
        col = np.array(base.col[:rowptr[-1]])
        _prefix[rows, heads, d] = c16.Case16(f"first{rows}-h{heads}d{d}", rowptr, col, np.array(base.x[:rows]), np.array(base.y),
                                             np.array(base.att), np.array(base.g[:rows]), heads, base.ns, BF)
    return _prefix[rows, heads, d]


@pytest.mark.parametrize("rows", (1, 3, 7, 8, 9))
@pytest.mark.parametrize("heads,d", ((1, 46), (8, 64)))
def test_rows_that_meet_the_barrier_with_nothing_to_do(gpu, rows, heads, d):
    """M smaller than the rows kernel's block, one short of it, exactly it and one past it, with datt asked: the waves past M
    contribute zeros."""
    case = prefix_case(rows, heads, d)
    assert case.m == rows and case.n == c16.N
    got = run_cabi(case, gpu)
    held(case, got)
    again = run_cabi(case, gpu)
    assert torch.equal(got["datt"], again["datt"])


def test_refusals_return_the_documented_codes_in_order_and_leave_the_outputs_untouched(gpu):
    from isplib_amd import cabi
    L = cabi.lib()
    case = c16.config_case(2, 8)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    m, nnz = case.m, col.numel()
    wide = torch.zeros(m, 520, device=gpu, dtype=BF)
    outs = {name: torch.full((m, 520), float("nan"), device=gpu, dtype=BF) for name in ("z", "dx", "dy")}
    tabs = {name: torch.full((m, 64), float("nan"), device=gpu) for name in ("lse", "D")}
    datt = torch.full((520,), float("nan"), device=gpu)
    work = torch.full((cabi.gatv2_16_bw_rows_workspace_bytes(m, 512) + 256,), 0xFF, device=gpu, dtype=torch.uint8)
    t_in = torch.zeros(m, 64, device=gpu)
    att = torch.zeros(520, device=gpu)
    rp, cp = rowptr.data_ptr(), colptr.data_ptr()

    def call(code=cabi.DTYPE_BF16, mm=m, k=16, heads=2, ld=520, ldo=520, off=0, null=False, ws=None, ws_off=0):
        y, t = wide.data_ptr() + 2 * off, t_in.data_ptr()
        ws = work.numel() - 256 if ws is None else ws
        fw = L.isplib_gatv2_16_csr_hip(code, mm, m, k, nnz, col.data_ptr(), rp, rp + 8, y, min(ld, ldo), y, ld, None if null else att.data_ptr(),
                                       heads, 0.2, outs["z"].data_ptr(), ldo, tabs["lse"].data_ptr(), None)
        e_fw = cabi.last_error()
        rows = L.isplib_gatv2_16_bw_rows_hip(code, mm, m, k, nnz, col.data_ptr(), rp, rp + 8, y, min(ld, ldo), y, ld,
                                             None if null else att.data_ptr(), heads, 0.2, y, min(ld, ldo), t, outs["dx"].data_ptr(), ldo,
                                             tabs["D"].data_ptr(), datt.data_ptr(), work.data_ptr() + ws_off, ws, None)
        e_rows = cabi.last_error()
        cols = L.isplib_gatv2_16_bw_cols_hip(code, mm, m, k, nnz, row_t.data_ptr(), cp, cp + 8, y, ld, y, min(ld, ldo),
                                             None if null else att.data_ptr(), heads, 0.2, y, ld, t, t, outs["dy"].data_ptr(), ldo, None)
        return (fw, rows, cols), (e_fw, e_rows, cabi.last_error())

    F, N_, MEM = cabi.FAIL, cabi.NO_OPT_IMPL, cabi.NOT_ENOUGH_MEM
    # (what, arguments, the three codes, a word of every message): each row adds one fault to the right of the previous one's kind, so the
    # earlier refusal must win
    for what, kwargs, want, word in (
            ("the fp32 dtype code", dict(code=0), (F, F, F), "dtype"),
            ("dtype before a negative dimension", dict(code=0, mm=-1), (F, F, F), "dtype"),
            ("a negative dimension before a pitch below K", dict(mm=-1, ldo=14), (F, F, F), "negative"),
            ("a pitch below K before k % heads", dict(k=18, heads=4, ldo=16), (F, F, F), "leading dimension"),
            ("k % heads before the domain", dict(k=18, heads=4), (F, F, F), "multiple of heads"),
            ("odd K", dict(k=15, heads=1), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("K = 6", dict(k=6, heads=1), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("K = 514", dict(k=514, heads=1), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("d = 4", dict(k=16, heads=4), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("d = 12", dict(k=24, heads=2), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("heads = 0", dict(heads=0), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("odd pitch", dict(ld=519), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("odd output pitch", dict(ldo=519), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("the domain before a null operand", dict(k=16, heads=4, null=True), (N_, N_, N_), "isplib_gatv2_16_serves"),
            ("a null operand before the workspace", dict(null=True, ws=0), (F, F, F), "null"),
            ("a workspace too small before alignment", dict(ws=255, off=1), (F, MEM, F), None),
            ("an unaligned workspace before alignment", dict(ws_off=128, off=1), (F, F, F), None),
            ("a base offset by one element", dict(off=1), (F, F, F), "4-byte aligned")):
        codes, messages = call(**kwargs)
        assert codes == want, (what, codes, messages)
        if word is not None:
            assert all(word in msg for msg in messages), (what, messages)
    _, messages = call(ws=255, off=1)
    assert "workspace too small" in messages[1] and "4-byte aligned" in messages[0] and "4-byte aligned" in messages[2]
    _, messages = call(ws_off=128, off=1)
    assert "256-byte aligned" in messages[1]
    torch.cuda.synchronize()
    for t in list(outs.values()) + list(tabs.values()) + [datt]:
        assert torch.isnan(t).all()
    assert (work == 0xFF).all()
    # nothing to do comes before everything but dtype and a negative dimension: success without a launch, whatever else is wrong
    codes, _ = call(mm=0, ldo=14, null=True)
    assert codes[:2] == (cabi.SUCCESS, cabi.SUCCESS)
    codes, _ = call(k=0, heads=0, null=True)
    assert codes == (cabi.SUCCESS,) * 3
    x16, y16, a2 = wide[:, :16], wide[:, :16], att[:16].view(2, 8)
    for xx, yy, aa, heads in ((x16.float(), y16, a2, 2), (x16, y16.to(FP), a2, 2), (x16, y16, a2.to(BF), 2), (wide[:, :15], wide[:, :15], att[:15].view(1, 15), 1),
                              (x16, y16, att[:16].view(4, 4), 4), (x16[:-1], y16, a2, 2), (x16, y16, a2, 3)):
        with pytest.raises(RuntimeError, match="gatv2_spmm16"):
            torch.ops.isplib.gatv2_spmm16(rowptr, col, colptr, row_t, xx, yy, aa, heads, 0.2)
    torch.cuda.synchronize()
    assert torch.isnan(outs["z"]).all()


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
def test_plugin_routes(gpu, dtype, monkeypatch):
    """unset -> the existing TypeError; convert -> the bits of the hand-written conversion; native inside the domain -> the operator's
    bits, within the bound; native at K = 6, at odd K and at (H, d) = (2, 4) -> the conversion route's bits, nothing raised; auto
    follows native_pays; ISPLIB_HALF=convert wins; mixed dtypes -> TypeError; fp32 calls are unaffected by any setting."""
    import isplib_amd
    from isplib_amd import cabi
    case = c16.config_case(8, 8, dtype)
    rowptr, col = dev_graph(case, gpu)
    colptr, row_t = transposed(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    g = dev(case.g16, gpu)

    def leaves(k=None, heads=None):
        x, y, att = dev(case.x16, gpu), dev(case.y16, gpu), dev(case.att, gpu)
        if k is not None:
            x, y, att = x[:, :k].contiguous(), y[:, :k].contiguous(), att.reshape(-1)[:k].reshape(heads, k // heads).contiguous()
        return x.requires_grad_(True), y.requires_grad_(True), att.requires_grad_(True)

    def by_hand(x, y, att, gg, heads):
        z = isplib_amd.gatv2_matmul(adj, x.float(), att, y.float(), heads, case.ns).to(dtype)
        z.backward(gg)
        return z.detach(), x.grad, y.grad, att.grad

    def through(x, y, att, gg, heads):
        z = adj.gatv2_matmul(x, att, y, heads, case.ns)
        z.backward(gg)
        assert z.dtype == x.grad.dtype == y.grad.dtype == dtype and att.grad.dtype == torch.float32
        return z.detach(), x.grad, y.grad, att.grad

    def same(a, b):
        return all(torch.equal(u, v) for u, v in zip(a, b))

    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.delenv("ISPLIB_HALF_GATV2", raising=False)
    x0, y0, a0 = leaves()
    with pytest.raises(TypeError, match="float32"):
        isplib_amd.gatv2_matmul(adj, x0, a0, y0, 8, case.ns)
    want = by_hand(*leaves(), g, 8)
    fp32 = isplib_amd.gatv2_matmul(adj, x0.detach().float(), a0.detach(), y0.detach().float(), 8, case.ns)

    monkeypatch.setenv("ISPLIB_HALF_GATV2", "convert")
    assert same(through(*leaves(), g, 8), want)
    assert torch.equal(isplib_amd.gatv2_matmul(adj, x0.detach().float(), a0.detach(), y0.detach().float(), 8, case.ns), fp32)

    monkeypatch.setenv("ISPLIB_HALF_GATV2", "native")
    xd, yd, ad = leaves()
    zd = torch.ops.isplib.gatv2_spmm16(rowptr, col, colptr, row_t, xd, yd, ad, 8, case.ns)
    zd.backward(g)
    native = (zd.detach(), xd.grad, yd.grad, ad.grad)
    got = through(*leaves(), g, 8)
    assert same(got, native)
    held(case, dict(z=got[0], dx=got[1], dy=got[2], datt=got[3]), OP_OUTPUTS, "gatv2_matmul")
    assert torch.equal(isplib_amd.gatv2_matmul(adj, x0.detach().float(), a0.detach(), y0.detach().float(), 8, case.ns), fp32)
    other = FP if dtype == BF else BF
    with pytest.raises(TypeError, match="share one 16-bit dtype"):
        adj.gatv2_matmul(xd.detach(), ad.detach(), yd.detach().to(other), 8, case.ns)
    with pytest.raises(TypeError, match="share one 16-bit dtype"):
        adj.gatv2_matmul(xd.detach(), ad.detach(), yd.detach().float(), 8, case.ns)
    with pytest.raises(TypeError, match="`x`'s dtype"):
        adj.gatv2_matmul(xd.detach(), ad.detach().to(other), yd.detach(), 8, case.ns)
    with pytest.raises(TypeError, match="float32"):
        adj.gatv2_matmul(xd.detach().float(), ad.detach().to(dtype), yd.detach().float(), 8, case.ns)
    # native at K = 6, at odd K and at (H, d) = (2, 4): outside the 16-bit domain, the conversion route's bits, nothing raised
    for k, heads in ((6, 1), (29, 1), (8, 2)):
        gg = g[:, :k].contiguous()
        assert same(through(*leaves(k, heads), gg, heads), by_hand(*leaves(k, heads), gg, heads)), (k, heads)
    # ISPLIB_HALF=convert wins over native
    monkeypatch.setenv("ISPLIB_HALF", "convert")
    assert same(through(*leaves(), g, 8), want)
    monkeypatch.delenv("ISPLIB_HALF")
    # auto: whatever the measured rule says for this class, and whatever it could say
    monkeypatch.setenv("ISPLIB_HALF_GATV2", "auto")
    assert same(through(*leaves(), g, 8), native if cabi.gatv2_16_native_pays(case.n, case.k) else want)
    for pays in (True, False):
        with monkeypatch.context() as mp:
            mp.setattr(cabi, "gatv2_16_native_pays", lambda rows, ld, pays=pays: pays)
            assert same(through(*leaves(), g, 8), native if pays else want)


@pytest.mark.parametrize("dtype", c16.DTYPES, ids=c16.dtype_name)
def test_att_in_the_operand_dtype(gpu, dtype, monkeypatch):
    """A 16-bit att through gatv2_matmul gives the bits of the same call with att widened by hand; its gradient has att's dtype: the
    fp32 gradient rounded once by the cast."""
    import isplib_amd
    case = c16.config_case(8, 8, dtype)
    rowptr, col = dev_graph(case, gpu)
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (case.m, case.m))
    g = dev(case.g16, gpu)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    for mode in ("native", "convert"):
        monkeypatch.setenv("ISPLIB_HALF_GATV2", mode)
        x, y = dev(case.x16, gpu).requires_grad_(True), dev(case.y16, gpu).requires_grad_(True)
        att = dev(case.att, gpu).to(dtype).requires_grad_(True)
        z = adj.gatv2_matmul(x, att, y, 8, case.ns)
        z.backward(g)
        xh, yh = dev(case.x16, gpu).requires_grad_(True), dev(case.y16, gpu).requires_grad_(True)
        ah = att.detach().float().requires_grad_(True)
        zh = adj.gatv2_matmul(xh, ah, yh, 8, case.ns)
        zh.backward(g)
        assert att.grad.dtype == dtype and z.dtype == x.grad.dtype == y.grad.dtype == dtype
        assert torch.equal(z, zh) and torch.equal(x.grad, xh.grad) and torch.equal(y.grad, yh.grad), mode
        assert torch.equal(att.grad, ah.grad.to(dtype)), mode
