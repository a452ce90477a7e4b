"""Parity of the attention families where a gather offset passes 2 GiB.

Every attention kernel (attention.hip, attention16.hip, gat.hip with its EDGE and DROP forms, gat16.hip, gatv2.hip with DROP, gatv2_16.hip,
mha.hip with DROP, mha16.hip: a forward, a rows backward and a columns backward each) forms a gather offset as (unsigned)id * pitch_bytes,
sizes its buffer descriptor from ((rows - 1) * ld + k) * elem and loads through raw_buffer_load with that offset cast to int.  The domain
functions promise this up to DENSE_BYTES_MAX = 3.5 GiB; between 2 GiB and there bit 31 is set in all three places, and on the 200 x 200 and
233 x 67 graphs of every other attention test it never is.  A range check that takes the extent as signed, a sign-extended offset or a
pitch * id formed in int would pass all of them.

Here the 200-row cases of the families' own *_cases.py run with their wide operands as row-strided views at the LAST pitch the domain
admits (tests/pitched_cases.py: 4,697,620 floats or 9,395,240 16-bit elements), in buffers of exactly the extent such a view owns,
NaN everywhere between the rows: rows 115..199 lie past 2^31 bytes, the hub column (in-degree 1000) among them, the extent is within one
row of 3.5 GiB.  Two layouts per kernel form and configuration, so that a gather fault is told from a store fault and a test never holds
more than four such buffers (3.74 GB each):
  * the operands some entry GATHERS lie pitched (y, then x and g; gat: y, then g; mha: k and v, then q and g), the rest is contiguous;
  * the operands read by row and every wide OUTPUT lie pitched (x / q, then g and z, then y / k / v; z, dx / dq, dy / dk / dv), the
    gathered ones are contiguous.
Each asserts: every output bit for bit what the same wrappers give on contiguous copies (the kernels never take the pitch into
arithmetic); every output inside the family's own bound against the fp64 reference, by the family's own `held` (imported from its GPU
test file -- nothing here has a tolerance of its own; the largest error / bound per output is printed, DESIGN.md 4.6b-4.6m record them);
exact zeros and lse = -inf for empty rows and unreferenced columns; every element of an output written and, where the outputs lie pitched,
every element between the rows still NaN.  Then one configuration per form goes through torch.ops.isplib.* and the plug-in on pitched
leaves, and every entry refuses the next pitch.  tests/test_attention_address_host.py shows on the CPU that each case leaves its bound when
the rows past 2^31 bytes read as zero.
"""
import gc

import pytest
import torch

from tests import pitched_cases as pc
from tests import test_gpu_attention as t_att
from tests import test_gpu_attention16 as t_att16
from tests import test_gpu_gat as t_gat
from tests import test_gpu_gat16 as t_gat16
from tests import test_gpu_gat_dropout as t_gdrop
from tests import test_gpu_gat_edge as t_edge
from tests import test_gpu_gatv2 as t_v2
from tests import test_gpu_gatv2_16 as t_v216
from tests import test_gpu_gatv2_dropout as t_v2drop
from tests import test_gpu_mha as t_mha
from tests import test_gpu_mha16 as t_mha16
from tests import test_gpu_mha_dropout as t_mhadrop
from tests.test_gpu_attention_rect import dev, exact_edges

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAIRS = pc.all_configs()
MODULE = {"attention": t_att, "attention16": t_att16, "gat": t_gat, "gat_edge": t_edge, "gat_drop": t_gdrop, "gat_drop_edge": t_gdrop,
          "gat16": t_gat16, "gatv2": t_v2, "gatv2_drop": t_v2drop, "gatv2_16": t_v216, "mha": t_mha, "mha_drop": t_mhadrop, "mha16": t_mha16}
ROW_SIDE = {"attention": ("z", "dx", "D"), "gat": ("z", "dadst", "D"), "gatv2": ("z", "dx", "D"), "mha": ("z", "dq", "D")}
COL_SIDE = {"attention": ("dy",), "gat": ("dy", "dasrc"), "gatv2": ("dy",), "mha": ("dk", "dv")}


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def held(form, case, got, what=""):
    """The family's own bound, by the family's own helper: error / bound <= 1 for every output the family states a bound for."""
    mod = MODULE[form]
    if form == "attention":
        return mod.held(case, got, ("z", "lse", "dx", "dy"))                    # the fp32 family states no bound for D: held through dy
    if pc.elem_bytes(form) == 2:
        return mod.held(case, got)
    if form in ("gat_drop", "gat_drop_edge"):
        return mod.held(case, got, mod.names_of(case), what)
    return mod.held(case, got, mod.OUTPUTS if hasattr(mod, "OUTPUTS") else mod.CABI_OUTPUTS, what)


class Layout:
    """How the wide tensors of one run lie: `gathered` / `resident` put the operands some entry gathers / the operands read by row and
    the wide outputs at `pitch` (tests/pitched_cases.pitched: an exact buffer, NaN between the rows); everything else is contiguous.
    Every output starts as NaN, whatever its layout."""

    def __init__(self, gpu, pitch=None, gathered=False, resident=False):
        self.gpu, self.pitch, self.gathered, self.resident = gpu, pitch, gathered, resident

    def gather(self, t):
        return pc.pitched(t, self.pitch) if self.gathered else t

    def own(self, t):
        return pc.pitched(t, self.pitch) if self.resident else t

    def wide(self, rows, k, dtype):
        if self.resident:
            return pc.pitched_out(rows, k, self.pitch, dtype, self.gpu)
        return torch.full((rows, k), NAN, dtype=dtype, device=self.gpu)

    def table(self, *shape):
        return torch.full(shape, NAN, device=self.gpu)

    def keep(self, out):
        """An output after its launch: every element written, the buffer between the rows untouched; a packed copy of a pitched one."""
        if out.is_contiguous():
            assert not torch.isnan(out).any(), "an element of the output was not written"
            return out
        pc.pads_keep_nan(out)
        return out.contiguous()


def direct(fn, *args, **kwargs):
    return fn(*args, **kwargs)


def structure(form, case, gpu):
    mod = MODULE[form]
    rowptr, col = mod.dev_graph(case, gpu)
    tr = mod.transposed(case, gpu)
    return rowptr, col, tr[0], tr[1], (tr[2] if len(tr) > 2 else None)


def mask_of(form, case):
    return (case.threshold, case.scale, case.seed) if form.endswith("_drop") or form == "gat_drop_edge" else ()


def run_attention(form, case, gpu, lay, call=direct):
    from isplib_amd import cabi
    half = form == "attention16"
    rowptr, col, colptr, row_t, _ = structure(form, case, gpu)
    x, y, g = (dev(a, gpu) for a in ((case.x16, case.y16, case.g16) if half else (case.x, case.y, case.g)))
    (m, k), n, dt = x.shape, y.size(0), x.dtype
    fw, rows, cols = ((cabi.attention16, cabi.attention16_bw_rows, cabi.attention16_bw_cols) if half else
                      (cabi.attention, cabi.attention_bw_rows, cabi.attention_bw_cols))
    yg, xo = lay.gather(y), lay.own(x)
    z, lse = call(fw, rowptr, col, xo, yg, case.p, out=(lay.wide(m, k, dt), lay.table(m)))
    go = lay.own(g)
    dx, D = call(rows, rowptr, col, xo, yg, go, *(() if half else (z,)), lse, case.p, out=(lay.wide(m, k, dt), lay.table(m)))   # 16 bits: z is not read
    got = dict(z=lay.keep(z), lse=lay.keep(lse), dx=lay.keep(dx), D=lay.keep(D))
    del yg, xo, go, z, dx
    xg, gg, yo = lay.gather(x), lay.gather(g), lay.own(y)
    got["dy"] = lay.keep(call(cols, colptr, row_t, xg, yo, gg, lse, D, case.p, out=lay.wide(n, k, dt)))
    return got


def run_gat(form, case, gpu, lay, call=direct):
    from isplib_amd import cabi
    half, drop = form == "gat16", mask_of(form, case)
    rowptr, col, colptr, row_t, csr2csc = structure(form, case, gpu)
    y, g = (dev(a, gpu) for a in ((case.y16, case.g16) if half else (case.y, case.g)))
    a_dst, a_src = dev(case.a_dst, gpu), dev(case.a_src, gpu)
    a_edge = dev(case.a_edge, gpu) if getattr(case, "a_edge", None) is not None else None
    edge = a_edge is not None
    (m, k), n, dt, H, ns, nnz = g.shape, y.size(0), y.dtype, case.heads, case.ns, col.numel()
    yg = lay.gather(y)
    out = (lay.wide(m, k, dt), lay.table(m, H))
    if half:
        z, lse = call(cabi.gat16_forward, rowptr, col, yg, a_dst, a_src, H, ns, out=out)
    elif drop:
        z, lse = call(cabi.gat_drop, rowptr, col, yg, a_dst, a_src, a_edge, *drop, H, ns, out=out)
    elif edge:
        z, lse = call(cabi.gat_edge, rowptr, col, yg, a_dst, a_src, a_edge, H, ns, out=out)
    else:
        z, lse = call(cabi.gat, rowptr, col, yg, a_dst, a_src, H, ns, out=out)
    go = lay.own(g)
    out = (lay.table(m, H), lay.table(m, H))
    out3 = out + ((lay.table(nnz, H) if edge else None),)
    daedge = None
    if half:
        dadst, D = call(cabi.gat16_backward_rows, rowptr, col, yg, a_dst, a_src, go, lse, H, ns, out=out)                  # z is not read
    elif drop:
        dadst, D, daedge = call(cabi.gat_drop_bw_rows, rowptr, col, yg, a_dst, a_src, a_edge, go, z, lse, *drop, H, ns, out=out3)
    elif edge:
        dadst, D, daedge = call(cabi.gat_edge_bw_rows, rowptr, col, yg, a_dst, a_src, a_edge, go, z, lse, H, ns, out=out3)
    else:
        dadst, D = call(cabi.gat_bw_rows, rowptr, col, yg, a_dst, a_src, go, z, lse, H, ns, out=out)
    got = dict(z=lay.keep(z), lse=lay.keep(lse), dadst=lay.keep(dadst), D=lay.keep(D))
    if edge:
        got["daedge"] = lay.keep(daedge)
    del yg, go, z
    gg, yo = lay.gather(g), lay.own(y)
    out = (lay.wide(n, k, dt), lay.table(n, H))
    if half:
        dy, dasrc = call(cabi.gat16_backward_cols, colptr, row_t, yo, a_dst, a_src, gg, lse, D, H, ns, out=out)
    elif drop:
        dy, dasrc = call(cabi.gat_drop_bw_cols, colptr, row_t, csr2csc, yo, a_dst, a_src, a_edge, gg, lse, D, *drop, H, ns, out=out)
    elif edge:
        dy, dasrc = call(cabi.gat_edge_bw_cols, colptr, row_t, csr2csc, yo, a_dst, a_src, a_edge, gg, lse, D, H, ns, out=out)
    else:
        dy, dasrc = call(cabi.gat_bw_cols, colptr, row_t, yo, a_dst, a_src, gg, lse, D, H, ns, out=out)
    got.update(dy=lay.keep(dy), dasrc=lay.keep(dasrc))
    return got


def run_gatv2(form, case, gpu, lay, call=direct):
    from isplib_amd import cabi
    half, drop = form == "gatv2_16", mask_of(form, case)
    rowptr, col, colptr, row_t, csr2csc = structure(form, case, gpu)
    x, y, g = (dev(a, gpu) for a in ((case.x16, case.y16, case.g16) if half else (case.x, case.y, case.g)))
    att = dev(case.att, gpu)
    (m, k), n, dt, H, ns = x.shape, y.size(0), x.dtype, case.heads, case.ns
    yg, xo = lay.gather(y), lay.own(x)
    out = (lay.wide(m, k, dt), lay.table(m, H))
    if half:
        z, lse = call(cabi.gatv2_16_forward, rowptr, col, xo, yg, att, H, ns, out=out)
    elif drop:
        z, lse = call(cabi.gatv2_drop, rowptr, col, xo, yg, att, *drop, H, ns, out=out)
    else:
        z, lse = call(cabi.gatv2, rowptr, col, xo, yg, att, H, ns, out=out)
    go = lay.own(g)
    out = (lay.wide(m, k, dt), lay.table(m, H), lay.table(H, k // H))
    if half:
        dx, D, datt = call(cabi.gatv2_16_backward_rows, rowptr, col, xo, yg, att, go, lse, H, ns, out=out)                 # z is not read
    elif drop:
        dx, D, datt = call(cabi.gatv2_drop_bw_rows, rowptr, col, xo, yg, att, go, z, lse, *drop, H, ns, out=out)
    else:
        dx, D, datt = call(cabi.gatv2_bw_rows, rowptr, col, xo, yg, att, go, z, lse, H, ns, out=out)
    got = dict(z=lay.keep(z), lse=lay.keep(lse), dx=lay.keep(dx), D=lay.keep(D), datt=lay.keep(datt))
    del yg, xo, go, z, dx
    xg, gg, yo = lay.gather(x), lay.gather(g), lay.own(y)
    out = lay.wide(n, k, dt)
    if half:
        dy = call(cabi.gatv2_16_backward_cols, colptr, row_t, xg, yo, att, gg, lse, D, H, ns, out=out)
    elif drop:
        dy = call(cabi.gatv2_drop_bw_cols, colptr, row_t, csr2csc, xg, yo, att, gg, lse, D, *drop, H, ns, out=out)
    else:
        dy = call(cabi.gatv2_bw_cols, colptr, row_t, xg, yo, att, gg, lse, D, H, ns, out=out)
    got["dy"] = lay.keep(dy)
    return got


def run_mha(form, case, gpu, lay, call=direct):
    from isplib_amd import cabi
    half, drop = form == "mha16", mask_of(form, case)
    rowptr, col, colptr, row_t, csr2csc = structure(form, case, gpu)
    q, k, v, g = (dev(a, gpu) for a in ((case.q16, case.k16, case.v16, case.g16) if half else (case.q, case.k, case.v, case.g)))
    (m, w), n, dt, H, p = q.shape, k.size(0), q.dtype, case.heads, (case.ps if drop else case.p)
    kg, vg, qo = lay.gather(k), lay.gather(v), lay.own(q)
    out = (lay.wide(m, w, dt), lay.table(m, H))
    if half:
        z, lse = call(cabi.mha16_forward, rowptr, col, qo, kg, vg, H, p, out=out)
    elif drop:
        z, lse = call(cabi.mha_drop, rowptr, col, qo, kg, vg, *drop, H, p, out=out)
    else:
        z, lse = call(cabi.mha, rowptr, col, qo, kg, vg, H, p, out=out)
    go = lay.own(g)
    out = (lay.wide(m, w, dt), lay.table(m, H))
    if half:
        dq, D = call(cabi.mha16_backward_rows, rowptr, col, qo, kg, vg, go, lse, H, p, out=out)                            # z is not read
    elif drop:
        dq, D = call(cabi.mha_drop_bw_rows, rowptr, col, qo, kg, vg, go, z, lse, *drop, H, p, out=out)
    else:
        dq, D = call(cabi.mha_bw_rows, rowptr, col, qo, kg, vg, go, z, lse, H, p, out=out)
    got = dict(z=lay.keep(z), lse=lay.keep(lse), dq=lay.keep(dq), D=lay.keep(D))
    del kg, vg, qo, go, z, dq
    qg, gg, ko, vo = lay.gather(q), lay.gather(g), lay.own(k), lay.own(v)
    out = (lay.wide(n, w, dt), lay.wide(n, w, dt))
    if half:
        dk, dv = call(cabi.mha16_backward_cols, colptr, row_t, qg, ko, vo, gg, lse, D, H, p, out=out)
    elif drop:
        dk, dv = call(cabi.mha_drop_bw_cols, colptr, row_t, csr2csc, qg, ko, vo, gg, lse, D, *drop, H, p, out=out)
    else:
        dk, dv = call(cabi.mha_bw_cols, colptr, row_t, qg, ko, vo, gg, lse, D, H, p, out=out)
    got.update(dk=lay.keep(dk), dv=lay.keep(dv))
    return got


RUN = {"attention": run_attention, "gat": run_gat, "gatv2": run_gatv2, "mha": run_mha}


def run(form, case, gpu, lay, call=direct):
    """Forward, then rows backward, then columns backward through the C ABI wrappers, as the family's run_cabi does."""
    return RUN[pc.kind_of(form)](form, case, gpu, lay, call)


_packed = {}


def packed_run(form, config, gpu):
    """The same wrappers on contiguous copies of the same operands: once per case, shared, never written."""
    if (form, config) not in _packed:
        _packed[(form, config)] = run(form, pc.case_of(form, config), gpu, Layout(gpu))
    return _packed[(form, config)]


def same_bits(name, a, b):
    ints = {4: torch.int32, 2: torch.int16}[a.element_size()]
    assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert not torch.isnan(a).any() and torch.equal(a.view(ints), b.view(ints)), f"{name}: not the bits of the contiguous run"


def at_the_limit(form, config):
    case, elem = pc.case_of(form, config), pc.elem_bytes(form)
    pitch = pc.limit_pitch(pc.ROWS, elem)
    far = pc.assert_reaches(case, pitch, elem)
    assert far == 115 and (pc.ROWS - 1) * pitch * elem > pc.FAR
    return case, pitch


def check(form, config, case, got, gpu, what):
    want = packed_run(form, config, gpu)
    assert set(got) == set(want)
    for name in want:
        same_bits(name, got[name], want[name])
    held(form, case, got, what)
    kind = pc.kind_of(form)
    exact_edges(case, pc.ROWS, got, ROW_SIDE[kind], COL_SIDE[kind])


@pytest.mark.parametrize("form,config", PAIRS, ids=pc.ids(PAIRS))
def test_gathered_operands_at_the_limit_pitch(gpu, form, config):
    """Every operand some entry gathers lies at the last pitch the domain admits: y in the forward and the rows backward, x and g in the
    columns backward (gat: y, then g; mha: k and v, then q and g); the other operands and the outputs are contiguous.  Rows 115..199 of
    each are gathered from past 2^31 bytes.  Peak device memory: two buffers of 3.74 GB."""
    case, pitch = at_the_limit(form, config)
    got = run(form, case, gpu, Layout(gpu, pitch, gathered=True))
    check(form, config, case, got, gpu, " gathered at the limit")


@pytest.mark.parametrize("form,config", PAIRS, ids=pc.ids(PAIRS))
def test_row_resident_operands_and_outputs_at_the_limit_pitch(gpu, form, config):
    """The operands read by row (x / q in the forward, g and z in the rows backward, y / k / v in the columns backward) and every wide
    output (z, dx / dq, dy / dk / dv) lie at the last pitch the domain admits, the outputs in NaN-filled buffers: rows 115..199 are read
    and stored past 2^31 bytes, every element of a view is written and nothing between the rows.  The gathered operands are contiguous.
    Peak device memory: four buffers of 3.74 GB (x, g, z and dx in the rows backward; mha: k, v, dk and dv in the columns backward)."""
    case, pitch = at_the_limit(form, config)
    got = run(form, case, gpu, Layout(gpu, pitch, resident=True))
    check(form, config, case, got, gpu, " stored at the limit")


# ---- the layers above: torch.ops.isplib.* under autograd and the plug-in, on the pitched views themselves as leaves ------------------------

def leaf(view):
    """The view itself as a leaf: it keeps its pitch and its buffer, and its gradient is a packed [rows, k] tensor."""
    out = view.detach().requires_grad_()
    assert out.stride() == view.stride() and out.data_ptr() == view.data_ptr()
    return out


def adjacency(form, case, gpu):
    import isplib_amd
    rowptr, col = MODULE[form].dev_graph(case, gpu)
    return isplib_amd.SparseTensor.from_csr(rowptr, col, None, (pc.ROWS, pc.ROWS))


def layers(form, case, gpu, wide, fresh):
    """-> [(name, outputs)] of the operator and of the plug-in method on the wide operands `wide` (name -> tensor; `fresh` makes the leaf
    of one); outputs: z and every gradient, named as the C ABI wrappers name them."""
    import isplib_amd
    ops, kind, half = torch.ops.isplib, pc.kind_of(form), pc.elem_bytes(form) == 2
    rowptr, col, colptr, row_t, csr2csc = structure(form, case, gpu)
    adj, g, H = adjacency(form, case, gpu), wide["g"], getattr(case, "heads", None)
    drop = dict(dropout=case.p, training=True, seed=case.seed) if mask_of(form, case) else {}
    runs = []
    for layer in ("operator", "plug-in"):
        op = layer == "operator"
        if kind == "attention":
            x, y = fresh(wide["x"]), fresh(wide["y"])
            z = (ops.attention_spmm16 if half else ops.attention_spmm)(rowptr, col, colptr, row_t, x, y, case.p) if op else \
                isplib_amd.attention_matmul(adj, x, y, case.p)
            grads = dict(dx=x, dy=y)
        elif kind == "gat":
            y, a_dst, a_src = fresh(wide["y"]), fresh(dev(case.a_dst, gpu)), fresh(dev(case.a_src, gpu))
            a_edge = fresh(dev(case.a_edge, gpu)) if getattr(case, "a_edge", None) is not None else None
            if not op:
                z = isplib_amd.gat_matmul(adj, y, a_dst, a_src, heads=H, negative_slope=case.ns, a_edge=a_edge, **drop)
            elif half:
                z = ops.gat_spmm16(rowptr, col, colptr, row_t, y, a_dst, a_src, H, case.ns)
            elif drop:
                z = ops.gat_drop_spmm(rowptr, col, colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, H, case.ns, case.p, case.seed)
            elif a_edge is not None:
                z = ops.gat_edge_spmm(rowptr, col, colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, H, case.ns)
            else:
                z = ops.gat_spmm(rowptr, col, colptr, row_t, y, a_dst, a_src, H, case.ns)
            grads = dict(dy=y, dadst=a_dst, dasrc=a_src, **(dict(daedge=a_edge) if a_edge is not None else {}))
        elif kind == "gatv2":
            x, y, att = fresh(wide["x"]), fresh(wide["y"]), fresh(dev(case.att, gpu))
            if not op:
                z = isplib_amd.gatv2_matmul(adj, x, att, y, heads=H, negative_slope=case.ns, **drop)
            elif half:
                z = ops.gatv2_spmm16(rowptr, col, colptr, row_t, x, y, att, H, case.ns)
            elif drop:
                z = ops.gatv2_drop_spmm(rowptr, col, colptr, row_t, csr2csc, x, y, att, H, case.ns, case.p, case.seed)
            else:
                z = ops.gatv2_spmm(rowptr, col, colptr, row_t, x, y, att, H, case.ns)
            grads = dict(dx=x, dy=y, datt=att)
        else:
            q, k, v = fresh(wide["q"]), fresh(wide["k"]), fresh(wide["v"])
            p = case.ps if drop else case.p
            if not op:
                z = isplib_amd.mha_matmul(adj, q, k, v, heads=H, scale=p, **drop)
            elif half:
                z = ops.mha_spmm16(rowptr, col, colptr, row_t, q, k, v, H, p)
            elif drop:
                z = ops.mha_drop_spmm(rowptr, col, colptr, row_t, csr2csc, q, k, v, H, p, case.p, case.seed)
            else:
                z = ops.mha_spmm(rowptr, col, colptr, row_t, q, k, v, H, p)
            grads = dict(dq=q, dk=k, dv=v)
        z.backward(g)
        for name, t in grads.items():
            assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == t.dtype, (layer, name)
        runs.append((layer, dict(z=z.detach(), **{name: t.grad for name, t in grads.items()})))
    return runs


WIDE = {"attention": ("x", "y", "g"), "gat": ("y", "g"), "gatv2": ("x", "y", "g"), "mha": ("q", "k", "v", "g")}


def wide_operands(form, case, gpu):
    half = pc.elem_bytes(form) == 2
    return {name: dev(getattr(case, name + "16" if half else name), gpu) for name in WIDE[pc.kind_of(form)]}


def layers_give_the_wrappers_bits(form, config, case, gpu, wide, what):
    want = packed_run(form, config, gpu)
    for layer, got in layers(form, case, gpu, wide, leaf):
        for name, t in got.items():
            assert tuple(t.shape) == tuple(want[name].shape), (layer, name)
            same_bits(f"{layer} {name} {what}", t, want[name])
        held(form, case, dict(want, **got), f" {layer} {what}")


FP32_FORMS = tuple(form for form in pc.CONFIGS if pc.elem_bytes(form) == 4)
HALF_FORMS = tuple(form for form in pc.CONFIGS if pc.elem_bytes(form) == 2)
HALF_SWITCH = {"attention16": "ISPLIB_HALF_ATTENTION", "gat16": "ISPLIB_HALF_GAT", "gatv2_16": "ISPLIB_HALF_GATV2", "mha16": "ISPLIB_HALF_MHA"}


@pytest.mark.parametrize("form", FP32_FORMS)
def test_fp32_operators_and_plugin_on_leaves_at_the_limit_pitch(gpu, form):
    """torch.ops.isplib.*_spmm under autograd and attention_matmul / gat_matmul / gatv2_matmul / mha_matmul with EVERY wide operand and the
    incoming gradient as views at the last pitch the domain admits, the views themselves the leaves: the output and every gradient are
    the bits of the C ABI wrappers on contiguous copies, and each gradient has its operand's shape.  Peak device memory: four buffers of
    3.74 GB (mha: q, k, v and g)."""
    config = pc.LAYER_CONFIG[form]
    case, pitch = at_the_limit(form, config)
    wide = {name: pc.pitched(t, pitch) for name, t in wide_operands(form, case, gpu).items()}
    layers_give_the_wrappers_bits(form, config, case, gpu, wide, "at the limit")


@pytest.mark.parametrize("form", HALF_FORMS)
def test_16_bit_operators_take_the_limit_pitch_as_it_lies_and_pack_the_next(gpu, form, monkeypatch):
    """torch.ops.isplib.*_spmm16 and the plug-in's native route (the family's ISPLIB_HALF_* switch set to native): at the last pitch the
    domain admits the views go in as they lie; at the next even pitch the operator packs them (tests/test_*16_host.py: too wide a pitch is
    packed).  Both give the bits of the C ABI wrappers on contiguous copies.  Peak device memory: four buffers of 3.74 GB."""
    from isplib_amd import cabi
    config = pc.LAYER_CONFIG[form]
    case, pitch = at_the_limit(form, config)
    monkeypatch.delenv("ISPLIB_HALF", raising=False)
    monkeypatch.setenv(HALF_SWITCH[form], "native")
    serves = getattr(cabi, f"{form}_serves")
    k = case.g16.size(1)
    shape = (k,) if form == "attention16" else (case.heads, k // case.heads)
    assert serves(pc.ROWS, *shape, pitch) and not serves(pc.ROWS, *shape, pitch + 2) and serves(pc.ROWS, *shape, k)
    for ld, what in ((pitch, "at the limit"), (pitch + 2, "one pitch past the limit, packed")):
        wide = {name: pc.pitched(t, ld) for name, t in wide_operands(form, case, gpu).items()}
        layers_give_the_wrappers_bits(form, config, case, gpu, wide, what)
        del wide


# ---- the entries themselves, one pitch past the limit ---------------------------------------------------------------------------------

@pytest.mark.parametrize("form", tuple(pc.CONFIGS))
def test_every_entry_refuses_the_next_pitch_before_a_launch(gpu, form, monkeypatch):
    """isplib_*_csr_hip, *_bw_rows_hip and *_bw_cols_hip of every form with a gathered operand declared at the first pitch past the
    limit: ISPLIB_NO_OPT_IMPL from the entry's own domain check, and after a synchronize every NaN-poisoned output is untouched.  No large
    buffer: the operands are the packed 200-row ones and only the pitch handed to the entry is false -- the wrappers' own refusal (a
    ValueError from cabi.*_serves, asserted first) is taken out of the way, so the call reaches the entry with the wrappers' marshalling.
    The families' own error-path tests cover the width, head and pitch-below-k refusals, none of them the byte limit of a wide operand."""
    from isplib_amd import cabi
    config = pc.LAYER_CONFIG[form]
    case, elem = pc.case_of(form, config), pc.elem_bytes(form)
    past = pc.limit_pitch(pc.ROWS, elem) + (1 if elem == 4 else 2)
    declared, outputs, refused = [], [], []
    dense = "_attn_dense" if elem == 4 else "_attn16_dense"
    real = getattr(cabi, dense)

    def false_pitch(t, *rest, **kw):
        ld = real(t, *rest, **kw)
        return past if any(t is d for d in declared) else ld

    class Declaring(Layout):
        def gather(self, t):
            declared.append(t[:])                                                # an alias: the same tensor read by row keeps its true pitch
            return declared[-1]

        def wide(self, rows, k, dtype):
            outputs.append(super().wide(rows, k, dtype))
            return outputs[-1]

        def table(self, *shape):
            outputs.append(super().table(*shape))
            return outputs[-1]

        def keep(self, out):
            return out

    def refusing(fn, *args, **kwargs):
        with monkeypatch.context() as mp:
            mp.setattr(cabi, dense, false_pitch)
            with pytest.raises(ValueError, match="domain"):                      # the wrapper's own check, on the Python *_serves
                fn(*args, **kwargs)
            for name in ("attention_serves", "gat_serves", "attention16_serves", "gat16_serves"):
                mp.setattr(cabi, name, lambda *a: True)
            with pytest.raises(cabi.IsplibError) as e:
                fn(*args, **kwargs)
        assert e.value.status == cabi.NO_OPT_IMPL and "_serves" in str(e.value), (fn.__name__, str(e.value))
        refused.append(fn.__name__)
        return kwargs["out"]                                                     # still poisoned: the next entry is refused on them too

    run(form, case, gpu, Declaring(gpu), refusing)
    torch.cuda.synchronize()
    assert len(refused) == 3 and len(set(refused)) == 3, refused
    assert outputs and all(torch.isnan(t).all() for t in outputs if t is not None)
