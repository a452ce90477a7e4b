"""The attention families past 2 GiB, host side (no GPU): the arithmetic of tests/pitched_cases.py, the conditions on the shared graph
that tests/test_gpu_attention_address_edges.py relies on, and that every case used there can SEE the fault those tests are there to catch.

The fault.  A range check that treats the descriptor's extent as signed, or an extent clipped to 2^31, answers 0 for every gather at or
past 2^31 bytes: the gathered rows >= first_far_row read as zero, the rows below are untouched.  Emulated in the families' own fp64
references by zeroing those rows of the operand:
  * forward and rows backward: the gathered operand is y (k and v for mha).  The reference is evaluated with its far rows zeroed; z and
    the rows-side gradients are compared.
  * columns backward: the gathered operands are x and g (g alone for gat; q and g for mha), read from correct lse and D tables.  The
    reference is evaluated with their far rows zeroed (z, lse and D of those rows change with them, which the kernel's tables would not).
    For attention, gat's dy and mha every term of a column's sum carries a factor g_i or x_i / q_i of the gathered row, so an entry of
    a far row adds exactly 0 either way and the emulation is exact; gatv2's dy keeps a garbage part ds_e att sl of such entries on the
    device that the emulation drops -- it shows the loss of the a_e g_i part alone.
Every case must leave its own bound (error / bound > 1) in z, in a rows-backward output and in a columns-backward output.
"""
import numpy as np
import pytest
import torch

from tests import attention_ref
from tests import gat_dropout_ref
from tests import gat_edge_ref
from tests import gat_ref
from tests import gatv2_dropout_ref
from tests import gatv2_ref
from tests import mha_dropout_ref
from tests import mha_ref
from tests import pitched_cases as pc

worst = attention_ref.worst
PAIRS = pc.all_configs()


@pytest.mark.parametrize("elem", (4, 2))
def test_the_limit_pitch_is_the_last_one_served_and_sets_bit_31(elem):
    from isplib_amd import cabi
    rows = pc.ROWS
    assert rows == 200 and cabi.DENSE_BYTES_MAX == 7 * 2 ** 29
    pitch = pc.limit_pitch(rows, elem)                    # asserts: served by every family, the next pitch by none
    assert pitch == {4: 4_697_620, 2: 9_395_240}[elem] and (elem == 4 or pitch % 2 == 0)
    assert rows * pitch * elem <= cabi.DENSE_BYTES_MAX < rows * (pitch + (1 if elem == 4 else 2)) * elem
    assert pitch * elem < 2 ** 32                          # the kernels' pitch in bytes is an unsigned 32-bit register
    for k in (1, 8, 47, 512):
        nbytes = pc.extent(rows, k, pitch) * elem
        assert nbytes & (1 << 31) and nbytes <= cabi.DENSE_BYTES_MAX < 2 ** 32 and nbytes > 3.7e9, (k, nbytes)
        assert cabi.DENSE_BYTES_MAX - nbytes < (pitch + 2 * rows) * elem          # within one row (and the division's remainder) of the limit
        assert (rows - 1) * pitch * elem + k * elem <= cabi.DENSE_OOB_OFFSET     # the last byte gathered lies below the poison offset
    far = pc.first_far_row(pitch, elem)
    assert far == 115 and (far - 1) * pitch * elem < pc.FAR <= far * pitch * elem
    assert pc.first_far_row(1 << 20, 4) == 512 and pc.first_far_row((1 << 20) + 1, 4) == 512 and pc.first_far_row((1 << 20) - 1, 4) == 513


def test_pitched_owns_exactly_its_extent_and_traps_the_pads():
    t = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    view = pc.pitched(t, 7)
    buf = pc.buffer_of(view)
    assert buf.numel() == 2 * 7 + 4 == pc.extent(3, 4, 7) and view.stride() == (7, 1) and torch.equal(view, t)
    assert view.data_ptr() == buf.data_ptr() and int(torch.isnan(buf).sum()) == buf.numel() - 12
    pc.pads_keep_nan(view)
    leaf = view.detach().requires_grad_()
    assert leaf.stride() == (7, 1) and leaf.data_ptr() == buf.data_ptr()                 # a leaf keeps the pitch and the buffer
    buf[5] = 0.0                                                                         # one element between the rows
    with pytest.raises(AssertionError, match="between the rows"):
        pc.pads_keep_nan(view)
    out = pc.pitched_out(3, 4, 7, torch.bfloat16, "cpu")
    assert out.dtype == torch.bfloat16 and torch.isnan(pc.buffer_of(out)).all()
    with pytest.raises(AssertionError, match="not written"):
        pc.pads_keep_nan(out)


def test_the_configurations_are_the_families_own():
    from tests import gat_dropout_cases, rect_cases
    assert pc.WIDTH_CONFIGS == ((8, 4), (1, 47), (4, 32), (8, 32), (1, 512)) == gat_dropout_cases.WIDTH_CONFIGS
    assert pc.ATTENTION_WIDTHS == (3, 33, 128, 257, 512) and pc.GAT16_SPECS is rect_cases.GAT16_SPECS
    assert {k for k, _ in pc.ATTENTION16_SPECS} == set(rect_cases.ATTENTION16_WIDTHS)
    assert len(pc.CONFIGS) == 13 and len(PAIRS) == 5 + 8 + 5 + 3 + 3 + 3 + 5 + 5 + 3 + 5 + 5 + 3 + 5
    assert set(pc.LAYER_CONFIG) == set(pc.CONFIGS) and all(config[:2] in ((128,), (128, pc.BF), (8, 8)) for config in pc.LAYER_CONFIG.values())


@pytest.mark.parametrize("form,config", PAIRS, ids=pc.ids(PAIRS))
def test_the_graph_of_every_case_reaches_both_sides_of_2_gib(form, config):
    case = pc.case_of(form, config)
    elem = pc.elem_bytes(form)
    assert case.rowptr.size - 1 == pc.ROWS
    far = pc.assert_reaches(case, pc.limit_pitch(pc.ROWS, elem), elem)
    assert far == 115
    assert (~case.live).any() and (np.bincount(case.col, minlength=pc.ROWS) == 0).any()   # the exact zeros the GPU tests assert exist


def zero_far(a, far):
    out = np.array(a)
    out[far:] = 0
    return out


def faulty(form, case, far):
    """-> (rows_side, cols_side): the family's reference with the operand(s) gathered by the forward and the rows backward zeroed from
    row `far` on, and with the operand(s) gathered by the columns backward zeroed."""
    kind, rp, cl, g = pc.kind_of(form), case.rowptr, case.col, case.g
    z = lambda a: zero_far(a, far)                                                       # noqa: E731
    if kind == "attention":
        return (attention_ref.attention(rp, cl, case.x, z(case.y), case.p, g), attention_ref.attention(rp, cl, z(case.x), case.y, case.p, z(g)))
    if kind == "gat":
        a_edge = getattr(case, "a_edge", None)
        if form.startswith("gat_drop"):
            run = lambda y, gg: gat_dropout_ref.gat_drop(rp, cl, y, case.a_dst, case.a_src, a_edge, case.heads, case.ns, case.p, case.seed, gg)  # noqa: E731
        elif a_edge is not None:
            run = lambda y, gg: gat_edge_ref.gat_edge(rp, cl, y, case.a_dst, case.a_src, a_edge, case.heads, case.ns, gg)   # noqa: E731
        else:
            run = lambda y, gg: gat_ref.gat(rp, cl, y, case.a_dst, case.a_src, case.heads, case.ns, gg)                   # noqa: E731
        return run(z(case.y), g), run(case.y, z(g))
    if kind == "gatv2":
        if form == "gatv2_drop":
            run = lambda x, y, gg: gatv2_dropout_ref.gatv2_drop(rp, cl, x, y, case.att, case.heads, case.ns, case.p, case.seed, gg)   # noqa: E731
        else:
            run = lambda x, y, gg: gatv2_ref.gatv2(rp, cl, x, y, case.att, case.heads, case.ns, gg)                        # noqa: E731
        return run(case.x, z(case.y), g), run(z(case.x), case.y, z(g))
    assert kind == "mha"
    if form == "mha_drop":
        run = lambda q, k, v, gg: mha_dropout_ref.mha_drop(rp, cl, q, k, v, case.heads, case.ps, case.p, case.seed, gg)    # noqa: E731
    else:
        run = lambda q, k, v, gg: mha_ref.mha(rp, cl, q, k, v, case.heads, case.p, gg)                                      # noqa: E731
    return run(case.q, z(case.k), z(case.v), g), run(z(case.q), case.k, case.v, z(g))


SEEN = {"attention": (("z", "dx"), ("dy",)), "gat": (("z", "dadst"), ("dy",)), "gatv2": (("z", "dx"), ("dy",)),
        "mha": (("z", "dq"), ("dk", "dv"))}


@pytest.mark.parametrize("form,config", PAIRS, ids=pc.ids(PAIRS))
def test_every_case_leaves_its_bound_when_the_far_rows_read_as_zero(form, config):
    case = pc.case_of(form, config)
    far = pc.first_far_row(pc.limit_pitch(pc.ROWS, pc.elem_bytes(form)), pc.elem_bytes(form))
    rows_side, cols_side = faulty(form, case, far)
    rows_names, cols_names = SEEN[pc.kind_of(form)]
    frac = {name: worst(rows_side[name], case.ref[name], case.bound[name]) for name in rows_names}
    frac.update({name: worst(cols_side[name], case.ref[name], case.bound[name]) for name in cols_names})
    print(f"far rows read as zero, {form} {case.name}: " + " ".join(f"{k}={v:.3g}" for k, v in frac.items()))
    assert all(v > 1.0 for v in frac.values()), (form, case.name, frac)
    # the rows below far keep their forward bit for bit in the first emulation, the rows that gather nothing past far too
    untouched = np.array([not (case.col[case.rowptr[i]:case.rowptr[i + 1]] >= far).any() for i in range(pc.ROWS)])
    assert untouched[:pc.ROWS // 2].all() and np.array_equal(rows_side["z"][untouched], case.ref["z"][untouched])
