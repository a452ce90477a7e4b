"""Rectangular attention cases, host side (no GPU): the two graphs of tests/rect_cases.py have the properties the GPU tests rely on,
every case stays inside the first-order range of its bound, every case can SEE an m / n mix-up in a gathered operand's extent (a clipped
buffer descriptor, emulated in the fp64 reference, leaves the case's own bound), and the 16-bit route functions answer per operand with
that operand's own row count.

The clipping emulation.  A buffer descriptor that is too short answers 0 for the rows past its extent.
  * wide (M < N), forward and rows kernel: `y` (and `a_src`) sized by M.  The reference is evaluated with the rows >= M of those operands
    set to 0; z, lse and the rows-side gradients are recomputed.
  * tall (M > N), columns kernel: the M-row operands (`x`, `g`, `a_dst`, `lse`, `D`) sized by N.  With those read as 0 an edge (i, j) with
    i >= N has t_e = 0 and D_i = 0, so ds_e = a_e (t_e - D_i) = 0 with a finite a_e, and its term a_e g_i is 0 too: it contributes exactly
    nothing to dy (and dasrc).  The emulation is therefore the reference evaluated on the structure with the rows >= N emptied -- the
    rows < N keep every entry, so their lse, D and per-edge parts are unchanged.
The opposite slip, a descriptor that is too long, reads a neighbour's memory and has no CPU emulation; the GPU parity tests cover it.
"""
import numpy as np
import pytest
import torch

from tests import attention_ref
from tests import gat_ref
from tests import gatv2_ref
from tests import rect_cases as rc

BF, FP = torch.bfloat16, torch.float16
worst = attention_ref.worst


@pytest.mark.parametrize("shape", rc.SHAPES)
def test_the_graphs_meet_every_loop_edge_on_both_sides(shape):
    m, n = rc.SHAPES[shape]
    rowptr, col = rc.graph(shape)
    assert rowptr.dtype == col.dtype == np.int64 and rowptr.size == m + 1 and rowptr[0] == 0 and rowptr[-1] == col.size == 2720
    assert col.min() >= 0 and col.max() == n - 1
    deg, indeg = np.diff(rowptr), np.bincount(col, minlength=n)
    want = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129, 1000)
    assert rc.ROW_LENGTHS == want
    assert tuple(deg[:rc.BLOCK]) == want and tuple(indeg[n - rc.BLOCK:]) == want          # a block of rows, a disjoint block of columns
    assert col[:rowptr[rc.BLOCK]].max() < n - rc.BLOCK                                    # the row block never enters the column block
    row = attention_ref.edge_rows(rowptr)
    assert row[col >= n - rc.BLOCK].min() >= rc.BLOCK
    assert deg[0] == 0 and indeg[n - rc.BLOCK] == 0                                       # an empty row, a column nothing points at
    assert deg[m - 1] > 0 and indeg[n - 1] > 0                                            # the highest index of each side is gathered
    assert any(np.unique(col[rowptr[i]:rowptr[i + 1]]).size < deg[i] for i in range(m))
    assert any(np.any(np.diff(col[rowptr[i]:rowptr[i + 1]]) < 0) for i in range(m))
    assert m % 2 == 1 and n % 2 == 1 and all(m % w and n % w for w in (2, 4, 8, 16))
    if shape == "tall":
        assert m > n and (row >= n).sum() > 100            # what a columns-kernel extent taken from n would clip
    else:
        assert m < n and (col >= m).sum() > 100            # what a forward extent taken from m would clip


def test_every_case_is_inside_the_first_order_range():
    cases = rc.all_cases()
    assert len(cases) == 2 * (4 + 8 + 4 + 4 + 5 + 5)
    for case in cases:
        top = float(case.bound["rho"].max())
        assert top <= rc.RHO_MAX, (case.name, top)
        m, n = rc.SHAPES[case.name.split("-")[0]]
        assert case.rowptr.size == m + 1 and case.y.shape[0] == n and case.g.shape[0] == m
    print("largest rho over the rectangular cases:", max(float(c.bound["rho"].max()) for c in cases))


def fraction(case, got, name):
    """error / bound of one output against the case's own reference; lse over the rows that have entries."""
    if name == "lse":
        live = case.live
        return worst(np.asarray(got["lse"])[live], case.ref["lse"][live], case.bound["lse"][live])
    return worst(got[name], case.ref[name], case.bound[name])


def leaves_the_bound(case, got, names):
    frac = {name: fraction(case, got, name) for name in names}
    print(f"clipped {case.name}: " + " ".join(f"{k}={v:.3g}" for k, v in frac.items()))
    assert all(v > 1.0 for v in frac.values()), (case.name, frac)


def clip_rows(a, rows):
    out = np.array(a)
    out[rows:] = 0
    return out


def rows_emptied(case, rows):
    """The structure with the rows >= `rows` emptied (see the module docstring: what the columns kernel computes when its M-row
    operands are clipped to `rows` rows)."""
    rowptr = np.array(case.rowptr)
    rowptr[rows:] = rowptr[rows]
    return rowptr, np.array(case.col[:rowptr[rows]])


def unclipped_passes(case, got, names):
    assert all(fraction(case, got, name) <= 1e-6 for name in names), case.name


ATTENTION = dict(attention=lambda s: rc.attention_case(s, 33), attention16_bf16=lambda s: rc.attention16_case(s, 34, BF),
                 attention16_fp16=lambda s: rc.attention16_case(s, 34, FP))
GAT = dict(gat=lambda s: rc.gat_case(s, 8, 8), gat16_bf16=lambda s: rc.gat16_case(s, 8, 8, BF), gat16_fp16=lambda s: rc.gat16_case(s, 8, 8, FP))
GATV2 = dict(gatv2=lambda s: rc.gatv2_case(s, 8, 8), gatv2_16_bf16=lambda s: rc.gatv2_16_case(s, 8, 8, BF),
             gatv2_16_fp16=lambda s: rc.gatv2_16_case(s, 8, 8, FP))


def rows_below_are_untouched(case, got, rows):
    """The rows the clipped descriptor still serves keep their lse and D bit for bit: only the clipped rows' edges went."""
    assert np.array_equal(got["lse"][:rows], case.ref["lse"][:rows]) and np.array_equal(got["D"][:rows], case.ref["D"][:rows])


@pytest.mark.parametrize("family", ATTENTION)
def test_attention_wide_sees_y_clipped_to_m_rows(family):
    case = ATTENTION[family]("wide")
    m = case.m
    assert case.y.shape[0] > m
    got = attention_ref.attention(case.rowptr, case.col, case.x, clip_rows(case.y, m), case.p, case.g)
    leaves_the_bound(case, got, ("z", "lse", "dx"))
    unclipped_passes(case, attention_ref.attention(case.rowptr, case.col, case.x, case.y, case.p, case.g), ("z", "lse", "dx", "dy"))


@pytest.mark.parametrize("family", ATTENTION)
def test_attention_tall_sees_x_g_lse_and_d_clipped_to_n_rows(family):
    case = ATTENTION[family]("tall")
    n = case.y.shape[0]
    assert case.m > n
    rowptr, col = rows_emptied(case, n)
    got = attention_ref.attention(rowptr, col, case.x, case.y, case.p, case.g)
    leaves_the_bound(case, got, ("dy",))
    rows_below_are_untouched(case, got, n)


@pytest.mark.parametrize("family", GAT)
def test_gat_wide_sees_y_and_a_src_clipped_to_m_rows(family):
    case = GAT[family]("wide")
    m = case.m
    assert case.n > m
    got = gat_ref.gat(case.rowptr, case.col, clip_rows(case.y, m), case.a_dst, clip_rows(case.a_src, m), case.heads, case.ns, case.g)
    leaves_the_bound(case, got, ("z", "lse", "dadst"))
    # a_src alone, and y alone (which the scores do not read): each descriptor has its own line in the host entry
    got = gat_ref.gat(case.rowptr, case.col, case.y, case.a_dst, clip_rows(case.a_src, m), case.heads, case.ns, case.g)
    leaves_the_bound(case, got, ("z", "lse", "dadst"))
    got = gat_ref.gat(case.rowptr, case.col, clip_rows(case.y, m), case.a_dst, case.a_src, case.heads, case.ns, case.g)
    leaves_the_bound(case, got, ("z", "dadst"))
    unclipped_passes(case, gat_ref.gat(case.rowptr, case.col, case.y, case.a_dst, case.a_src, case.heads, case.ns, case.g),
                     ("z", "lse", "dadst", "dy", "dasrc"))


@pytest.mark.parametrize("family", GAT)
def test_gat_tall_sees_g_a_dst_lse_and_d_clipped_to_n_rows(family):
    case = GAT[family]("tall")
    assert case.m > case.n
    rowptr, col = rows_emptied(case, case.n)
    got = gat_ref.gat(rowptr, col, case.y, case.a_dst, case.a_src, case.heads, case.ns, case.g)
    leaves_the_bound(case, got, ("dy", "dasrc"))
    rows_below_are_untouched(case, got, case.n)


@pytest.mark.parametrize("family", GATV2)
def test_gatv2_wide_sees_y_clipped_to_m_rows(family):
    case = GATV2[family]("wide")
    m = case.m
    assert case.n > m
    got = gatv2_ref.gatv2(case.rowptr, case.col, case.x, clip_rows(case.y, m), case.att, case.heads, case.ns, case.g)
    leaves_the_bound(case, got, ("z", "lse", "dx", "datt"))
    unclipped_passes(case, gatv2_ref.gatv2(case.rowptr, case.col, case.x, case.y, case.att, case.heads, case.ns, case.g),
                     ("z", "lse", "dx", "dy", "datt"))


@pytest.mark.parametrize("family", GATV2)
def test_gatv2_tall_sees_x_g_lse_and_d_clipped_to_n_rows(family):
    case = GATV2[family]("tall")
    assert case.m > case.n
    rowptr, col = rows_emptied(case, case.n)
    got = gatv2_ref.gatv2(rowptr, col, case.x, case.y, case.att, case.heads, case.ns, case.g)
    leaves_the_bound(case, got, ("dy",))
    rows_below_are_untouched(case, got, case.n)


def _spy(monkeypatch, cabi, name, seen):
    real = getattr(cabi, name)

    def wrapper(rows, *rest):
        seen.append((name, rows))
        return real(rows, *rest)
    monkeypatch.setattr(cabi, name, wrapper)


ROUTES = (("attention16", lambda plugin, dtype, k, pitch, rows, mode: plugin.attention16_route(dtype, k, pitch, rows, mode),
           lambda cabi, rows, k, ld: cabi.attention16_serves(rows, k, ld)),
          ("gat16", lambda plugin, dtype, k, pitch, rows, mode: plugin.gat16_route(dtype, 8, k // 8, pitch, rows, mode),
           lambda cabi, rows, k, ld: cabi.gat16_serves(rows, 8, k // 8, ld)),
          ("gatv2_16", lambda plugin, dtype, k, pitch, rows, mode: plugin.gatv2_16_route(dtype, 8, k // 8, pitch, rows, mode),
           lambda cabi, rows, k, ld: cabi.gatv2_16_serves(rows, 8, k // 8, ld)))


@pytest.mark.parametrize("family,route,serves", ROUTES, ids=[r[0] for r in ROUTES])
def test_the_16_bit_routes_answer_with_the_operands_own_row_count(family, route, serves, monkeypatch):
    """route(rows = M, pitch) and route(rows = N, pitch) are independent: each equals the rule written out with cabi.*16_serves and
    cabi.*16_native_pays at the SAME row count, at pitches the two counts answer differently, and neither function is ever asked with the
    other operand's count."""
    from isplib_amd import cabi, plugin
    m, n = rc.SHAPES["tall"]
    k = 64
    between = cabi.DENSE_BYTES_MAX // (2 * 150) // 2 * 2              # an even pitch that n = 67 rows fit in one descriptor and m = 233 do not
    assert serves(cabi, n, k, between) and not serves(cabi, m, k, between) and serves(cabi, m, k, k)
    pays = getattr(cabi, f"{family}_native_pays")

    def written_out(rows, pitch, mode):
        ld = pitch if serves(cabi, rows, k, pitch) else k if serves(cabi, rows, k, k) else None
        if ld is None or mode == "convert":
            return "convert"
        return family if mode == "native" or pays(rows, ld) else "convert"

    for dtype in (BF, FP):
        for pitch in (k, k + 6, k + 1, between):
            for mode in ("native", "auto", "convert"):
                for rows in (m, n):
                    assert route(plugin, dtype, k, pitch, rows, mode) == written_out(rows, pitch, mode), (dtype, pitch, mode, rows)
    assert route(plugin, torch.float32, k, k, m, "native") == "convert"
    # the measured rule, replaced by one that tells the counts apart: each answer follows its own count
    for rows_that_pay in (m, n):
        with monkeypatch.context() as mp:
            mp.setattr(cabi, f"{family}_native_pays", lambda rows, ld, want=rows_that_pay: rows == want)
            for rows in (m, n):
                assert route(plugin, BF, k, k, rows, "auto") == (family if rows == rows_that_pay else "convert")
                assert route(plugin, BF, k, k, rows, "native") == family
    # and a domain that tells them apart: the pitch `between` is taken as it lies for n rows, packed for m rows
    with monkeypatch.context() as mp:
        mp.setattr(cabi, f"{family}_native_pays", lambda rows, ld: ld == between)
        assert route(plugin, BF, k, between, n, "auto") == family and route(plugin, BF, k, between, m, "auto") == "convert"
    # neither function is asked with a count other than the one passed
    for rows in (m, n):
        seen = []
        with monkeypatch.context() as mp:
            for name in (f"{family}_serves", f"{family}_native_pays") + (("gat16_serves",) if family == "gatv2_16" else ()):
                _spy(mp, cabi, name, seen)
            for pitch in (k, between):
                route(plugin, BF, k, pitch, rows, "auto")
        assert seen and {r for _, r in seen} == {rows}, (rows, seen)
