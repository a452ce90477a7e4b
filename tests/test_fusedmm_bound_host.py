"""CPU tests of the FusedMM accuracy contract itself (tests/fusedmm_bound.py): not too tight for correct fp32 code -- the C oracle
(glibc expf, IEEE division, sequential sums) passes it with C_f = 1 on every input the GPU tests use --, not too loose to matter
-- faults planted in an fp64 copy of the reference are rejected, two of them faults the former 1e-4 * max|z| rule accepts --,
and consistent with the reference it is computed from."""
import numpy as np
import pytest

from tests import fusedmm_bound as fb
from tests import fusedmm_cases as fc
from tests import fusedmm_ref


def _oracle_case(oracle, word, rowptr, col, x, y, fn, what):
    kind = fb.KINDS[fn]
    ref, bound, aux = fb.fusedmm_bound(word, rowptr, col, None, x, y, kind, fc.PARAM, c_f=fb.C_F["oracle"])
    st, z, arg = oracle.fusedmm_general(word, rowptr, col, None, x, y, kind, fc.PARAM)
    assert st == 0
    fb.assert_within(z, ref, bound, aux["mag"], what)
    if arg is not None:
        fb.assert_arg_within(arg, rowptr, col.size, ref, bound, aux, ((word >> 16) & 0xF) == 2, what)


@pytest.mark.parametrize("k", (5, 8, 32, 41, 64, 128, 300))
def test_oracle_within_bound_on_prescribed_s(oracle_mod, k):
    rowptr, col = fc.prescribed_graph()
    x, y = fc.prescribed_operands(k)
    for fn in fc.menu_on(fc.DOT_WORD):
        _oracle_case(oracle_mod, fc.DOT_WORD, rowptr, col, x, y, fn, (fn, k))


@pytest.mark.parametrize("word", (fc.DOT_WORD, fc.NORM_WORD))
@pytest.mark.parametrize("k", (32, 128, 602))
def test_oracle_within_bound_on_spread_s(oracle_mod, word, k):
    rowptr, col = fc.named_graph()
    x, y = fc.spread_operands(word, 400, 300, k)
    for fn in fc.menu_on(word):
        _oracle_case(oracle_mod, word, rowptr, col, x, y, fn, (hex(word), fn, k))


@pytest.mark.parametrize("k", (5, 41, 300))
def test_oracle_within_bound_on_other_stage_combinations(oracle_mod, k):
    rowptr, col = fc.combo_graph(k)
    for word in fc.combo_words():
        x, y = fc.spread_operands(word, 70, 55, k)
        for fn in ("sigmoid", "leaky_exp"):
            _oracle_case(oracle_mod, word, rowptr, col, x, y, fn, (hex(word), fn, k))


# ---- planted faults -------------------------------------------------------------------------------------------------------

def _bf16(s):
    b = np.asarray(s, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def _rcp_bits(v, bits):
    """1 / v with the mantissa truncated to `bits` bits."""
    mant, expo = np.frexp(1.0 / v)
    return np.ldexp(np.floor(mant * 2.0 ** bits) / 2.0 ** bits, expo)


def _menu_with(kind, f):
    return lambda kd, s, p: f(s, p) if kd == kind else fusedmm_ref.sop_menu(kd, s, p)


def _old_rule_accepts(z, ref):
    return bool(np.all(np.abs(z - ref) <= 1e-4 * np.abs(ref).max() + 1e-7))


def _faulty(word, rowptr, col, x, y, fn, menu):
    """(rejected by the bound, accepted by the old rule) for the reference run with a modified menu function.  The bound is
    computed with the LARGEST device C_f, the loosest it is ever used with."""
    kind = fb.KINDS[fn]
    ref, bound, aux = fb.fusedmm_bound(word, rowptr, col, None, x, y, kind, fc.PARAM, c_f=max(v for v in fb.C_F["stream"].values()))
    with np.errstate(over="ignore", under="ignore"):
        z, _ = fusedmm_ref.fusedmm(word, rowptr, col, None, x, y, kind, fb.f32(fc.PARAM), menu=menu)
    return fb.violations(z, ref, bound, aux["mag"])[0].size > 0, _old_rule_accepts(z, ref)


def _sig(s):
    return 1.0 / (1.0 + np.exp(-s))


def test_bound_rejects_faults_in_the_exponentials_at_prescribed_s():
    rowptr, col = fc.prescribed_graph()
    x, y = fc.prescribed_operands(32)
    # leaky_exp ignoring p for s < 0
    assert _faulty(fc.DOT_WORD, rowptr, col, x, y, "leaky_exp", _menu_with(6, lambda s, p: np.exp(s)))[0]
    # exp clamped at e^60
    assert _faulty(fc.DOT_WORD, rowptr, col, x, y, "exp", _menu_with(5, lambda s, p: np.exp(np.minimum(s, 60.0))))[0]


@pytest.mark.parametrize("k", (32, 128))
def test_bound_rejects_low_precision_stages_the_old_rule_accepts(k):
    """On the wide-spread data (every value of the prescribed-s grid but 1e-3 is a bf16 number, so rounding s shows nothing
    there).  The 1e-4 * max|z| rule does catch the two coarsest faults on this data, s in bf16 and a 12-bit truncated
    reciprocal; it accepts the next finer ones, s in fp16 and a 13-bit truncated reciprocal, which the bound still rejects."""
    rowptr, col = fc.named_graph()
    x, y = fc.spread_operands(fc.DOT_WORD, 400, 300, k)
    assert _faulty(fc.DOT_WORD, rowptr, col, x, y, "sigmoid", _menu_with(1, lambda s, p: _sig(_bf16(s))))[0]
    half = _menu_with(1, lambda s, p: _sig(s.astype(np.float16).astype(np.float64)))
    assert _faulty(fc.DOT_WORD, rowptr, col, x, y, "sigmoid", half) == (True, True)
    x, y = fc.spread_operands(fc.NORM_WORD, 400, 300, k)
    assert _faulty(fc.NORM_WORD, rowptr, col, x, y, "tdist", _menu_with(3, lambda s, p: _rcp_bits(1.0 + s, 12)))[0]
    assert _faulty(fc.NORM_WORD, rowptr, col, x, y, "tdist", _menu_with(3, lambda s, p: _rcp_bits(1.0 + s, 13))) == (True, True)


def test_bound_rejects_a_sigmoid_that_flushes_its_tail():
    """sigmoid returning 0 for s < -20.  In a row that also holds an ordinary edge the lost 1e-9 is below that edge's own
    rounding, so no per-element rule over real rows can see it (the prescribed-s graph has no row of saturated edges only):
    the single-edge probe of the transfer-curve test does, because the model error of sigmoid is relative in sigma."""
    fn, kind = "sigmoid", fb.KINDS["sigmoid"]
    s = fc.probe_grid(fn, 512)
    rowptr, col = fc.probe_graph(s.size)
    x, y = fc.probe_dot(s)
    ref, bound, aux = fb.fusedmm_bound(fc.DOT_WORD, rowptr, col, None, x, y, kind, 0.0, c_f=fb.C_F["stream"])
    with np.errstate(over="ignore"):
        flushed = _menu_with(1, lambda v, p: np.where(v < -20.0, 0.0, 1.0 / (1.0 + np.exp(-v))))
        z, _ = fusedmm_ref.fusedmm(fc.DOT_WORD, rowptr, col, None, x, y, kind, 0.0, menu=flushed)
    tol = fb.C_F["stream"][kind] * fb.sop_model(kind, s.astype(np.float64), 0.0) + fb.FLT_MIN      # the transfer-curve rule
    assert np.any(np.abs(z[:, 1] - ref[:, 1]) > tol) and _old_rule_accepts(z, ref)
    assert fb.violations(z, ref, bound, aux["mag"])[0].size > 0                                    # and the element bound there


def test_bound_rejects_a_dropped_edge():
    """The lowest-magnitude edge of one ordinary row left out."""
    rowptr, col = fc.named_graph()
    x, y = fc.spread_operands(fc.DOT_WORD, 400, 300, 32)
    kind = fb.KINDS["sigmoid"]
    ref, bound, aux = fb.fusedmm_bound(fc.DOT_WORD, rowptr, col, None, x, y, kind, 0.0, c_f=fb.C_F["stream"])
    row = 20
    b, e = rowptr[row], rowptr[row + 1]
    assert 10 <= e - b <= 40                                                     # an ordinary row
    drop = b + int(np.argmin(np.abs(aux["T_out"][b:e]).sum(1)))
    rowptr2 = rowptr.copy()
    rowptr2[row + 1:] -= 1
    z, _ = fusedmm_ref.fusedmm(fc.DOT_WORD, rowptr2, np.delete(col, drop), None, x, y, kind, 0.0)
    bad = fb.violations(z, ref, bound, aux["mag"])
    assert bad[0].size > 0 and np.all(bad[0] == row)
    assert _old_rule_accepts(z, ref)


# ---- self-consistency --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", fc.MENU)
def test_derivative_agrees_with_a_central_difference_of_the_reference_menu(fn):
    kind, p = fb.KINDS[fn], fb.f32(fc.PARAM)
    s = np.concatenate((np.linspace(-30.0, 30.0, 241) + 0.0625, [1e-3, -1e-3]))
    if fn == "tdist":
        s = np.abs(s)
    h = 1e-5 * np.maximum(1.0, np.abs(s))
    central = (fusedmm_ref.sop_menu(kind, s + h, p) - fusedmm_ref.sop_menu(kind, s - h, p)) / (2.0 * h)
    # truncation: h^2 |f'''| / 6 <= 1e-9 of |f'| here; cancellation: the reference forms 1 - sigma and 1 + e^-s, so a value carries
    # 2^-53 of max(1, |f|), and a difference of two of them 2^-52 of that over 2 h
    got = fb.sop_prime(kind, s, p)
    f = np.abs(fusedmm_ref.sop_menu(kind, s, p))
    assert np.all(np.abs(got - central) <= 1e-6 * np.abs(central) + 2.0 ** -52 * np.maximum(1.0, f) / h)


def test_bound_parts_add_up_on_a_hand_case():
    """One row, two edges, k = 2, dot word with SCALE: every part of the bound written out by hand."""
    rowptr, col = np.array([0, 2], np.int64), np.array([0, 1], np.int64)
    x = np.array([[1.0, 2.0]], np.float32)
    y = np.array([[3.0, -1.0], [0.5, 4.0]], np.float32)
    ref, bound, aux = fb.fusedmm_bound(fc.DOT_WORD, rowptr, col, None, x, y, fb.SCALE, 0.5, c_f=8.0)
    s = np.array([1.0, 8.5])
    f = 0.5 * s
    assert np.array_equal(aux["s"], s) and np.array_equal(aux["f"], f)
    assert np.array_equal(ref, [[f[0] * 3.0 + f[1] * 0.5, f[0] * -1.0 + f[1] * 4.0]])
    ds = fb.REL * np.array([3.0 + 2.0, 0.5 + 8.0])
    for c, t in enumerate(([3.0, 0.5], [1.0, 4.0])):
        t = np.array(t)
        want = fb.REL * (f * t).sum() + (0.5 * ds * t).sum() + 8.0 * (fb.EPS * f * t).sum() + fb.FLT_MIN * t.sum() + 1e-30
        assert abs(bound[0, c] - want) <= 1e-12 * want
