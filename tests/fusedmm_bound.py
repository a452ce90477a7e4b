"""The per-element accuracy contract of the FusedMM kernels, computed from the fp64 reference of
tests/fusedmm_ref.py.  NumPy fp64 throughout; no code shared with the kernels or with the C oracle.

For output element (i, c) over the edges e of row i, with T the vector stage's output, s the reduce stage's, s' = f(s) the scalar
stage's and w_e[c] the factor by which an error of s'_e reaches the element (|T_e[c]| under VSC_MUL / MEAN, 1 under VSC_ADD):

    bound[i, c] =   REL * sum_e |terms_e[c]|                  accumulation: BASELINE.md section 3 (|s' T|; VSC_ADD: |s'| + |T|)
                  + sum_e |f'(s_e)| * ds_e * w_e[c]           reduce stage: ds_e = REL * sum_c |products of the reduction|
                  + C_f * sum_e df(s_e) * w_e[c]              scalar stage: df = the model error of one evaluation of f (sop_model)
                  + FLT_MIN * sum_e w_e[c] + 1e-30            the fast intrinsics may return 0 for a subnormal result

Under AOP_MAX / AOP_MIN the element is ONE of the edges' T', so the sums over e become maxima over e (|max a - max b| <= max |a - b|).
The division of VSC_MEAN scales every part by 1 / max(deg, 1).
"""
import numpy as np

from tests import fusedmm_ref

REL = 1e-5
EPS = 2.0 ** -24                # half an ulp of 1.0f
FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)

SIGMOID, ONE_MINUS_SIGMOID, TDIST, SCALE, EXP, LEAKY_EXP = 1, 2, 3, 4, 5, 6
KINDS = {"sigmoid": SIGMOID, "one_minus_sigmoid": ONE_MINUS_SIGMOID, "tdist": TDIST, "scale": SCALE, "exp": EXP, "leaky_exp": LEAKY_EXP}

# C_f per kernel file and menu entry: four times the largest |f_dev - f_64| / df that scripts/fusedmm_sop_accuracy.py observed on
# the MI355X over its whole grid, rounded up to a power of two.  The observed maxima are in profiles/fusedmm_sop_accuracy.txt
# and in DESIGN.md 4.6a; "oracle" is the C oracle (glibc expf, IEEE division: sub-ulp), held to one model unit.
C_F = {
    "oracle": {SIGMOID: 1.0, ONE_MINUS_SIGMOID: 1.0, TDIST: 1.0, SCALE: 1.0, EXP: 1.0, LEAKY_EXP: 1.0},
    # fusedmm_general.hip (row and task forms): observed 1.972, 1.405, 1.476, 0.949, 1.217, 1.356
    "general": {SIGMOID: 8.0, ONE_MINUS_SIGMOID: 8.0, TDIST: 8.0, SCALE: 4.0, EXP: 8.0, LEAKY_EXP: 8.0},
    # fusedmm_stream.hip (reciprocals by v_rcp_f32): observed 2.080, 1.471, 1.813, 0.949, 1.217, 1.356
    "stream": {SIGMOID: 16.0, ONE_MINUS_SIGMOID: 8.0, TDIST: 8.0, SCALE: 4.0, EXP: 8.0, LEAKY_EXP: 8.0},
}


def f32(p):
    """The menu parameter as the kernels receive it: a float."""
    return float(np.float32(p))


def sop_prime(kind, s, p):
    """f'(s), analytic (tests/test_fusedmm_bound_host.py holds it to a central difference of fusedmm_ref.sop_menu)."""
    with np.errstate(over="ignore", under="ignore"):
        f = fusedmm_ref.sop_menu(kind, s, p)
        if kind in (SIGMOID, ONE_MINUS_SIGMOID):
            sg = f if kind == SIGMOID else 1.0 - f
            return (sg * (1.0 - sg)) * (1.0 if kind == SIGMOID else -1.0)
        if kind == TDIST:
            return -f * f
        if kind == SCALE:
            return np.full_like(s, p)
        if kind == EXP:
            return f
        if kind == LEAKY_EXP:
            return f * np.where(s > 0, 1.0, p)
    return np.ones_like(s)


def sop_model(kind, s, p):
    """df(s): the error model of ONE evaluation of the menu entry in fp32, in units of which C_f is measured."""
    with np.errstate(over="ignore", under="ignore"):
        f = fusedmm_ref.sop_menu(kind, s, p)
        if kind == SIGMOID:                     # relative in sigma: a kernel that returns 0 at s = -30 fails
            return EPS * f * (1.0 + (1.0 - f) * np.abs(s))
        if kind == ONE_MINUS_SIGMOID:           # absolute: formed as 1 - sigma(s), 0 for s >~ 17 where the truth is e^-s
            return np.full_like(s, EPS)
        if kind in (TDIST, SCALE):
            return EPS * np.abs(f)
        if kind == EXP:                         # exp2(a * log2 e): the relative error grows with the argument
            return EPS * (1.0 + np.abs(s)) * f
        if kind == LEAKY_EXP:
            return EPS * (1.0 + np.abs(np.where(s > 0, s, p * s))) * f
    return np.zeros_like(s)


def _segment(values, rowptr, m, how):
    """Per-row sum or maximum of a per-edge [nnz, k] array -> [m, k] (empty rows: 0)."""
    out = np.zeros((m, values.shape[1]))
    if how == "sum":
        np.add.at(out, np.repeat(np.arange(m), np.diff(rowptr)), values)
    else:
        live = np.flatnonzero(np.diff(rowptr) > 0)
        if live.size:
            out[live] = np.maximum.reduceat(values, rowptr[live], axis=0)
    return out


def fusedmm_bound(imsg, rowptr, col, val, x, y, sop_udef=0, sop_param=0.0, c_f=1.0, menu=None):
    """-> (ref, bound, aux).  ref = fusedmm_ref.fusedmm's z; bound as in the module text, [m, k] fp64;
    aux: per-edge "s", "f" (= s'), "T_out" (= T'), the reference "arg" (None under AOP_ADD) and "mag" [m, k], the
    sum (max under AOP_MAX / MIN) of |terms| that the accumulation part is REL times, and "scalar" [m, k], the same of df * w: under
    AOP_ADD the bound for another C_f is bound + (C_f' - C_f) * scalar, without a second pass over the reference.  `c_f`: a number, or a dict over
    menu entries such as C_F["stream"].  `menu` is handed to the reference (planted faults)."""
    vop, rop, sop, vsc, aop = imsg & 0xF, (imsg >> 4) & 0xF, (imsg >> 8) & 0xF, (imsg >> 12) & 0xF, (imsg >> 16) & 0xF
    p = f32(sop_param)
    m, k = rowptr.size - 1, y.shape[1]
    parts = {}
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ref, arg = fusedmm_ref.fusedmm(imsg, rowptr, col, val, x, y, sop_udef, p, menu=menu, parts=parts)
        xe, T, s, s_out, T_out = parts["xe"], parts["T"], parts["s"], parts["s_out"], parts["T_out"]
        absT = np.abs(T)
        if vsc in (1, 3):
            terms, w = np.abs(T_out), absT
        elif vsc == 2:
            terms, w = np.abs(s_out)[:, None] + absT, np.ones_like(T)
        else:
            terms, w = absT, np.zeros_like(T)
        ds = REL * {0: np.zeros_like(s), 1: np.abs(xe * T).sum(1), 2: np.abs(xe).sum(1), 3: absT.sum(1), 4: (xe * xe).sum(1),
                    5: (T * T).sum(1)}[rop]
        if sop == 0xF:
            kind = int(sop_udef)
            cf = float(c_f[kind] if isinstance(c_f, dict) else c_f)
            per_s = np.abs(sop_prime(kind, s, p)) * ds + cf * sop_model(kind, s, p)
        elif sop == 0:
            per_s = ds
        else:
            per_s = np.zeros_like(s)
        per_edge = REL * terms + per_s[:, None] * w + FLT_MIN * w
        how = "sum" if aop == 1 else "max"
        bound = _segment(per_edge, rowptr, m, how) + 1e-30
        mag = _segment(terms, rowptr, m, how)
        scalar = _segment((sop_model(int(sop_udef), s, p) if sop == 0xF else np.zeros_like(s))[:, None] * w, rowptr, m, how)
        if vsc == 3:
            deg = np.maximum(np.diff(rowptr), 1)[:, None]
            bound, mag, scalar = bound / deg, mag / deg, scalar / deg
    return ref, bound, {"s": s, "f": s_out, "T_out": T_out, "arg": arg, "mag": mag, "scalar": scalar, "row": parts["row"]}


def violations(got, ref, bound, mag):
    """Indices (as a tuple of arrays) of the elements of `got` outside the contract.  Where every term is finite in fp32 and
    their magnitudes sum below FLT_MAX no ordering of the partial sums can overflow: |got - ref| <= bound.  Where they do not,
    an fp32 sum may be +-inf: it must then be the reference's sign of infinity, and it MUST be infinite when the reference
    itself lies more than the bound beyond FLT_MAX; a finite answer is still held to the bound.  NaN never passes."""
    got = np.asarray(got, np.float64)
    safe = mag <= FLT_MAX * (1.0 - 2.0 ** -10)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got - ref)
        close = err <= bound
        right_inf = np.isinf(got) & (np.sign(got) == np.sign(ref))
        must_inf = np.abs(ref) - bound > FLT_MAX * (1.0 + 2.0 ** -10)
        ok = np.where(safe, close, np.where(must_inf, right_inf, right_inf | close))
    return np.nonzero(~ok)


def assert_within(got, ref, bound, mag, what=""):
    """Raises on any element outside the contract; -> the largest |got - ref| / bound among the finite elements."""
    bad = violations(got, ref, bound, mag)
    if bad[0].size:
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ratio = np.abs(np.asarray(got, np.float64)[bad] - ref[bad]) / bound[bad]
        w = int(np.nanargmax(ratio)) if np.any(~np.isnan(ratio)) else 0
        at = tuple(int(b[w]) for b in bad)
        raise AssertionError(f"{what}: {bad[0].size} elements outside the bound; worst at {at}: got {np.asarray(got)[at]!r}, "
                             f"reference {ref[at]!r}, bound {bound[at]!r} (error / bound = {ratio[w]:.3g})")
    fin = np.isfinite(got)
    return float(np.max(np.abs(np.asarray(got, np.float64)[fin] - ref[fin]) / bound[fin])) if np.any(fin) else 0.0


def assert_arg_within(got_arg, rowptr, nnz, ref, bound, aux, maximum, what=""):
    """The device's winner positions: inside the row, and the fp64 T' there within `bound` of the reference extreme (ties and
    near-ties may fall either way); nnz on empty rows.  No element is excluded."""
    got_arg = np.asarray(got_arg)
    m, k = ref.shape
    deg = np.diff(rowptr)
    empty = deg == 0
    assert np.all(got_arg[empty] == nnz), f"{what}: empty rows must hold nnz"
    lo, hi = rowptr[:-1][:, None], rowptr[1:][:, None]
    live = ~empty
    assert np.all((got_arg[live] >= np.broadcast_to(lo, got_arg.shape)[live]) & (got_arg[live] < np.broadcast_to(hi, got_arg.shape)[live])), \
        f"{what}: a winner outside its row"
    cols = np.broadcast_to(np.arange(k), got_arg.shape)
    at = aux["T_out"][got_arg[live], cols[live]]
    gap = (ref[live] - at) if maximum else (at - ref[live])
    assert np.all(gap <= bound[live]), f"{what}: a winner whose value is {np.max(gap / bound[live]):.3g} bounds from the extreme"


def probe_excess(kind, p, s, got, factor=None):
    """The single-edge probe (tests/fusedmm_cases.py: probe_dot, probe_norm): `got` is the device's f(s), or f(s) * factor on the
    norm word, where the product is rounded once more.  -> (excess, df): the error beyond the floor FLT_MIN (and beyond the
    product's own half ulp), and the model error it is held to C_f times of, both scaled by |factor|."""
    s = np.asarray(s, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        f = fusedmm_ref.sop_menu(kind, s, f32(p))
        df = sop_model(kind, s, f32(p))
        if factor is None:
            want, slack = f, FLT_MIN
        else:
            a = np.abs(np.asarray(factor, np.float64))
            want = f * np.asarray(factor, np.float64)
            slack, df = FLT_MIN * a + EPS * np.abs(want) + 2.0 ** -149, df * a
        return np.maximum(np.abs(np.asarray(got, np.float64) - want) - slack, 0.0), df
