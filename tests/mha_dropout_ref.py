"""Sparse multi-head dot-product attention (q, k, v) with attention dropout (include/isplib_hip_mha_drop.h: isplib_qkv_drop_csr_hip and
its two backward entries) stated in vectorised NumPy, fp64 -- the yardstick of tests/test_mha_dropout_host.py and
tests/test_gpu_mha_dropout.py -- and the per-element error bound a fp32 implementation is held to.  tests/mha_ref.py with
a keep bit q_e,h in {0, 1} per stored entry and head and c = float32(1 / (1 - p)); p_s is the score scale mha_ref calls p:

    s_e, a_e, lse[i,h]  exactly as without dropout: the softmax runs over ALL stored entries
    z_i[head h]  = c sum_e q_e a_e v_j[head h]            D[i,h] = <g_i, z_i>_h
    t_e          = q_e c <g_i, v_j>_h                     ds_e = a_e (t_e - D[i,h])
    dq_i[head h] = p_s sum_e ds_e k_j[head h]             dk_j[head h] = p_s sum_{e -> j} ds_e q_i[head h]
    dv_j[head h] = sum_{e -> j} q_e c a_e g_i[head h]

The keep bit is the one of the GAT dropout, tests/gat_dropout_ref.keep, taken through tests/gatv2_dropout_ref (the library states it in
isplib_amd/csrc/gat_dropout.h); the bit is exact and c is the float32 value, everything else is fp64.
"""
import numpy as np

from tests import mha_ref
from tests.attention_ref import ACC, C_EXP, EPS, RHO_MAX, edge_rows, segment_sum, worst  # noqa: F401  (one set of constants)
from tests.gat_ref import per_head  # noqa: F401
from tests.gatv2_dropout_ref import keep, scale, threshold  # noqa: F401


def mha_drop(rowptr, col, q, k, v, heads, ps, p, seed, g=None, fwd=None, mask=None):
    """-> the dict of mha_ref.mha with z, D, t, ds, dq, dk, dv those of the function above, and q (bool [nnz, H]: the keep bits), c
    (float), qc (= q c, fp64 [nnz, H]).  `ps`: the score scale; `p`: the dropout probability.  `fwd`: the reference of the same operands
    without dropout -- row, s, a and lse do not depend on the mask and are taken from it.  `mask`: a mask to use in place of
    keep(seed, ...) (the cases' counter-examples)."""
    m, n, K = rowptr.size - 1, k.shape[0], k.shape[1]
    if fwd is None:
        fwd = mha_ref.mha(rowptr, col, q, k, v, heads, ps)
    out = {name: fwd[name] for name in ("row", "s", "a", "lse")}
    row, a = out["row"], out["a"]
    if mask is None:
        mask = keep(seed, col.size, heads, p)
    c = float(scale(p))
    qc = mask.astype(np.float64) * c
    ve = per_head(v.astype(np.float64), heads)[col]                       # [nnz, H, d]
    out.update(q=mask, c=c, qc=qc, z=segment_sum((qc * a)[:, :, None] * ve, row, m).reshape(m, K))
    if g is not None:
        qe = per_head(q.astype(np.float64), heads)[row]
        ke = per_head(k.astype(np.float64), heads)[col]
        g3 = per_head(g.astype(np.float64), heads)
        D = (g3 * per_head(out["z"], heads)).sum(2)
        t = qc * (g3[row] * ve).sum(2)
        ds = a * (t - D[row])
        out.update(D=D, t=t, ds=ds, dq=float(ps) * segment_sum(ds[:, :, None] * ke, row, m).reshape(m, K),
                   dk=float(ps) * segment_sum(ds[:, :, None] * qe, col, n).reshape(n, K),
                   dv=segment_sum((qc * a)[:, :, None] * g3[row], col, n).reshape(n, K))
    return out


def bounds(rowptr, col, q, k, v, heads, ps, ref, g=None):
    """The per-element bound on |fp32 result - ref| (ref = mha_drop(...) of the same operands): mha_ref.bounds with the mask carried
    through, by the substitutions DESIGN.md 4.6i made for GAT and 4.6j for GATv2.  No new constants.

    The forward accumulates sum_e q_e w_e v_j beside the unmasked l = sum_e w_e and writes c (acc / l): each kept term carries the
    relative error of its a_e (2 rho) and of the accumulation (1e-5), a dropped term is an exact zero, and the final multiply by c adds
    one rounding of the result.  So q_e c a_e replaces a_e in the value sum, and eps |z| is added:

        delta s_e, rho, lse, rhob_e                                       unchanged: the softmax does not see the mask
        z[i,c]       = (1e-5 + 2 rho[i,h]) sum_e q_e c a_e |v_jc| + eps |z_ic| + 1e-30

    The backward forms t_e = (q_e c) <g_i, v_j>_h: the dot product's accumulation error (1e-5 sum_c |g_ic v_jc|) is scaled by q_e c, and
    the rounding of that one multiply, eps q_e c |<g_i, v_j>|, lies inside the same term (eps << 1e-5).  So q_e c goes inside t, in the
    value and in the accumulation term; D's bound is formed from the new z:

        eta_e        = a_e (rhob_e |t_e - D[i,h]| + 1e-5 (q_e c sum_c |g_ic v_jc|_h + sum_c |g_ic z_ic|_h))
        carry_e      = eta_e + 1e-5 |ds_e|
        dq[i,c]      = |p_s| sum_e carry_e |k_jc| + 1e-30
        dk[j,c]      = |p_s| sum_{e->j} carry_e |q_ic| + 1e-30
        D[i,h]       = sum_c |g_ic| z[i,c] + 1e-5 sum_c |g_ic z_ic|_h + 1e-30

    The columns kernel forms the value coefficient q_e ? a_e c : 0 per edge and head -- one more rounding, eps, on the coefficient whose
    relative error was rhob_e + 1e-5:

        dv[j,c]      = sum_{e->j} (rhob_e + 1e-5 + eps) q_e c a_e |g_ic| + 1e-30

    With every bit kept and c = 1 each line is the line of mha_ref.bounds plus a non-negative eps term: never tighter.
    """
    m, n, K = rowptr.size - 1, k.shape[0], k.shape[1]
    row, s, a, qc = ref["row"], ref["s"], ref["a"], ref["qc"]
    ap = abs(float(ps))
    qe = np.abs(per_head(q.astype(np.float64), heads))[row]
    ke = np.abs(per_head(k.astype(np.float64), heads))[col]
    ve = np.abs(per_head(v.astype(np.float64), heads))[col]
    dscore = ACC * ap * (qe * ke).sum(2)
    deg = np.diff(rowptr).astype(np.float64)
    hi, lo, dmax = np.full((m, heads), -np.inf), np.full((m, heads), np.inf), np.zeros((m, heads))
    np.maximum.at(hi, row, s)
    np.minimum.at(lo, row, s)
    np.maximum.at(dmax, row, dscore)
    live = (deg > 0)[:, None]
    rng = np.where(live, hi - np.where(live, lo, 0.0), 0.0)
    rho = dmax + C_EXP * EPS * (rng + deg[:, None] + 4.0)
    lse0 = np.where(live, ref["lse"], 0.0)
    zb = ((ACC + 2.0 * rho)[:, :, None] * segment_sum((qc * a)[:, :, None] * ve, row, m)).reshape(m, K) + EPS * np.abs(ref["z"]) + 1e-30
    out = dict(rho=rho, z=zb, lse=np.where(live, rho + ACC + 2.0 * EPS * np.abs(lse0), 0.0))
    if g is not None:
        g3 = np.abs(per_head(g.astype(np.float64), heads))
        ge = g3[row]
        rhob = dscore + out["lse"][row] + C_EXP * EPS * (1.0 + np.abs(s - lse0[row]))
        gz = (g3 * np.abs(per_head(ref["z"], heads))).sum(2)
        eta = a * (rhob * np.abs(ref["t"] - ref["D"][row]) + ACC * (qc * (ge * ve).sum(2) + gz[row]))
        carry = eta + ACC * np.abs(ref["ds"])
        out.update(dq=ap * segment_sum(carry[:, :, None] * ke, row, m).reshape(m, K) + 1e-30,
                   dk=ap * segment_sum(carry[:, :, None] * qe, col, n).reshape(n, K) + 1e-30,
                   dv=segment_sum(((rhob + ACC + EPS) * qc * a)[:, :, None] * ge, col, n).reshape(n, K) + 1e-30,
                   D=(g3 * per_head(zb, heads)).sum(2) + ACC * gz + 1e-30)
    return out
