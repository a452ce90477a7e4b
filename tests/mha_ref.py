"""Sparse multi-head dot-product attention with separate keys and values (include/isplib_hip_mha.h: isplib_mha_csr_hip and its two
backward entries) stated in vectorised NumPy, fp64, per edge and head -- the yardstick of tests/test_mha_host.py and
tests/test_gpu_mha.py (the reference project has no such operator) -- and the per-element error bound a fp32 implementation is held to
(DESIGN.md 4.6k).

For the stored entries e = (i, j) of a CSR structure, q [m, H*d], k and v [n, H*d] (head h owns the columns [h*d, (h+1)*d)), a scalar p
and g = dL/dz, for every head h:
    s_e  = p <q_i, k_j>_h         a_e = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)
    z_i[head h] = sum_e a_e v_j[head h]                            (empty row: 0, -inf)
    D[i,h] = <g_i, z_i>_h         t_e = <g_i, v_j>_h               ds_e = a_e (t_e - D[i,h])
    dq_i[head h] = p sum_e ds_e k_j[head h]     dk_j[head h] = p sum_{e->j} ds_e q_i[head h]     dv_j[head h] = sum_{e->j} a_e g_i[head h]
"""
import numpy as np

from tests.attention_ref import ACC, C_EXP, EPS, RHO_MAX, edge_rows, segment_sum, worst  # noqa: F401  (one set of constants)
from tests.gat_ref import per_head


def mha(rowptr, col, q, k, v, heads, p, g=None):
    """-> dict of fp64 arrays: z [m, K], lse [m, H]; with g also D [m, H], dq [m, K], dk, dv [n, K]; and the per-edge parts row and
    s, a, t, ds [nnz, H]."""
    m, n, K = rowptr.size - 1, k.shape[0], k.shape[1]
    row = edge_rows(rowptr)
    qe = per_head(q.astype(np.float64), heads)[row]                       # [nnz, H, d]
    ke = per_head(k.astype(np.float64), heads)[col]
    ve = per_head(v.astype(np.float64), heads)[col]
    s = float(p) * (qe * ke).sum(2)
    deg = np.diff(rowptr)
    smax = np.full((m, heads), -np.inf)
    np.maximum.at(smax, row, s)
    live = (deg > 0)[:, None]
    shift = np.where(live, smax, 0.0)
    w = np.exp(s - shift[row])
    lse = np.where(live, shift + np.log(np.maximum(segment_sum(w, row, m), 1e-300)), -np.inf)
    a = np.exp(s - np.where(live, lse, 0.0)[row])
    out = dict(row=row, s=s, a=a, lse=lse, z=segment_sum(a[:, :, None] * ve, row, m).reshape(m, K))
    if g is not None:
        g3 = per_head(g.astype(np.float64), heads)
        D = (g3 * per_head(out["z"], heads)).sum(2)
        t = (g3[row] * ve).sum(2)
        ds = a * (t - D[row])
        out.update(D=D, t=t, ds=ds, dq=float(p) * segment_sum(ds[:, :, None] * ke, row, m).reshape(m, K),
                   dk=float(p) * segment_sum(ds[:, :, None] * qe, col, n).reshape(n, K),
                   dv=segment_sum(a[:, :, None] * g3[row], col, n).reshape(n, K))
    return out


def bounds(rowptr, col, q, k, v, heads, p, ref, g=None):
    """The per-element bound on |fp32 result - ref| (ref = mha(...) of the same operands): attention_ref.bounds taken per head, with
    the value term split off the key term.  rho, lse [m, H]; z [m, K]; with g also D [m, H], dq [m, K], dk, dv [n, K].

        delta s_e    = 1e-5 |p| sum_{c in h} |q_ic k_jc|                the project's SDDMM rule
        rho[i,h]     = max_e delta s_e + 8 eps (R + deg_i + 4)          R: the score range of row i, head h
        z[i,c]       = (1e-5 + 2 rho[i,h]) sum_e a_e |v_jc| + 1e-30
        lse[i,h]     = rho[i,h] + 1e-5 + 2 eps |lse[i,h]|
        rhob_e       = delta s_e + lse[i,h] + 8 eps (1 + |s_e - lse[i,h]|)
        eta_e        = a_e (rhob_e |t_e - D[i,h]| + 1e-5 (sum_c |g_ic v_jc|_h + sum_c |g_ic z_ic|_h))
        carry_e      = eta_e + 1e-5 |ds_e|
        dq[i,c]      = |p| sum_e carry_e |k_jc| + 1e-30
        dk[j,c]      = |p| sum_{e->j} carry_e |q_ic| + 1e-30
        dv[j,c]      = sum_{e->j} (rhob_e + 1e-5) a_e |g_ic| + 1e-30
        D[i,h]       = sum_c |g_ic| z[i,c] + 1e-5 sum_c |g_ic z_ic|_h + 1e-30            (as gatv2_ref.bounds)
    """
    m, n, K = rowptr.size - 1, k.shape[0], k.shape[1]
    row, s, a = ref["row"], ref["s"], ref["a"]
    ap = abs(float(p))
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
    zb = ((ACC + 2.0 * rho)[:, :, None] * segment_sum(a[:, :, None] * ve, row, m)).reshape(m, K) + 1e-30
    out = dict(rho=rho, z=zb, lse=np.where(live, rho + ACC + 2.0 * EPS * np.abs(lse0), 0.0))
    if g is not None:
        g3 = np.abs(per_head(g.astype(np.float64), heads))
        ge = g3[row]
        rhob = dscore + out["lse"][row] + C_EXP * EPS * (1.0 + np.abs(s - lse0[row]))
        gz = (g3 * np.abs(per_head(ref["z"], heads))).sum(2)
        eta = a * (rhob * np.abs(ref["t"] - ref["D"][row]) + ACC * ((ge * ve).sum(2) + gz[row]))
        carry = eta + ACC * np.abs(ref["ds"])
        out.update(dq=ap * segment_sum(carry[:, :, None] * ke, row, m).reshape(m, K) + 1e-30,
                   dk=ap * segment_sum(carry[:, :, None] * qe, col, n).reshape(n, K) + 1e-30,
                   dv=segment_sum(((rhob + ACC) * a)[:, :, None] * ge, col, n).reshape(n, K) + 1e-30,
                   D=(g3 * per_head(zb, heads)).sum(2) + ACC * gz + 1e-30)
    return out
