"""The GATv2 attention aggregation (include/isplib_hip.h: isplib_gatv2_csr_hip and its two backward entries) stated in vectorised
NumPy, fp64, per edge, head and column -- the yardstick of tests/test_gatv2_host.py and tests/test_gpu_gatv2.py (the reference project
has no such operator) -- and the per-element error bound a fp32 implementation is held to.

For the stored entries e = (i, j) of a CSR structure, x [m, H*d], y [n, H*d] (head h owns the columns [h*d, (h+1)*d)), att [H, d], a
slope ns and g = dL/dz, for every head h and c over the head's columns:
    u_ec = x_ic + y_jc            sl_ec = (u_ec > 0 ? 1 : ns)      v_ec = sl_ec u_ec
    s_e  = sum_c att_c v_ec       a_e = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)
    z_i[head h] = sum_e a_e y_j[head h]                            (empty row: 0, -inf)
    D[i,h] = <g_i, z_i>_h         t_e = <g_i, y_j>_h               ds_e = a_e (t_e - D[i,h])
    q_ec   = ds_e att_c sl_ec
    dx_ic  = sum_e q_ec           dy_jc = sum_{e->j} (a_e g_ic + q_ec)      datt_c = sum_{all e} ds_e v_ec
"""
import numpy as np

from tests.attention_ref import ACC, C_EXP, EPS, RHO_MAX, edge_rows, segment_sum, worst  # noqa: F401  (one set of constants)
from tests.gat_ref import per_head


def gatv2(rowptr, col, x, y, att, heads, ns, g=None):
    """-> dict of fp64 arrays: z [m, K], lse [m, H]; with g also D [m, H], dx [m, K], dy [n, K], datt [H, d]; and the per-edge parts
    row, s, a, t, ds [nnz, H] and u, sl, v [nnz, H, d]."""
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row = edge_rows(rowptr)
    ye = per_head(y.astype(np.float64), heads)[col]                       # [nnz, H, d]
    u = per_head(x.astype(np.float64), heads)[row] + ye                   # exact: the sum of two fp32 numbers
    sl = np.where(u > 0, 1.0, float(ns))
    v = sl * u
    att3 = att.astype(np.float64).reshape(1, heads, K // heads)
    s = (att3 * v).sum(2)
    deg = np.diff(rowptr)
    smax = np.full((m, heads), -np.inf)
    np.maximum.at(smax, row, s)
    live = (deg > 0)[:, None]
    shift = np.where(live, smax, 0.0)
    w = np.exp(s - shift[row])
    lse = np.where(live, shift + np.log(np.maximum(segment_sum(w, row, m), 1e-300)), -np.inf)
    a = np.exp(s - np.where(live, lse, 0.0)[row])
    out = dict(row=row, u=u, sl=sl, v=v, s=s, a=a, lse=lse, z=segment_sum(a[:, :, None] * ye, row, m).reshape(m, K))
    if g is not None:
        g3 = per_head(g.astype(np.float64), heads)
        D = (g3 * per_head(out["z"], heads)).sum(2)
        t = (g3[row] * ye).sum(2)
        ds = a * (t - D[row])
        q = ds[:, :, None] * att3 * sl
        out.update(D=D, t=t, ds=ds, dx=segment_sum(q, row, m).reshape(m, K),
                   dy=segment_sum(a[:, :, None] * g3[row] + q, col, n).reshape(n, K), datt=(ds[:, :, None] * v).sum(0))
    return out


def bounds(rowptr, col, x, y, att, heads, ns, ref, g=None):
    """The per-element bound on |fp32 result - ref| (ref = gatv2(...) of the same operands): attention_ref.bounds taken per head.
    rho, lse [m, H]; z [m, K]; with g also D [m, H], dx [m, K], dy [n, K], datt [H, d].

        delta s_e    = 1e-5 sum_c |att_c v_ec|                         the project's SDDMM rule
        rho[i,h]     = max_e delta s_e + 8 eps (R + deg_i + 4)         R: the score range of row i, head h
        z[i,c]       = (1e-5 + 2 rho[i,h]) sum_e a_e |y_jc| + 1e-30
        lse[i,h]     = rho[i,h] + 1e-5 + 2 eps |lse[i,h]|
        rhob_e       = delta s_e + lse[i,h] + 8 eps (1 + |s_e - lse[i,h]|)
        eta_e        = a_e (rhob_e |t_e - D[i,h]| + 1e-5 (sum_c |g_ic y_jc|_h + sum_c |g_ic z_ic|_h))
        carry_e      = eta_e + 1e-5 |ds_e|
        dx[i,c]      = sum_e carry_e |att_c| |sl_ec| + 1e-30
        dy[j,c]      = sum_{e->j} ((rhob_e + 1e-5) a_e |g_ic| + carry_e |att_c| |sl_ec|) + 1e-30
        datt[c]      = sum_{all e} (carry_e + 1e-5 |ds_e|) |v_ec| + 1e-30
        D[i,h]       = sum_c |g_ic| z[i,c] + 1e-5 sum_c |g_ic z_ic|_h + 1e-30
    """
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row, s, a = ref["row"], ref["s"], ref["a"]
    ye = np.abs(per_head(y.astype(np.float64), heads))[col]
    att3 = np.abs(att.astype(np.float64)).reshape(1, heads, K // heads)
    dscore = ACC * (att3 * np.abs(ref["v"])).sum(2)
    deg = np.diff(rowptr).astype(np.float64)
    hi, lo, dmax = np.full((m, heads), -np.inf), np.full((m, heads), np.inf), np.zeros((m, heads))
    np.maximum.at(hi, row, s)
    np.minimum.at(lo, row, s)
    np.maximum.at(dmax, row, dscore)
    live = (deg > 0)[:, None]
    rng = np.where(live, hi - np.where(live, lo, 0.0), 0.0)
    rho = dmax + C_EXP * EPS * (rng + deg[:, None] + 4.0)
    lse0 = np.where(live, ref["lse"], 0.0)
    zb = ((ACC + 2.0 * rho)[:, :, None] * segment_sum(a[:, :, None] * ye, row, m)).reshape(m, K) + 1e-30
    out = dict(rho=rho, z=zb, lse=np.where(live, rho + ACC + 2.0 * EPS * np.abs(lse0), 0.0))
    if g is not None:
        g3 = np.abs(per_head(g.astype(np.float64), heads))
        ge = g3[row]
        rhob = dscore + out["lse"][row] + C_EXP * EPS * (1.0 + np.abs(s - lse0[row]))
        gz = (g3 * np.abs(per_head(ref["z"], heads))).sum(2)
        eta = a * (rhob * np.abs(ref["t"] - ref["D"][row]) + ACC * ((ge * ye).sum(2) + gz[row]))
        ads = np.abs(ref["ds"])
        carry = eta + ACC * ads
        qb = carry[:, :, None] * att3 * np.abs(ref["sl"])
        out.update(dx=segment_sum(qb, row, m).reshape(m, K) + 1e-30,
                   dy=segment_sum(((rhob + ACC) * a)[:, :, None] * ge + qb, col, n).reshape(n, K) + 1e-30,
                   datt=((carry + ACC * ads)[:, :, None] * np.abs(ref["v"])).sum(0) + 1e-30,
                   D=(g3 * per_head(zb, heads)).sum(2) + ACC * gz + 1e-30)
    return out
