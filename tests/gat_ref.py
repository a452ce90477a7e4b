"""The GAT attention aggregation (include/isplib_hip.h: isplib_gat_csr_hip and its two backward entries) stated in vectorised NumPy,
fp64, per edge and per head -- the yardstick of tests/test_gat_host.py and tests/test_gpu_gat.py (the reference project has no such
operator) -- and the per-element error bound a fp32 implementation is held to.

For the stored entries e = (i, j) of a CSR structure, y [n, H*d] (head h owns the columns [h*d, (h+1)*d)), a_dst [m, H], a_src [n, H],
a slope ns and g = dL/dz, for every head h:
    u_e = a_dst[i,h] + a_src[j,h]     s_e = u_e > 0 ? u_e : ns u_e
    a_e = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)       z_i[head h] = sum_e a_e y_j[head h]       (empty row: 0, -inf)
    D[i,h] = <g_i, z_i>_h             t_e = <g_i, y_j>_h            ds_e = a_e (t_e - D[i,h])     du_e = ds_e (u_e > 0 ? 1 : ns)
    d a_dst[i,h] = sum_e du_e         d a_src[j,h] = sum_{e->j} du_e                              dy_j[head h] = sum_{e->j} a_e g_i[head h]
"""
import numpy as np

from tests.attention_ref import ACC, C_EXP, EPS, RHO_MAX, edge_rows, segment_sum, worst  # noqa: F401  (one set of constants)


def per_head(a, heads):
    """[rows, H*d] -> [rows, H, d]"""
    return a.reshape(a.shape[0], heads, a.shape[1] // heads)


def gat(rowptr, col, y, a_dst, a_src, heads, ns, g=None):
    """-> dict of fp64 arrays: z [m, K], lse [m, H]; with g also D [m, H], dadst [m, H], dasrc [n, H], dy [n, K]; and the per-edge
    parts row, u, s, a, t, ds, du, each [nnz, H]."""
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row = edge_rows(rowptr)
    ye = per_head(y.astype(np.float64), heads)[col]                       # [nnz, H, d]
    u = a_dst.astype(np.float64)[row] + a_src.astype(np.float64)[col]     # exact: the sum of two fp32 numbers
    s = np.where(u > 0, u, float(ns) * u)
    deg = np.diff(rowptr)
    smax = np.full((m, heads), -np.inf)
    np.maximum.at(smax, row, s)
    live = (deg > 0)[:, None]
    shift = np.where(live, smax, 0.0)
    w = np.exp(s - shift[row])
    lse = np.where(live, shift + np.log(np.maximum(segment_sum(w, row, m), 1e-300)), -np.inf)
    a = np.exp(s - np.where(live, lse, 0.0)[row])
    out = dict(row=row, u=u, s=s, a=a, lse=lse, z=segment_sum(a[:, :, None] * ye, row, m).reshape(m, K))
    if g is not None:
        g3 = per_head(g.astype(np.float64), heads)
        D = (g3 * per_head(out["z"], heads)).sum(2)
        t = (g3[row] * ye).sum(2)
        ds = a * (t - D[row])
        du = ds * np.where(u > 0, 1.0, float(ns))
        out.update(D=D, t=t, ds=ds, du=du, dadst=segment_sum(du, row, m), dasrc=segment_sum(du, col, n),
                   dy=segment_sum(a[:, :, None] * g3[row], col, n).reshape(n, K))
    return out


def bounds(rowptr, col, y, a_dst, a_src, heads, ns, ref, g=None):
    """The per-element bound on |fp32 result - ref| (ref = gat(...) of the same operands): attention_ref.bounds taken per head, with the
    score term of a score that is one add and one multiply.  rho, lse [m, H]; z [m, K]; with g also D, dadst [m, H], dasrc [n, H],
    dy [n, K].

        delta s_e    = 2 eps |u_e|                                                    one add, one multiply
        rho[i,h]     = max_e delta s_e + 8 eps (R + deg_i + 4)                        R: the score range of row i, head h
        z[i,c]       = (1e-5 + 2 rho[i,h]) sum_e a_e |y_jc| + 1e-30
        lse[i,h]     = rho[i,h] + 1e-5 + 2 eps |lse[i,h]|
        rhob_e       = delta s_e + lse[i,h] + 8 eps (1 + |s_e - lse[i,h]|)
        eta_e        = a_e (rhob_e |t_e - D[i,h]| + 1e-5 (sum_c |g_ic y_jc|_h + sum_c |g_ic z_ic|_h))
        dadst[i,h]   = sum_e sl_e (eta_e + 1e-5 |ds_e|) + 1e-30,   sl_e = (u_e > 0 ? 1 : |ns|)
        dasrc[j,h]   = the same sum over e -> j
        dy[j,c]      = sum_{e->j} (rhob_e + 1e-5) a_e |g_ic| + 1e-30
        D[i,h]       = sum_c |g_ic| z[i,c] + 1e-5 sum_c |g_ic z_ic|_h + 1e-30         the dot product of g with the fp32 z: z's own
                                                                                      bound through |g|, and the accumulation rule
    """
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row, u, s, a = ref["row"], ref["u"], ref["s"], ref["a"]
    ye = np.abs(per_head(y.astype(np.float64), heads))[col]
    dscore = 2.0 * EPS * np.abs(u)
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
        carry = np.where(u > 0, 1.0, abs(float(ns))) * (eta + ACC * np.abs(ref["ds"]))
        out.update(dadst=segment_sum(carry, row, m) + 1e-30, dasrc=segment_sum(carry, col, n) + 1e-30,
                   dy=segment_sum(((rhob + ACC) * a)[:, :, None] * ge, col, n).reshape(n, K) + 1e-30,
                   D=(g3 * per_head(zb, heads)).sum(2) + ACC * gz + 1e-30)
    return out
