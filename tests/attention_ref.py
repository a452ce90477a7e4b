"""The row-softmax attention aggregation (include/isplib_hip.h: isplib_attention_csr_hip and its two backward entries) stated in
vectorised NumPy, fp64, per edge -- the yardstick of tests/test_attention_host.py and tests/test_gpu_attention.py (the reference project
has no such operator) -- and the per-element error bound a fp32 implementation is held to.

For the stored entries e = (i, j) of a CSR structure, x [m, k], y [n, k], a scalar p and g = dL/dz:
    s_e = p <x_i, y_j>      a_e = exp(s_e - lse_i),  lse_i = log sum_e exp(s_e)      z_i = sum_e a_e y_j        (empty row: 0, -inf)
    D_i = <g_i, z_i>        t_e = <g_i, y_j>         ds_e = a_e (t_e - D_i)
    dx_i = p sum_e ds_e y_j                          dy_j = sum_{e -> j} (a_e g_i + p ds_e x_i)
"""
import numpy as np

EPS = 2.0 ** -24          # unit roundoff of fp32
C_EXP = 8.0               # C_f of `exp` in DESIGN.md 4.6a: |__expf(s) - exp(s)| <= C_f eps (1 + |s|) exp(s)
ACC = 1e-5                # the accumulation rule of BASELINE.md section 3 and the project's SDDMM rule
RHO_MAX = 1e-3            # the bound is first order in rho


def edge_rows(rowptr):
    return np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))


def segment_sum(values, ids, count):
    out = np.zeros((count,) + values.shape[1:])
    np.add.at(out, ids, values)
    return out


def attention(rowptr, col, x, y, p, g=None):
    """-> dict of fp64 arrays: z [m, k], lse [m]; with g also dx [m, k], dy [n, k], D [m]; and the per-edge parts row, s, a, t, ds."""
    m, n = rowptr.size - 1, y.shape[0]
    row = edge_rows(rowptr)
    xe, ye = x[row].astype(np.float64), y[col].astype(np.float64)
    s = float(p) * (xe * ye).sum(1)
    deg = np.diff(rowptr)
    smax = np.full(m, -np.inf)
    np.maximum.at(smax, row, s)
    shift = np.where(deg > 0, smax, 0.0)
    w = np.exp(s - shift[row])
    lse = np.where(deg > 0, shift + np.log(np.maximum(segment_sum(w, row, m), 1e-300)), -np.inf)
    a = np.exp(s - np.where(deg > 0, lse, 0.0)[row])
    out = dict(row=row, s=s, a=a, lse=lse, z=segment_sum(a[:, None] * ye, row, m))
    if g is not None:
        g64 = g.astype(np.float64)
        D = (g64 * out["z"]).sum(1)
        t = (g64[row] * ye).sum(1)
        ds = a * (t - D[row])
        out.update(D=D, t=t, ds=ds, dx=float(p) * segment_sum(ds[:, None] * ye, row, m),
                   dy=segment_sum(a[:, None] * g64[row] + (float(p) * ds)[:, None] * xe, col, n))
    return out


def bounds(rowptr, col, x, y, p, ref, g=None):
    """The per-element bound on |fp32 result - ref| (ref = attention(...) of the same operands), as a dict: rho [m], z [m, k],
    lse [m] (0 for an empty row: -inf is compared for equality); with g also dx [m, k] and dy [n, k].

        ds_e  (delta s) = 1e-5 |p| sum_c |x_ic y_jc|                                  the project's SDDMM rule
        rho_i           = max_e delta s_e + 8 eps (R_i + deg_i + 4)                   R_i: the row's score range; 8 = C_f of exp; one
                                                                                      factor per possible rescale of a slot
        z[i,c]          = (1e-5 + 2 rho_i) sum_e a_e |y_jc| + 1e-30
        lse[i]          = rho_i + 1e-5 + 2 eps |lse_i|
        rhob_e          = delta s_e + lse[i] + 8 eps (1 + |s_e - lse_i|)
        eta_e           = a_e (rhob_e |t_e - D_i| + 1e-5 (sum_c |g_ic y_jc| + sum_c |g_ic z_ic|))
        dx[i,c]         = |p| sum_e (eta_e + 1e-5 |ds_e|) |y_jc| + 1e-30
        dy[j,c]         = sum_{e->j} ((rhob_e + 1e-5) a_e |g_ic| + |p| (eta_e + 1e-5 |ds_e|) |x_ic|) + 1e-30
    """
    m, n = rowptr.size - 1, y.shape[0]
    row, s, a = ref["row"], ref["s"], ref["a"]
    ap = abs(float(p))
    xe, ye = np.abs(x[row].astype(np.float64)), np.abs(y[col].astype(np.float64))
    dscore = ACC * ap * (xe * ye).sum(1)
    deg = np.diff(rowptr).astype(np.float64)
    hi, lo, dmax = np.full(m, -np.inf), np.full(m, np.inf), np.zeros(m)
    np.maximum.at(hi, row, s)
    np.minimum.at(lo, row, s)
    np.maximum.at(dmax, row, dscore)
    live = deg > 0
    rng = np.where(live, hi - np.where(live, lo, 0.0), 0.0)
    rho = dmax + C_EXP * EPS * (rng + deg + 4.0)
    lse0 = np.where(live, ref["lse"], 0.0)
    out = dict(rho=rho, z=(ACC + 2.0 * rho)[:, None] * segment_sum(a[:, None] * ye, row, m) + 1e-30,
               lse=np.where(live, rho + ACC + 2.0 * EPS * np.abs(lse0), 0.0))
    if g is not None:
        ge = np.abs(g[row].astype(np.float64))
        rhob = dscore + out["lse"][row] + C_EXP * EPS * (1.0 + np.abs(s - lse0[row]))
        gz = (np.abs(g.astype(np.float64)) * np.abs(ref["z"])).sum(1)
        eta = a * (rhob * np.abs(ref["t"] - ref["D"][row]) + ACC * ((ge * ye).sum(1) + gz[row]))
        carry = eta + ACC * np.abs(ref["ds"])
        out.update(dx=ap * segment_sum(carry[:, None] * ye, row, m) + 1e-30,
                   dy=segment_sum(((rhob + ACC) * a)[:, None] * ge + (ap * carry)[:, None] * xe, col, n) + 1e-30)
    return out


def worst(got, want, bound):
    """The largest error / bound over the elements (NaN or Inf in `got` where `want` is finite counts as infinite)."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    err = np.where(np.isfinite(got), err, np.inf)
    return float((err / bound).max()) if err.size else 0.0
