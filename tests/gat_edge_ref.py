"""The GAT attention aggregation with a per-edge score term (include/isplib_hip.h: isplib_gat_edge_csr_hip and its two backward entries)
stated in vectorised NumPy, fp64, per edge and per head -- the yardstick of tests/test_gat_edge_host.py and tests/test_gpu_gat_edge.py
-- and the per-element error bound a fp32 implementation is held to.  tests/gat_ref.py with one more operand:

    u_e = (a_dst[i,h] + a_src[j,h]) + a_edge[e,h]        a_edge [nnz, H], one row per stored entry in CSR position order
    s_e, a_e, lse, z, D, t_e, ds_e, du_e, d a_dst, d a_src, dy as in tests/gat_ref.py            d a_edge[e,h] = du_e

Everything is fp64 EXCEPT the slope branch of every edge and head, which is taken on the float32 value the kernels form,
float32(float32(a_dst[i] + a_src[j]) + a_edge[e]): with three terms the sign of the fp32 sum is no longer the sign of the exact sum, and
the operator's contract is that branch.  The value of s is continuous across the kink, so a branch that differs from the exact sign
moves s by at most max(1, |ns|) times the rounding error of u, which the bound's score term covers.
"""
import numpy as np

from tests.attention_ref import ACC, C_EXP, EPS, RHO_MAX, edge_rows, segment_sum, worst  # noqa: F401  (one set of constants)
from tests.gat_ref import per_head  # noqa: F401


def branch(a_dst, a_src, a_edge, row, col):
    """u_e > 0 on the fp32 value the kernels compute: two fp32 adds in the contract's order.  -> bool [nnz, H]"""
    f32 = np.float32
    u32 = (a_dst.astype(f32)[row] + a_src.astype(f32)[col]).astype(f32)
    return (u32 + a_edge.astype(f32)).astype(f32) > 0


def gat_edge(rowptr, col, y, a_dst, a_src, a_edge, heads, ns, g=None):
    """-> dict of fp64 arrays: z [m, K], lse [m, H]; with g also D [m, H], dadst [m, H], dasrc [n, H], dy [n, K], daedge [nnz, H]; and
    the per-edge parts row, u0 (= a_dst + a_src), u, pos (the fp32 branch), s, a, t, ds, du, each [nnz, H]."""
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row = edge_rows(rowptr)
    a_edge = a_edge.reshape(col.size, heads)
    ye = per_head(y.astype(np.float64), heads)[col]                       # [nnz, H, d]
    u0 = a_dst.astype(np.float64)[row] + a_src.astype(np.float64)[col]    # exact: the sum of two fp32 numbers
    u = u0 + a_edge.astype(np.float64)
    pos = branch(a_dst, a_src, a_edge, row, col)
    s = np.where(pos, u, float(ns) * u)
    deg = np.diff(rowptr)
    smax = np.full((m, heads), -np.inf)
    np.maximum.at(smax, row, s)
    live = (deg > 0)[:, None]
    shift = np.where(live, smax, 0.0)
    w = np.exp(s - shift[row])
    lse = np.where(live, shift + np.log(np.maximum(segment_sum(w, row, m), 1e-300)), -np.inf)
    a = np.exp(s - np.where(live, lse, 0.0)[row])
    out = dict(row=row, u0=u0, u=u, pos=pos, s=s, a=a, lse=lse, z=segment_sum(a[:, :, None] * ye, row, m).reshape(m, K))
    if g is not None:
        g3 = per_head(g.astype(np.float64), heads)
        D = (g3 * per_head(out["z"], heads)).sum(2)
        t = (g3[row] * ye).sum(2)
        ds = a * (t - D[row])
        du = ds * np.where(pos, 1.0, float(ns))
        out.update(D=D, t=t, ds=ds, du=du, dadst=segment_sum(du, row, m), dasrc=segment_sum(du, col, n), daedge=du,
                   dy=segment_sum(a[:, :, None] * g3[row], col, n).reshape(n, K))
    return out


def bounds(rowptr, col, y, a_dst, a_src, a_edge, heads, ns, ref, g=None):
    """The per-element bound on |fp32 result - ref| (ref = gat_edge(...) of the same operands): tests/gat_ref.bounds with two changes.

        delta s_e    = max(1, |ns|) (eps |a_dst + a_src| + 2 eps |u_e|)               two adds and one multiply; a branch that differs
                                                                                      from the exact sign is inside this term
        daedge[e,h]  = sl_e (eta_e + 1e-5 |ds_e|) + 1e-30                             the single-edge term of the dadst sum

    and rho, z, lse, rhob, eta, dadst, dasrc, dy, D exactly as there (the constants are those of tests/attention_ref.py).
    """
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row, u, s, a = ref["row"], ref["u"], ref["s"], ref["a"]
    ye = np.abs(per_head(y.astype(np.float64), heads))[col]
    dscore = max(1.0, abs(float(ns))) * (EPS * np.abs(ref["u0"]) + 2.0 * EPS * np.abs(u))
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
        carry = np.where(ref["pos"], 1.0, abs(float(ns))) * (eta + ACC * np.abs(ref["ds"]))
        out.update(dadst=segment_sum(carry, row, m) + 1e-30, dasrc=segment_sum(carry, col, n) + 1e-30, daedge=carry + 1e-30,
                   dy=segment_sum(((rhob + ACC) * a)[:, :, None] * ge, col, n).reshape(n, K) + 1e-30,
                   D=(g3 * per_head(zb, heads)).sum(2) + ACC * gz + 1e-30)
    return out
