"""The GATv2 attention aggregation with attention dropout (include/isplib_hip.h: isplib_gatv2_drop_csr_hip and its two backward entries)
stated in vectorised NumPy, fp64 -- the yardstick of tests/test_gatv2_dropout_host.py and tests/test_gpu_gatv2_dropout.py -- and the
per-element error bound a fp32 implementation is held to.  tests/gatv2_ref.py with a keep bit q_e,h in {0, 1} per stored
entry and head and c = float32(1 / (1 - p)); r_ec is what gatv2_ref calls q_ec:

    u_ec, sl_ec, v_ec, s_e, a_e, lse   exactly as without dropout: the softmax runs over ALL stored entries
    z_i[head h]  = c sum_e q_e a_e y_j[head h]            D[i,h] = <g_i, z_i>_h
    t_e          = q_e c <g_i, y_j>_h                     ds_e = a_e (t_e - D[i,h])      r_ec = ds_e att_c sl_ec
    dx_ic        = sum_e r_ec                             dy_jc = sum_{e -> j} (q_e c a_e g_ic + r_ec)
    datt_c       = sum_{all e} ds_e v_ec

The keep bit is the one of the GAT dropout, tests/gat_dropout_ref.keep (the library states it in isplib_amd/csrc/gat_dropout.h); q is
exact and c is the float32 value, everything else is fp64.
"""
import numpy as np

from tests import gatv2_ref
from tests.attention_ref import ACC, C_EXP, EPS, RHO_MAX, edge_rows, segment_sum, worst  # noqa: F401  (one set of constants)
from tests.gat_dropout_ref import keep, scale, threshold  # noqa: F401
from tests.gat_ref import per_head  # noqa: F401


def gatv2_drop(rowptr, col, x, y, att, heads, ns, p, seed, g=None, fwd=None, q=None):
    """-> the dict of gatv2_ref.gatv2 with z, D, t, ds, dx, dy, datt those of the function above, and q (bool [nnz, H]), c (float), qc
    (= q c, fp64 [nnz, H]).  `fwd`: the reference of the same operands without dropout -- row, u, sl, v, s, a and lse do not depend on
    the mask and are taken from it.  `q`: a mask to use in place of keep(seed, ...) (the cases' counter-examples)."""
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    if fwd is None:
        fwd = gatv2_ref.gatv2(rowptr, col, x, y, att, heads, ns)
    out = {name: fwd[name] for name in ("row", "u", "sl", "v", "s", "a", "lse")}
    row, a, sl, v = out["row"], out["a"], out["sl"], out["v"]
    if q is None:
        q = keep(seed, col.size, heads, p)
    c = float(scale(p))
    qc = q.astype(np.float64) * c
    ye = per_head(y.astype(np.float64), heads)[col]                       # [nnz, H, d]
    out.update(q=q, c=c, qc=qc, z=segment_sum((qc * a)[:, :, None] * ye, row, m).reshape(m, K))
    if g is not None:
        att3 = att.astype(np.float64).reshape(1, heads, K // heads)
        g3 = per_head(g.astype(np.float64), heads)
        D = (g3 * per_head(out["z"], heads)).sum(2)
        t = qc * (g3[row] * ye).sum(2)
        ds = a * (t - D[row])
        r = ds[:, :, None] * att3 * sl
        out.update(D=D, t=t, ds=ds, dx=segment_sum(r, row, m).reshape(m, K),
                   dy=segment_sum((qc * a)[:, :, None] * g3[row] + r, col, n).reshape(n, K), datt=(ds[:, :, None] * v).sum(0))
    return out


def bounds(rowptr, col, x, y, att, heads, ns, ref, g=None):
    """The per-element bound on |fp32 result - ref| (ref = gatv2_drop(...) of the same operands): gatv2_ref.bounds with the mask carried
    through, by the substitutions DESIGN.md 4.6i made for GAT.  No new constants.

    The forward accumulates sum_e q_e w_e y_j beside the unmasked l = sum_e w_e and writes c (acc / l): each kept term carries the
    relative error of its a_e (2 rho) and of the accumulation (1e-5), a dropped term is an exact zero, and the final multiply by c adds
    one rounding of the result.  So q_e c a_e replaces a_e in the value sum, and eps |z| is added:

        delta s_e, rho, lse, rhob_e                                       unchanged: the softmax does not see the mask
        z[i,c]       = (1e-5 + 2 rho[i,h]) sum_e q_e c a_e |y_jc| + eps |z_ic| + 1e-30

    The backward forms t_e = (q_e c) <g_i, y_j>_h: the dot product's accumulation error (1e-5 sum_c |g_ic y_jc|) is scaled by q_e c, and
    the rounding of that one multiply, eps q_e c |<g_i, y_j>|, lies inside the same term (eps << 1e-5).  So q_e c goes inside t, in the
    value and in the accumulation term; D's bound is formed from the new z:

        eta_e        = a_e (rhob_e |t_e - D[i,h]| + 1e-5 (q_e c sum_c |g_ic y_jc|_h + sum_c |g_ic z_ic|_h))
        carry_e      = eta_e + 1e-5 |ds_e|
        dx[i,c]      = sum_e carry_e |att_c| |sl_ec| + 1e-30
        datt[c]      = sum_{all e} (carry_e + 1e-5 |ds_e|) |v_ec| + 1e-30
        D[i,h]       = sum_c |g_ic| z[i,c] + 1e-5 sum_c |g_ic z_ic|_h + 1e-30

    dy mixes a masked term with an unmasked one, so c cannot multiply the finished row: the columns kernel forms the value coefficient
    q_e ? a_e c : 0 per edge and head -- one more rounding, eps, on the coefficient whose relative error was rhob_e + 1e-5:

        dy[j,c]      = sum_{e->j} ((rhob_e + 1e-5 + eps) q_e c a_e |g_ic| + carry_e |att_c| |sl_ec|) + 1e-30
    """
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row, s, a, qc = ref["row"], ref["s"], ref["a"], ref["qc"]
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
    zb = ((ACC + 2.0 * rho)[:, :, None] * segment_sum((qc * a)[:, :, None] * ye, row, m)).reshape(m, K) + EPS * np.abs(ref["z"]) + 1e-30
    out = dict(rho=rho, z=zb, lse=np.where(live, rho + ACC + 2.0 * EPS * np.abs(lse0), 0.0))
    if g is not None:
        g3 = np.abs(per_head(g.astype(np.float64), heads))
        ge = g3[row]
        rhob = dscore + out["lse"][row] + C_EXP * EPS * (1.0 + np.abs(s - lse0[row]))
        gz = (g3 * np.abs(per_head(ref["z"], heads))).sum(2)
        eta = a * (rhob * np.abs(ref["t"] - ref["D"][row]) + ACC * (qc * (ge * ye).sum(2) + gz[row]))
        ads = np.abs(ref["ds"])
        carry = eta + ACC * ads
        rb = carry[:, :, None] * att3 * np.abs(ref["sl"])
        out.update(dx=segment_sum(rb, row, m).reshape(m, K) + 1e-30,
                   dy=segment_sum(((rhob + ACC + EPS) * qc * a)[:, :, None] * ge + rb, col, n).reshape(n, K) + 1e-30,
                   datt=((carry + ACC * ads)[:, :, None] * np.abs(ref["v"])).sum(0) + 1e-30,
                   D=(g3 * per_head(zb, heads)).sum(2) + ACC * gz + 1e-30)
    return out
