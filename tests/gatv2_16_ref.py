"""The per-element error bound the 16-bit GATv2 entries (include/isplib_hip_gatv2_16.h: isplib_gatv2_16_csr_hip and its two backward entries;
DESIGN.md 4.6g) are held to.  The reference is tests/gatv2_ref.py's `gatv2` (fp64) on the WIDENED 16-bit operands (att is fp32 as it
is); B32 = gatv2_ref.bounds(...) of the same operands is what an fp32 implementation may miss it by, and this module adds

  * what the rows kernel pays for forming D[i,h] itself, in fp32, from the row's own edges instead of <g_i, z_i>_h, and for the
    subtractions P_c - D Q_c and R_c - D S_c of its one-pass form (|sl_ec| = u_ec > 0 ? 1 : |ns|):
        dD[i,h]       = sum_e a_e (rhob_e |t_e - D[i,h]| + 1e-5 sum_c |g_ic y_jc|_h)
        bound_D[i,h]  = dD[i,h] + 1e-5 |D[i,h]|
        pre_dx[i,c]   = B32.dx[i,c] + |att_c| (dD[i,h] sum_e a_e |sl_ec| + 1e-5 (sum_e a_e |sl_ec| |t_e| + |D[i,h]| sum_e a_e |sl_ec|))
        pre_dy[j,c]   = B32.dy[j,c] + sum_{e->j} a_e |att_c| |sl_ec| dD[i,h]
        bound_datt[c] = B32.datt[c] + sum_e a_e |v_ec| dD[i,h] + 1e-5 sum_e a_e |v_ec| (|t_e| + |D[i,h]|)
  * the ONE rounding of z, dx and dy to the operands' dtype (u: its unit roundoff; sub: half the spacing of fp16's subnormals):
        bound(v)      = pre + u (|ref| + pre) + sub            pre = B32.z for z, pre_dx, pre_dy
    lse stays fp32 and keeps B32.lse.

rhob_e is gatv2_ref's.  No further term was needed: the fp32 emulation of tests/test_gatv2_16_host.py, in the kernels' own form, passes
on every case.  The bound is a worst-case statement; half an ulp of the one rounding is most of z's, dx's and dy's, so their largest
observed error / bound is expected near 1.
"""
import numpy as np

from tests import gatv2_ref as ref
from tests import half_ref
from tests.attention16_ref import SUB
from tests.gat_ref import per_head


def bounds16(rowptr, col, x, y, att, heads, ns, r, b32, g, dtype):
    """x, y, g: the widened operands (fp32 arrays); r = gatv2_ref.gatv2(...) and b32 = gatv2_ref.bounds(...) of them.
    -> dict: rho, lse, D [m, H]; z, dx [m, K]; dy [n, K]; datt [H, d]."""
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row, s, a, t, D = r["row"], r["s"], r["a"], r["t"], r["D"]
    u, sub = half_ref.UNIT_ROUNDOFF[dtype], SUB[dtype]
    ye = np.abs(per_head(y.astype(np.float64), heads))[col]
    ge = np.abs(per_head(g.astype(np.float64), heads))[row]
    att3 = np.abs(att.astype(np.float64)).reshape(1, heads, K // heads)
    live = (np.diff(rowptr) > 0)[:, None]
    lse0 = np.where(live, r["lse"], 0.0)
    dscore = ref.ACC * (att3 * np.abs(r["v"])).sum(2)
    rhob = dscore + b32["lse"][row] + ref.C_EXP * ref.EPS * (1.0 + np.abs(s - lse0[row]))
    dD = ref.segment_sum(a * (rhob * np.abs(t - D[row]) + ref.ACC * (ge * ye).sum(2)), row, m)              # [m, H]
    asl = a[:, :, None] * np.abs(r["sl"])                                                                   # [nnz, H, d]
    sum_asl = ref.segment_sum(asl, row, m)                                                                  # [m, H, d]
    canc = ref.ACC * (ref.segment_sum(asl * np.abs(t)[:, :, None], row, m) + np.abs(D)[:, :, None] * sum_asl)
    pre_dx = b32["dx"] + (att3 * (dD[:, :, None] * sum_asl + canc)).reshape(m, K)
    pre_dy = b32["dy"] + ref.segment_sum(asl * att3 * dD[row][:, :, None], col, n).reshape(n, K)
    av = a[:, :, None] * np.abs(r["v"])
    datt = b32["datt"] + (av * dD[row][:, :, None]).sum(0) + ref.ACC * (av * (np.abs(t) + np.abs(D)[row])[:, :, None]).sum(0)
    out = dict(rho=b32["rho"], lse=b32["lse"], D=dD + ref.ACC * np.abs(D), datt=datt)      # D: 0 on an empty row, compared for equality
    for name, pre in (("z", b32["z"]), ("dx", pre_dx), ("dy", pre_dy)):
        out[name] = pre + u * (np.abs(r[name]) + pre) + sub
    return out
