"""The per-element error bound the 16-bit GAT entries (include/isplib_hip.h: isplib_gat16_csr_hip and its two backward entries;
DESIGN.md 4.6e) are held to.  The reference is tests/gat_ref.py's `gat` (fp64) on the WIDENED 16-bit operands (the scores are fp32
as they are); B32 = gat_ref.bounds(...) of the same operands is what an fp32 implementation may miss it by, and this module adds

  * what the rows kernel pays for forming D[i,h] itself, in fp32, from the row's own edges instead of <g_i, z_i>_h, and for the
    subtraction P - D Q of its one-pass form (sl_e = u_e > 0 ? 1 : |ns|):
        dD[i,h]          = sum_e a_e (rhob_e |t_e - D[i,h]| + 1e-5 sum_c |g_ic y_jc|_h)
        bound_D[i,h]     = dD[i,h] + 1e-5 |D[i,h]|
        bound_dadst[i,h] = B32.dadst[i,h] + sum_e a_e sl_e dD[i,h] + 1e-5 (sum_e a_e sl_e |t_e| + |D[i,h]| sum_e a_e sl_e)
        bound_dasrc[j,h] = B32.dasrc[j,h] + sum_{e->j} a_e sl_e dD[i,h]
  * the ONE rounding of z and dy to the operand's dtype (u: its unit roundoff; sub: half the spacing of fp16's subnormals):
        bound(v)         = pre + u (|ref| + pre) + sub            pre = B32.v for v in z, dy (dy carries nothing from D)
    lse stays fp32 and keeps B32.lse.

rhob_e is gat_ref's.  No further term was needed: the fp32 emulation of tests/test_gat16_host.py passes on every case.  The bound is
a worst-case statement; half an ulp of the one rounding is most of z's and dy's, so their largest observed error / bound is expected
near 1.
"""
import numpy as np

from tests import gat_ref as ref
from tests import half_ref
from tests.attention16_ref import SUB


def bounds16(rowptr, col, y, a_dst, a_src, heads, ns, r, b32, g, dtype):
    """y, g: the widened operands (fp32 arrays); r = gat_ref.gat(...) and b32 = gat_ref.bounds(...) of them.
    -> dict: rho, lse, D, dadst [m, H]; dasrc [n, H]; z [m, K]; dy [n, K]."""
    m, n = rowptr.size - 1, y.shape[0]
    row, u_e, s, a = r["row"], r["u"], r["s"], r["a"]
    u, sub = half_ref.UNIT_ROUNDOFF[dtype], SUB[dtype]
    ye = np.abs(ref.per_head(y.astype(np.float64), heads))[col]
    ge = np.abs(ref.per_head(g.astype(np.float64), heads))[row]
    live = (np.diff(rowptr) > 0)[:, None]
    lse0 = np.where(live, r["lse"], 0.0)
    rhob = 2.0 * ref.EPS * np.abs(u_e) + b32["lse"][row] + ref.C_EXP * ref.EPS * (1.0 + np.abs(s - lse0[row]))
    dD = ref.segment_sum(a * (rhob * np.abs(r["t"] - r["D"][row]) + ref.ACC * (ge * ye).sum(2)), row, m)
    asl = a * np.where(u_e > 0, 1.0, abs(float(ns)))
    canc = ref.ACC * (ref.segment_sum(asl * np.abs(r["t"]), row, m) + np.abs(r["D"]) * ref.segment_sum(asl, row, m))
    out = {name: b32[name] + u * (np.abs(r[name]) + b32[name]) + sub for name in ("z", "dy")}
    out.update(rho=b32["rho"], lse=b32["lse"], D=dD + ref.ACC * np.abs(r["D"]),        # 0 on an empty row: D is compared for equality there
               dadst=b32["dadst"] + ref.segment_sum(asl, row, m) * dD + canc, dasrc=b32["dasrc"] + ref.segment_sum(asl * dD[row], col, n))
    return out
