"""The per-element error bound the 16-bit attention entries (include/isplib_hip.h: isplib_attention16_csr_hip and its two backward
entries) are held to.  The reference is tests/attention_ref.py's `attention` (fp64) on the WIDENED 16-bit operands;
B32 = attention_ref.bounds(...) of the same operands is what an fp32 implementation may miss it by, and this module adds

  * what the rows kernel pays for forming D_i itself, in fp32, from the row's own edges instead of <g_i, z_i>:
        dD_i        = sum_e a_e (rhob_e |t_e - D_i| + 1e-5 sum_c |g_ic y_jc|)
        canc[i,c]   = 1e-5 (sum_e a_e |t_e| |y_jc| + |D_i| sum_e a_e |y_jc|)          the subtraction A1 - D Z of the one-pass form
        pre_dx[i,c] = B32.dx[i,c] + |p| (dD_i sum_e a_e |y_jc| + canc[i,c])
        pre_dy[j,c] = B32.dy[j,c] + |p| sum_{e->j} a_e dD_i |x_ic|
  * the ONE rounding of z, dx and dy to the operands' dtype (u: its unit roundoff; sub: half the spacing of fp16's subnormals):
        bound(v)    = pre + u (|ref| + pre) + sub            pre = B32.z for z
    lse and D stay fp32: lse keeps B32.lse, D is held to dD_i + 1e-5 |D_i|.

rhob_e is attention_ref's.  The bound is a worst-case statement; half an ulp of the one rounding is most of it, so the largest observed
error / bound is expected near 1.
"""
import numpy as np
import torch

from tests import attention_ref as ref
from tests import half_ref

SUB = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}


def bounds16(rowptr, col, x, y, p, r, b32, g, dtype):
    """x, y, g: the widened operands (fp32 arrays); r = attention_ref.attention(...) and b32 = attention_ref.bounds(...) of them.
    -> dict: rho [m], z [m, k], lse [m], dx [m, k], dy [n, k], D [m]."""
    m, n = rowptr.size - 1, y.shape[0]
    row, s, a = r["row"], r["s"], r["a"]
    ap = abs(float(p))
    u, sub = half_ref.UNIT_ROUNDOFF[dtype], SUB[dtype]
    xe, ye, ge = (np.abs(v.astype(np.float64)) for v in (x[row], y[col], g[row]))
    live = np.diff(rowptr) > 0
    lse0 = np.where(live, r["lse"], 0.0)
    dscore = ref.ACC * ap * (xe * ye).sum(1)
    rhob = dscore + b32["lse"][row] + ref.C_EXP * ref.EPS * (1.0 + np.abs(s - lse0[row]))
    dD = ref.segment_sum(a * (rhob * np.abs(r["t"] - r["D"][row]) + ref.ACC * (ge * ye).sum(1)), row, m)
    ay = ref.segment_sum(a[:, None] * ye, row, m)
    canc = ref.ACC * (ref.segment_sum((a * np.abs(r["t"]))[:, None] * ye, row, m) + np.abs(r["D"])[:, None] * ay)
    pre = dict(z=b32["z"], dx=b32["dx"] + ap * (dD[:, None] * ay + canc),
               dy=b32["dy"] + ap * ref.segment_sum((a * dD[row])[:, None] * xe, col, n))
    out = {name: v + u * (np.abs(r[name]) + v) + sub for name, v in pre.items()}
    out.update(rho=b32["rho"], lse=b32["lse"], D=dD + ref.ACC * np.abs(r["D"]))        # 0 on an empty row: D is compared for equality there
    return out
