"""The per-element error bound the 16-bit multi-head attention entries with attention dropout (include/isplib_hip_mha16_drop.h:
isplib_qkv_half_drop_csr_hip and its two backward entries) are held to.  The reference is
tests/mha_dropout_ref.py's `mha_drop` (fp64) on the WIDENED 16-bit operands; B32 = mha_dropout_ref.bounds(...) of the same operands is
what an fp32 implementation may miss it by, and this module adds the two additions of tests/mha16_ref.bounds16 with the mask carried
through as mha_dropout_ref carries it -- q_e c inside t_e and inside t_e's accumulation term:

  * what the rows kernel pays for forming D[i,h] itself, in fp32, from the row's own edges (with the masked t_e) instead of
    <g_i, z_i>_h, and for the subtraction P_c - D Q_c of its one-pass form:
        dD[i,h]      = sum_e a_e (rhob_e |t_e - D[i,h]| + 1e-5 q_e c sum_c |g_ic v_jc|_h)          t_e = q_e c <g_i, v_j>_h
        bound_D[i,h] = dD[i,h] + 1e-5 |D[i,h]| + 1e-30        (B32.D's floor: a live (row, head) with every entry dropped has D = 0 exactly)
        pre_dq[i,c]  = B32.dq[i,c] + |p_s| (dD[i,h] sum_e a_e |k_jc| + 1e-5 (sum_e a_e |t_e| |k_jc| + |D[i,h]| sum_e a_e |k_jc|))
        pre_dk[j,c]  = B32.dk[j,c] + |p_s| sum_{e->j} a_e |q_ic| dD[i,h]
    The sums over a_e are unmasked, as l and Q_c are in the kernel: a dropped edge still carries -a_e D.
  * the ONE rounding of z, dq, dk and dv to the operands' dtype (u: its unit roundoff; sub: half the spacing of fp16's subnormals):
        bound(x)     = pre + u (|ref| + pre) + sub            pre = B32.z for z, pre_dq, pre_dk, B32.dv for dv
    lse stays fp32 and keeps B32.lse.

rhob_e is mha_dropout_ref's.  No new constants, and no further term was needed: the fp32 emulation of tests/test_mha16_dropout_host.py,
in the kernels' own form, passes on every case.  With every bit kept and c = 1 each line is the line of mha16_ref.bounds16 over a B32
that is never tighter than mha_ref.bounds.
"""
import numpy as np

from tests import half_ref
from tests import mha_dropout_ref as ref
from tests.attention16_ref import SUB
from tests.gat_ref import per_head


def bounds16(rowptr, col, q, k, v, heads, ps, r, b32, g, dtype):
    """q, k, v, g: the widened operands (fp32 arrays); r = mha_dropout_ref.mha_drop(...) and b32 = mha_dropout_ref.bounds(...) of them.
    -> dict: rho, lse, D [m, H]; z, dq [m, K]; dk, dv [n, K]."""
    m, n, K = rowptr.size - 1, k.shape[0], k.shape[1]
    row, s, a, t, D, qc = r["row"], r["s"], r["a"], r["t"], r["D"], r["qc"]
    u, sub, ap = half_ref.UNIT_ROUNDOFF[dtype], SUB[dtype], abs(float(ps))
    qe = np.abs(per_head(q.astype(np.float64), heads))[row]                                                 # [nnz, H, d]
    ke = np.abs(per_head(k.astype(np.float64), heads))[col]
    ve = np.abs(per_head(v.astype(np.float64), heads))[col]
    ge = np.abs(per_head(g.astype(np.float64), heads))[row]
    live = (np.diff(rowptr) > 0)[:, None]
    lse0 = np.where(live, r["lse"], 0.0)
    dscore = ref.ACC * ap * (qe * ke).sum(2)
    rhob = dscore + b32["lse"][row] + ref.C_EXP * ref.EPS * (1.0 + np.abs(s - lse0[row]))
    dD = ref.segment_sum(a * (rhob * np.abs(t - D[row]) + ref.ACC * qc * (ge * ve).sum(2)), row, m)          # [m, H]
    ak = a[:, :, None] * ke                                                                                 # [nnz, H, d]
    sum_ak = ref.segment_sum(ak, row, m)                                                                    # [m, H, d]
    canc = ref.ACC * (ref.segment_sum(ak * np.abs(t)[:, :, None], row, m) + np.abs(D)[:, :, None] * sum_ak)
    pre_dq = b32["dq"] + ap * (dD[:, :, None] * sum_ak + canc).reshape(m, K)
    pre_dk = b32["dk"] + ap * ref.segment_sum(a[:, :, None] * qe * dD[row][:, :, None], col, n).reshape(n, K)
    out = dict(rho=b32["rho"], lse=b32["lse"], D=dD + ref.ACC * np.abs(D) + 1e-30)         # 0 on an empty row, compared for equality
    for name, pre in (("z", b32["z"]), ("dq", pre_dq), ("dk", pre_dk), ("dv", b32["dv"])):
        out[name] = pre + u * (np.abs(r[name]) + pre) + sub
    return out
