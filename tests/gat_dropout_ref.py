"""The GAT attention aggregation with attention dropout (include/isplib_hip.h: isplib_gat_drop_csr_hip and its two backward entries)
stated in vectorised NumPy -- the yardstick of tests/test_gat_dropout_host.py and tests/test_gpu_gat_dropout.py -- and the per-element
error bound a fp32 implementation is held to.  tests/gat_edge_ref.py (a_edge = None: tests/gat_ref.py) with a keep bit
q_e,h in {0, 1} per stored entry and head and c = float32(1 / (1 - p)):

    u_e, s_e, a_e, lse      exactly as without dropout: the softmax runs over ALL stored entries
    z_i[head h]  = c sum_e q_e a_e y_j[head h]            D[i,h] = <g_i, z_i>_h
    t_e          = q_e c <g_i, y_j>_h                     ds_e = a_e (t_e - D[i,h])      du_e = ds_e slope_e
    d a_dst, d a_src, d a_edge: sums of du_e              dy_j[head h] = c sum_{e -> j} q_e a_e g_i[head h]

The keep bit is the contract's, restated here in NumPy uint32 arithmetic (the library's own statement is isplib_amd/csrc/gat_dropout.h):

    fmix32(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16
    word(seed, pos, h) = fmix32( fmix32(uint32(pos) ^ uint32(seed)) + uint32(h) * 0x9E3779B9 + uint32(seed >> 32) )
    T(p) = min(2^32 - 1, floor(p * 2^32))  in double      q = word >= T

q is exact and c is the float32 value; everything else is fp64 (and the slope branch that of the reference without dropout).
"""
import math

import numpy as np

from tests import gat_edge_ref, gat_ref
from tests.attention_ref import ACC, C_EXP, EPS, RHO_MAX, edge_rows, segment_sum, worst  # noqa: F401  (one set of constants)
from tests.gat_ref import per_head  # noqa: F401

GOLDEN = 0x9E3779B9


def fmix32(x):
    """Elementwise on a uint32 array (products wrap modulo 2^32)."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def word(seed, pos, head):
    """seed: a Python int in [0, 2^63) or an array of such; pos, head: ints or integer arrays; the three broadcast.  -> uint32 array"""
    seed = np.asarray(seed, dtype=np.uint64)
    pos = np.asarray(pos, dtype=np.int64).astype(np.uint64)
    head = np.asarray(head, dtype=np.int64).astype(np.uint64)
    low = np.uint64(0xFFFFFFFF)
    inner = fmix32(((pos ^ seed) & low).astype(np.uint32)).astype(np.uint64)
    total = inner + ((head & low) * np.uint64(GOLDEN) & low) + (seed >> np.uint64(32))        # below 2^34: no wrap in uint64
    return fmix32((total & low).astype(np.uint32))


def threshold(p):
    """T(p) as a Python int; p * 2^32 is exact in double (a power of two)."""
    return min(2 ** 32 - 1, max(0, int(math.floor(float(p) * 4294967296.0))))


def scale(p):
    return np.float32(1.0 / (1.0 - float(p)))


def keep(seed, nnz, heads, p):
    """-> bool [nnz, heads]: q of every stored entry (its CSR position) and head"""
    return word(int(seed), np.arange(nnz, dtype=np.int64)[:, None], np.arange(heads, dtype=np.int64)[None, :]) >= np.uint32(threshold(p))


def gat_drop(rowptr, col, y, a_dst, a_src, a_edge, heads, ns, p, seed, g=None, fwd=None):
    """-> the dict of gat_edge_ref.gat_edge (a_edge None: gat_ref.gat, with pos = u > 0 and u0 = u added) with z, D, t, ds, du and the
    gradients those of the function above, and q (bool [nnz, H]), c (float), qc (= q c, fp64 [nnz, H]).  `fwd`: the forward part already
    computed for the same operands (gat / gat_edge without or with g) -- a, lse, s, u do not depend on the mask."""
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    if fwd is None:
        fwd = (gat_ref.gat(rowptr, col, y, a_dst, a_src, heads, ns) if a_edge is None else
               gat_edge_ref.gat_edge(rowptr, col, y, a_dst, a_src, a_edge, heads, ns))
    out = {name: fwd[name] for name in ("row", "u", "s", "a", "lse")}
    out["pos"] = fwd["pos"] if "pos" in fwd else fwd["u"] > 0
    out["u0"] = fwd["u0"] if "u0" in fwd else fwd["u"]
    row, a = out["row"], out["a"]
    q = keep(seed, col.size, heads, p)
    c = float(scale(p))
    qc = q.astype(np.float64) * c
    ye = per_head(y.astype(np.float64), heads)[col]                       # [nnz, H, d]
    out.update(q=q, c=c, qc=qc, z=segment_sum((qc * a)[:, :, None] * ye, row, m).reshape(m, K))
    if g is not None:
        g3 = per_head(g.astype(np.float64), heads)
        D = (g3 * per_head(out["z"], heads)).sum(2)
        t = qc * (g3[row] * ye).sum(2)
        ds = a * (t - D[row])
        du = ds * np.where(out["pos"], 1.0, float(ns))
        out.update(D=D, t=t, ds=ds, du=du, dadst=segment_sum(du, row, m), dasrc=segment_sum(du, col, n), daedge=du,
                   dy=segment_sum((qc * a)[:, :, None] * g3[row], col, n).reshape(n, K))
    return out


def bounds(rowptr, col, y, a_dst, a_src, a_edge, heads, ns, ref, g=None):
    """The per-element bound on |fp32 result - ref| (ref = gat_drop(...) of the same operands): gat_edge_ref.bounds (a_edge None:
    gat_ref.bounds, whose score term is delta s_e = 2 eps |u_e|) with the mask carried through.

    The forward accumulates sum_e q_e w_e y_j beside the unmasked l = sum_e w_e and writes c (acc / l): each kept term carries the
    relative error of its a_e (2 rho) and of the accumulation (1e-5), a dropped term is an exact zero, and the final multiply by c adds
    one rounding of the result.  So q_e c a_e replaces a_e in the value sum, and eps |z| is added:

        z[i,c]       = (1e-5 + 2 rho[i,h]) sum_e q_e c a_e |y_jc| + eps |z_ic| + 1e-30
        lse, rho, rhob_e                                                  unchanged: the softmax does not see the mask

    The backward forms t_e = (q_e c) <g_i, y_j>_h: the dot product's accumulation error (1e-5 sum_c |g_ic y_jc|) is scaled by q_e c, and
    the rounding of that one multiply, eps q_e c |<g_i, y_j>|, lies inside the same term (eps << 1e-5).  So q_e c goes inside t, in the
    value and in the accumulation term, and D's bound is formed from the new z:

        eta_e        = a_e (rhob_e |t_e - D[i,h]| + 1e-5 (q_e c sum_c |g_ic y_jc|_h + sum_c |g_ic z_ic|_h))
        dadst, dasrc, daedge                                              from eta_e and ds_e as before
        dy[j,c]      = sum_{e->j} (rhob_e + 1e-5) q_e c a_e |g_ic| + eps |dy_jc| + 1e-30      c multiplies the finished row: one rounding
        D[i,h]       = sum_c |g_ic| z[i,c] + 1e-5 sum_c |g_ic z_ic|_h + 1e-30
    """
    m, n, K = rowptr.size - 1, y.shape[0], y.shape[1]
    row, u, s, a, qc = ref["row"], ref["u"], ref["s"], ref["a"], ref["qc"]
    ye = np.abs(per_head(y.astype(np.float64), heads))[col]
    if a_edge is None:
        dscore = 2.0 * EPS * np.abs(u)
    else:
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
    zb = ((ACC + 2.0 * rho)[:, :, None] * segment_sum((qc * a)[:, :, None] * ye, row, m)).reshape(m, K) + EPS * np.abs(ref["z"]) + 1e-30
    out = dict(rho=rho, z=zb, lse=np.where(live, rho + ACC + 2.0 * EPS * np.abs(lse0), 0.0))
    if g is not None:
        g3 = np.abs(per_head(g.astype(np.float64), heads))
        ge = g3[row]
        rhob = dscore + out["lse"][row] + C_EXP * EPS * (1.0 + np.abs(s - lse0[row]))
        gz = (g3 * np.abs(per_head(ref["z"], heads))).sum(2)
        eta = a * (rhob * np.abs(ref["t"] - ref["D"][row]) + ACC * (qc * (ge * ye).sum(2) + gz[row]))
        carry = np.where(ref["pos"], 1.0, abs(float(ns))) * (eta + ACC * np.abs(ref["ds"]))
        out.update(dadst=segment_sum(carry, row, m) + 1e-30, dasrc=segment_sum(carry, col, n) + 1e-30, daedge=carry + 1e-30,
                   dy=segment_sum(((rhob + ACC) * qc * a)[:, :, None] * ge, col, n).reshape(n, K) + EPS * np.abs(ref["dy"]) + 1e-30,
                   D=(g3 * per_head(zb, heads)).sum(2) + ACC * gz + 1e-30)
    return out
