"""NumPy statements of the two kernels of the owner-bucketed max / min backward (include/isplib_hip.h:
isplib_minmax_bw_bucket_hip, isplib_scatter_keys_det_hip), shared by the host and the GPU tests of the exchange."""
import numpy as np


def bucket_pairs(arg, edge0, col, val, grad_out, cuts):
    """(keys uint32, vals float32, seg_off int64[world + 1]): owner p's pairs are [seg_off[p], seg_off[p + 1]), each segment in
    ascending t = i * k + c (a stable split); the value is the float32 product val[a] * grad_out[i, c]."""
    arg, grad_out, col = np.asarray(arg, np.int64), np.asarray(grad_out, np.float32), np.asarray(col, np.int64)
    cuts = np.asarray(cuts, np.int64)
    world = cuts.size - 1
    m, k = arg.shape
    a = arg.reshape(-1) - int(edge0)
    ok = (a >= 0) & (a < col.size)
    at = np.where(ok, a, 0)
    d = col[at] if col.size else np.zeros(a.size, np.int64)
    ok &= (d >= cuts[0]) & (d < cuts[world])
    owner = np.minimum(np.searchsorted(cuts[1:], d, side="right"), world - 1)
    key = (d - cuts[owner]) * k + np.arange(m * k, dtype=np.int64) % max(k, 1)
    g = grad_out.reshape(-1)
    v = g.copy() if val is None else (np.asarray(val, np.float32)[at] if col.size else np.zeros(a.size, np.float32)) * g
    owner, key, v = owner[ok], key[ok], v[ok].astype(np.float32)
    order = np.argsort(owner, kind="stable")
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(owner, minlength=world))]).astype(np.int64)
    return key[order].astype(np.uint32), v[order], seg_off


def scatter_keys(keys, vals, n, k):
    """grad[key // k, key % k] = sum of vals over equal keys in the order given (np.add.at adds in that order); keys >= n * k
    are ignored."""
    keys, vals = np.asarray(keys).astype(np.uint32).astype(np.int64), np.asarray(vals, np.float32)
    out = np.zeros(n * k, np.float32)
    mine = keys < n * k
    np.add.at(out, keys[mine], vals[mine])
    return out.reshape(n, k)
