"""CPU tests of the owner-bucketed exchange of the partitioned max / min backward (ISPLIB_DIST_MINMAX_BW=owner): the cabi
wrappers refuse bad operands before any library call, the Python mirror of the domain predicate agrees with the header's, and
the exchange itself -- over gloo, with NumPy statements of the two kernels in their place -- gives every rank exactly what the
all-gathered form gives it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import owner_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_exchange_wrappers_refuse_bad_operands_before_any_library_call(monkeypatch):
    """minmax_bw_bucket hands the kernel an [m, k] arg / grad_out pair, col / val of one length and world + 1 ascending cuts;
    scatter_keys_det as many keys as values.  Everything else is a ValueError raised before the library is touched (it is
    stubbed so that any call fails); well-formed host tensors get as far as the device check, which refuses them too."""
    from isplib_amd import cabi

    class LibraryCalled(Exception):
        pass

    def no_library(*a, **k):
        raise LibraryCalled()
    monkeypatch.setattr(cabi, "lib", no_library)
    m, k, nnz = 6, 8, 10
    arg = torch.zeros((m, k), dtype=torch.int64)
    g = torch.ones((m, k))
    col = torch.zeros(nnz, dtype=torch.int64)
    val = torch.ones(nnz)
    cuts = [0, 3, 5]
    good = dict(arg=arg, edge0=0, col=col, val=val, grad_out=g, cuts=cuts)
    bad = {
        "arg dtype": dict(arg=arg.to(torch.int32)),
        "arg 1-D": dict(arg=arg.reshape(-1)),
        "arg 3-D": dict(arg=arg[None]),
        "arg strided": dict(arg=torch.zeros((m, 2 * k), dtype=torch.int64)[:, ::2]),
        "grad dtype": dict(grad_out=g.double()),
        "grad shape": dict(grad_out=torch.ones((m + 1, k))),
        "grad width": dict(grad_out=torch.ones((m, k + 1))),
        "grad strided": dict(grad_out=torch.ones((k, m)).t()),
        "grad 1-D": dict(grad_out=torch.ones(m * k)),
        "col dtype": dict(col=col.to(torch.int32)),
        "col 2-D": dict(col=col[None]),
        "col strided": dict(col=torch.zeros(2 * nnz, dtype=torch.int64)[::2]),
        "val length": dict(val=torch.ones(nnz + 1)),
        "val dtype": dict(val=val.double()),
        "val strided": dict(val=torch.ones(2 * nnz)[::2]),
        "cuts descend": dict(cuts=[0, 5, 3]),
        "cuts too short": dict(cuts=[0]),
        "cuts too many": dict(cuts=list(range(cabi.OWNER_WORLD_MAX + 2))),
        "keys of an owner": dict(cuts=[0, 2 ** 32 // k]),                      # rows * k + 1 == 2^32: one past the last served
    }
    for name, change in bad.items():
        with pytest.raises(ValueError):
            cabi.minmax_bw_bucket(**dict(good, **change))
    big = cabi.MINMAX_BW_PAIRS_END // 2                                          # m * k at the first refused pair count (meta: nothing allocated)
    with pytest.raises(ValueError, match="owner exchange"):
        cabi.minmax_bw_bucket(torch.empty((big, 2), dtype=torch.int64, device="meta"), 0, col, val,
                              torch.empty((big, 2), dtype=torch.float32, device="meta"), cuts)
    out = (torch.zeros(m * k, dtype=torch.int32), torch.zeros(m * k), torch.zeros(3, dtype=torch.int64))
    for name, wrong in {"keys dtype": (out[0].long(), out[1], out[2]), "short vals": (out[0], out[1][:-1], out[2]),
                        "seg_off length": (out[0], out[1], torch.zeros(4, dtype=torch.int64))}.items():
        with pytest.raises(ValueError):
            cabi.minmax_bw_bucket(**good, out=wrong)
    with pytest.raises(ValueError, match="GPU tensor"):                          # well-formed: on to the device check
        cabi.minmax_bw_bucket(**good)
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.minmax_bw_bucket(**dict(good, val=None), out=out)

    keys, vals = torch.zeros(12, dtype=torch.int32), torch.ones(12)
    for name, (kk, vv, n_, k_) in {"count": (keys, vals[:-1], 3, 4), "keys dtype": (keys.long(), vals, 3, 4), "vals dtype": (keys, vals.double(), 3, 4),
                                   "keys 2-D": (keys.view(3, 4), vals, 3, 4), "strided": (torch.zeros(24, dtype=torch.int32)[::2], vals, 3, 4),
                                   "negative n": (keys, vals, -1, 4), "n * k": (keys, vals, 2 ** 32 // 4, 4)}.items():
        with pytest.raises(ValueError):
            cabi.scatter_keys_det(kk, vv, n_, k_)
    with pytest.raises(ValueError, match="`out`"):
        cabi.scatter_keys_det(keys, vals, 3, 4, out=torch.zeros((4, 3)))
    with pytest.raises(ValueError, match="GPU tensor"):
        cabi.scatter_keys_det(keys, vals, 3, 4)


_PREDICATE_SRC = r"""
#include "isplib_hip.h"
extern "C" int owner_serves(long long m, long long k, int world, const long long *cuts) {
   return isplib_owner_exchange_serves(m, k, world, (const int64_t *)cuts);
}
extern "C" int product_within(long long rows, long long k, unsigned long long most) { return isplib_product_within(rows, k, most); }
"""


def test_owner_exchange_domain_mirror_agrees_with_the_header(tmp_path):
    """isplib_owner_exchange_serves (include/isplib_hip.h, a static inline: compiled here into a scrap library) against
    cabi.owner_exchange_serves at and around every edge: world 1 / 64 / 65 / 0, m * k at the last served and first refused pair
    count, an owner's rows * k + 1 at 2^32 - 1, 2^32 and past it, descending cuts, an empty shard; the limits' values; and
    the workspace queries of the library refuse what the predicate refuses."""
    from isplib_amd import cabi
    src, so = tmp_path / "pred.cpp", tmp_path / "pred.so"
    src.write_text(_PREDICATE_SRC)
    subprocess.run(["g++", "-shared", "-fPIC", "-O1", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True, timeout=120)
    L = ctypes.CDLL(str(so))
    L.owner_serves.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)]

    def header(m, k, world, cuts):
        return bool(L.owner_serves(m, k, world, (ctypes.c_longlong * len(cuts))(*cuts)))
    assert (cabi.MINMAX_BW_PAIRS_END, cabi.MINMAX_BW_KEYS_MAX, cabi.OWNER_WORLD_MAX) == (2 ** 32 - 2, 2 ** 32 - 2, 64)
    text = open(os.path.join(ROOT, "include", "isplib_hip.h")).read()
    for name, value in (("MINMAX_BW_PAIRS_END", "0xFFFFFFFEu"), ("MINMAX_BW_KEYS_MAX", "0xFFFFFFFEu"), ("OWNER_WORLD_MAX", "64")):
        assert f"#define ISPLIB_{name} " in " ".join(text.split()) and f"ISPLIB_{name} {value}" in " ".join(text.split()), name
    end = cabi.MINMAX_BW_PAIRS_END
    cases_ = []
    for world in (0, 1, 2, 63, 64, 65):
        cases_.append((10, 8, world, list(range(0, 5 * (max(world, 0) + 1), 5))))
    for k in (1, 2, 7, 64):                                                       # m * k around the pair limit
        for m in ((end - 1) // k, (end - 1) // k + 1, end // k + 1):
            cases_.append((m, k, 2, [0, 5, 9]))
    for k in (1, 3, 64, 4096):                                                    # an owner's rows * k + 1 around 2^32
        rows = (2 ** 32 - 2) // k
        for r in (rows - 1, rows, rows + 1):
            cases_ += [(4, k, 1, [0, r]), (4, k, 3, [7, 7, 7 + r, 7 + r + 2]), (4, k, 2, [0, 1, 1 + r])]
    cases_ += [(4, 8, 2, [0, 5, 3]), (4, 8, 2, [3, 3, 3]), (0, 8, 2, [0, 1, 2]), (4, 0, 2, [0, 1, 2]), (-1, 8, 1, [0, 1]), (4, -1, 1, [0, 1])]
    seen = set()
    for m, k, world, cuts in cases_:
        want = header(m, k, world, cuts) if 1 <= world <= 64 else False          # (the header loop reads cuts[world]: only asked in range)
        got = cabi.owner_exchange_serves(m, k, world, cuts)
        assert got == want, (m, k, world, cuts[:4], got, want)
        seen.add(got)
    assert seen == {True, False}
    assert header(end // 2 - 1, 2, 1, [0, 1]) and not header(end // 2, 2, 1, [0, 1])          # the pair limit itself, spelled out
    assert header(1, 1, 1, [0, 2 ** 32 - 2]) and not header(1, 1, 1, [0, 2 ** 32 - 1])        # rows * k + 1 < 2^32
    lib = cabi.lib()
    assert lib.isplib_minmax_bw_bucket_workspace_bytes(0, 8, 2) == 256
    assert lib.isplib_minmax_bw_bucket_workspace_bytes(end // 2, 2, 2) == 0 and lib.isplib_minmax_bw_bucket_workspace_bytes(10, 8, 65) == 0
    assert lib.isplib_minmax_bw_bucket_workspace_bytes(10, 8, 0) == 0
    assert lib.isplib_scatter_keys_workspace_bytes(end, 4, 4) == 0 and lib.isplib_scatter_keys_workspace_bytes(16, 2 ** 30, 4) == 0
    assert lib.isplib_scatter_keys_workspace_bytes(0, 4, 4) == 256
    assert cabi.scatter_keys_serves(end - 1, (2 ** 32 - 2) // 4, 4) and not cabi.scatter_keys_serves(end, 4, 4)
    assert not cabi.scatter_keys_serves(4, (2 ** 32 - 2) // 4 + 1, 4)


def test_numpy_statements_of_the_two_kernels_compose_to_the_oracle_backward():
    """The reference the other tests lean on, checked once against the oracle: bucket_pairs for one owner (world 1) followed by
    scatter_keys is the max / min backward's grad_mat, exactly (integer data: every sum is exact)."""
    import oracle
    from tests import cases
    rowptr, col = cases.random_csr(97, 97, 11.0, seed=5, empty_rows=(0, 50), hub=(3, 400))
    val = cases.weights(col.size, 4, "signed_int")
    x, g = cases.dense(97, 24, 3, "integer"), cases.dense(97, 24, 7, "integer")
    _, arg = oracle.spmm_fw(rowptr, col, val, x, "max")
    _, want = oracle.spmm_minmax_bw(col, val, x, arg, g)
    keys, vals, seg = owner_ref.bucket_pairs(arg, 0, col, val, g, [0, 97])
    assert seg.tolist() == [0, int((arg != col.size).sum())] and keys.size == seg[-1]
    assert np.array_equal(owner_ref.scatter_keys(keys, vals, 97, 24), want)
    # three owners, one of them empty: segments ascend in t, keys are local to the owner
    keys, vals, seg = owner_ref.bucket_pairs(arg, 0, col, val, g, [0, 40, 40, 97])
    assert seg[1] == seg[2] and seg[-1] == keys.size
    got = np.concatenate([owner_ref.scatter_keys(keys[seg[p]:seg[p + 1]], vals[seg[p]:seg[p + 1]], n_, 24)
                          for p, n_ in enumerate((40, 0, 57))])
    assert np.array_equal(got, want)


_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
import oracle
from isplib_amd.dist import RowPartition
from tests import cases, owner_ref
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
t = torch.from_numpy
rowptr, col = cases.random_csr(97, 97, 11.0, seed=5, empty_rows=(0, 50), hub=(3, 400))
K = 24

# NumPy statements in place of the three local kernels
def scatter(dest, gval, lo, n_):
    d, g_ = dest.numpy().astype(np.int64) - lo, gval.numpy()
    out = np.zeros((n_, g_.shape[1]), np.float32)
    rows, cols = np.nonzero((dest.numpy() >= 0) & (d >= 0) & (d < n_))
    np.add.at(out, (d[rows, cols], cols), g_[rows, cols])
    return t(out)
calls = []
def bucket(arg, edge0, col_, val_, grad_out, cuts):
    keys, vals, seg = owner_ref.bucket_pairs(arg.numpy(), edge0, col_.numpy(), None if val_ is None else val_.numpy(), grad_out.numpy(), cuts)
    calls.append(np.diff(seg))
    return t(keys.view(np.int32).copy()), t(vals.copy()), t(seg.copy())
def scatter_keys(keys, vals, n_, k_):
    return t(owner_ref.scatter_keys(keys.numpy().view(np.uint32), vals.numpy(), n_, k_))
RowPartition.scatter_rows = staticmethod(scatter)
RowPartition.bucket_pairs = staticmethod(bucket)
RowPartition.scatter_keys = staticmethod(scatter_keys)

g = cases.dense(97, K, 7, "integer")
saw_empty_segment = False
for weighted in (True, False):
    # integer-valued weights (1..4) and gradients: every product and every sum is exact, so any order of the additions gives the same bits
    val = (np.floor(cases.weights(col.size, 4) * 4) + 1).astype(np.float32) if weighted else None
    w_ = val if weighted else np.ones(col.size, np.float32)
    part = RowPartition(t(rowptr), t(col), None if val is None else t(val), 97, rank, world)
    r0, r1 = part.row_cuts[rank], part.row_cuts[rank + 1]
    x0, x1 = part.x_cuts[rank], part.x_cuts[rank + 1]
    for red in ("max", "min"):
        for shunned in (False, True):
            x = cases.dense(97, K, 3, "integer")
            if shunned:      # rank 0's rows of x never win where a row has a choice: the other ranks have nothing to send it
                x[:part.x_cuts[1]] += -100.0 if red == "max" else 100.0
            ref, ref_arg = oracle.spmm_fw(rowptr, col, w_, x, red)
            _, want = oracle.spmm_minmax_bw(col, w_, x, ref_arg, g)
            got = {{}}
            for mode in ("gather", "owner"):
                os.environ["ISPLIB_DIST_MINMAX_BW"] = mode
                got[mode] = part.minmax_backward(t(ref_arg[r0:r1].copy()), t(g[r0:r1].copy())).numpy()
                assert got[mode].shape == (x1 - x0, K), (mode, got[mode].shape)
            assert np.array_equal(got["owner"], got["gather"]), (weighted, red, shunned)
            assert np.array_equal(got["owner"], want[x0:x1]) and np.array_equal(got["gather"], want[x0:x1]), (weighted, red, shunned)
            # the count matrix of this exchange, from the statement itself (every rank holds the whole graph here)
            matrix = np.stack([np.diff(owner_ref.bucket_pairs(ref_arg[part.row_cuts[p]:part.row_cuts[p + 1]], int(rowptr[part.row_cuts[p]]),
                                                               col[rowptr[part.row_cuts[p]]:rowptr[part.row_cuts[p + 1]]], None,
                                                               g[part.row_cuts[p]:part.row_cuts[p + 1]], part.x_cuts)[2]) for p in range(world)])
            assert np.array_equal(matrix[rank], calls[-1]), (matrix, calls[-1])
            assert matrix.sum() == (ref_arg != col.size).sum()
            off_diag = matrix[~np.eye(world, dtype=bool)]
            if shunned:
                assert (off_diag == 0).any(), ("expected an empty outgoing segment", matrix)
                saw_empty_segment = True
            assert (off_diag > 0).any()
assert saw_empty_segment
os.environ["ISPLIB_DIST_MINMAX_BW"] = "neither"
try:
    part.minmax_backward(t(ref_arg[r0:r1].copy()), t(g[r0:r1].copy()))
    raise SystemExit("an unknown ISPLIB_DIST_MINMAX_BW was accepted")
except ValueError as e:
    assert "ISPLIB_DIST_MINMAX_BW" in str(e)
# a local kernel failure on ONE rank: the exchange still completes on every rank (nobody is left in a receive), the failing
# rank raises afterwards and is told that it is still in step with its peers
os.environ["ISPLIB_DIST_MINMAX_BW"] = "owner"
for failing in ("bucket", "scatter"):
    if rank == 0:
        if failing == "bucket":
            part.fail_next_kernel = RuntimeError("injected")
        else:
            def boom(*a):
                raise RuntimeError("injected")
            RowPartition.scatter_keys = staticmethod(boom)
    try:
        out = part.minmax_backward(t(ref_arg[r0:r1].copy()), t(g[r0:r1].copy()))
        assert rank != 0
        if failing == "scatter":             # peers of a rank whose receive side failed are complete and right
            assert np.array_equal(out.numpy(), want[x0:x1])
    except RuntimeError as e:
        assert rank == 0 and "injected" in str(e) and getattr(e, "collectives_complete", False)
    RowPartition.scatter_keys = staticmethod(scatter_keys)
    dist.barrier()
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("world", (2, 3))
def test_owner_exchange_equals_the_all_gathered_backward_gloo(tmp_path, world):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29561 + world), WORLD_SIZE=str(world), OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
        assert f"rank {r} ok" in o


def test_owner_exchange_world1_runs_bucket_then_scatter_without_a_collective(monkeypatch):
    """world == 1: no process group exists here, so any collective would raise; the two hooks run back to back."""
    import oracle
    from isplib_amd.dist import RowPartition
    from tests import cases
    rowptr, col = cases.random_csr(97, 97, 11.0, seed=5, empty_rows=(0, 50), hub=(3, 400))
    val = cases.weights(col.size, 4, "signed_int")
    x, g = cases.dense(97, 24, 3, "integer"), cases.dense(97, 24, 7, "integer")
    t = torch.from_numpy

    def bucket(arg, edge0, col_, val_, grad_out, cuts):
        keys, vals, seg = owner_ref.bucket_pairs(arg.numpy(), edge0, col_.numpy(), val_.numpy(), grad_out.numpy(), cuts)
        return t(keys.view(np.int32).copy()), t(vals), t(seg)
    monkeypatch.setattr(RowPartition, "bucket_pairs", staticmethod(bucket))
    monkeypatch.setattr(RowPartition, "scatter_keys", staticmethod(
        lambda keys, vals, n_, k_: t(owner_ref.scatter_keys(keys.numpy().view(np.uint32), vals.numpy(), n_, k_))))
    monkeypatch.setenv("ISPLIB_DIST_MINMAX_BW", "owner")
    part = RowPartition(t(rowptr), t(col), t(val), 97, 0, 1)
    _, arg = oracle.spmm_fw(rowptr, col, val, x, "min")
    _, want = oracle.spmm_minmax_bw(col, val, x, arg, g)
    assert np.array_equal(part.minmax_backward(t(arg), t(g)).numpy(), want)
