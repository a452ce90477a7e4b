"""GPU tests of the owner-bucketed exchange of the partitioned max / min backward: the stable multi-way split
(isplib_minmax_bw_bucket_hip) against a NumPy statement of it, the receiver's half (isplib_scatter_keys_det_hip) bit for bit
against today's isplib_scatter_rows_det_hip, the whole exchange with the ranks emulated in one process, two real ranks sharing
the GPU over gloo, and both kernels in a captured graph."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cases, owner_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 2048                # BUCKET_TILE of isplib_amd/csrc/owner_exchange.hip: pairs per block
NO_WINNER = 1 << 40        # far past any edge0 + nnz


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_bucket(gpu, arg, edge0, col, val, g, cuts):
    """Two launches on one input: the same bytes, and exactly the NumPy statement's (values: the same float32 product)."""
    from isplib_amd import cabi
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    dev = [d(arg), d(col), d(val), d(g)]
    runs = []
    for _ in range(2):
        keys, vals, seg = cabi.minmax_bw_bucket(dev[0], edge0, dev[1], dev[2], dev[3], cuts)
        total = int(seg[-1])
        runs.append((seg.cpu().numpy(), keys[:total].cpu().numpy().view(np.uint32), vals[:total].cpu().numpy()))
    want_keys, want_vals, want_seg = owner_ref.bucket_pairs(arg, edge0, col, val, g, cuts)
    for seg, keys, vals in runs:
        assert np.array_equal(seg, want_seg), (seg, want_seg)
        assert np.array_equal(keys, want_keys)
        assert np.array_equal(_bits(vals), _bits(want_vals))
    return runs[0]


def _random_case(m, k, n, nnz, edge0, seed, weighted=True, none_share=0.1):
    rng = np.random.default_rng(seed)
    col = rng.integers(0, max(n, 1), nnz).astype(np.int64)
    val = (rng.random(nnz, np.float32) + 0.5).astype(np.float32) if weighted else None
    arg = rng.integers(edge0, edge0 + max(nnz, 1), (m, k)).astype(np.int64)
    arg[rng.random((m, k)) < none_share] = NO_WINNER
    g = (rng.random((m, k), np.float32) * 2 - 1).astype(np.float32)
    return arg, col, val, g


def _even_cuts(n, world):
    return [n * p // world for p in range(world + 1)]


@pytest.mark.parametrize("total", (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 17,
                                   TILE - 1, TILE, TILE + 1))
def test_bucket_kernel_at_the_edges_of_its_tile(gpu, total):
    """K = 1, rows = total pairs: one lane, one wave +- 1, one iteration of a block +- 1, one tile +- 1, several tiles and a
    ragged last one; three owners, a tenth of the pairs without a winner."""
    arg, col, val, g = _random_case(total, 1, 500, 700, 11, seed=total)
    _check_bucket(gpu, arg, 11, col, val, g, [0, 170, 330, 500])


@pytest.mark.parametrize("k", (4, 33, 64))
@pytest.mark.parametrize("world", (1, 2, 3, 8, 64))
def test_bucket_kernel_widths_and_world_sizes(gpu, k, world):
    """About 3,000 rows (several blocks at every K); keys are local to their owner: (row - cuts[p]) * k + feature."""
    n = 3001
    arg, col, val, g = _random_case(2999, k, n, 40_000, 123, seed=7 * k + world)
    seg, keys, _ = _check_bucket(gpu, arg, 123, col, val, g, _even_cuts(n, world))
    assert seg[-1] > 0 and all(int(keys[seg[p]:seg[p + 1]].max(initial=0)) < (n // world + 1) * k for p in range(world))


def test_bucket_kernel_cases(gpu):
    """Every pair to one owner; an owner with no pair; an empty shard; no winner anywhere; positions below edge0 and past
    edge0 + nnz; destinations outside [cuts[0], cuts[world]); m == 0; unit weights; edge0 > 0 and edge0 == 0; nnz == 0."""
    from isplib_amd import cabi
    m, k, n, nnz, edge0 = 700, 9, 400, 900, 37
    arg, col, val, g = _random_case(m, k, n, nnz, edge0, seed=1)
    seg, _, _ = _check_bucket(gpu, arg, edge0, np.full(nnz, 150, np.int64), val, g, [0, 100, 200, 300, 400])     # all to owner 1
    assert seg[1] == 0 and seg[2] == seg[-1] > 0
    lo_cols = np.where(col >= 300, col - 300, col)                                                                # owner 3 gets nothing
    seg, _, _ = _check_bucket(gpu, arg, edge0, lo_cols, val, g, [0, 100, 200, 300, 400])
    assert seg[3] == seg[4] and seg[3] > seg[2] > seg[1] > 0
    seg, _, _ = _check_bucket(gpu, arg, edge0, col, val, g, [0, 100, 100, 100, 400])                             # two empty shards
    assert seg[1] == seg[2] == seg[3] and 0 < seg[1] < seg[4]
    seg, _, _ = _check_bucket(gpu, np.full((m, k), NO_WINNER, np.int64), edge0, col, val, g, [0, 200, 400])      # no winner anywhere
    assert seg.tolist() == [0, 0, 0]
    wild = arg.copy()
    wild[::3] = edge0 - 1 - (np.arange(wild[::3].size).reshape(wild[::3].shape) % 50)                              # below edge0 (some negative)
    wild[1::3, ::2] = edge0 + nnz + (np.arange(wild[1::3, ::2].size).reshape(wild[1::3, ::2].shape) % 7)          # edge0 + nnz and past it
    seg, _, _ = _check_bucket(gpu, wild, edge0, col, val, g, [0, 200, 400])
    assert 0 < seg[-1] < m * k // 2
    seg, _, _ = _check_bucket(gpu, arg, edge0, col, val, g, [120, 200, 310])                                     # rows nobody here owns
    assert 0 < seg[-1] < m * k
    _check_bucket(gpu, arg, edge0, col, None, g, [0, 130, 400])                                                  # unit weights
    _check_bucket(gpu, arg - edge0, 0, col, val, g, [0, 130, 400])                                               # edge0 == 0
    seg, keys, vals = _check_bucket(gpu, np.zeros((0, k), np.int64), edge0, col, val, np.zeros((0, k), np.float32), [0, 130, 400])
    assert seg.tolist() == [0, 0, 0] and keys.size == 0
    seg, _, _ = _check_bucket(gpu, arg, edge0, np.zeros(0, np.int64), None, g, [0, 130, 400])                    # an empty graph
    assert seg.tolist() == [0, 0, 0]
    with pytest.raises(cabi.IsplibError) as info:                                                                # a short workspace is refused
        d = lambda a: torch.from_numpy(a).to(gpu)  # noqa: E731
        cabi.minmax_bw_bucket(d(arg), edge0, d(col), d(val), d(g), [0, 130, 400], workspace=torch.empty(256, dtype=torch.uint8, device=gpu))
    assert info.value.status == cabi.NOT_ENOUGH_MEM


def test_scatter_keys_equals_scatter_rows_bit_for_bit(gpu):
    """The in-range pairs of a destination array, in ascending t, through scatter_keys_det: the bits of
    scatter_rows_det(dest, gval, lo, n).  lo > 0; destination 5 of feature 0 wins in 9,000 rows (its run crosses 32-pair chunks
    and the 8,192-pair tile of the run sums), destination 6 of feature 1 in 40 consecutive rows placed to cross exactly one
    chunk border; keys >= n * k ride along and are ignored; non-integer gradients."""
    from isplib_amd import cabi
    m, k, lo, n = 12_000, 3, 100, 50
    rng = np.random.default_rng(3)
    dest = rng.integers(lo - 30, lo + n + 30, (m, k)).astype(np.int32)
    dest[rng.random((m, k)) < 0.05] = -1
    dest[dest == lo + 6] = lo + 7
    dest[:9000, 0] = lo + 5
    dest[5000:5040, 1] = lo + 6
    # the 40-pair run starts behind every smaller key; drop a few of those (no winner) until it begins at most 24 pairs into its chunk
    smaller = lambda: int(np.count_nonzero((dest >= lo) & (dest < lo + 6))) + int(np.count_nonzero(dest[:, 0] == lo + 6))  # noqa: E731
    tail_rows = 9000 + np.flatnonzero((dest[9000:, 0] >= lo) & (dest[9000:, 0] < lo + 5))
    dest[tail_rows[:max(smaller() % 32 - 24, 0)], 0] = -1
    assert smaller() % 32 <= 24
    gval = (rng.random((m, k), np.float32) * 2 - 1).astype(np.float32)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    want = cabi.scatter_rows_det(d(dest), d(gval), lo, n)
    flat, t = dest.reshape(-1).astype(np.int64), np.arange(m * k)
    mine = (flat >= lo) & (flat < lo + n)
    keys = ((flat - lo) * k + t % k)[mine].astype(np.uint32)
    vals = gval.reshape(-1)[mine]
    assert np.count_nonzero(keys == 5 * k) >= 9000 and np.count_nonzero(keys == 6 * k + 1) == 40
    order = np.argsort(keys, kind="stable")                                       # where the runs lie after the stable sort
    run = np.flatnonzero(keys[order] == 6 * k + 1)
    assert run[0] // 32 + 1 == run[-1] // 32, "the 40-pair run must cross exactly one chunk border"
    run = np.flatnonzero(keys[order] == 5 * k)
    assert run[-1] // 8192 > run[0] // 8192, "the hub run must cross a tile of the run sums"
    got = cabi.scatter_keys_det(d(keys.view(np.int32)), d(vals), n, k)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # (and, loosely, the NumPy statement's: a sum of N terms in another association differs by at most ~N * 2^-24 * sum |v|)
    bound = 2.0 ** -24 * np.bincount(keys, minlength=n * k) * np.bincount(keys, np.abs(vals), minlength=n * k)
    assert np.all(np.abs(got.cpu().numpy().reshape(-1) - owner_ref.scatter_keys(keys, vals, n, k).reshape(-1)) <= bound + 1e-30)
    # foreign keys (>= n * k, some with the low bits of real destinations) between the pairs: ignored, never written
    at = np.sort(rng.choice(keys.size, 500, replace=False))
    junk = np.concatenate([np.uint32(n * k) + (np.arange(250, dtype=np.uint32) % 4), np.uint32(1 << 20) + np.arange(250, dtype=np.uint32) % np.uint32(n * k)])
    keys2, vals2 = np.insert(keys, at, junk), np.insert(vals, at, np.float32(1e6))
    got = cabi.scatter_keys_det(d(keys2.view(np.int32)), d(vals2), n, k)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # nothing to add, nowhere to add it
    empty_k, empty_v = torch.empty(0, dtype=torch.int32, device=gpu), torch.empty(0, dtype=torch.float32, device=gpu)
    out = cabi.scatter_keys_det(empty_k, empty_v, n, k, out=torch.full((n, k), 7.0, device=gpu))
    assert out.shape == (n, k) and not bool(out.any())
    assert cabi.scatter_keys_det(d(keys.view(np.int32)), d(vals), 0, k).shape == (0, k)


@pytest.fixture(scope="module")
def dist_graph(oracle_mod):
    """The graph of tests/test_gpu_dist.py with the oracle's max / min winners and backward, weighted and unit; computed once."""
    n, k = 3000, 32
    rowptr, col = cases.random_csr(n, n, 90.0, seed=5, empty_rows=(0, 1500), hub=(7, 2900))
    x, g = cases.dense(n, k, 3), cases.dense(n, k, 5)
    ref = {}
    for weighted in (True, False):
        w = cases.weights(col.size, 4) if weighted else np.ones(col.size, np.float32)
        for red in ("max", "min"):
            _, arg = oracle_mod.spmm_fw(rowptr, col, w, x, red)
            ref[weighted, red] = (arg, oracle_mod.spmm_minmax_bw(col, w, x, arg, g)[1],
                                  oracle_mod.spmm_minmax_bw(col, np.abs(w), x, arg, np.abs(g))[1])
    return n, k, rowptr, col, cases.weights(col.size, 4), g, ref


@pytest.mark.parametrize("world", (2, 3, 8))
@pytest.mark.parametrize("weighted", (True, False))
def test_whole_exchange_with_emulated_ranks(gpu, dist_graph, world, weighted):
    """Every rank's bucket kernel, every owner's scatter over the senders' segments side by side in rank order -- no collective
    -- against scatter_rows_det over the arrays minmax_backward all-gathers today (bitwise) and the oracle (1e-5 * dmag)."""
    from isplib_amd import cabi
    from isplib_amd.dist import nnz_balanced_cuts
    n, k, rowptr, col, val, g, ref = dist_graph
    arg, dref, dmag = ref[weighted, "max"]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    cuts = nnz_balanced_cuts(torch.from_numpy(rowptr), world)
    pad = max(cuts[p + 1] - cuts[p] for p in range(world))
    col_d, val_d, arg_d, g_d = d(col), d(val) if weighted else None, d(arg), d(g)
    # today's exchange: destinations and weighted gradients of all rows, every shard padded to the longest
    ok = arg_d != col.size
    a = arg_d.clamp(0, col.size - 1)
    dest = torch.where(ok, col_d[a], col_d.new_full((), -1)).to(torch.int32)
    gval = torch.where(ok, g_d if val_d is None else val_d[a] * g_d, g_d.new_zeros(()))
    d_all = torch.full((world * pad, k), -1, dtype=torch.int32, device=gpu)
    g_all = torch.zeros((world * pad, k), dtype=torch.float32, device=gpu)
    for p in range(world):
        d_all[p * pad: p * pad + cuts[p + 1] - cuts[p]] = dest[cuts[p]:cuts[p + 1]]
        g_all[p * pad: p * pad + cuts[p + 1] - cuts[p]] = gval[cuts[p]:cuts[p + 1]]
    # the owner exchange: each sender's partition-local operands, exactly as RowPartition holds them
    sent = []
    for p in range(world):
        e0, e1 = int(rowptr[cuts[p]]), int(rowptr[cuts[p + 1]])
        keys, vals, seg = cabi.minmax_bw_bucket(arg_d[cuts[p]:cuts[p + 1]].contiguous(), e0, col_d[e0:e1].contiguous(),
                                                None if val_d is None else val_d[e0:e1].contiguous(), g_d[cuts[p]:cuts[p + 1]].contiguous(), cuts)
        sent.append((keys, vals, seg.cpu().tolist()))
    assert sum(s[2][-1] for s in sent) == int(ok.sum())
    for owner in range(world):
        r_keys = torch.cat([keys[seg[owner]:seg[owner + 1]] for keys, _, seg in sent])
        r_vals = torch.cat([vals[seg[owner]:seg[owner + 1]] for _, vals, seg in sent])
        rows = cuts[owner + 1] - cuts[owner]
        got = cabi.scatter_keys_det(r_keys, r_vals, rows, k)
        want = cabi.scatter_rows_det(d_all, g_all, cuts[owner], rows)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (world, weighted, owner)
        sl = slice(cuts[owner], cuts[owner + 1])
        assert np.all(np.abs(got.cpu().numpy() - dref[sl]) <= 1e-5 * dmag[sl] + 1e-30), (world, weighted, owner)


_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
import oracle
from isplib_amd.dist import DistGraph
from tests import cases
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
n, k = 3000, 32
rowptr, col = cases.random_csr(n, n, 90.0, seed=5, empty_rows=(0, 1500), hub=(7, 2900))
val = cases.weights(col.size, 4)
x, g = cases.dense(n, k, 3), cases.dense(n, k, 5)
t = lambda a: torch.from_numpy(a).to(dev)
for weighted in (True, False):
    w_ = val if weighted else np.ones(col.size, np.float32)
    graph = DistGraph(t(rowptr), t(col), t(val) if weighted else None, n, rank, world)
    r0, r1 = graph.row0, graph.row0 + graph.rows
    for red in ("max", "min"):
        grads = {{}}
        for mode in ("gather", "owner"):
            os.environ["ISPLIB_DIST_MINMAX_BW"] = mode
            xs = t(x[r0:r1].copy()).requires_grad_(True)
            graph.matmul(xs, red).backward(t(g[r0:r1].copy()))
            torch.cuda.synchronize()
            grads[mode] = xs.grad
        assert torch.equal(grads["owner"].view(torch.int32), grads["gather"].view(torch.int32)), (weighted, red)
        _, ref_arg = oracle.spmm_fw(rowptr, col, w_, x, red)
        dref = oracle.spmm_minmax_bw(col, w_, x, ref_arg, g)[1]
        dmag = oracle.spmm_minmax_bw(col, np.abs(w_), x, ref_arg, np.abs(g))[1]
        assert np.all(np.abs(grads["owner"].cpu().numpy() - dref[r0:r1]) <= 1e-5 * dmag[r0:r1] + 1e-30), (weighted, red)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_two_ranks_sharing_the_gpu_over_gloo(gpu, tmp_path):
    """DistGraph.matmul(x, red).backward(g), max and min, weighted and unit: x.grad under ISPLIB_DIST_MINMAX_BW=owner is bit for
    bit the all-gathered form's and within the bound of the oracle."""
    world = 2
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29567", WORLD_SIZE=str(world), OMP_NUM_THREADS="4")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o[-3000:]}"
        assert f"rank {r} ok" in o


def test_both_halves_capture_in_one_graph(gpu):
    """After a warm-up call, bucket + scatter on fixed buffers are captured (neither allocates or synchronises); the replay on new
    inputs reproduces the eager bytes.  One owner, and the key buffer pre-filled with an ignored key inside the graph, so that
    the scatter takes a fixed count whatever the number of winners."""
    from isplib_amd import cabi
    m, k, n, nnz = 1500, 16, 600, 5000
    inputs = [_random_case(m, k, n, nnz, 5, seed=s) for s in (1, 2)]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)  # noqa: E731
    arg, col, val, g = [d(a) for a in inputs[0]]
    keys = torch.empty(m * k, dtype=torch.int32, device=gpu)
    vals = torch.zeros(m * k, dtype=torch.float32, device=gpu)
    seg = torch.empty(2, dtype=torch.int64, device=gpu)
    out = torch.empty((n, k), dtype=torch.float32, device=gpu)
    lib = cabi.lib()
    ws_b = torch.empty(lib.isplib_minmax_bw_bucket_workspace_bytes(m, k, 1), dtype=torch.uint8, device=gpu)
    ws_s = torch.empty(lib.isplib_scatter_keys_workspace_bytes(m * k, n, k), dtype=torch.uint8, device=gpu)

    def step():
        keys.fill_(-1)
        cabi.minmax_bw_bucket(arg, 5, col, val, g, [0, n], out=(keys, vals, seg), workspace=ws_b)
        cabi.scatter_keys_det(keys, vals, n, k, out=out, workspace=ws_s)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                     # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for case in inputs[::-1]:
        for dst, src in zip((arg, col, val, g), case):
            dst.copy_(d(src))
        step()
        torch.cuda.synchronize()
        eager = (out.clone(), keys.clone(), seg.clone())
        out.fill_(float("nan"))
        keys.zero_()
        seg.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), eager[0].view(torch.int32)) and torch.equal(keys, eager[1]) and torch.equal(seg, eager[2])
        total = int(seg[-1])
        want_keys, want_vals, want_seg = owner_ref.bucket_pairs(case[0], 5, case[1], case[2], case[3], [0, n])
        assert total == want_seg[-1] and np.array_equal(keys[:total].cpu().numpy().view(np.uint32), want_keys)
        assert np.allclose(out.cpu().numpy(), owner_ref.scatter_keys(want_keys, want_vals, n, k), rtol=1e-5, atol=1e-5)
