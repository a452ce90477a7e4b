"""CPU tests of the host side (no GPU, no compute calls into the HIP library):
the C ABI library loads and exports every symbol include/isplib_hip.h declares,
the torch operator surface has the reference's names, CPU tensors are refused
loudly (no silent fallback), the plug-in patches/unpatches LIFO, and the 1-D row
partition is equivalent to the whole graph on a 2-rank gloo job.
"""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "isplib_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?(?:int|void|size_t|char)\s*\*?\s*(\w+)\s*\(", text, flags=re.M)
    return sorted(set(names))


def test_header_declares_expected_entry_points():
    names = _declared_functions()
    for must in ("fusedMM_csr_hip", "fusedMM_csr_sliced_hip", "performDummySpMM_hip", "isplib_spmm_minmax_bw_hip",
                 "isplib_sddmm_csr_hip", "isplib_csr2csc_hip", "isplib_spmm_slices_build_hip"):
        assert must in names


def test_cabi_library_exports_every_declared_symbol():
    from isplib_amd import _lib, cabi
    assert os.path.exists(_lib.CABI_PATH), "libisplib_hip.so not built (python -c 'import __graft_entry__ as g; g.build()')"
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.CABI_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = _declared_functions()
    missing = [n for n in declared if n not in exported]
    assert not missing, f"declared in include/isplib_hip.h but not exported: {missing}"
    assert sorted(cabi.EXPORTS) == declared, "isplib_amd.cabi.EXPORTS out of sync with the header"
    L = cabi.lib()
    for n in declared:
        getattr(L, n)
    assert L.isplib_hip_abi_version() == 1
    assert cabi.last_error() == ""


def test_experimental_library_exports_its_own_header_and_nothing_of_it_is_in_the_default_one():
    """include/isplib_hip_experimental.h <-> libisplib_hip_exp.so (the measured losers: sweep schedule, LDS hot-row hybrid,
    stream-plan SDDMM, their knobs): every declared symbol is exported there, none of them by the default library, and the
    default header declares none of them -- a binding of the reference's path never sees them."""
    import re
    from isplib_amd import _lib, cabi
    text = open(os.path.join(ROOT, "include", "isplib_hip_experimental.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"^\s*(?:const\s+)?(?:int|void|size_t|char)\s*\*?\s*(\w+)\s*\(", text, flags=re.M)))
    assert sorted(cabi.EXP_EXPORTS) == declared
    exp_path = os.path.join(os.path.dirname(_lib.CABI_PATH), "libisplib_hip_exp.so")
    assert os.path.exists(exp_path), "libisplib_hip_exp.so not built"
    sym = lambda path: {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", path], text=True).splitlines() if " T " in ln}  # noqa: E731
    assert not [n for n in declared if n not in sym(exp_path)]
    core = sym(_lib.CABI_PATH)
    assert not [n for n in declared if n in core], "an experimental entry is still exported by the default library"
    assert not set(declared) & set(_declared_functions())
    L = cabi.exp_lib()
    for n in declared:
        getattr(L, n)
    assert L.isplib_hip_tune_experimental(9, 64) == 0 and L.isplib_hip_tune_experimental(10, 1) == cabi.FAIL
    assert cabi.lib().isplib_hip_tune(9, 64) == cabi.FAIL, "knobs 9-12 left the default library"


def test_cabi_argument_validation_without_gpu():
    """Status codes that are decided before any HIP call."""
    from isplib_amd import cabi
    L = cabi.lib()
    st = L.fusedMM_csr_hip(0x11108, 1, 1, 1, 1.0, 0, 1, 1, None, None, None, None, None, 1, None, 1, 0.0, None, 1, None, None)
    assert st == cabi.NO_OPT_IMPL and "VOP" in cabi.last_error()          # a flag value the header does not define
    st = L.fusedMM_csr_hip(0x11F02, 1, 1, 1, 1.0, 0, 1, 1, None, None, None, None, None, 1, None, 1, 0.0, None, 1, None, None)
    assert st == cabi.UNDEFINED_USER_FUNCTION                             # SOP_UDEF through the entry without a menu
    st = L.fusedMM_csr_hip(cabi.MSG_SPMM_SUM, 1, 1, 1, 1.0, 0, 1, 1, None, None, None, None, None, 1, None, 1, 0.5, None, 1, None, None)
    assert st == cabi.FAIL and "beta" in cabi.last_error()
    st = L.fusedMM_csr_hip(cabi.MSG_SPMM_SUM, 0, 0, 4, 1.0, 0, 0, 0, None, None, None, None, None, 4, None, 4, 0.0, None, 4, None, None)
    assert st == cabi.SUCCESS            # m == 0: nothing to do
    st = L.fusedMM_csr_hip(cabi.MSG_SPMM_SUM, 2, 1 << 31, 4, 1.0, 0, 2, 2, None, None, None, None, None, 4, None, 4, 0.0, None, 4, None, None)
    assert st == cabi.FAIL and "2^31" in cabi.last_error()
    assert L.isplib_spmm_slices_bytes(10, 8) == 10 * 9 * 8
    assert L.isplib_spmm_sliced_workspace_bytes(cabi.MSG_SPMM_SUM, 10, 4, 8) >= 8 * 10 * 4 * 4
    assert L.isplib_spmm_sliced_workspace_bytes(cabi.MSG_SPMM_MAX, 10, 4, 8) >= 2 * 8 * 10 * 4 * 4


def test_torch_ops_have_reference_names_and_schemas():
    import isplib_amd  # noqa: F401
    ops = torch.ops.isplib
    s = str(ops.fusedmm_spmm.default._schema)
    assert "Tensor? row, Tensor rowptr, Tensor col, Tensor? value, Tensor? colptr, Tensor? csr2csc, Tensor mat" in s
    assert "value_index_select" in s and "row_index_select" in s
    s = str(ops.fusedmm_spmm_mean.default._schema)
    assert "Tensor? rowcount" in s and "new_row" in s and "new_rowcount" in s
    for name in ("fusedmm_spmm_max", "fusedmm_spmm_min"):
        s = str(getattr(ops, name).default._schema)
        assert "Tensor rowptr, Tensor col, Tensor? value, Tensor mat" in s and "-> (Tensor, Tensor)" in s
    assert "int flag" in str(ops.performDummySpMM.default._schema)
    for name in ("fusedmm_spmm_max_values", "fusedmm_spmm_min_values"):      # not the reference's: the plug-in's no-gradient path
        s = str(getattr(ops, name).default._schema)
        assert "Tensor rowptr, Tensor col, Tensor? value, Tensor mat, Tensor[] plan" in s and s.endswith("-> Tensor")


def test_cpu_tensors_are_refused_not_silently_served():
    import isplib_amd
    rowptr, col = torch.tensor([0, 1, 2]), torch.tensor([0, 1])
    x = torch.ones(2, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.isplib.fusedmm_spmm(None, rowptr, col, None, None, None, x, None, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.isplib.fusedmm_spmm_max(rowptr, col, None, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        torch.ops.isplib.fusedmm_spmm_max_values(rowptr, col, None, x, [])
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        isplib_amd.matmul(adj, x)
    with pytest.raises(ValueError, match="unknown reduce"):
        isplib_amd.matmul(adj, x, "prod")
    with pytest.raises(RuntimeError, match="no CPU path"):
        isplib_amd.cabi.spmm(rowptr, col, None, x)


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "isplib_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "fusedmm_oracle" not in text, f


def test_sparse_tensor_coo_to_csr_keeps_torch_sparse_order():
    import isplib_amd
    # README.md:105-110: duplicates (0,0) keep their input order (3 then -2)
    adj = isplib_amd.SparseTensor(row=torch.tensor([2, 0, 1, 0, 0]), col=torch.tensor([1, 0, 0, 2, 0]),
                                  value=torch.tensor([3., 3., 4., 2., -2.]), sparse_sizes=(3, 3))
    rowptr, col, val = adj.csr()
    e_rowptr, e_col, e_val, *_ = cases.readme_case()
    assert rowptr.tolist() == e_rowptr.tolist() and col.tolist() == e_col.tolist() and val.tolist() == e_val.tolist()
    assert adj.storage.rowcount().tolist() == [3, 1, 1]
    with pytest.raises(ValueError, match="out of range"):
        isplib_amd.SparseTensor(row=torch.tensor([0]), col=torch.tensor([5]), sparse_sizes=(2, 2))
    with pytest.raises(ValueError, match="monotone"):
        isplib_amd.SparseTensor(rowptr=torch.tensor([0, 2, 1]), col=torch.tensor([0]), sparse_sizes=(2, 2))


def test_patch_unpatch_is_lifo_and_restores(monkeypatch):
    import isplib_amd
    from isplib_amd import plugin
    fake_ts = types.SimpleNamespace(matmul=lambda *a, **k: "torch_sparse.matmul")
    fake_typing = types.SimpleNamespace(WITH_PT2=True, WITH_PT20=True)
    monkeypatch.setattr(plugin, "_torch_sparse", fake_ts)
    monkeypatch.setattr(plugin, "_pyg_typing", fake_typing)
    orig_ts, orig_mm = fake_ts.matmul, torch.sparse.mm
    assert not isplib_amd.iSpLibPlugin.is_patched()
    isplib_amd.iSpLibPlugin.patch_pyg()
    assert fake_ts.matmul is plugin.spmm_autotuned and torch.sparse.mm is not orig_mm
    assert fake_typing.WITH_PT2 is False and fake_typing.WITH_PT20 is False       # isplib/__init__.py:168-169
    isplib_amd.iSpLibPlugin.patch_pyg()                                            # nested
    isplib_amd.iSpLibPlugin.unpatch_pyg()
    assert fake_ts.matmul is plugin.spmm_autotuned                                 # still patched (LIFO)
    isplib_amd.iSpLibPlugin.unpatch_pyg()
    assert fake_ts.matmul is orig_ts and torch.sparse.mm is orig_mm
    assert fake_typing.WITH_PT2 is True and fake_typing.WITH_PT20 is True
    isplib_amd.iSpLibPlugin.unpatch_pyg()                                          # extra unpatch is a no-op (:190)

    @isplib_amd.isplib_autotune
    def inside():
        return fake_ts.matmul is plugin.spmm_autotuned

    assert inside() and fake_ts.matmul is orig_ts


def test_patched_sparse_mm_still_serves_torch_sparse_tensors():
    import isplib_amd
    a = torch.eye(3).to_sparse()
    isplib_amd.iSpLibPlugin.patch_pyg()
    try:
        out = torch.sparse.mm(a, torch.ones(3, 2))
    finally:
        isplib_amd.iSpLibPlugin.unpatch_pyg()
    assert torch.equal(out, torch.ones(3, 2))


def test_synthetic_graphs_have_dataset_shapes():
    from isplib_amd import synth
    rowptr, col, n = synth.dataset_like("cora")
    assert n == 2708 and col.numel() == 10556 and rowptr.numel() == n + 1
    deg = rowptr[1:] - rowptr[:-1]
    row = torch.repeat_interleave(torch.arange(n), deg)
    key = row * n + col
    assert bool((key[1:] > key[:-1]).all()), "rows / in-row columns must be sorted, no duplicates"
    assert torch.equal(torch.sort(col * n + row).values, key), "must be symmetric"
    assert bool((row != col).all())
    # B_alg of config 2
    assert synth.algorithmic_bytes(232965, 232965, 114615892, 128) == 1615810592


# ---- 1-D row partition, world_size 2 over gloo -----------------------------------------------

_WORKER = r"""
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch, torch.distributed as dist
import oracle
from isplib_amd.dist import RowPartition
from tests import cases
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
rowptr, col = cases.random_csr(97, 97, 11.0, seed=5, empty_rows=(0, 50), hub=(3, 400))
val = cases.weights(col.size, 4)
x = cases.dense(97, 24, 3, "integer")
t = torch.from_numpy
part = RowPartition(t(rowptr), t(col), t(val), 97, rank, world)
buf = part.gather_buffer(24)
part.all_gather(part.shard(t(x)), buf)                      # the ONE collective
assert torch.equal(part.unpad(buf), t(x))
for red in ("sum", "mean", "max", "min"):
    ref, ref_arg = oracle.spmm_fw(rowptr, col, val, x, red)
    # local SpMM of this rank's rows straight from the padded gather buffer (oracle stands in for the GPU kernel)
    out, arg = oracle.spmm_fw(part.rowptr.numpy(), part.col_padded.numpy(), part.val.numpy(), buf.numpy(), red)
    r0, r1 = part.row_cuts[rank], part.row_cuts[rank + 1]
    assert np.array_equal(out, ref[r0:r1]), red             # bit-identical to the single-device rows
    if arg is not None:
        garg = np.where(arg == part.nnz, part.total_nnz, arg + part.edge0)
        assert np.array_equal(garg, ref_arg[r0:r1]), red
# the direct per-peer exchange (P-1 send / receive pairs in 1, 2 or P-1 groups) fills the same buffer as the all-gather
want = buf.clone()
shard = part.shard(t(x))
for nb in sorted({{1, 2, max(world - 1, 1)}}):
    got = torch.full_like(buf, float("nan"))
    landed = set()
    for d0, d1, reqs in part.post_direct(shard, got, nb):
        for req in reqs:
            req.wait()
        landed.update((rank - d) % world for d in range(d0, d1))
    assert landed == set(range(world)) - {{rank}}
    got[rank * part.max_rows:(rank + 1) * part.max_rows] = shard
    assert torch.equal(got, want), nb
    dist.barrier()
sizes = [part.row_cuts[i + 1] - part.row_cuts[i] for i in range(world)]
assert sum(sizes) == 97
# the exchange of the max / min backward (RowPartition.minmax_backward: destinations + weighted gradients all-gathered in
# global row order, every rank keeps what lands in its own rows); the local kernel is replaced by a NumPy statement of it
def scatter(dest, gval, lo, n_):
    d, g_ = dest.numpy().astype(np.int64) - lo, gval.numpy()
    out = np.zeros((n_, g_.shape[1]), np.float32)
    rows, cols = np.nonzero((dest.numpy() >= 0) & (d >= 0) & (d < n_))
    np.add.at(out, (d[rows, cols], cols), g_[rows, cols])        # row-major = ascending global row: the kernel's order
    return t(out)
RowPartition.scatter_rows = staticmethod(scatter)
g = cases.dense(97, 24, 7)
r0, r1 = part.row_cuts[rank], part.row_cuts[rank + 1]
for red in ("max", "min"):
    ref, ref_arg = oracle.spmm_fw(rowptr, col, val, x, red)
    _, want = oracle.spmm_minmax_bw(col, val, x, ref_arg, g)
    got = part.minmax_backward(t(ref_arg[r0:r1].copy()), t(g[r0:r1].copy()))
    x0, x1 = part.x_cuts[rank], part.x_cuts[rank + 1]
    assert got.shape == (x1 - x0, 24)
    assert np.allclose(got.numpy(), want[x0:x1], rtol=1e-6, atol=1e-6), red
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


@pytest.mark.parametrize("world", (2, 3))
def test_row_partition_equivalence_gloo(tmp_path, world):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29541 + world), WORLD_SIZE=str(world), OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o}"
        assert f"rank {r} ok" in o


_REPL_WORKER = r"""
import importlib.util, os, sys
sys.path.insert(0, {root!r})
import torch, torch.distributed as dist
spec = importlib.util.spec_from_file_location("bench_mod", os.path.join({root!r}, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
calls = []
def make():
    calls.append(1)
    g = torch.Generator().manual_seed(1234)                    # only rank 0 may get here
    rowptr = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int64), torch.randint(0, 9, (50,), generator=g)]), 0)
    return rowptr, torch.randint(0, 50, (int(rowptr[-1]),), generator=g), 50
rowptr, col, n = bench.replicated_graph(make, torch.device("cpu"), rank, world)
assert (len(calls) == 1) == (rank == 0), "rank 0 generates, the others receive"
g = torch.Generator().manual_seed(1234)
want_rowptr = torch.cumsum(torch.cat([torch.zeros(1, dtype=torch.int64), torch.randint(0, 9, (50,), generator=g)]), 0)
want_col = torch.randint(0, 50, (int(want_rowptr[-1]),), generator=g)
assert n == 50 and torch.equal(rowptr, want_rowptr) and torch.equal(col, want_col)
dist.barrier()
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_bench_graph_is_generated_once_and_replicated_gloo(tmp_path):
    """bench.py at N > 1: rank 0 generates the graph, every other rank receives its copy (sizes first), so the partition
    can never differ between ranks."""
    world = 3
    script = tmp_path / "worker.py"
    script.write_text(_REPL_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561", WORLD_SIZE=str(world), OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = [p.communicate(timeout=240)[0] for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{o}"
        assert f"rank {r} ok" in o


def test_nnz_balanced_cuts():
    from isplib_amd.dist import nnz_balanced_cuts
    rowptr, _ = cases.random_csr(1000, 1000, 20.0, seed=1, hub=(10, 5000))
    cuts = nnz_balanced_cuts(torch.from_numpy(rowptr), 4)
    assert cuts[0] == 0 and cuts[-1] == 1000 and cuts == sorted(cuts)
    per = [int(rowptr[cuts[i + 1]] - rowptr[cuts[i]]) for i in range(4)]
    assert max(per) - min(per) <= 5000 + 60


def test_task_entry_argument_validation_without_gpu():
    """fusedMM_csr_tasks_hip / plan builders: every rejection that is decided before a HIP call."""
    import ctypes
    from isplib_amd import cabi
    L = cabi.lib()
    lane = (ctypes.c_int64 * 9)(*([0] * 9))
    one = ctypes.c_void_p(8)      # never dereferenced: validation fails first

    def call(msg=cabi.MSG_SPMM_SUM, m=4, n=4, k=8, n_tasks=0, slices=8, ws=None, ws_bytes=0, lane_off=lane):
        return L.fusedMM_csr_tasks_hip(msg, m, n, k, 0, None, one, None, one, one, n_tasks, one, one, one, one, slices, lane_off,
                                       one, k, one, k, None, ws, ws_bytes, None)
    assert call(msg=0x11103) == cabi.NO_OPT_IMPL
    assert call(slices=0) == cabi.FAIL and "[1, 4096]" in cabi.last_error()
    assert call(k=3) == cabi.FAIL and "k >= 4" in cabi.last_error()
    assert call(n=1 << 30, k=8) == cabi.FAIL and "3.5 GiB" in cabi.last_error()
    assert call() == cabi.NOT_ENOUGH_MEM
    assert call(m=0) == cabi.SUCCESS
    bad = (ctypes.c_int64 * 9)(0, 0, 0, 0, 0, 0, 0, 0, 5)
    assert call(ws=ctypes.c_void_p(256), ws_bytes=1 << 20, lane_off=bad) == cabi.FAIL and "lane_off" in cabi.last_error()
    info = cabi.TaskPlanInfo()
    assert L.isplib_spmm_tasks_count_hip(4, one, one, one, 0, 1024, 128, one, one, 1 << 20, ctypes.byref(info), None) == cabi.FAIL
    assert L.isplib_spmm_tasks_count_hip(4, one, one, one, 8, 8, 128, one, one, 1 << 20, ctypes.byref(info), None) == cabi.FAIL
    assert L.isplib_spmm_tasks_workspace_bytes(cabi.MSG_SPMM_MAX, 10, 16) >= 2 * 10 * 16 * 4
    assert L.isplib_spmm_slices_build_hip(4, 4, 0, one, one, None, 4097, one, None, None) == cabi.FAIL
    assert L.fusedMM_csr_sliced_phase_hip(cabi.MSG_SPMM_SUM, 4, 4, 8, 0, None, one, one, one, one, 8, 8, 4, 1, one, 8, one, 8,
                                          None, ctypes.c_void_p(256), 1 << 20, None) == cabi.FAIL
    assert "slice range" in cabi.last_error()


def test_stream_entries_argument_validation_without_gpu():
    """The five entries on the stream front end (sum / mean, max / min, the FusedMM words, and in the experimental library the
    stream SDDMM and the LDS hybrid): every rejection that is decided before a HIP call, one violation per call, over a plan
    whose pointers are never dereferenced.  No call here may reach a launch."""
    import ctypes
    from isplib_amd import cabi
    L, X = cabi.lib(), cabi.exp_lib()
    one, al16 = ctypes.c_void_p(8), ctypes.c_void_p(16)      # never dereferenced: validation fails first

    def geometry(fn, streams):
        rpw, res = ctypes.c_int(0), ctypes.c_int(0)
        assert fn(streams, ctypes.byref(rpw), ctypes.byref(res)) == cabi.SUCCESS
        return rpw.value
    rpw_sum, rpw_mm, rpw_gen = (geometry(f, 4) for f in (L.isplib_spmm_stream_geometry, L.isplib_spmm_stream_minmax_geometry,
                                                         L.isplib_fusedmm_stream_geometry))
    hyb = [ctypes.c_int(0) for _ in range(4)]
    assert X.isplib_spmm_hybrid_geometry(4, *[ctypes.byref(v) for v in hyb]) == cabi.SUCCESS
    rpw_hyb, table_rows, hot_cap = hyb[0].value, hyb[2].value, hyb[3].value
    assert (rpw_sum, rpw_mm, rpw_gen) == (64, 32, 32)

    def plan(rpw, **over):
        p = cabi.StreamPlanStruct(rows=40, cols=40, slices=2, gens=1, waves_per_gen=8, rows_per_wave=rpw, streams=4, chunk=64,
                                  n_steps=1, n_parts=0, n_hub=0, words=8, vals=8, wave_step_off=8, wave_row=8, wave_part=8,
                                  hub_row=8, hub_off=8, perm=8)
        for name, v in over.items():
            setattr(p, name, v)
        return p

    udef_word = cabi.PATTERNS["sigmoid_embedding"][0]

    # every entry as call(plan fields to override, m, n, k, nnz, ldy, y, msg, sop, ws, ws_bytes)
    def sum_entry(pl, m, n, k, nnz, ldy, y, msg, sop, ws, wsb):
        return L.fusedMM_csr_stream_hip(cabi.MSG_SPMM_SUM if msg is None else msg, m, n, k, nnz, one, one, ctypes.byref(plan(rpw_sum, **pl)),
                                        y, ldy, one, k, ws, wsb, None, None)

    def mm_entry(pl, m, n, k, nnz, ldy, y, msg, sop, ws, wsb):
        return L.fusedMM_csr_stream_minmax_hip(cabi.MSG_SPMM_MAX if msg is None else msg, m, n, k, nnz, one, one,
                                               ctypes.byref(plan(rpw_mm, **pl)), y, ldy, one, k, one, ws, wsb, None)

    def udef_entry(pl, m, n, k, nnz, ldy, y, msg, sop, ws, wsb):
        return L.fusedMM_csr_udef_stream_hip(udef_word if msg is None else msg, m, n, k, nnz, one, one, ctypes.byref(plan(rpw_gen, **pl)),
                                             al16, 8, y, ldy, al16, 8, cabi.SOP_UDEF["sigmoid"] if sop is None else sop, 0.0, ws, wsb, None)

    def sddmm_entry(pl, m, n, k, nnz, ldy, y, msg, sop, ws, wsb):
        return X.isplib_sddmm_stream_hip(m, n, k, nnz, one, one, ctypes.byref(plan(rpw_sum, **pl)), y, ldy, one, 8, 0, one, None)

    def hybrid_entry(pl, m, n, k, nnz, ldy, y, msg, sop, ws, wsb):
        hp = cabi.HybridPlanStruct(cold=plan(rpw_hyb, **dict({"vals": None}, **pl)), table_rows=table_rows, hot_cap=hot_cap,
                                   n_hot_steps=1, hot_rows=8, hot_words=8, hot_step_off=8, hot_perm=8)
        return X.fusedMM_csr_hybrid_hip(cabi.MSG_SPMM_SUM if msg is None else msg, m, n, k, nnz, one, one, ctypes.byref(hp), y, ldy,
                                        one, k, ws, wsb, None, None)

    # (the two SpMM entries share one driver, which reports under the sum entry's name)
    entries = {
        "sum": (sum_entry, ("fusedMM_csr_stream_hip:",), rpw_mm, cabi.MSG_SPMM_MAX),
        "minmax": (mm_entry, ("fusedMM_csr_stream_minmax_hip:", "fusedMM_csr_stream_hip:"), rpw_sum, cabi.MSG_SPMM_SUM),
        "udef": (udef_entry, ("fusedMM_csr_udef_stream_hip:",), rpw_sum, cabi.MSG_SPMM_SUM),
        "sddmm": (sddmm_entry, ("isplib_sddmm_stream_hip:",), rpw_mm, None),
        "hybrid": (hybrid_entry, ("fusedMM_csr_hybrid_hip:",), rpw_mm, cabi.MSG_SPMM_MAX),
    }
    for name, (entry, prefixes, other_rpw, wrong_word) in entries.items():
        def refused(status, reason=None, pl=None, m=40, n=40, k=8, nnz=100, ldy=8, y=one, msg=None, sop=None, ws=None, wsb=0):
            got = entry(pl or {}, m, n, k, nnz, ldy, y, msg, sop, ws, wsb)
            assert got == status, (name, reason, got, cabi.last_error())
            assert cabi.last_error().startswith(prefixes), (name, cabi.last_error())
            if reason:
                assert reason in cabi.last_error(), (name, reason, cabi.last_error())

        if wrong_word is not None:
            refused(cabi.NO_OPT_IMPL, msg=wrong_word)
        if name == "udef":
            refused(cabi.UNDEFINED_USER_FUNCTION, "SOP_UDEF", sop=cabi.SOP_UDEF["none"])
            refused(cabi.UNDEFINED_USER_FUNCTION, "SOP_UDEF", sop=7)
        refused(cabi.FAIL, "another shape", m=41)
        refused(cabi.FAIL, "another shape", n=41)
        refused(cabi.FAIL, "24-bit address arithmetic", pl={"cols": 1 << 24}, n=1 << 24)
        refused(cabi.FAIL, "24-bit address arithmetic", ldy=1 << 22)
        refused(cabi.FAIL, "streams", pl={"streams": 3})
        refused(cabi.FAIL, "bad plan geometry", pl={"rows_per_wave": other_rpw})
        refused(cabi.FAIL, "bad plan geometry", pl={"gens": 0})
        refused(cabi.FAIL, "bad plan geometry", pl={"waves_per_gen": 0})
        # (the FusedMM entry has k and leading-dimension rules of its own, which these two calls break as well)
        refused(cabi.FAIL, None if name == "udef" else "k >= 4", k=3)
        refused(cabi.FAIL, None if name == "udef" else "leading dimension smaller than k", ldy=4)
        if name == "minmax":
            refused(cabi.FAIL, None, pl={"cols": 1 << 20}, n=1 << 20, ldy=1024)              # past 3.5 GiB, and past 2 GiB
            refused(cabi.FAIL, "2 GiB", pl={"cols": 1 << 20}, n=1 << 20, ldy=640)             # 2.5 GiB: the max / min limit alone
            refused(cabi.FAIL, "4- or 8-stream", pl={"streams": 2})
        else:
            refused(cabi.FAIL, "3.5 GiB", pl={"cols": 1 << 20}, n=1 << 20, ldy=1024)
        if name in ("minmax", "sddmm"):
            refused(cabi.FAIL, "perm", pl={"perm": None})
        refused(cabi.FAIL, "null operand", y=None)
        refused(cabi.FAIL, "null operand", pl={"wave_row": None})
        refused(cabi.FAIL, "null operand", pl={"words": None})
        if name != "sddmm":                                                                   # the SDDMM writes no partial rows
            refused(cabi.FAIL, "null operand", pl={"n_hub": 1, "hub_off": None})
            refused(cabi.NOT_ENOUGH_MEM, "workspace too small", pl={"n_parts": 5})
            refused(cabi.NOT_ENOUGH_MEM, "workspace too small", pl={"n_parts": 5}, ws=ctypes.c_void_p(256), wsb=16)
            refused(cabi.FAIL, "256-byte aligned", pl={"n_parts": 5}, ws=ctypes.c_void_p(264), wsb=1 << 20)
            # a refusal with another status keeps its place: the message word before the plan, the plan before the workspace
            if wrong_word is not None:
                refused(cabi.NO_OPT_IMPL, msg=wrong_word, pl={"streams": 3, "n_parts": 5})
            refused(cabi.FAIL, "streams", pl={"streams": 3, "n_parts": 5})
        if name == "udef":
            refused(cabi.UNDEFINED_USER_FUNCTION, "SOP_UDEF", sop=cabi.SOP_UDEF["none"], pl={"streams": 3})
        assert entry({}, 0, 40, 8, 100, 8, one, None, None, None, 0) == cabi.SUCCESS, name     # m = 0: nothing to do
        assert cabi.last_error() == ""
        if name == "sddmm":
            assert entry({}, 40, 40, 8, 0, 8, one, None, None, None, 0) == cabi.SUCCESS
        else:
            assert entry({}, 40, 40, 0, 100, 8, one, None, None, None, 0) == cabi.SUCCESS      # k = 0


def test_stream_geometry_of_every_family():
    """Rows per wave and resident waves of the three plan families at every slot width, the stream counts each geometry entry
    refuses, and the FusedMM suggest rule on the Reddit shape (recorded answers: the rule is arithmetic on the geometry)."""
    import ctypes
    from isplib_amd import cabi
    L = cabi.lib()

    def geometry(fn, streams):
        rpw, res = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = fn(streams, ctypes.byref(rpw), ctypes.byref(res))
        return rc, rpw.value, res.value
    # without a device the library assumes the MI355X's 256 CUs
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    want = {
        "isplib_spmm_stream_geometry": {2: 32, 4: 64, 8: 128},
        "isplib_spmm_stream_minmax_geometry": {4: 32, 8: 64},
        "isplib_fusedmm_stream_geometry": {2: 16, 4: 32, 8: 64},
    }
    for name, rows in want.items():
        fn = getattr(L, name)
        for streams in (0, 1, 2, 3, 4, 5, 6, 8, 16):
            rc, rpw, res = geometry(fn, streams)
            if streams in rows:
                assert (rc, rpw) == (cabi.SUCCESS, rows[streams]), (name, streams)
                assert res == 8 * cus, (name, streams, res)          # two workgroups of four waves per CU
            else:
                assert rc == cabi.FAIL and cabi.last_error().startswith(name + ": streams must be"), (name, streams)
                assert (rpw, res) == (-1, -1), "a refusal writes nothing"
        assert fn(4, None, None) == cabi.SUCCESS                      # both outputs are optional
    if cus == 256:
        word = cabi.PATTERNS["sigmoid_embedding"][0]
        recorded = {32: (8, 8, 1457), 64: (4, 16, 1457), 128: (2, 46, 1457)}      # (streams, slices, chunk)
        for k, triple in recorded.items():
            st, sl, ch = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
            assert L.isplib_suggest_fusedmm_stream(word, 232965, 232965, 114615892, k, ctypes.byref(st), ctypes.byref(sl), ctypes.byref(ch)) == 1
            assert (st.value, sl.value, ch.value) == triple, (k, st.value, sl.value, ch.value)
        assert L.isplib_suggest_fusedmm_stream(word, 232965, 232965, 114615892, 256, None, None, None) == 0      # wider than a slot
        assert L.isplib_suggest_fusedmm_stream(cabi.MSG_SPMM_SUM, 232965, 232965, 114615892, 64, None, None, None) == 0


# ---- MatrixMarket I/O (the reference tuner's graph format, README.md:147-168) -------------------

def test_mtx_round_trip_and_readme_case(tmp_path):
    import scipy.io
    import scipy.sparse as sp
    from isplib_amd import mtx
    from tests import cases
    rowptr, col, val, *_ = cases.readme_case()
    path = tmp_path / "readme.mtx"
    mtx.write_mtx(path, torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(val), (3, 3), "README.md:105-116")
    rp, cl, vl, sizes = mtx.read_mtx(path)
    assert sizes == (3, 3) and rp.tolist() == rowptr.tolist() and cl.tolist() == col.tolist()      # duplicate (0,0) kept
    assert vl.tolist() == val.tolist()
    # pattern files: unit weights
    mtx.write_mtx(path, torch.from_numpy(rowptr), torch.from_numpy(col), None, (3, 3))
    rp, cl, vl, _ = mtx.read_mtx(path)
    assert vl is None and cl.tolist() == col.tolist()
    # a file written by scipy (symmetric storage, comments) expands to both triangles, in (row, col) order
    a = sp.random(40, 40, 0.1, random_state=3, format="coo")
    a = (a + a.T).tocoo()
    scipy.io.mmwrite(str(tmp_path / "sym.mtx"), a, comment="written by scipy", symmetry="symmetric")
    rp, cl, vl, sizes = mtx.read_mtx(tmp_path / "sym.mtx")
    want = a.tocsr()
    want.sort_indices()
    assert sizes == (40, 40) and rp.tolist() == want.indptr.tolist() and cl.tolist() == want.indices.tolist()
    assert np.allclose(vl.numpy(), want.data, rtol=1e-6)


def test_mtx_rejects_what_it_cannot_represent(tmp_path):
    from isplib_amd import mtx
    bad = tmp_path / "bad.mtx"
    bad.write_text("%%MatrixMarket matrix array real general\n2 2\n1\n2\n3\n4\n")
    with pytest.raises(ValueError, match="coordinate"):
        mtx.read_mtx(bad)
    bad.write_text("%%MatrixMarket matrix coordinate complex general\n2 2 1\n1 1 1 0\n")
    with pytest.raises(ValueError, match="field"):
        mtx.read_mtx(bad)
    bad.write_text("%%MatrixMarket matrix coordinate real general\n2 2 2\n1 1 1.0\n")
    with pytest.raises(ValueError, match="promises"):
        mtx.read_mtx(bad)
    bad.write_text("%%MatrixMarket matrix coordinate real general\n2 2 1\n3 1 1.0\n")
    with pytest.raises(ValueError, match="outside"):
        mtx.read_mtx(bad)
    empty = tmp_path / "empty.mtx"
    empty.write_text("%%MatrixMarket matrix coordinate pattern general\n% nothing\n3 4 0\n")
    rp, cl, vl, sizes = mtx.read_mtx(empty)
    assert sizes == (3, 4) and rp.tolist() == [0, 0, 0, 0] and cl.numel() == 0 and vl is None


def test_tuning_table_persists_by_graph_signature(tmp_path):
    from isplib_amd import plugin
    from isplib_amd.sparse import SparseStorage
    rowptr = torch.tensor([0, 2, 2, 5], dtype=torch.int64)
    col = torch.tensor([0, 1, 0, 1, 2], dtype=torch.int64)
    st = SparseStorage(rowptr, col, None, (3, 3))
    sig = plugin.graph_signature(st)
    assert sig == "3x3:5:1,2"                  # degrees 2, 0, 3 -> floor(log2(max(d,1))) = 1, 0, 1
    plugin._tuning_db.clear()
    plugin._tuning_db[sig] = {"3:128:0": 16}
    path = tmp_path / "tune.json"
    plugin.iSpLibPlugin.save_tuning(path)
    plugin._tuning_db.clear()
    assert plugin.choose_slices(st, 3, 128) == 0                      # the rule: tiny graph, plain kernel
    assert plugin.iSpLibPlugin.load_tuning(path) == 1
    assert plugin.choose_slices(st, 3, 128) == 16                     # the persisted measurement wins
    same_shape = SparseStorage(rowptr.clone(), col.clone(), None, (3, 3))
    assert plugin.choose_slices(same_shape, 3, 128) == 16             # keyed by content, not by object or pointer
    assert plugin.choose_slices(same_shape, 3, 64) == 0
    plugin._tuning_db.clear()


def test_slice_rule_lives_in_the_c_abi_and_handle_entries_validate():
    import ctypes
    from isplib_amd import cabi, plugin
    L = cabi.lib()
    n, nnz = 232965, 114615892                                     # the Reddit shape: K=32 -> 4, 64 -> 8, >=128 -> 16
    assert [L.isplib_suggest_slices(n, n, nnz, k, 0) for k in (32, 64, 128, 256, 608)] == [4, 8, 8, 8, 8]   # 64-column panels
    assert [L.isplib_suggest_slices(n, n, nnz, k, 1) for k in (32, 64, 128, 256)] == [4, 8, 8, 8]
    assert [L.isplib_suggest_slices(n, n, nnz, k, 0) for k in (41, 100, 602)] == [5, 13, 16]               # ragged rows: one pass / 128-column panels
    assert L.isplib_suggest_slices(2449029, 2449029, 123718280, 256, 0) == 0      # products: mean degree 50 -> plain
    assert L.isplib_suggest_slices(2708, 2708, 10556, 16, 0) == 0                  # Cora: launch-bound, no preparation
    assert plugin.suggest_slices(n, n, nnz, 128, True) == 8 and plugin.suggest_slices(n, n, nnz, 100) == 13                    # the Python name is the same rule
    assert L.isplib_graph_spmm(None, cabi.MSG_SPMM_SUM, 8, None, 8, None, 8, None, None) == cabi.FAIL
    assert "null handle" in cabi.last_error()
    assert L.isplib_graph_set_slices(None, 4) == cabi.FAIL
    out = ctypes.c_void_p()
    assert L.isplib_graph_create(4, 1 << 31, 0, ctypes.c_void_p(8), None, None, ctypes.byref(out)) == cabi.FAIL
    assert L.isplib_graph_create(-1, 4, 0, ctypes.c_void_p(8), None, None, ctypes.byref(out)) == cabi.FAIL
    L.isplib_graph_destroy(None)                                   # a no-op, like free(NULL)


def test_stream_rule_offers_only_what_the_stream_entries_accept():
    """The schedule rule and the entries it feeds share one domain: a shape the stream entry / plan builder would refuse
    (dense operand beyond one 3.5 GiB buffer descriptor, 32-bit edge positions) is not offered the stream schedule, so it
    reaches the task list / plain kernel as it did before the schedule existed instead of raising (round-2 advisor)."""
    import ctypes
    from isplib_amd import cabi
    L = cabi.lib()

    def offered(fn, m, n, nnz, k):
        st, sl, ch = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        return bool(fn(m, n, nnz, k, ctypes.byref(st), ctypes.byref(sl), ctypes.byref(ch)))
    for fn in (L.isplib_suggest_stream, L.isplib_suggest_stream_minmax):
        assert offered(fn, 232965, 232965, 114615892, 64)                         # the Reddit shape: yes
        assert not offered(fn, 1_000_000, 1_000_000, 500_000_000, 1024)           # 4.1 GB of y: one descriptor cannot hold it
        assert offered(fn, 1_000_000, 1_000_000, 500_000_000, 512)                # 2 GB: fine
        assert not offered(fn, 2_000_000, 2_000_000, (1 << 31) + 5, 64)           # edge positions beyond 32 bits
    assert cabi.suggest_stream(1_000_000, 1_000_000, 500_000_000, 1024) is None   # what plugin.choose_stream asks
    # the Reddit shape: 64-column slots, 31 slices; a WEIGHTED plan at whole multiples of 128 columns rides 128-column slots
    # (its weight stream is read once per panel: round 4, 2.90 -> 2.82 ms at K=128, 5.89 -> 5.74 at K=256)
    n, nnz = 232965, 114615892
    assert cabi.suggest_stream(n, n, nnz, 128) == (4, 31, 2057) == cabi.suggest_stream(n, n, nnz, 128, False)
    assert cabi.suggest_stream(n, n, nnz, 128, True) == (2, 63, 2057) and cabi.suggest_stream(n, n, nnz, 256, True)[0] == 2
    assert cabi.suggest_stream(n, n, nnz, 192, True)[0] == 4 and cabi.suggest_stream(n, n, nnz, 64, True) == cabi.suggest_stream(n, n, nnz, 64)
    # max / min (round 4: the row's pair rides in registers, a change of row is an LDS swap): slices of ~3.3 MB of the panel
    assert cabi.stream_minmax_geometry(4)[0] == 32 and cabi.stream_minmax_geometry(8)[0] == 64
    st, sl, ch = cabi.suggest_stream_minmax(n, n, nnz, 64)
    assert (st, sl) == (4, 18) and 2800 <= ch <= 3200
    assert cabi.suggest_stream_minmax(n, n, nnz, 32)[:2] == (8, 9)
    assert not offered(L.isplib_suggest_stream_minmax, 1_100_000, 1_100_000, 500_000_000, 512)   # 2.25 GB: the max / min entry stops at 2 GiB
    assert offered(L.isplib_suggest_stream, 1_100_000, 1_100_000, 500_000_000, 512)
    # exactly at every limit of the domain (include/isplib_hip.h, "address domains"): offered just inside, not just outside
    for fn in (L.isplib_suggest_stream, L.isplib_suggest_stream_minmax):
        assert offered(fn, 1000, cabi.STREAM_N_END - 1, 1 << 30, 16)              # n < 2^24 (1 GiB of y, few long rows)
        assert not offered(fn, 1000, cabi.STREAM_N_END, 1 << 30, 16)
        assert offered(fn, 232965, 232965, cabi.STREAM_NNZ_END - 1, 64)           # nnz < 2^31
        assert not offered(fn, 232965, 232965, cabi.STREAM_NNZ_END, 64)
    n_at = cabi.DENSE_BYTES_MAX // (1024 * 4)                                     # 917,504 rows of 1024 floats: 3.5 GiB exactly
    assert n_at * 1024 * 4 == cabi.DENSE_BYTES_MAX
    assert offered(L.isplib_suggest_stream, n_at, n_at, 500_000_000, 1024)        # n * k * 4 <= 3.5 GiB: the limit itself is served
    assert not offered(L.isplib_suggest_stream, n_at + 1, n_at + 1, 500_000_000, 1024)
    n_at = cabi.STREAM_MINMAX_BYTES_END // (512 * 4)                              # 1,048,576 rows of 512 floats: 2 GiB exactly
    assert n_at * 512 * 4 == cabi.STREAM_MINMAX_BYTES_END
    assert offered(L.isplib_suggest_stream_minmax, n_at - 1, n_at - 1, 500_000_000, 512)   # max / min: n * k * 4 < 2 GiB
    assert not offered(L.isplib_suggest_stream_minmax, n_at, n_at, 500_000_000, 512)
    assert offered(L.isplib_suggest_stream, n_at, n_at, 500_000_000, 512)         # (sum / mean go on to 3.5 GiB)


def test_cabi_mirrors_the_headers_limits_and_status_codes():
    """include/isplib_hip.h is the one statement of the kernel families' address domains and of the status codes; the names
    isplib_amd.cabi gives the Python layers carry the header's values, and both spellings of a status code are one value."""
    from isplib_amd import cabi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "isplib_hip.h")).read(), flags=re.S)
    header = {}
    for name, expr in re.findall(r"^#define\s+ISPLIB_(\w+)[ \t]+(\S.*?)\s*$", text, flags=re.M):
        expr = re.sub(r"(?<=[0-9a-fA-F])(?:ull|ULL|ll|LL|u|U)\b", "", expr)       # integer suffixes
        if re.fullmatch(r"[0-9a-fA-FxX()<\s-]+", expr):                           # literals and shifts; not the composed message words
            header[name] = eval(expr)
    limits = ("DENSE_BYTES_MAX", "DENSE_OOB_OFFSET", "STREAM_N_END", "STREAM_LDY_END", "STREAM_NNZ_END", "STREAM_MINMAX_BYTES_END",
              "K_MIN", "SDDMM_TASKS_K_MAX")
    codes = ("SUCCESS", "FAIL", "NOT_ENOUGH_MEM", "UNDEFINED_USER_FUNCTION", "NO_OPT_IMPL", "HIP_ERROR")
    for name in limits + codes:
        assert name in header, f"ISPLIB_{name} is not a plain constant of include/isplib_hip.h"
        assert getattr(cabi, name) == header[name], name
    for name in codes:
        if name != "UNDEFINED_USER_FUNCTION":
            assert getattr(cabi, "ISPLIB_" + name) == header[name], name
    assert (header["DENSE_BYTES_MAX"], header["STREAM_MINMAX_BYTES_END"]) == (7 << 29, 1 << 31)        # 3.5 GiB, 2 GiB
    assert (header["STREAM_N_END"], header["STREAM_LDY_END"], header["STREAM_NNZ_END"]) == (2 ** 24, 2 ** 22, 2 ** 31)
    assert (header["K_MIN"], header["SDDMM_TASKS_K_MAX"]) == (4, 1024)


def test_degree_skew_adjustment_of_the_slice_rule():
    from isplib_amd import plugin
    flat = torch.arange(0, 101 * 50, 50, dtype=torch.int64)                       # every row has 50 entries
    assert plugin.degree_cv2(flat) == 0.0 and plugin.skew_adjusted(flat, 8) == 12 and plugin.skew_adjusted(flat, 0) == 0
    deg = torch.tensor([1] * 90 + [500] * 10, dtype=torch.int64)                   # a few hubs: strongly skewed
    skewed = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)])
    assert plugin.degree_cv2(skewed) > 2.0 and plugin.skew_adjusted(skewed, 8) == 8
    assert plugin.skew_adjusted(flat, 60) == 64                                     # capped like the rule itself


def test_bench_self_launches_one_rank_per_gpu_and_refuses_missing_gpus():
    """`python bench.py --gpus N` with no launcher (WORLD_SIZE unset) must start N ranks itself, before touching the
    GPU, and must fail loudly -- never print an n_gpus=1 line -- when fewer than N GPUs are visible."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cmd = bench.launcher_command(4, ["--gpus", "4", "--steps", "3"], 29512)
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29512"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"] and cmd[-5].endswith("bench.py")
    src = open(os.path.join(ROOT, "bench.py")).read()
    launch_at = src.index("raise SystemExit(self_launch(")
    assert launch_at < src.index("torch.cuda.is_available()"), "the launcher must run before anything initialises the GPU"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    if torch.cuda.device_count() < 8:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"],
                           capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode != 0 and "refusing" in r.stderr and '"metric"' not in r.stdout
    # the launcher parent counts devices from sysfs and never through torch.cuda / HIP / amdsmi
    import ast
    used = {}
    for fn in ast.parse(src).body:
        if isinstance(fn, ast.FunctionDef) and fn.name in ("self_launch", "visible_gpu_count", "launcher_command"):
            used[fn.name] = {n.id for n in ast.walk(fn) if isinstance(n, ast.Name)} | \
                            {a_.name.split(".")[0] for n in ast.walk(fn) if isinstance(n, (ast.Import, ast.ImportFrom)) for a_ in n.names}
    assert set(used) == {"self_launch", "visible_gpu_count", "launcher_command"}
    for name, ids in used.items():
        assert not ids & {"torch", "ctypes", "amdsmi", "cabi", "isplib_amd"}, f"{name} must not reach HIP: {ids}"
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        sysfs, dri = os.path.join(tmp, "nodes"), os.path.join(tmp, "dri")
        os.makedirs(dri)
        for i, (simd, minor) in enumerate(((0, -1), (0, -1), (1024, 128), (1024, 129), (1024, 130), (1024, 131))):   # 2 CPU + 4 GPU nodes
            os.makedirs(os.path.join(sysfs, str(i)))
            with open(os.path.join(sysfs, str(i), "properties"), "w") as f:
                f.write(f"cpu_cores_count {0 if simd else 64}\nsimd_count {simd}\ndrm_render_minor {minor}\ngfx_target_version 90500\n")
            if simd and minor != 131:                                   # the fourth GPU's render node is not ours to open
                open(os.path.join(dri, f"renderD{minor}"), "w").close()
        count = lambda **env: bench.visible_gpu_count(sysfs, dri, env)  # noqa: E731
        assert count() == 3
        assert count(HIP_VISIBLE_DEVICES="0,2") == 2 and count(ROCR_VISIBLE_DEVICES="1") == 1
        assert count(ROCR_VISIBLE_DEVICES="0,1", HIP_VISIBLE_DEVICES="0,1,2") == 2      # the second list indexes what the first left
        assert count(HIP_VISIBLE_DEVICES="0,7,1") == 1 and count(HIP_VISIBLE_DEVICES="") == 0 and count(CUDA_VISIBLE_DEVICES="-1") == 0
        assert count(ROCR_VISIBLE_DEVICES="GPU-0123456789abcdef") == 1
        assert bench.visible_gpu_count(os.path.join(tmp, "missing"), dri, {}) in (0, None)
    # a launcher that disagrees with --gpus is an error too, not a silent single-rank run
    env2 = dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True, env=env2, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_bench_output_sample_is_whole_rows_seeded_and_within_budget(tmp_path):
    """`bench.py --dump-outputs`: outputs that fit are written whole; larger ones as a seeded sample of whole rows (the same
    rows of `out` and `arg`, the same rows on every call), within the byte budget, float32 values and float64 positions."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    out = torch.arange(1000 * 8, dtype=torch.float32).reshape(1000, 8)
    arg = torch.arange(1000 * 8, dtype=torch.int64).reshape(1000, 8) + (1 << 40)
    whole = bench.sample_outputs(out, arg)
    assert set(whole) == {"out", "arg"} and whole["out"].dtype == np.float32 and whole["arg"].dtype == np.float64
    assert np.array_equal(whole["out"], out.numpy()) and np.array_equal(whole["arg"].astype(np.int64), arg.numpy())
    budget = 100 * (8 * 4 + 8 * 8)
    part = bench.sample_outputs(out, arg, budget=budget)
    assert part["out"].shape == (100, 8) and part["out"].nbytes + part["arg"].nbytes <= budget
    rows = part["out"][:, 0].astype(np.int64) // 8
    assert np.all(np.diff(rows) > 0) and np.array_equal(part["out"], out.numpy()[rows])
    assert np.array_equal(part["arg"].astype(np.int64), arg.numpy()[rows])
    again = bench.sample_outputs(out, arg, budget=budget)
    assert np.array_equal(again["out"], part["out"]) and np.array_equal(again["arg"], part["arg"])
    assert set(bench.sample_outputs(out, budget=budget)) == {"out"}
    bench.dump_outputs(str(tmp_path / "d"), part)
    assert sorted(os.listdir(tmp_path / "d")) == ["arg.npy", "out.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "out.npy"), part["out"])


def _slice_table_np(rowptr, col, n, slices):
    w = -(-n // slices)
    m = rowptr.size - 1
    table = np.zeros((m, slices + 1), np.int64)
    for i in range(m):
        c = col[rowptr[i]:rowptr[i + 1]]
        table[i] = rowptr[i] + np.searchsorted(c, np.arange(slices + 1) * w, side="left")
        table[i, slices] = rowptr[i + 1]
    return table


@pytest.mark.parametrize("geom", ((8, 8, 8, 512, 4), (5, 3, 16, 64, 16), (16, 2, 32, 100000, 1), (1, 4, 8, 40, 1000)))
def test_sweep_plan_covers_every_edge_once_in_csr_order(geom):
    """Host logic of the sweep schedule's plan (isplib_amd/plan.py: sweep_plan_arrays), replayed on the CPU the way
    the kernel walks it: every stored entry belongs to exactly one task of the wave that owns its (virtual) row, a
    row's tasks are met in ascending CSR order, a wave's tasks are in (slice, slot) order, hub rows are cut into
    chunks whose partial rows are contiguous and in CSR order, and the replay reproduces A @ X."""
    from isplib_amd.plan import sweep_plan_arrays
    slices, wpg, rpw, chunk, min_seg = geom
    m, n = 300, 257
    rowptr, col = cases.random_csr(m, n, 30, 1, empty_rows=(0, 5, 299), hub=(7, 5000))
    table = _slice_table_np(rowptr, col, n, slices)
    p = sweep_plan_arrays(torch.from_numpy(rowptr), torch.from_numpy(table), slices, wpg, rpw, chunk, min_seg)
    nw = p["gens"] * p["waves_per_gen"]
    wr = p["wave_row"].numpy().reshape(nw, rpw)
    wp = p["wave_part"].numpy().reshape(nw, rpw)
    off, tb, tm = p["wave_task_off"].numpy(), p["task_b"].numpy(), p["task_meta"].numpy()
    x = np.random.default_rng(0).random((n, 3))
    out, parts = np.zeros((m, 3)), np.zeros((p["n_parts"], 3))
    cover = np.zeros(col.size, int)
    width = -(-n // slices)
    rows_seen = np.zeros(m, int)
    for w in range(nw):
        acc = np.zeros((rpw, 3))
        last_pos = np.full(rpw, -1, np.int64)
        last_key = -1
        slot_edges = np.zeros(rpw, np.int64)
        for t in range(off[w], off[w + 1]):
            slot_edges[int(tm[t]) >> 24] += int(tm[t]) & 0xFFFFFF
        for t in range(off[w], off[w + 1]):
            slot, ln, b = int(tm[t]) >> 24, int(tm[t]) & 0xFFFFFF, int(tb[t])
            r = wr[w, slot]
            assert r >= 0 and ln > 0 and rowptr[r] <= b and b + ln <= rowptr[r + 1]
            assert b > last_pos[slot], "a row's tasks must come in ascending CSR order"
            last_pos[slot] = b
            if min_seg == 1 and slot_edges[slot] >= slices:    # no slice groups: a task's phase is the slice of its first edge
                key = int(col[b]) // width * rpw + slot
                assert key > last_key, "a wave's tasks must be in (slice, slot) order"
                last_key = key
            cover[b:b + ln] += 1
            acc[slot] += x[col[b:b + ln]].sum(0)
        for j in range(rpw):
            if wr[w, j] < 0:
                continue
            if wp[w, j] >= 0:
                parts[wp[w, j]] = acc[j]
            else:
                out[wr[w, j]] = acc[j]
                rows_seen[wr[w, j]] += 1
    hr, ho = p["hub_row"].numpy(), p["hub_off"].numpy()
    for h in range(hr.size):
        out[hr[h]] = parts[ho[h]:ho[h + 1]].sum(0)
        rows_seen[hr[h]] += 1
    assert (cover == 1).all() and (rows_seen == 1).all()
    ref = np.stack([x[col[rowptr[i]:rowptr[i + 1]]].sum(0) for i in range(m)])
    assert np.allclose(out, ref, rtol=1e-12, atol=1e-12)
    assert int((p["task_meta"] & 0xFFFFFF).sum()) == col.size


@pytest.mark.parametrize("streams,rpw", ((4, 32), (8, 64)))
def test_stream_order_keeps_the_lowest_csr_position_on_ties(streams, rpw):
    """The argument behind spmm_stream_minmax_kernel, replayed on the CPU: for rows whose columns ascend, a stream lists a
    row's edges in CSR order (slice by slice, CSR order inside a slice), so "only a strictly better candidate replaces
    the one held" -- tracked by WORD INDEX, translated through perm at the end -- leaves the lowest CSR position among
    equal candidates; the pieces of a hub row are merged by explicit position compare.  Integer operands: ties everywhere.
    Against the oracle, values and arg.  And: the plan builder refuses a graph with an unsorted row."""
    import oracle
    from isplib_amd.plan import build_stream_plan, stream_plan_arrays
    m, n, slices, wpg, chunk = 120, 90, 5, 3, 40
    rowptr, col = cases.random_csr(m, n, 25, 3, empty_rows=(0, 50), hub=(7, 700), duplicates=True)
    val = cases.weights(col.size, 4, "signed_int")
    x = cases.dense(n, 5, 3, "integer")
    p = stream_plan_arrays(torch.from_numpy(rowptr), torch.from_numpy(col), n, slices, wpg, rpw, streams, chunk)
    nw = p["gens"] * wpg
    words = p["words"].numpy().astype(np.int64) & 0xFFFFFFFF
    perm, off = p["perm"].numpy(), p["wave_step_off"].numpy()
    wr, wp = p["wave_row"].numpy().reshape(nw, rpw), p["wave_part"].numpy().reshape(nw, rpw)
    k = x.shape[1]
    lowest = np.finfo(np.float32).min
    out, arg = np.zeros((m, k), np.float32), np.full((m, k), col.size, np.int64)
    part_v, part_i = np.full((p["n_parts"], k), lowest, np.float32), np.full((p["n_parts"], k), np.iinfo(np.int64).max, np.int64)
    for w in range(nw):
        best = np.full((rpw, k), lowest, np.float32)
        widx = np.full((rpw, k), -1, np.int64)
        for st in range(off[w], off[w + 1]):
            for g in range(streams):
                i = st * streams + g
                c, lr = words[i] & 0xFFFFFF, words[i] >> 24
                if c == n:
                    continue                                     # padding: the kernel steers it to a spare row
                t = np.float32(val[perm[i]]) * x[c]
                win = t > best[lr]                               # strict, in stream order
                best[lr][win], widx[lr][win] = t[win], i
        for j in range(rpw):
            if wr[w, j] < 0:
                continue
            pos = np.where(widx[j] >= 0, perm[np.maximum(widx[j], 0)], np.iinfo(np.int64).max)
            if wp[w, j] >= 0:
                part_v[wp[w, j]], part_i[wp[w, j]] = best[j], pos
            elif rowptr[wr[w, j] + 1] > rowptr[wr[w, j]]:
                out[wr[w, j]], arg[wr[w, j]] = best[j], np.where(widx[j] >= 0, pos, col.size)
    hr, ho = p["hub_row"].numpy(), p["hub_off"].numpy()
    for h in range(hr.size):
        v, a = np.full(k, lowest, np.float32), np.full(k, np.iinfo(np.int64).max, np.int64)
        for q in range(ho[h], ho[h + 1]):
            take = (part_v[q] > v) | ((part_v[q] == v) & (part_i[q] < a))
            v[take], a[take] = part_v[q][take], part_i[q][take]
        out[hr[h]], arg[hr[h]] = v, a
    ref, ref_arg = oracle.spmm_fw(rowptr, col, val, x, "max")
    assert np.array_equal(out, ref) and np.array_equal(arg, ref_arg)
    # unsorted rows: no plan (the stream order would no longer be the CSR order)
    r2, c2 = cases.random_csr(40, 30, 6, 9, sort_cols=False)
    assert build_stream_plan(torch.from_numpy(r2), torch.from_numpy(c2), None, 30, 2, 3, rpw, streams, 16, minmax=True) is None


@pytest.mark.parametrize("geom", ((8, 8, 16, 4, 512), (5, 3, 32, 8, 64), (3, 2, 16, 2, 100000)))
def test_stream_plan_lists_every_edge_once_slice_by_slice(geom):
    """Host logic of the stream plan (isplib_amd/plan.py: stream_plan_arrays), replayed on the CPU the way
    spmm_stream_kernel walks it: every stored entry appears in exactly one stream, in the stream of the slot that owns
    its (virtual) row; a stream visits the column slices in ascending order and inside a slice its rows one after the
    other, each in ascending CSR order; hub rows are dealt round robin to virtual rows, whose partial rows are
    contiguous; padding words name column n and a row of the stream's own slot; the replay reproduces A @ X."""
    from isplib_amd.plan import stream_plan_arrays
    slices, wpg, rpw, streams, chunk = geom
    m, n = 300, 257
    rowptr, col = cases.random_csr(m, n, 30, 1, empty_rows=(0, 5, 299), hub=(7, 5000))
    p = stream_plan_arrays(torch.from_numpy(rowptr), torch.from_numpy(col), n, slices, wpg, rpw, streams, chunk)
    nw = p["gens"] * wpg
    words = p["words"].numpy().astype(np.int64) & 0xFFFFFFFF
    perm = p["perm"].numpy()
    off = p["wave_step_off"].numpy()
    wr, wp = p["wave_row"].numpy().reshape(nw, rpw), p["wave_part"].numpy().reshape(nw, rpw)
    per, width = rpw // streams, -(-n // slices)
    x = np.random.default_rng(0).random((n, 3))
    out, parts, seen = np.zeros((m, 3)), np.zeros((p["n_parts"], 3)), np.zeros(col.size, int)
    for w in range(nw):
        acc = np.zeros((rpw, 3))
        last = [(-1, -1, -1)] * streams                         # (slice, local row, CSR position) of the stream's previous word
        for st in range(off[w], off[w + 1]):
            for g in range(streams):
                wd = words[st * streams + g]
                c, lr = wd & 0xFFFFFF, wd >> 24
                assert lr // per == g, "a word names a row of its own slot"
                if c == n:
                    assert perm[st * streams + g] == -1
                    continue
                e = perm[st * streams + g]
                r = wr[w, lr]
                assert col[e] == c and rowptr[r] <= e < rowptr[r + 1]
                key = (c // width, lr, e)
                assert key > last[g], "streams go slice by slice, row by row, in CSR order"
                last[g] = key
                seen[e] += 1
                acc[lr] += x[c]
        for j in range(rpw):
            if wr[w, j] < 0:
                continue
            if wp[w, j] >= 0:
                parts[wp[w, j]] = acc[j]
            else:
                out[wr[w, j]] = acc[j]
    hr, ho = p["hub_row"].numpy(), p["hub_off"].numpy()
    for h in range(hr.size):
        out[hr[h]] = parts[ho[h]:ho[h + 1]].sum(0)
    assert (seen == 1).all()
    ref = np.stack([x[col[rowptr[i]:rowptr[i + 1]]].sum(0) for i in range(m)])
    assert np.allclose(out, ref, rtol=1e-12, atol=1e-12)
    if chunk < 5000:                                            # the hub row's pieces all span the whole column range
        hub_slots = [(w, j) for w in range(nw) for j in range(rpw) if wr[w, j] == 7]
        assert len(hub_slots) == -(-5000 // chunk)


@pytest.mark.parametrize("geom", ((4, 8, 8, 5, 16, 3, 100), (8, 16, 8, 12, 8, 2, 64), (4, 64, 16, 3, 32, 64, 50), (8, 128, 8, 40, 256, 64, 1000)))
def test_hybrid_plan_serves_every_edge_once_from_the_table_or_the_gather_stream(geom):
    """Host logic of the hybrid schedule's plan (isplib_amd/plan.py: hybrid_plan_arrays), replayed on the CPU the way the
    kernel walks it: every stored entry is either a cold word of its wave's stream (column = the entry's column) or a hot
    word of its wave's chunk of the entry's slice (the table row holds the entry's column); local rows stay inside their
    slot; chunks respect the cap; padding points at the zero row / column n; and the replay reproduces A x."""
    from isplib_amd.plan import hybrid_plan_arrays
    streams, rpw, wpg, slices, table_rows, cap, chunk = geom
    n = 700
    rowptr, col = cases.random_csr(n, n, 40.0, seed=3, empty_rows=(0, 350), hub=(9, 650), duplicates=True)
    a = hybrid_plan_arrays(torch.from_numpy(rowptr), torch.from_numpy(col), n, slices, wpg, rpw, streams, chunk, table_rows, cap)
    c = a["cold"]
    rng = np.random.default_rng(0)
    x = rng.integers(-3, 4, (n, 3)).astype(np.float64)
    xz = np.vstack([x, np.zeros((1, 3))])
    nw, per, width = c["gens"] * c["waves_per_gen"], rpw // streams, -(-n // slices)
    acc = np.zeros((nw, rpw, 3))
    seen = np.zeros(col.size, np.int64)
    words, perm, wso = c["words"].numpy().astype(np.int64) & 0xFFFFFFFF, c["perm"].numpy(), c["wave_step_off"].numpy()
    hw, hp, hso = a["hot_words"].numpy().astype(np.int64) & 0xFFFFFFFF, a["hot_perm"].numpy(), a["hot_step_off"].numpy()
    table = a["hot_rows"].numpy().reshape(slices, table_rows)
    assert np.all(table[:, table_rows - 1] == n), "the last table row is the zero row in every slice"
    for w in range(nw):
        for s in range(wso[w], wso[w + 1]):
            for g in range(streams):
                wd = words[s * streams + g]
                lr, cc, e = wd >> 24, wd & 0xFFFFFF, perm[s * streams + g]
                assert g * per <= lr < (g + 1) * per
                assert (col[e] == cc) if e >= 0 else (cc == n)
                acc[w, lr] += xz[cc]
                if e >= 0:
                    seen[e] += 1
        for sl in range(slices):
            o0, o1 = hso[w * slices + sl], hso[w * slices + sl + 1]
            assert 0 <= o1 - o0 <= cap
            for s in range(o0, o1):
                for g in range(streams):
                    wd = hw[s * streams + g]
                    lr, ti, e = wd >> 24, wd & 0xFFFF, hp[s * streams + g]
                    assert g * per <= lr < (g + 1) * per and ti < table_rows
                    cc = table[sl, ti]
                    assert (col[e] == cc and cc // width == sl) if e >= 0 else (ti == table_rows - 1)
                    acc[w, lr] += xz[cc]
                    if e >= 0:
                        seen[e] += 1
    assert np.all(seen == 1) and a["hot_edges"] == int((hp >= 0).sum()) and a["hot_edges"] > 0
    out = np.zeros((n, 3))
    wr = c["wave_row"].numpy().reshape(nw, rpw)
    for w in range(nw):
        for l in range(rpw):
            if wr[w, l] >= 0:
                out[wr[w, l]] += acc[w, l]
    ref = np.zeros((n, 3))
    np.add.at(ref, np.repeat(np.arange(n), np.diff(rowptr)), x[col])
    assert np.array_equal(out, ref)


# ---- bench.py at N > 1: failure containment (class Guard, explore_candidates), on the CPU over gloo ------------------------
_GUARD_WORKER = r"""
import importlib.util, json, os, sys, time
from datetime import timedelta
sys.path.insert(0, {root!r})
import torch, torch.distributed as dist
spec = importlib.util.spec_from_file_location("bench_mod", os.path.join({root!r}, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
mode = os.environ["GUARD_MODE"]
guard = bench.Guard(rank, world)
guard.arm("north_star form", float(os.environ.get("T_SAFE", "20")))
dist.init_process_group("gloo", timeout=timedelta(seconds=30))
t = torch.ones(4)
parked = []                                    # what isplib_amd.dist.RowPartition._kernel / _raise_parked do for a real schedule

agree = bench.StoreAgreement(dist.distributed_c10d._get_default_store(), rank, world, timeout_s=float(os.environ.get("T_CAND", "6")) + 4)

def exchange():                                # a schedule: its collectives always complete, a local failure is raised after them
    dist.all_reduce(t)
    dist.all_reduce(t)
    if parked:
        e = parked.pop()
        e.collectives_complete = True
        raise e

def clock(fn):
    fn()
    return 1.0

if mode == "hang-before-result" and rank == 1:
    time.sleep(1e6)
dist.all_reduce(t)                             # the north_star form, measured: from here on there is a result
guard.offer({{"metric": "edges_aggregated_per_sec", "value": 1.0, "n_gpus": world}} if rank == 0 else None)
if mode == "sigterm":
    guard.arm("holding the result", 120)
    open(os.path.join(os.environ["HOLD_DIR"], f"holding.{{rank}}"), "w").close()
    time.sleep(1e6)
cands = {{"A": exchange, "B": exchange, "C": exchange}}
broken = None
times = {{}}
try:
    times = bench.explore_candidates(cands, check=lambda name, fn: (fn(), True)[1], clock=clock, agree=agree, guard=guard, rank=rank,
                                     per_candidate_s=float(os.environ.get("T_CAND", "6")), until_s=120.0, on_fault=parked.append)
except Exception as e:
    broken = repr(e)
res = {{"metric": "edges_aggregated_per_sec", "value": 1.0, "n_gpus": world, "candidates_ms": times}}
if broken:
    res["abandoned"] = broken
guard.emit(res)
sys.stdout.flush()
os._exit(0)
"""


def _run_guard_workers(tmp_path, mode, port, inject="", world=2, timeout=90, extra_env=None):
    script = tmp_path / "guard_worker.py"
    script.write_text(_GUARD_WORKER.format(root=ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), OMP_NUM_THREADS="1",
               GUARD_MODE=mode, ISPLIB_BENCH_INJECT=inject, **(extra_env or {}))
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(world)]
    return procs


def _json_lines(text):
    import json
    return [json.loads(ln) for ln in text.splitlines() if ln.startswith("{") and '"metric"' in ln]


def test_bench_candidate_that_fails_on_one_rank_is_dropped_on_every_rank(tmp_path):
    """A local kernel failure inside an optional exchange schedule on ONE rank (parked until the schedule's collectives are
    done, as isplib_amd.dist does): the schedule is dropped on every rank and the job goes on with the remaining ones."""
    import time as _t
    t0 = _t.time()
    procs = _run_guard_workers(tmp_path, "explore", 29571, inject="kernel:B:1")
    outs = [p.communicate(timeout=90) for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[1][-2000:] for o in outs]
    lines = _json_lines(outs[0][0])
    assert len(lines) == 1 and sorted(lines[0]["candidates_ms"]) == ["A", "C"] and "abandoned" not in lines[0]
    assert _json_lines(outs[1][0]) == [] and "dropped on every rank" in outs[0][1]
    assert _t.time() - t0 < 60


def test_bench_rank_that_never_arrives_ends_the_job_nonzero_within_the_deadline(tmp_path):
    """Before any result exists a rank that blocks for ever must not hang the job: every rank's guard ends it with a
    non-zero exit code and no JSON line inside the phase's deadline."""
    import time as _t
    t0 = _t.time()
    procs = _run_guard_workers(tmp_path, "hang-before-result", 29572, extra_env={"T_SAFE": "6"})
    outs = [p.communicate(timeout=90) for p in procs]
    # (exit code 5 from a rank's own guard; a rank whose peer's guard fired first may instead see its collective fail)
    assert all(p.returncode != 0 for p in procs) and 5 in [p.returncode for p in procs], [o[1][-2000:] for o in outs]
    assert _json_lines(outs[0][0]) == [] and _json_lines(outs[1][0]) == []
    both = outs[0][1] + outs[1][1]
    assert "deadline passed in phase 'north_star form'" in both and "no result yet" in both and _t.time() - t0 < 60


@pytest.mark.parametrize("kind", ("hang", "raise"))
def test_bench_optional_schedule_that_hangs_or_desynchronises_cannot_lose_the_measured_result(tmp_path, kind):
    """After the north_star form has been measured, an optional schedule in which one rank never comes back (hang) or
    raises before its first collective while its peers wait in it (raise) ends with exit code 0 and rank 0's ONE JSON
    line: the result already measured, marked with what was abandoned."""
    import time as _t
    t0 = _t.time()
    procs = _run_guard_workers(tmp_path, "explore", 29573 + (kind == "raise"), inject=f"{kind}:B:1", extra_env={"T_CAND": "5"})
    outs = [p.communicate(timeout=120) for p in procs]
    assert all(p.returncode == 0 for p in procs), [(p.returncode, o[1][-2000:]) for p, o in zip(procs, outs)]
    lines = _json_lines(outs[0][0])
    assert len(lines) == 1 and lines[0]["value"] == 1.0 and lines[0]["n_gpus"] == 2
    if kind == "hang":
        assert "optional schedule 'B'" in lines[0]["abandoned"]
    assert _json_lines(outs[1][0]) == [] and _t.time() - t0 < 90


def test_bench_sigterm_from_the_launcher_prints_the_measured_result(tmp_path):
    """torchrun ends the surviving ranks with SIGTERM when one rank dies: rank 0's guard takes the signal on its own
    thread (the main thread may sit in a collective) and prints the result it holds before leaving."""
    import signal as _sig
    import time as _t
    procs = _run_guard_workers(tmp_path, "sigterm", 29575, extra_env={"HOLD_DIR": str(tmp_path)})
    deadline = _t.time() + 90
    while not all((tmp_path / f"holding.{r}").exists() for r in range(2)) and _t.time() < deadline:      # both ranks hold the result
        _t.sleep(0.2)
    assert all((tmp_path / f"holding.{r}").exists() for r in range(2))
    for p in procs:
        p.send_signal(_sig.SIGTERM)
    outs = [p.communicate(timeout=30) for p in procs]
    assert [p.returncode for p in procs] == [0, 0], [o[1][-1500:] for o in outs]
    lines = _json_lines(outs[0][0])
    assert len(lines) == 1 and "SIGTERM" in lines[0]["abandoned"] and _json_lines(outs[1][0]) == []


def test_bench_launcher_has_a_time_limit_and_ends_the_process_group(tmp_path, monkeypatch):
    """`python bench.py --gpus N` as its own launcher: ranks that never finish are ended (whole process group) when the
    limit passes, the launcher returns 124 and prints no line; the second attempt (north_star form only) is a fresh set
    of children, never a re-used process."""
    import importlib.util
    import time as _t
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    marker = tmp_path / "started"
    sleeper = tmp_path / "sleeper.py"
    sleeper.write_text("import os, sys, time\nopen(sys.argv[1], 'a').write(os.environ.get('ISPLIB_OVERLAP', '1') + '\\n')\ntime.sleep(1e6)\n")
    monkeypatch.setattr(bench, "launcher_command", lambda gpus, argv, port: [sys.executable, str(sleeper), str(marker)])
    monkeypatch.setattr(bench, "visible_gpu_count", lambda *a_, **k_: 8)
    monkeypatch.setenv("ISPLIB_BENCH_LAUNCH_TIMEOUT", "3")
    t0 = _t.time()
    rc = bench.self_launch(types.SimpleNamespace(gpus=2), ["--gpus", "2"])
    assert rc == 124 and _t.time() - t0 < 40
    assert marker.read_text().split() == ["1"]            # no time left for a second attempt: none was started
    monkeypatch.setenv("ISPLIB_BENCH_LAUNCH_TIMEOUT", "200")
    quick = tmp_path / "quick.py"
    quick.write_text("import os, sys\nopen(sys.argv[1], 'a').write(os.environ.get('ISPLIB_OVERLAP', '1') + '\\n')\nsys.exit(7)\n")
    marker.write_text("")
    monkeypatch.setattr(bench, "launcher_command", lambda gpus, argv, port: [sys.executable, str(quick), str(marker)])
    assert bench.self_launch(types.SimpleNamespace(gpus=2), ["--gpus", "2"]) == 7
    assert marker.read_text().split() == ["1", "0"]       # first the full run, then once more restricted to the north_star form


def test_bench_launcher_stamps_a_retry_into_the_line_it_relays(tmp_path, monkeypatch, capsys):
    """A first attempt that fails without a JSON line and a clean retry must not look like a clean run: the relayed line
    carries `launch` = attempts, the first attempt's exit code / time-limit flag, and that the retry was restricted to the
    north_star form.  A clean first attempt says attempts = 1 and has no `first_attempt`."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    child = tmp_path / "child.py"
    # first attempt (ISPLIB_OVERLAP unset): dies with exit 9 and no line; the retry (ISPLIB_OVERLAP=0) prints a result
    child.write_text("import json, os, sys\n"
                     "if os.environ.get('ISPLIB_OVERLAP', '1') != '0' and os.environ.get('CLEAN') != '1':\n"
                     "    print('rank 1 aborted'); sys.exit(9)\n"
                     "print(json.dumps({'metric': 'edges_aggregated_per_sec', 'value': 1.0, 'n_gpus': 2}))\n")
    monkeypatch.setattr(bench, "launcher_command", lambda gpus, argv, port: [sys.executable, str(child)])
    monkeypatch.setattr(bench, "visible_gpu_count", lambda *a_, **k_: 8)
    monkeypatch.setenv("ISPLIB_BENCH_LAUNCH_TIMEOUT", "200")
    assert bench.self_launch(types.SimpleNamespace(gpus=2), ["--gpus", "2"]) == 0
    lines = _json_lines(capsys.readouterr().out)
    assert len(lines) == 1
    launch = lines[0]["launch"]
    assert launch["attempts"] == 2 and launch["restricted_to_north_star_form"] is True
    assert launch["first_attempt"]["rc"] == 9 and launch["first_attempt"]["timed_out"] is False
    assert launch["this_attempt"] == {"rc": 0, "timed_out": False}
    monkeypatch.setenv("CLEAN", "1")
    assert bench.self_launch(types.SimpleNamespace(gpus=2), ["--gpus", "2"]) == 0
    lines = _json_lines(capsys.readouterr().out)
    assert lines[0]["launch"] == {"attempts": 1, "restricted_to_north_star_form": False, "this_attempt": {"rc": 0, "timed_out": False}}


def test_exchange_schedules_park_local_kernel_errors_until_their_collectives_are_done():
    """isplib_amd.dist.RowPartition._kernel / _raise_parked: the first local kernel failure of an exchange is parked (later
    kernels of the same exchange are skipped, its communication is not), raised once the exchange is complete and marked
    `collectives_complete` -- what lets bench.py drop a schedule on every rank instead of leaving peers in a collective."""
    from isplib_amd.dist import RowPartition
    rowptr = torch.tensor([0, 2, 3, 5], dtype=torch.int64)
    col = torch.tensor([0, 2, 1, 0, 1], dtype=torch.int64)
    part = RowPartition(rowptr, col, None, 3, 0, 1)
    ran = []
    part._kernel(ran.append, "a")
    part.fail_next_kernel = RuntimeError("boom")
    part._kernel(ran.append, "b")                    # fails (injected): parked, not raised
    part._kernel(ran.append, "c")                    # skipped: the exchange's result is void anyway
    assert ran == ["a"] and part.fail_next_kernel is None
    with pytest.raises(RuntimeError, match="boom") as info:
        part._raise_parked()
    assert info.value.collectives_complete is True
    part._raise_parked()                             # nothing parked any more
    part._kernel(ran.append, "d")
    assert ran == ["a", "d"]
    # round-4 advisor: an error parked by an exchange whose waits raised before _raise_parked must not be what the NEXT exchange
    # reports (and must not make it skip its kernels): every schedule starts with a clean slate
    part._parked = RuntimeError("stale error of an earlier exchange")
    x = torch.zeros((part.max_rows, 4))
    out = torch.zeros((part.rows, 4))
    with pytest.raises(Exception) as info:           # (no GPU here: the schedule's own first kernel call fails -- THAT is what surfaces)
        part.spmm_pipelined(x, out, ([(0, 4)], [torch.zeros((part.max_rows, 4))], [torch.zeros((part.ncols_padded, 4))], object(), None), "sum")
    assert "stale" not in str(info.value) and part._parked is None


def test_fusedmm_wrappers_refuse_misshaped_operands_before_any_library_call(monkeypatch):
    """The FusedMM kernels read x[i, :k] for every row i of the graph and y[j, :k] for every stored column id j; the C
    entries cannot know either tensor's row count, so a wrong-shaped operand is an out-of-bounds device read unless the
    wrapper refuses it.  cabi.fusedmm, cabi.fusedmm_stream and plugin.fusedmm raise ValueError on a wrong x (rows,
    width, 1-D), a 1-D y, and a plan built for another shape -- before the library is touched (it is stubbed here so
    that any call fails).  Correct shapes get past the check (to the GPU-tensor check or the stubbed library)."""
    import isplib_amd
    from isplib_amd import cabi

    class LibraryCalled(Exception):
        pass

    def no_library(*a, **k):
        raise LibraryCalled()
    monkeypatch.setattr(cabi, "lib", no_library)
    m, n, k = 6, 5, 8
    rowptr = torch.tensor([0, 2, 3, 3, 5, 6, 8], dtype=torch.int64)
    col = torch.tensor([0, 4, 1, 2, 3, 4, 0, 1], dtype=torch.int64)
    x, y = torch.ones((m, k)), torch.ones((n, k))
    sig = cabi.PATTERNS["sigmoid_embedding"][0]
    tdist = cabi.PATTERNS["tdist_embedding"][0]
    bad_x = {"rows": torch.ones((m + 1, k)), "fewer rows": torch.ones((m - 1, k)), "width": torch.ones((m, k + 4)),
             "1-D": torch.ones(m * k), "3-D": torch.ones((1, m, k))}
    bad_y = {"1-D": torch.ones(n * k), "3-D": torch.ones((1, n, k))}
    stream_plan = types.SimpleNamespace(rows=m, cols=n, slices=1)
    task_plan = types.SimpleNamespace(slices=2, seg_off=torch.zeros(2 * m + 1, dtype=torch.int32))

    # the generic pipeline (plain and task forms); copy_lhs, add, dot and norml words read x
    for word in (sig, tdist, cabi.VOP["copy_lhs"] | cabi.AOP["add"], cabi.VOP["copy_rhs"] | cabi.ROP["norml"] | cabi.SOP["copy"] | cabi.AOP["max"]):
        for plan in (None, task_plan):
            for name, xb in bad_x.items():
                with pytest.raises(ValueError, match="`x`"):
                    cabi.fusedmm(word, rowptr, col, None, xb, y, sop_udef="sigmoid", plan=plan)
            for name, yb in bad_y.items():
                with pytest.raises(ValueError, match="`y`"):
                    cabi.fusedmm(word, rowptr, col, None, x, yb, sop_udef="sigmoid", plan=plan)
            with pytest.raises(RuntimeError, match="GPU tensor"):           # well-shaped: on to the device check
                cabi.fusedmm(word, rowptr, col, None, x, y, sop_udef="sigmoid", plan=plan)
    with pytest.raises(RuntimeError, match="GPU tensor"):                       # x is not read: its shape is not the kernel's business
        cabi.fusedmm(cabi.MSG_SPMM_SUM, rowptr, col, None, bad_x["rows"], y)
    for seg_rows in (m - 1, m + 1):                                               # a task plan built for another row count
        other = types.SimpleNamespace(slices=2, seg_off=torch.zeros(2 * seg_rows + 1, dtype=torch.int32))
        with pytest.raises(ValueError, match="plan"):
            cabi.fusedmm(sig, rowptr, col, None, x, y, sop_udef="sigmoid", plan=other)

    # the stream front end: it loads x[i] of every row it owns, whatever the word
    for word in (sig, tdist, cabi.MSG_SPMM_SUM):
        for name, xb in bad_x.items():
            with pytest.raises(ValueError, match="`x`"):
                cabi.fusedmm_stream(word, rowptr, col.numel(), stream_plan, xb, y, sop_udef="sigmoid")
        for name, yb in bad_y.items():
            with pytest.raises(ValueError, match="`y`"):
                cabi.fusedmm_stream(word, rowptr, col.numel(), stream_plan, x, yb, sop_udef="sigmoid")
        with pytest.raises(ValueError, match="`x`"):
            cabi.fusedmm_stream(word, rowptr, col.numel(), stream_plan, None, y, sop_udef="sigmoid")
        for plan in (types.SimpleNamespace(rows=m, cols=n + 1, slices=1), types.SimpleNamespace(rows=m, cols=n - 1, slices=1),
                     types.SimpleNamespace(rows=m + 1, cols=n, slices=1)):
            with pytest.raises(ValueError, match="plan"):                     # built for another shape
                cabi.fusedmm_stream(word, rowptr, col.numel(), plan, x, y, sop_udef="sigmoid")
        with pytest.raises(RuntimeError, match="GPU tensor"):
            cabi.fusedmm_stream(word, rowptr, col.numel(), stream_plan, x, y, sop_udef="sigmoid")

    # the plug-in: the same checks, and y's rows against the sparse matrix's column count
    adj = isplib_amd.SparseTensor.from_csr(rowptr, col, None, (m, n), validate=False)
    for pattern in ("sigmoid_embedding", "tdist_embedding", "attention_sum"):
        for name, xb in bad_x.items():
            with pytest.raises(ValueError, match="`x`"):
                isplib_amd.fusedmm(adj, xb, y, pattern)
        for name, yb in bad_y.items():
            with pytest.raises(ValueError, match="`y`"):
                isplib_amd.fusedmm(adj, x, yb, pattern)
        for rows in (n - 1, n + 1):
            with pytest.raises(ValueError, match="`y`"):
                isplib_amd.fusedmm(adj, x, torch.ones((rows, k)), pattern)
        with pytest.raises(LibraryCalled):                                      # well-shaped: on to the schedule rule
            isplib_amd.fusedmm(adj, x, y, pattern)
    assert not cabi.reads_x(cabi.MSG_SPMM_SUM) and all(cabi.reads_x(w) for w in (sig, tdist, cabi.VOP["add"] | cabi.AOP["max"]))


# ---- the constructors of tests/cases.py whose stream plan is known: what tests/test_gpu_stream_edges.py relies on --------

def _stream_families():
    """[(family, streams, rows per wave)] from the library's geometry entries (they answer without a device)."""
    from isplib_amd import cabi
    fams = []
    for family, fn, widths in (("sum", cabi.stream_geometry, (2, 4, 8)), ("minmax", cabi.stream_minmax_geometry, (4, 8)),
                               ("fusedmm", cabi.fusedmm_stream_geometry, (2, 4, 8))):
        fams += [(family, streams, fn(streams)[0]) for streams in widths]
    return fams


def _plan_of(rowptr, col, n, slices, wpg, rpw, streams, chunk, family):
    from isplib_amd.plan import stream_plan_arrays
    return stream_plan_arrays(torch.from_numpy(rowptr), torch.from_numpy(col), n, slices, wpg, rpw, streams, chunk,
                              pad_row=rpw if family != "sum" else None)


def test_stream_ladder_gives_every_wave_the_steps_it_names():
    """cases.stream_ladder: with waves_per_gen = len(LADDER), one generation and no hub row, wave w of the plan walks exactly
    LADDER[w] steps, none of them padding, whatever the family, the slot width and the slice count -- and LADDER holds every
    multiple of the batch length up to four batches with both neighbours, 0-5 and a wave of no steps."""
    assert [(f, s, r) for f, s, r in _stream_families()] == [("sum", 2, 32), ("sum", 4, 64), ("sum", 8, 128), ("minmax", 4, 32), ("minmax", 8, 64),
                                                             ("fusedmm", 2, 16), ("fusedmm", 4, 32), ("fusedmm", 8, 64)]
    lad = cases.LADDER
    assert list(lad) == sorted(lad, reverse=True) and lad[-1] == 0
    for b in (32, 64, 96, 128):
        assert {b - 1, b, b + 1} <= set(lad)
    assert {0, 1, 2, 3, 4, 5, 15, 16, 17} <= set(lad) and max(lad) > 4 * 32 + 32
    for family, streams, rpw in _stream_families():
        rowptr, col = cases.stream_ladder(streams)
        deg = np.diff(rowptr)
        assert rowptr.size - 1 == len(lad) * streams and np.array_equal(deg, np.repeat(lad, streams))
        for r in range(deg.size):
            c = col[rowptr[r]:rowptr[r + 1]]
            assert np.all(np.diff(c) >= 0) and (c.size < 2 or np.any(np.diff(c) == 0)), "columns ascend and hold a duplicate"
        for slices in (1, 3):
            p = _plan_of(rowptr, col, 97, slices, len(lad), rpw, streams, 256, family)
            assert p["gens"] == 1 and p["n_hub"] == 0 and p["n_parts"] == 0, (family, streams)
            assert np.array_equal(np.diff(p["wave_step_off"].numpy()), lad), (family, streams)
            assert int((p["perm"] < 0).sum()) == 0 and p["n_steps"] == sum(lad)
            wr = p["wave_row"].numpy().reshape(len(lad), rpw)
            per = rpw // streams
            assert np.array_equal(wr[:, ::per].ravel(), np.arange(deg.size)), "stream i holds row i"


@pytest.mark.parametrize("length", (1, 31, 32, 33, 64, 97))
def test_stream_uneven_wave_is_one_wave_of_that_many_steps_mostly_padding(length):
    for family, streams, rpw in _stream_families():
        rowptr, col = cases.stream_uneven_wave(streams, length)
        assert rowptr.size - 1 == streams
        p = _plan_of(rowptr, col, 97, 2, 1, rpw, streams, 256, family)
        assert p["gens"] == 1 and p["n_hub"] == 0
        assert np.array_equal(p["wave_step_off"].numpy(), [0, length]), (family, streams)
        nnz = length + length // 2 + (1 if streams > 2 else 0)
        assert col.size == nnz and int((p["perm"] < 0).sum()) == streams * length - nnz
        words = p["words"].numpy().astype(np.int64) & 0xFFFFFFFF
        pad = p["perm"].numpy() < 0
        assert np.all((words[pad] & 0xFFFFFF) == 97)
        if family != "sum":
            assert np.all((words[pad] >> 24) == rpw), "max / min and FusedMM plans pad with the spare row"


def test_stream_shape_cases_have_the_plan_shapes_they_are_named_for():
    """cases.stream_shape_cases on the sum / mean and the max / min geometry: hubs, parts and generations follow from the degrees
    (a row over `chunk` edges is a hub of ceil(deg / chunk) parts; a generation holds waves_per_gen * rows_per_wave virtual
    rows), the step counts of the recorded cases are the recorded ones, and every plan lists every edge once."""
    from isplib_amd import cabi
    steps = {"one_row_empty": 0, "one_row_one_edge": 1, "one_row_hub": 50, "all_empty": 0, "hub_threshold": 129}
    for family, geometry in (("sum", cabi.stream_geometry), ("minmax", cabi.stream_minmax_geometry)):
        shapes = cases.stream_shape_cases(geometry(4)[0])
        assert len({c[0] for c in shapes}) == len(shapes) == 12
        seen = {}
        for name, rowptr, col, n, (slices, wpg, streams, chunk) in shapes:
            rpw = geometry(streams)[0]
            m, deg = rowptr.size - 1, np.diff(rowptr)
            p = _plan_of(rowptr, col, n, slices, wpg, rpw, streams, chunk, family)
            parts = -(-deg // chunk)
            nv = int(np.maximum(parts, 1).sum())
            want = dict(n_hub=int((deg > chunk).sum()), n_parts=int(parts[deg > chunk].sum()), gens=max(1, -(-nv // (wpg * rpw))))
            assert {key: p[key] for key in want} == want, (family, name)
            if name in steps:
                assert p["n_steps"] == steps[name], (family, name)
            perm = p["perm"].numpy()
            assert np.array_equal(np.sort(perm[perm >= 0]), np.arange(col.size)), (family, name)
            assert p["n_steps"] == int(p["wave_step_off"][-1]) and perm.size == p["n_steps"] * streams
            wr, wp = p["wave_row"].numpy(), p["wave_part"].numpy()
            assert np.array_equal(np.sort(wr[wr >= 0]), np.repeat(np.arange(m), np.maximum(parts, 1)))
            assert np.array_equal(np.sort(wp[wp >= 0]), np.arange(want["n_parts"])) and np.all(wp[wr < 0] < 0)
            assert int(p["hub_off"][-1]) == want["n_parts"] and p["hub_off"].numel() == want["n_hub"] + 1
            seen[name] = (m, n, deg, p, want, slices, wpg, streams, rpw)
        m, n, deg, p, want, *_ = seen["one_row_hub"]
        assert (m, n, want["n_hub"], want["n_parts"]) == (1, 1, 1, 4)
        assert seen["all_empty"][3]["words"].numel() == 0, "the Python builder hands the entries a null `words`"
        m, n, deg, p, want, slices, *_ = seen["n_below_slices"]
        assert n < slices
        m, n, deg, p, want, *_ = seen["hub_threshold"]
        assert list(deg) == [63, 64, 65, 128, 129] and p["hub_row"].tolist() == [2, 3, 4] and p["hub_off"].tolist() == [0, 2, 4, 7]
        assert np.diff(p["wave_step_off"].numpy()).tolist() == [64, 65]
        m, n, deg, p, want, *_ = seen["hubs_first_and_last"]
        assert p["hub_row"].tolist() == [0, m - 1]
        m, n, deg, p, want, *_ = seen["hubs_adjacent"]
        assert p["hub_row"].tolist() == [2, 3]
        m, n, deg, p, want, *_ = seen["every_row_a_hub"]
        assert want["n_hub"] == m and np.array_equal(p["wave_part"].numpy() >= 0, p["wave_row"].numpy() >= 0), "no whole row"
        m, n, deg, p, want, slices, wpg, streams, rpw = seen["full_gen"]
        assert m == wpg * rpw and want == dict(n_hub=0, n_parts=0, gens=1) and int((p["wave_row"] < 0).sum()) == 0
        m, n, deg, p, want, slices, wpg, streams, rpw = seen["full_gen_plus_one"]
        assert m == wpg * rpw + 1 and want["gens"] == 2 and int((p["wave_row"] >= 0).sum()) == m
        m, n, deg, p, want, slices, wpg, streams, rpw = seen["m_below_streams"]
        assert m < streams and want["gens"] == 1
        wr = p["wave_row"].numpy().reshape(wpg, rpw)
        assert np.all(wr[1] == -1) and np.diff(p["wave_step_off"].numpy()).tolist() == [5, 0], "a wave without rows walks no steps"
