"""iSpLibPlugin -- the reference's drop-in surface (isplib/__init__.py:34-210).

``iSpLibPlugin.patch_pyg()`` swaps ``torch_sparse.matmul`` and
``torch.sparse.mm`` for ``spmm_autotuned`` so that PyG's GCNConv / SAGEConv /
GINConv, which aggregate through ``torch_sparse.matmul(adj_t, x, reduce)``, run
on the HIP kernels unchanged; ``unpatch_pyg()`` restores LIFO;
``@isplib_autotune`` wraps a function in the pair.

Differences from the reference, each a defect there:
  * per-graph operands live on the graph's storage object (or in a table that
    checks the tensors are still the same live objects), not in class-level
    dicts keyed by raw data pointers that go stale (:35-40,50);
  * a ``mean`` call no longer poisons a later ``sum`` on the same graph (:85,141);
  * the mean-backward weights use the intended pairing
    value[csr2csc] / max(rowcount,1)[row[csr2csc]] (csrc/fusedmm.cpp:357-364), not
    the mixed CSR/CSC order of :86-91;
  * unit weights are never materialised (:51-57): ``value=None`` reaches the kernel;
  * max/min return the tensor, like ``torch_sparse.matmul`` does, not the
    ``(out, arg)`` tuple of :143,145 (the tuple stays available at the op level);
  * an unknown ``reduce`` raises ValueError instead of returning None (:154-155);
  * the patched ``torch.sparse.mm`` still serves ordinary torch sparse tensors.

Environment: ISPLIB_SLICES=<n> forces the task list with n column slices (0: plain kernel); ISPLIB_STREAM=0 keeps
sum / mean off the stream schedule; ISPLIB_STREAM_GEOM=streams:slices:chunk forces it with that plan geometry;
ISPLIB_HALF=auto|native|convert picks the route of bf16 / fp16 features (half_route; rows16_route for calls on the plain kernel);
ISPLIB_HALF_MINMAX=convert|native|auto does the same for max / min (rows16_minmax_route), ISPLIB_HALF_MEAN_BW=convert|native|auto
for the backward of a 16-bit `mean` on an unweighted graph (rows16_mean_bw_route), ISPLIB_HALF_DA=convert|native|auto for the value
gradient of a 16-bit sum / mean (rows16_da_route), ISPLIB_HALF_GCN=convert|native|auto for gcn_norm_matmul on 16-bit features
(rows16_gcn_route; unset: such a call raises, as it always did), ISPLIB_HALF_ATTENTION=convert|native|auto for attention_matmul on
16-bit operands (attention16_route; unset: such a call raises, as it always did), ISPLIB_HALF_GAT=convert|native|auto for gat_matmul on
a 16-bit `y` (gat16_route; unset: such a call raises, as it always did), ISPLIB_HALF_GATV2=convert|native|auto for gatv2_matmul on
16-bit `x` and `y` (gatv2_16_route; unset: such a call raises, as it always did), ISPLIB_HALF_MHA=convert|native|auto for mha_matmul
on 16-bit `q`, `k` and `v` (mha16_route; unset: such a call raises, as it always did), and on top of it
ISPLIB_HALF_MHA_DROP=convert|native|auto for such a call with active dropout (mha16_drop_route; unset: convert, and it is read only
where ISPLIB_HALF_MHA is set); the first three default to convert;
ISPLIB_TUNE_FILE names a tuning table to load at import; ISPLIB_DEBUG=1 prints per-operator device times.
"""
from __future__ import annotations

import json
import math
import os
import weakref
from typing import Optional

import torch

from . import _lib
from .sparse import SparseStorage, SparseTensor

_lib.load_ops()

try:  # optional third-party modules the patch targets (absent in this image)
    import torch_sparse as _torch_sparse  # type: ignore
except Exception:  # pragma: no cover
    _torch_sparse = None
try:
    import torch_geometric.typing as _pyg_typing  # type: ignore
except Exception:  # pragma: no cover
    _pyg_typing = None


class _ForeignGraphs:
    """Prepared storage for SparseTensor objects that are not ours (torch_sparse).
    Keyed by data pointers like the reference (:50) but every hit is validated
    against weak references to the very tensors it was built from."""

    def __init__(self):
        self._table = {}

    def get(self, rowptr, col, value, sizes) -> SparseStorage:
        key = (rowptr.data_ptr(), col.data_ptr(), 0 if value is None else value.data_ptr(), col.numel())
        hit = self._table.get(key)
        if hit is not None:
            refs, versions, storage = hit
            same = refs[0]() is rowptr and refs[1]() is col and (value is None or refs[2]() is value)
            if same and versions == (rowptr._version, col._version, None if value is None else value._version):
                return storage
        self._table = {k: v for k, v in self._table.items() if all(r() is not None for r in v[0])}
        storage = SparseStorage(rowptr, col, value, sizes)
        refs = (weakref.ref(rowptr), weakref.ref(col), weakref.ref(value if value is not None else col))
        self._table[key] = (refs, (rowptr._version, col._version, None if value is None else value._version), storage)
        return storage

    def clear(self):
        self._table.clear()


_foreign = _ForeignGraphs()


def _storage_of(src, other: torch.Tensor) -> SparseStorage:
    st = getattr(src, "storage", None)
    if isinstance(st, SparseStorage):
        return st
    rowptr, col, value = src.csr()                                   # :49
    try:
        sizes = tuple(src.sparse_sizes())
    except Exception:
        sizes = (rowptr.numel() - 1, other.size(-2))
    return _foreign.get(rowptr, col, value, sizes)


def suggest_slices(m: int, n: int, nnz: int, k: int, minmax: bool = False) -> int:
    """Column-slice count for an M x N, nnz-entry SpMM over K fp32 features (0 = plain kernel).

    Measured on MI355X (scripts/exp_small.py; DESIGN.md section 5, task-list schedule): (i) a slice of the
    dense operand should be about 7 MB (2x an XCD's 4 MiB L2: the hot rows stay resident); (ii) below that,
    a few slices still pay because they cut rows into more, shorter tasks -- K/20 of them (6 at K=128, 2 at
    K=32) -- as long as the graph has work for the whole chip; (iii) a row must keep ~20 edges per slice or
    per-task overhead and the partial rows eat the gain.  Reddit-shaped graph (mean degree 492): K=32 -> 4,
    K=64 -> 8, K >= 96 with rows of whole cache lines (64-column panels) -> 8, ragged K=100 -> 13, K=602 -> 16;
    a tenth of the graph at K=128 -> 6;
    ogbn-products-shaped (mean degree 50) or under a million edges -> 0 (plain kernel, no preparation)."""
    from . import cabi
    return int(cabi.lib().isplib_suggest_slices(int(m), int(n), int(nnz), int(k), int(bool(minmax))))   # one rule, in the C ABI


# Measured choices that outlive the process: {graph signature: {"rows:k:minmax": ["stream", streams, slices, chunk] |
# ["tasks", slices] | ["plain"]}} (tables from before round 5: a bare slice count).  Filled by
# iSpLibPlugin.autotune, written/merged by save_tuning/load_tuning; ISPLIB_TUNE_FILE names a file read at import.
_tuning_db: dict = {}


def _as_choice(entry):
    """A tuning-table entry as a schedule choice: ("plain",) | ("tasks", slices) | ("stream", streams, slices, chunk).
    Tables written before round 5 hold bare slice counts (0 = plain kernel)."""
    if isinstance(entry, (int, float)):
        return ("tasks", int(entry)) if int(entry) > 0 else ("plain",)
    entry = tuple(entry)
    return (str(entry[0]),) + tuple(int(v) for v in entry[1:])


def tuned_choice(storage: SparseStorage, rows: int, k: int, minmax: bool = False):
    """What `iSpLibPlugin.autotune` measured best for an SpMM of this graph whose dense operand has `rows` rows and k
    columns (this process, or a loaded tuning table keyed by the graph's signature); None = nothing measured: the rules."""
    key = (int(rows), int(k), bool(minmax))
    hit = storage._tuned.get(key)
    if hit is None and _tuning_db:
        entry = _tuning_db.get(graph_signature(storage), {}).get(f"{key[0]}:{key[1]}:{int(key[2])}")
        if entry is not None:
            hit = storage._tuned[key] = _as_choice(entry)
    return hit


def graph_signature(storage: SparseStorage) -> str:
    """Content key of a graph for the persisted tuning table: shape, nnz and the histogram of floor(log2(degree)).
    Two graphs with the same key get the same schedule, which is all the key is for (one host sync, cached)."""
    sig = getattr(storage, "_signature", None)
    if sig is None:
        deg = storage.rowcount()
        hist = torch.bincount(torch.log2(deg.clamp(min=1).to(torch.float32)).to(torch.int64)).tolist() if deg.numel() else []
        m, n = storage.sparse_sizes()
        sig = storage._signature = f"{m}x{n}:{storage._col.numel()}:" + ",".join(str(c) for c in hist)
    return sig


def degree_cv2(rowptr: torch.Tensor) -> float:
    """Squared coefficient of variation of the row degrees (one host sync)."""
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.float64)
    if deg.numel() == 0 or float(deg.sum()) == 0.0:
        return 0.0
    mean = deg.mean()
    return max(0.0, float((deg * deg).mean() / (mean * mean)) - 1.0)


def skew_adjusted(storage_or_rowptr, slices: int, cap: int = 64) -> int:
    """The rule's 7 MB per slice leans on the popularity skew of real degree distributions (hot rows of the dense operand
    stay in the L2).  A graph whose degrees hardly vary (CV^2 < 0.25) has no hot rows and wants slices closer to the L2
    size: half as many columns per slice again (uniform random graph of the Reddit size, K=128: 4.09 -> 3.49 ms on the
    task list; on the stream schedule 31 -> 47 slices: 3.21 -> 3.00 ms).  The same test lives in the C handle
    (graph_runtime.hip)."""
    if slices <= 0:
        return slices
    if isinstance(storage_or_rowptr, torch.Tensor):
        cv2 = degree_cv2(storage_or_rowptr)
    else:
        cv2 = getattr(storage_or_rowptr, "_cv2", None)
        if cv2 is None:
            cv2 = storage_or_rowptr._cv2 = degree_cv2(storage_or_rowptr._rowptr)
    return slices if cv2 >= 0.25 else min(cap, int(1.5 * slices + 0.5))


def choose_slices(storage: SparseStorage, rows: int, k: int, minmax: bool = False, transposed: bool = False) -> int:
    """Slice count for a graph held in `storage` (transposed: for its A^T, the backward's operand; `rows` = rows of the
    dense operand either way): ISPLIB_SLICES=<n> (0 disables) > a count measured by `iSpLibPlugin.autotune` for this
    graph and width (this process, or a loaded tuning file) > the `suggest_slices` rule."""
    env = os.environ.get("ISPLIB_SLICES")
    if env is not None:
        n = int(env)
        return n if 1 <= n <= 4096 else 0
    tuned = tuned_choice(storage, rows, k, minmax)
    if tuned is not None and tuned[0] == "tasks":
        return tuned[1]
    if tuned is not None and tuned[0] == "plain":
        return 0
    ruled = storage._tuned.get((rows, k, minmax, transposed))          # the rule's answer for this side, from last time
    if ruled is not None:
        return ruled
    m, nnz = storage.sparse_sizes()[1 if transposed else 0], storage._col.numel()
    s = skew_adjusted(storage, suggest_slices(m, rows, nnz, k, minmax))
    if s > 0:
        # the panel rule halves the slice count to make tasks long enough; on hub-dominated graphs they are long anyway
        # (>= 120 edges per task on the panel plan) and the whole-row plan, run in one pass, is the better schedule
        from . import cabi
        whole = int(cabi.lib().isplib_suggest_slices_whole_rows(m, rows, nnz, k))
        if whole > s:
            plan_p = storage.plan_t(s) if transposed else storage.plan(s)
            if plan_p and nnz / max(plan_p[0].numel(), 1) >= 120.0:
                s = whole
        storage._tuned[(rows, k, minmax, transposed)] = s
    return s


def choose_stream(storage: SparseStorage, m: int, n: int, k: int, weighted: bool = False):
    """(streams, slices, chunk) when sum / mean of this shape should run on the stream schedule, else None; `weighted`:
    the plan will carry edge weights (the rule then prefers wider column panels: the weight stream is read once per panel).
    ISPLIB_STREAM=0 disables it, ISPLIB_SLICES (the task list's override) disables it too: explicit schedules win."""
    if os.environ.get("ISPLIB_STREAM", "1") == "0" or os.environ.get("ISPLIB_SLICES") is not None:
        return None
    from . import cabi
    if k < cabi.K_MIN or n >= cabi.STREAM_N_END:
        return None
    forced = os.environ.get("ISPLIB_STREAM_GEOM")          # "streams:slices:chunk": tests and experiments
    if forced:
        return tuple(int(v) for v in forced.split(":"))
    tuned = tuned_choice(storage, n, k, False)             # a measured choice for this graph and width beats the rule
    if tuned is not None:
        return tuple(tuned[1:]) if tuned[0] == "stream" else None
    return stream_rule(storage, m, n, k, weighted)


def stream_rule(storage: SparseStorage, m: int, n: int, k: int, weighted: bool = False):
    """The rule's own answer (isplib_suggest_stream_weighted + the degree-skew adjustment), whatever was tuned."""
    from . import cabi
    geom = cabi.suggest_stream(m, n, storage._col.numel(), k, weighted)
    return None if geom is None else (geom[0], skew_adjusted(storage, geom[1], cap=512), geom[2])


def choose_stream_minmax(storage: SparseStorage, m: int, n: int, k: int):
    """(streams, slices, chunk) when max / min of this shape should run on the stream schedule (column-sorted rows; the
    plan builder has the last word), else None.  Same switches as choose_stream."""
    if os.environ.get("ISPLIB_STREAM", "1") == "0" or os.environ.get("ISPLIB_SLICES") is not None:
        return None
    from . import cabi
    if k < cabi.K_MIN or n >= cabi.STREAM_N_END or storage._col.numel() >= cabi.STREAM_NNZ_END:
        return None
    forced = os.environ.get("ISPLIB_STREAM_MINMAX_GEOM")   # "streams:slices:chunk": tests and experiments
    if forced:
        return tuple(int(v) for v in forced.split(":"))
    tuned = tuned_choice(storage, n, k, True)
    if tuned is not None:
        return tuple(tuned[1:]) if tuned[0] == "stream" else None
    return stream_minmax_rule(storage, m, n, k)


def stream_minmax_rule(storage: SparseStorage, m: int, n: int, k: int):
    """The rule's own answer for max / min (isplib_suggest_stream_minmax + the degree-skew adjustment)."""
    from . import cabi
    geom = cabi.suggest_stream_minmax(m, n, storage._col.numel(), k)
    return None if geom is None else (geom[0], skew_adjusted(storage, geom[1], cap=512), geom[2])


HALF_DTYPES = (torch.bfloat16, torch.float16)


def half_route(dtype, reduce: str, k: int, pitch: int, mode: Optional[str] = None, streams: Optional[int] = 4, weighted: bool = False,
               n: int = 1, nnz: int = 0) -> str:
    """Which way a matmul with features of `dtype` goes: "fp32" (float32: the path as it always was), "native" (bf16 / fp16 on
    the 16-bit stream kernel, fusedMM_csr_stream16_hip) or "convert" (bf16 / fp16 through `x.float()` -> the fp32 path -> `.to(dtype)`:
    the same result, the finished fp32 row rounded once).  Any other dtype raises TypeError.  A pure function -- no device, no
    library call:
      * native needs a sum / mean, a stream plan for the call (`streams` = its slot count; None: the call has none) and a shape
        inside the entry's domain (cabi.stream16_serves) at the operand's own row pitch or, failing that, packed (pitch = k);
      * `mode` is ISPLIB_HALF (None: read from the environment; default "auto"): "convert" always converts, "native" goes native
        wherever the above holds, "auto" only in the classes (slot width x weighted plan) where every native run measured faster
        than every run of the conversion route (cabi.stream16_native_pays, profiles/stream16_ab.txt).  None of them raises."""
    if dtype == torch.float32:
        return "fp32"
    if dtype not in HALF_DTYPES:
        raise TypeError(f"isplib_amd: features must be float32, bfloat16 or float16, got {dtype}")
    from . import cabi
    if mode is None:
        mode = os.environ.get("ISPLIB_HALF", "auto")
    if mode == "convert" or reduce not in ("sum", "add", "mean") or streams is None:
        return "convert"
    if not (cabi.stream16_serves(n, k, pitch, k, nnz) or cabi.stream16_serves(n, k, k, k, nnz)):
        return "convert"
    if mode == "native":
        return "native"
    return "native" if cabi.stream16_native_pays(int(streams), bool(weighted)) else "convert"


def _rows16_gate(dtype, mode: Optional[str], opt_in: Optional[str], n: int, k: int, pitch: int, pays) -> str:
    """The gate the three routes of the 16-bit row family share: 16-bit features, the mode, and the entry's domain
    (cabi.rows16_serves) at the operand's own row pitch or, failing that, packed.  `mode` None is read from the environment:
    ISPLIB_HALF (default "auto") when `opt_in` is None, else the variable `opt_in` names (default "convert"; ISPLIB_HALF=convert wins
    over it, and only "native" / "auto" leave the conversion route).  `pays(cabi, ld)` is the route's own measured class table,
    asked under "auto" at the pitch the entry would be given."""
    if dtype not in HALF_DTYPES:
        return "convert"
    from . import cabi
    if mode is None:
        mode = os.environ.get("ISPLIB_HALF", "auto")
        if opt_in is not None and mode != "convert":
            mode = os.environ.get(opt_in, "convert")
    if mode == "convert" or (opt_in is not None and mode not in ("native", "auto")):
        return "convert"
    if cabi.rows16_serves(n, k, pitch, k):
        ld = pitch
    elif cabi.rows16_serves(n, k, k, k):
        ld = k
    else:
        return "convert"
    return "rows16" if mode == "native" or pays(cabi, ld) else "convert"


def rows16_route(dtype, reduce: str, k: int, pitch: int, mode: Optional[str] = None, n: int = 1, ordered: bool = False,
                 weighted: bool = False) -> str:
    """Which way a matmul with 16-bit features goes when half_route said "convert", the call has no stream plan and the plain
    row-per-wave kernel serves it: "rows16" (the 16-bit row kernel, fusedMM_csr_rows16_hip: no fp32 copy of the operand, half the
    gathered bytes) or "convert".  A pure function -- no device, no library call:
      * rows16 needs a sum / mean of bf16 / fp16 features and a shape inside the entry's domain (cabi.rows16_serves) at the
        operand's own row pitch or, failing that, packed (pitch = k);
      * `mode` is ISPLIB_HALF (None: read from the environment; default "auto"): "convert" always converts, "native" takes the
        kernel wherever the above holds, "auto" only in the classes -- (operand beyond 256 MiB or not) x `ordered` (the rows come
        in a community order) x `weighted` -- where every native run measured faster than every run of the conversion route
        (cabi.rows16_native_pays, profiles/rows16_ab.txt).  Nothing raises."""
    if reduce not in ("sum", "add", "mean"):
        return "convert"
    return _rows16_gate(dtype, mode, None, n, k, pitch, lambda cabi, ld: cabi.rows16_native_pays(n, ld, bool(ordered), bool(weighted)))


def rows16_minmax_route(dtype, reduce: str, k: int, pitch: int, mode: Optional[str] = None, n: int = 1, ordered: bool = False,
                        weighted: bool = False, want_arg: bool = True) -> str:
    """Which way a max / min matmul with 16-bit features goes when the call has no stream plan and the plain row-per-wave kernel
    serves it: "rows16" (the 16-bit max / min row kernel, fusedMM_csr_rows16_minmax_hip: no fp32 copy of the operand, half the
    gathered bytes, values and positions bit-equal to the conversion route) or "convert".  A pure function -- no device, no library
    call:
      * rows16 needs a max / min of bf16 / fp16 features and a shape inside the entry's domain (cabi.rows16_serves) at the
        operand's own row pitch or, failing that, packed (pitch = k);
      * `mode` is ISPLIB_HALF_MINMAX (None: read from the environment; default "convert", and ISPLIB_HALF=convert wins over it):
        "convert" always converts, "native" takes the kernel wherever the above holds, "auto" only in the classes -- those of
        rows16_route x `want_arg` (positions wanted) -- where every native run measured faster than every run of the conversion
        route (cabi.rows16_minmax_native_pays, profiles/rows16_minmax_ab.txt).  Nothing raises."""
    if reduce not in ("max", "min"):
        return "convert"
    return _rows16_gate(dtype, mode, "ISPLIB_HALF_MINMAX", n, k, pitch,
                        lambda cabi, ld: cabi.rows16_minmax_native_pays(n, ld, bool(ordered), bool(weighted), bool(want_arg)))


def rows16_mean_bw_route(dtype, k: int, m_rows: int, ordered: bool = False, mode: Optional[str] = None) -> str:
    """Which way the backward of a `mean` with 16-bit features on an UNWEIGHTED graph goes when the plain row-per-wave kernel
    serves its SpMM on A^T: "rows16" (the column-scaled 16-bit row kernel, fusedMM_csr_rows16_colscale_hip, on dY as it is: 1 / deg
    is applied per gathered row inside the kernel -- no fp32 dY / deg, no conversion of dX) or "convert" (widen dY, divide, the fp32
    row kernel, narrow dX).  A pure function -- no device, no library call:
      * rows16 needs bf16 / fp16 and dY's shape, [m_rows, k] packed, inside the entry's domain (cabi.rows16_serves);
      * `mode` is ISPLIB_HALF_MEAN_BW (None: read from the environment; default "convert", and ISPLIB_HALF=convert wins over it):
        "convert" always converts, "native" takes the kernel wherever the above holds, "auto" only in the classes -- (dY beyond
        256 MiB or not) x `ordered` (the rows of A^T come in a community order) -- where every native run measured faster than
        every run of the conversion route (cabi.rows16_colscale_native_pays, profiles/rows16_colscale_ab.txt).  Nothing raises."""
    return _rows16_gate(dtype, mode, "ISPLIB_HALF_MEAN_BW", m_rows, k, k, lambda cabi, ld: cabi.rows16_colscale_native_pays(m_rows, k, bool(ordered)))


def rows16_da_route(dtype, k: int, pitch: int, n: int, ordered: bool = False, mode: Optional[str] = None, whole_row_slices: int = 0) -> str:
    """Which way the value gradient (dA, the SDDMM) of a sum / mean with 16-bit features goes when its forward went to the 16-bit
    row kernel: "rows16" (the 16-bit SDDMM row kernel, isplib_sddmm_csr_rows16_hip, on X and dY as they are: no fp32 copy of either,
    half the gathered bytes, dA in fp32) or "convert" (widen both, the fp32 SDDMM).  A pure function -- no device, no library call:
      * rows16 needs bf16 / fp16 and X's shape, [n, k] at its own row pitch or, failing that, packed, inside the entry's domain
        (cabi.sddmm_rows16_serves: the row kernel's, and k <= 1024);
      * `whole_row_slices` > 0 (isplib_suggest_slices_whole_rows for the graph): the handle's task-list SDDMM keeps the graph --
        "convert", whatever the mode;
      * `mode` is ISPLIB_HALF_DA (None: read from the environment; default "convert", and ISPLIB_HALF=convert wins over it):
        "convert" always converts, "native" takes the kernel wherever the above holds, "auto" only in the classes -- (X beyond
        256 MiB or not) x `ordered` (the rows come in a community order) -- where every native run measured faster than every run
        of the conversion route (cabi.sddmm_rows16_native_pays, profiles/sddmm_rows16_ab.txt).  Nothing raises."""
    if whole_row_slices > 0 or k > 1024:
        return "convert"
    return _rows16_gate(dtype, mode, "ISPLIB_HALF_DA", n, k, pitch, lambda cabi, ld: cabi.sddmm_rows16_native_pays(n, ld, bool(ordered)))


def rows16_gcn_route(dtype, k: int, pitch: int, n: int, ordered: bool = False, mode: Optional[str] = None) -> str:
    """Which way gcn_norm_matmul with 16-bit features goes once ISPLIB_HALF_GCN is set: "rows16" (the 16-bit row kernel with the fused
    epilogue, fusedMM_csr_rows16_epilogue_hip, forward and backward: X is gathered as it lies, D^-1/2 per gathered row, self loop, left
    D^-1/2, bias and ReLU on the finished fp32 row, rounded once -- no fp32 [N, K] tensor in either direction) or "convert"
    (`x.float()` -> the fp32 layer -> `.to(dtype)`).  A pure function -- no device, no library call:
      * rows16 needs bf16 / fp16 and X's shape, [n, k] at its own row pitch or, failing that, packed, inside the entry's domain
        (cabi.rows16_serves);
      * `mode` is ISPLIB_HALF_GCN (None: read from the environment; unset counts as "convert" here -- gcn_norm_matmul itself raises
        before it asks -- and ISPLIB_HALF=convert wins over it): "convert" always converts, "native" takes the kernel wherever the
        above holds, "auto" only in the classes -- (X beyond 256 MiB or not) x `ordered` (the rows come in a community order) -- where
        every native run measured faster than every run of the conversion route (cabi.rows16_gcn_native_pays,
        profiles/rows16_gcn_ab.txt).  Nothing raises."""
    return _rows16_gate(dtype, mode, "ISPLIB_HALF_GCN", n, k, pitch, lambda cabi, ld: cabi.rows16_gcn_native_pays(n, ld, bool(ordered)))


def attention16_route(dtype, k: int, pitch: int, n: int, mode: Optional[str] = None) -> str:
    """Which way attention_matmul with 16-bit operands goes once ISPLIB_HALF_ATTENTION is set, asked per GATHERED operand (y with its
    rows for the forward, x with its rows for the backward over the columns): "attention16" (torch.ops.isplib.attention_spmm16 on the
    16-bit kernels, isplib_attention16_*_hip: x, y and the gradients as they lie, half the gathered bytes, no fp32 [*, K] tensor in
    either direction) or "convert" (`x.float()` -> the fp32 operator -> `.to(dtype)`).  A pure function -- no device, no library call:
      * attention16 needs bf16 / fp16 and the operand's shape, [n, k] at its own row pitch or, failing that, packed, inside the
        entries' domain (cabi.attention16_serves: 8 <= k <= 512, k and the pitch even);
      * `mode` is ISPLIB_HALF_ATTENTION (None: read from the environment; unset counts as "convert" here -- attention_matmul itself
        raises before it asks -- and ISPLIB_HALF=convert wins over it): "convert" always converts, "native" takes the kernels wherever
        the above holds, "auto" only in the classes -- the gathered operand beyond 256 MiB or not -- where every native run measured
        faster than every run of the conversion route (cabi.attention16_native_pays, profiles/attention16_ab.txt).  Nothing raises."""
    if dtype not in HALF_DTYPES:
        return "convert"
    from . import cabi
    if mode is None:
        mode = os.environ.get("ISPLIB_HALF", "auto")
        if mode != "convert":
            mode = os.environ.get("ISPLIB_HALF_ATTENTION", "convert")
    if mode not in ("native", "auto"):
        return "convert"
    if cabi.attention16_serves(n, k, pitch):
        ld = pitch
    elif cabi.attention16_serves(n, k, k):
        ld = k
    else:
        return "convert"
    return "attention16" if mode == "native" or cabi.attention16_native_pays(n, ld) else "convert"


def gat16_route(dtype, heads: int, d: int, pitch: int, n: int, mode: Optional[str] = None) -> str:
    """Which way gat_matmul with a 16-bit `y` goes once ISPLIB_HALF_GAT is set, asked per GATHERED wide operand (y with its rows for the
    forward and the rows kernel, the gradient with its rows, packed, for the backward over the columns): "gat16"
    (torch.ops.isplib.gat_spmm16 on the 16-bit kernels, isplib_gat16_*_hip: y and the gradients as they lie, half the gathered bytes, no
    fp32 [*, K] tensor in either direction) or "convert" (`y.float()` -> the fp32 operator -> `.to(dtype)`).  A pure function -- no
    device, no library call:
      * gat16 needs bf16 / fp16 and the operand's shape, [n, heads * d] at its own row pitch or, failing that, packed, inside the
        entries' domain (cabi.gat16_serves: 8 <= heads * d <= 512, heads == 1 with d even or d a power of two >= 8, the pitch even);
      * `mode` is ISPLIB_HALF_GAT (None: read from the environment; unset counts as "convert" here -- gat_matmul itself raises before
        it asks -- and ISPLIB_HALF=convert wins over it): "convert" always converts, "native" takes the kernels wherever the above
        holds, "auto" only in the classes -- the gathered operand beyond 256 MiB or not -- where every native run measured faster than
        every run of the conversion route (cabi.gat16_native_pays, profiles/gat16_ab.txt).  Nothing raises."""
    if dtype not in HALF_DTYPES:
        return "convert"
    from . import cabi
    if mode is None:
        mode = os.environ.get("ISPLIB_HALF", "auto")
        if mode != "convert":
            mode = os.environ.get("ISPLIB_HALF_GAT", "convert")
    if mode not in ("native", "auto"):
        return "convert"
    k = heads * d
    if cabi.gat16_serves(n, heads, d, pitch):
        ld = pitch
    elif cabi.gat16_serves(n, heads, d, k):
        ld = k
    else:
        return "convert"
    return "gat16" if mode == "native" or cabi.gat16_native_pays(n, ld) else "convert"


def gatv2_16_route(dtype, heads: int, d: int, pitch: int, n: int, mode: Optional[str] = None) -> str:
    """Which way gatv2_matmul with 16-bit `x` and `y` goes once ISPLIB_HALF_GATV2 is set, asked per GATHERED wide operand (y with its
    rows for the forward and the rows kernel; x with its rows and the gradient with its rows, packed, for the backward over the
    columns): "gatv2_16" (torch.ops.isplib.gatv2_spmm16 on the 16-bit kernels, isplib_gatv2_16_*_hip: x, y and the gradients as they
    lie, half the gathered bytes, no fp32 [*, K] tensor in either direction) or "convert" (`x.float()`, `y.float()` -> the fp32
    operator -> `.to(dtype)`).  A pure function -- no device, no library call:
      * gatv2_16 needs bf16 / fp16 and the operand's shape, [n, heads * d] at its own row pitch or, failing that, packed, inside the
        entries' domain (cabi.gatv2_16_serves = gat16_serves: 8 <= heads * d <= 512, heads == 1 with d even or d a power of two >= 8,
        the pitch even);
      * `mode` is ISPLIB_HALF_GATV2 (None: read from the environment; unset counts as "convert" here -- gatv2_matmul itself raises
        before it asks -- and ISPLIB_HALF=convert wins over it): "convert" always converts, "native" takes the kernels wherever the
        above holds, "auto" only in the classes -- the gathered operand beyond 256 MiB or not -- where every native run measured
        faster than every run of the conversion route (cabi.gatv2_16_native_pays, profiles/gatv2_16_ab.txt).  Nothing raises."""
    if dtype not in HALF_DTYPES:
        return "convert"
    from . import cabi
    if mode is None:
        mode = os.environ.get("ISPLIB_HALF", "auto")
        if mode != "convert":
            mode = os.environ.get("ISPLIB_HALF_GATV2", "convert")
    if mode not in ("native", "auto"):
        return "convert"
    k = heads * d
    if cabi.gatv2_16_serves(n, heads, d, pitch):
        ld = pitch
    elif cabi.gatv2_16_serves(n, heads, d, k):
        ld = k
    else:
        return "convert"
    return "gatv2_16" if mode == "native" or cabi.gatv2_16_native_pays(n, ld) else "convert"


def mha16_route(dtype, heads: int, d: int, pitch: int, n: int, mode: Optional[str] = None) -> str:
    """Which way mha_matmul with 16-bit `q`, `k` and `v` goes once ISPLIB_HALF_MHA is set, asked per GATHERED wide operand (k and v with
    their rows for the forward and the rows kernel; q with its rows and the gradient with its rows, packed, for the backward over the
    columns): "mha16" (torch.ops.isplib.mha_spmm16 on the 16-bit kernels, isplib_qkv16_*_hip: q, k, v and the gradients as they lie,
    half the gathered bytes, no fp32 [*, K] tensor in either direction) or "convert" (`.float()` -> the fp32 operator ->
    `.to(dtype)`).  A pure function -- no device, no library call:
      * mha16 needs bf16 / fp16 and the operand's shape, [n, heads * d] at its own row pitch or, failing that, packed, inside the
        entries' domain (cabi.mha16_serves = gat16_serves: 8 <= heads * d <= 512, heads == 1 with d even or d a power of two >= 8,
        the pitch even);
      * `mode` is ISPLIB_HALF_MHA (None: read from the environment; unset counts as "convert" here -- mha_matmul itself raises before
        it asks -- and ISPLIB_HALF=convert wins over it): "convert" always converts, "native" takes the kernels wherever the above
        holds, "auto" only in the classes -- the gathered operand beyond 256 MiB or not -- where every native run measured faster than
        every run of the conversion route (cabi.mha16_native_pays, profiles/mha16_ab.txt).  Nothing raises."""
    if dtype not in HALF_DTYPES:
        return "convert"
    from . import cabi
    if mode is None:
        mode = os.environ.get("ISPLIB_HALF", "auto")
        if mode != "convert":
            mode = os.environ.get("ISPLIB_HALF_MHA", "convert")
    if mode not in ("native", "auto"):
        return "convert"
    k = heads * d
    if cabi.mha16_serves(n, heads, d, pitch):
        ld = pitch
    elif cabi.mha16_serves(n, heads, d, k):
        ld = k
    else:
        return "convert"
    return "mha16" if mode == "native" or cabi.mha16_native_pays(n, ld) else "convert"


def mha16_drop_route(dtype, heads: int, d: int, pitch: int, n: int, mode: Optional[str] = None) -> str:
    """Which way mha_matmul with 16-bit `q`, `k` and `v` AND active dropout goes once ISPLIB_HALF_MHA is set, asked per GATHERED wide
    operand as mha16_route is: "mha16drop" (torch.ops.isplib.mha_drop_spmm16 on the 16-bit DROP kernels, isplib_qkv_half_drop_*_hip) or
    "convert" (`.float()` -> the fp32 dropout operator -> `.to(dtype)`).  A pure function -- no device, no library call:
      * "mha16drop" only where mha16_route says "mha16" for the operand: ISPLIB_HALF=convert, ISPLIB_HALF_MHA=convert (or unset) and the
        family's domain all win;
      * on top of that `mode`, which is ISPLIB_HALF_MHA_DROP (None: read from the environment; unset counts as "convert"), must be
        "native", or "auto" with cabi.mha16_drop_native_pays(n, ld) for the pitch the operand goes in at -- the classes in which every
        native run measured faster than every run of the conversion route (profiles/mha16_dropout_ab.txt).  Nothing raises."""
    if mha16_route(dtype, heads, d, pitch, n) != "mha16":
        return "convert"
    from . import cabi
    if mode is None:
        mode = os.environ.get("ISPLIB_HALF_MHA_DROP", "convert")
    if mode == "native":
        return "mha16drop"
    if mode != "auto":
        return "convert"
    ld = pitch if cabi.mha16_serves(n, heads, d, pitch) else heads * d
    return "mha16drop" if cabi.mha16_drop_native_pays(n, ld) else "convert"


_ROWS16_MARK = torch.tensor([16], dtype=torch.int32)      # second tensor of a 16-bit row plan (torch_ops.cpp: is_rows16_plan)
_ROWS16_DA_MARK = torch.tensor([0xDA], dtype=torch.int32)  # third tensor of a forward plan whose dA runs in 16 bits (is_rows16_da_plan)


def _rows16_plan(s: SparseStorage, transposed: bool, k: int, device) -> list:
    """[row order or an empty int32 tensor (index order), marker]: the plan form that sends a 16-bit operand to the row kernel."""
    order = s.row_order(transposed, k, itemsize=2)
    return [order[0] if order else torch.empty(0, dtype=torch.int32, device=device), _ROWS16_MARK]


def _rows16_plan_where(goes, s: SparseStorage, transposed: bool, k: int, device) -> Optional[list]:
    """The 16-bit row plan of a call whose route, goes(ordered) -> bool, says "rows16", else None.  `ordered` is what the kernel
    will be given, so the community order (judged at 2 bytes per element) is looked for only when some answer to it can send the
    call there, and the route is then asked about the order that was found."""
    if not (goes(False) or goes(True)):
        return None
    plan = _rows16_plan(s, transposed, k, device)
    return plan if goes(plan[0].numel() > 0) else None


def spmm_autotuned(src, other: torch.Tensor, reduce: str = "sum") -> torch.Tensor:
    """``torch_sparse.matmul(src, other, reduce)`` on the HIP path (isplib/__init__.py:48-157)."""
    if reduce not in ("sum", "add", "mean", "max", "min"):
        raise ValueError(f"isplib: unknown reduce '{reduce}' (expected sum|add|mean|max|min)")
    if not isinstance(other, torch.Tensor) or not other.is_cuda:
        raise RuntimeError("isplib_amd: `other` must be a GPU tensor -- there is no CPU path")
    if other.dtype != torch.float32 and other.dtype not in HALF_DTYPES:
        raise TypeError(f"isplib_amd: features must be float32, bfloat16 or float16 (csrc/fusedmm.cpp:44 takes float32 only), got {other.dtype}")
    half = other.dtype != torch.float32
    s = _storage_of(src, other)
    rowptr, col, value = s._rowptr, s._col, s._value
    if value is not None and value.dtype != (torch.float32 if half else other.dtype):
        value = value.to(torch.float32 if half else other.dtype)     # :63-64 (16-bit features: the weights stay fp32)
    squeeze = other.dim() == 1
    mat = other.unsqueeze(-1) if squeeze else other
    needs_grad = torch.is_grad_enabled() and mat.requires_grad       # :69-73
    ops = torch.ops.isplib
    k = mat.size(-1)
    m_rows = rowptr.numel() - 1
    # sum / mean on graphs with work for the whole chip: the stream schedule (rows resident in LDS, the plan's own copy
    # of the edges; include/isplib_hip.h: fusedMM_csr_stream_hip) -- measured 15-18 % ahead of the task list
    if reduce in ("sum", "add", "mean"):
        geom = choose_stream(s, m_rows, mat.size(0), k, s._value is not None)
        plan = s.stream_plan(False, geom) if geom is not None else None
    else:                                                            # max / min: its own kernel geometry, sorted rows only
        geom = choose_stream_minmax(s, m_rows, mat.size(0), k)
        plan = s.stream_plan(False, geom, "minmax") if geom is not None else None
    ran = ("stream",) + tuple(int(v) for v in geom) if plan is not None else None
    rows16 = False
    if half:
        # bf16 / fp16 features: the 16-bit stream kernel on the same plan, or the conversion route (half_route)
        pitch = mat.stride(0) if mat.dim() == 2 and mat.size(0) > 1 and mat.stride(-1) == 1 else k
        route = half_route(mat.dtype, reduce, k, pitch, None, None if plan is None else int(geom[0]), s._value is not None,
                           mat.size(0), col.numel())
        if route == "convert" and plan is None and mat.dim() == 2 and reduce in ("sum", "add", "mean") and not s.plan(choose_slices(s, mat.size(0), k)):
            # no stream plan, and the plain kernel would serve the fp32 call: the 16-bit row kernel where rows16_route says so
            weighted = s._value is not None
            plan = _rows16_plan_where(lambda ordered: rows16_route(mat.dtype, reduce, k, pitch, None, mat.size(0), ordered, weighted) == "rows16",
                                      s, False, k, mat.device)
            rows16 = plan is not None
        if route == "convert" and plan is None and mat.dim() == 2 and reduce in ("max", "min") and \
                os.environ.get("ISPLIB_HALF_MINMAX", "convert") != "convert" and not s.plan(choose_slices(s, mat.size(0), k, True)):
            # max / min, opt-in (ISPLIB_HALF_MINMAX): the same question put to rows16_minmax_route; positions are wanted exactly when
            # the call below goes to the *_planned operators
            weighted = s._value is not None
            want_arg = needs_grad or (value is not None and torch.is_grad_enabled() and value.requires_grad)
            plan = _rows16_plan_where(
                lambda ordered: rows16_minmax_route(mat.dtype, reduce, k, pitch, None, mat.size(0), ordered, weighted, want_arg) == "rows16",
                s, False, k, mat.device)
            rows16 = plan is not None
        if rows16:
            ran = ("rows16mm" if reduce in ("max", "min") else "rows16",) + (("ordered",) if plan[0].numel() > 0 else ())
        elif route == "convert":
            out = spmm_autotuned(src, other.to(torch.float32), reduce)
            s._last_schedule = ("convert",) + tuple(s._last_schedule or ())
            return out.to(other.dtype)
        else:
            ran = ("stream16",) + tuple(int(v) for v in geom)
    if plan is None:
        n_sl = choose_slices(s, mat.size(0), k, reduce in ("max", "min"))
        plan = s.plan(n_sl)                                          # per-graph, built once on the device
        ran = ("tasks", int(n_sl)) if plan else ("plain",)
        if not plan:                                                 # the plain kernel: rows in a community order where that pays
            plan = s.row_order(False, k)
    s._last_schedule = ran                                           # what this call's forward runs on (autotune checks it)
    if reduce in ("sum", "add", "mean"):
        colptr = val_t = row_t = None
        plan_t = []
        if rows16 and value is not None and torch.is_grad_enabled() and value.requires_grad and \
                os.environ.get("ISPLIB_HALF_DA", "convert") != "convert":
            # dA of a row-kernel call, opt-in (ISPLIB_HALF_DA): rows16_da_route's answer travels with the plan as a second marker,
            # which the operator strips before its forward and reads in its backward
            from . import cabi
            whole = int(cabi.lib().isplib_suggest_slices_whole_rows(m_rows, mat.size(0), col.numel(), k)) if k >= 4 else 0
            if rows16_da_route(mat.dtype, k, pitch, mat.size(0), plan[0].numel() > 0, None, whole) == "rows16":
                plan = list(plan) + [_ROWS16_DA_MARK]
        if needs_grad:                                               # :76-80 / :83-99 (built once per graph)
            colptr, row_t = s.colptr(), s.row_t()
            # mean: the intended pairing, val[csr2csc] / max(deg, 1) -- for an unweighted graph that is
            # 1 / deg of the edge's row in A, which the operator applies to the rows of dY instead: no weights at all
            unit_mean = reduce == "mean" and s._value is None
            val_t = None if unit_mean else (s.mean_val_t() if reduce == "mean" else s.val_t())
            geom_t = choose_stream(s, mat.size(0), m_rows, k, val_t is not None)
            if rows16 and not unit_mean and geom_t is not None and \
                    half_route(mat.dtype, reduce, k, k, None, int(geom_t[0]), val_t is not None, m_rows, col.numel()) == "convert":
                # the operators run a 16-bit dY on a stream plan natively whatever the mode: where half_route would convert
                # (auto: the 16-bit stream kernel never pays), the backward of a row-kernel call stays off the stream plan
                geom_t = None
            plan_t = s.stream_plan(True, geom_t, "mean" if reduce == "mean" and not unit_mean else "sum") if geom_t is not None else None
            if plan_t is None:
                plan_t = s.plan_t(choose_slices(s, m_rows, k, transposed=True))
                if not plan_t:
                    # the backward (A^T dY) of a 16-bit call: the same route under the same rule, on the transposed arrays.  The
                    # unit-weight mean backward forms dY / deg in fp32 first: an fp32 operand, its row order judged at 4 bytes --
                    # unless rows16_mean_bw_route (opt-in: ISPLIB_HALF_MEAN_BW) sends it to the column-scaled 16-bit kernel, which
                    # takes dY as it is and 1 / deg as a table
                    plan16 = None
                    if half and not unit_mean:         # (dY: [m_rows, k], packed, of mat's dtype)
                        weighted_t = val_t is not None
                        plan16 = _rows16_plan_where(lambda ordered: rows16_route(mat.dtype, reduce, k, k, None, m_rows, ordered, weighted_t) == "rows16",
                                                    s, True, k, mat.device)
                    elif half:
                        plan16 = _rows16_plan_where(lambda ordered: rows16_mean_bw_route(mat.dtype, k, m_rows, ordered) == "rows16", s, True, k, mat.device)
                        plan16 = plan16 + [s.inv_rowcount()] if plan16 is not None else None
                    plan_t = plan16 if plan16 is not None else s.row_order(True, k)
        if reduce == "mean":
            out = ops.fusedmm_spmm_mean_planned(rowptr, col, value, colptr, mat, row_t, val_t, plan, plan_t)
        else:
            out = ops.fusedmm_spmm_planned(rowptr, col, value, colptr, mat, val_t, row_t, plan, plan_t)
    elif not needs_grad and not (value is not None and torch.is_grad_enabled() and value.requires_grad):
        # max / min with nothing to differentiate (inference): the patched matmul returns the tensor alone (:143,145), so the
        # winners' positions would be computed and dropped -- the values-only launch leaves them out (stream plans: 12 % less)
        out = (ops.fusedmm_spmm_max_values if reduce == "max" else ops.fusedmm_spmm_min_values)(rowptr, col, value, mat, plan)
    elif reduce == "max":
        out = ops.fusedmm_spmm_max_planned(rowptr, col, value, mat, plan)[0]   # :143
    else:
        out = ops.fusedmm_spmm_min_planned(rowptr, col, value, mat, plan)[0]   # :145
    return out.squeeze(-1) if squeeze else out


matmul = spmm_autotuned


def fusedmm(src, x: Optional[torch.Tensor], y: torch.Tensor, pattern="sigmoid_embedding", sop_param: float = 0.0,
            sop_udef: Optional[str] = None) -> torch.Tensor:
    """The generic FusedMM pipeline over the stored entries of `src` (include/isplib_hip.h, fusedMM_csr_udef_hip):
    ``z[i] = AOP_j VSC(SOP(ROP(VOP(x[i], y[j]))))``.  `pattern` is a name from ``cabi.PATTERNS`` (sigmoid_embedding,
    tdist_embedding, attention_sum, spmm) or a raw message word built from ``cabi.VOP/ROP/SOP/VSC/AOP``; for a raw
    word with SOP_UDEF, `sop_udef` names the built-in function.  Forward only (the reference has no such op:
    these words are defined by csrc/fusedMM.h:18-74 but never sent by iSpLib)."""
    from . import cabi
    if isinstance(pattern, str):
        word, fn = cabi.PATTERNS[pattern]
    else:
        word, fn = int(pattern), (sop_udef or "none")
    if y.dim() != 2:
        raise ValueError(f"isplib_amd: `y` must be 2-D [n, k], got shape {tuple(y.shape)}")
    st = _storage_of(src, y)
    k = y.size(1)
    m_rows = st._rowptr.numel() - 1
    # before any library call: the kernels read x[i] for every row and y[j] for every stored column id, and the plans
    # cached on the storage were built for its column count
    cabi.check_fusedmm_operands(word, m_rows, x, y)
    if y.size(0) != st._sparse_sizes[1]:
        raise ValueError(f"isplib_amd: `y` must have one row per column of the sparse matrix ({st._sparse_sizes[1]}), got {y.size(0)}")
    # the two hot SDDMM-fused words on graphs with work for the whole chip: the stream front end (rows of x and z resident in
    # LDS; include/isplib_hip.h: fusedMM_csr_udef_stream_hip) -- Reddit shape K=128: 6.3 ms on the task list below
    geom = None
    if x is not None and x.is_contiguous() and y.is_contiguous() and os.environ.get("ISPLIB_STREAM", "1") != "0" and os.environ.get("ISPLIB_SLICES") is None:
        geom = cabi.suggest_fusedmm_stream(word, m_rows, y.size(0), st._col.numel(), k)
    if geom is not None:
        plans = st.__dict__.setdefault("_fusedmm_streams", {})
        if geom not in plans:
            try:
                plans[geom] = cabi.NativeStreamPlan(st._rowptr, st._col, None, y.size(0), geom[0], geom[1], geom[2], 0, fusedmm=True)
            except cabi.IsplibError:
                plans[geom] = None                        # outside the builder's domain / no room: the task list serves the call
        if plans[geom] is not None:
            kind = sop_udef or fn
            return cabi.fusedmm_stream(word, st._rowptr, st._col.numel(), plans[geom], x, y, sop_udef=kind, sop_param=sop_param)[1]
    # the reduce stage needs whole rows of y, so there are no column panels here: slices for the full width
    plan = None
    nbytes = y.size(0) * k * 4
    slices = int(cabi.lib().isplib_suggest_slices_whole_rows(st._rowptr.numel() - 1, y.size(0), st._col.numel(), k))
    if 4 <= k <= 1024 and slices > 0 and nbytes >= (14 << 20):
        held = st.plan(slices)
        if held:
            from .plan import TaskPlan
            plan = TaskPlan(slices, held[0].numel(), held[0], held[1], held[2], held[3], [int(v) for v in held[4]], 1024, 128, held[5])
    return cabi.fusedmm(word, st._rowptr, st._col, st._value, x, y, sop_udef=sop_udef or fn, sop_param=sop_param, plan=plan)[1]


def attention_matmul(src, x: torch.Tensor, y: Optional[torch.Tensor] = None, scale: Optional[float] = None) -> torch.Tensor:
    """Row-softmax attention aggregation over the stored entries of `src` (include/isplib_hip.h, isplib_attention_csr_hip):
    ``z[i] = sum_j softmax_j(scale * <x[i], y[j]>) y[j]`` over the entries (i, j) of row i -- the aggregation of AGNNConv and of the
    dot-product attention of TransformerConv / graph transformers, with its autograd backward (torch.ops.isplib.attention_spmm).  The
    stored values of `src` are not read; an empty row gives 0.  `x` [M, K], `y` [N, K] float32 GPU tensors; ``y=None`` means
    ``y = x`` (a square `src`; ``x.grad`` receives both contributions); ``scale=None`` means ``1 / sqrt(K)``.  Row-strided views keep
    their pitch, so multi-head use is one call per head on column views such as ``x[:, h*d:(h+1)*d]``.  The backward keeps x, y, z and
    one scalar per row -- nothing per edge -- and walks the storage's cached transposed structure (colptr / row_t).  fp32 only by
    default; there is no fallback route: outside isplib_attention_serves the call raises.  bf16 / fp16 operands (both of one dtype) are
    opt-in: with ISPLIB_HALF_ATTENTION=convert|native|auto set they go where attention16_route says -- the 16-bit operator
    (torch.ops.isplib.attention_spmm16, which keeps x, y and lse for its backward and no z) or `x.float()` -> this function ->
    `.to(dtype)`; the result and the gradients have the operands' dtype."""
    from . import cabi
    shared = y is None
    half = isinstance(x, torch.Tensor) and x.dtype in HALF_DTYPES and os.environ.get("ISPLIB_HALF_ATTENTION") is not None
    for name, t in (("x", x),) + (() if shared else (("y", y),)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"isplib_amd: `{name}` must be a tensor, got {type(t).__name__}")
        if t.dim() != 2:
            raise ValueError(f"isplib_amd: `{name}` must be 2-D [rows, k], got shape {tuple(t.shape)}")
        if t.dtype != torch.float32 and not (half and t.dtype in HALF_DTYPES):
            raise TypeError(f"isplib_amd: `{name}` must be float32, got {t.dtype} (the attention operator is fp32 only)")
    if shared:
        y = x
    if half and y.dtype != x.dtype:
        raise TypeError(f"isplib_amd: `x` and `y` must have one dtype (both bfloat16 or both float16), got {x.dtype} and {y.dtype}")
    st = _storage_of(src, y)
    m_rows, n_cols = st._rowptr.numel() - 1, st._sparse_sizes[1]
    if shared and m_rows != n_cols:
        raise ValueError(f"isplib_amd: y=None needs a square sparse matrix, got {m_rows} x {n_cols}")
    if x.size(0) != m_rows:
        raise ValueError(f"isplib_amd: `x` must have one row per row of the sparse matrix ({m_rows}), got {x.size(0)}")
    if y.size(0) != n_cols:
        raise ValueError(f"isplib_amd: `y` must have one row per column of the sparse matrix ({n_cols}), got {y.size(0)}")
    k = x.size(1)
    if y.size(1) != k:
        raise ValueError(f"isplib_amd: `x` and `y` must have one width, got {k} and {y.size(1)}")
    if half:
        # bf16 / fp16 operands, opt-in (ISPLIB_HALF_ATTENTION): the 16-bit operator where attention16_route admits BOTH gathered operands
        # (y by the forward and the rows kernel, x by the columns kernel), else the conversion route, which raises what fp32 raises
        def pitch_of(t, rows):
            return t.stride(0) if rows > 1 and t.stride(1) == 1 and t.stride(0) >= k else k
        native = all(attention16_route(t.dtype, k, pitch_of(t, rows), rows) == "attention16" for t, rows in ((y, n_cols), (x, m_rows)))
        if not native or not x.is_cuda or not y.is_cuda:
            x32 = x.float()
            return attention_matmul(src, x32, None if shared else y.float(), scale).to(x.dtype)
        if x.device != y.device or st._rowptr.device != x.device:
            raise ValueError("isplib_amd: `x`, `y` and the sparse matrix must be on one device")
        p = float(scale) if scale is not None else 1.0 / float(k) ** 0.5
        return torch.ops.isplib.attention_spmm16(st._rowptr, st._col, st.colptr(), st.row_t(), x, y, p)
    if not 1 <= k <= cabi.ATTENTION_K_MAX:
        raise ValueError(f"isplib_amd: attention_matmul serves 1 <= K <= {cabi.ATTENTION_K_MAX} (a row sits in registers), got K = {k}")
    for name, t, rows in (("x", x, m_rows), ("y", y, n_cols)):     # y is gathered by the forward, x by the backward over the columns
        pitch = t.stride(0) if rows > 1 and t.stride(1) == 1 and t.stride(0) >= k else k
        if not cabi.attention_serves(rows, k, pitch):
            raise ValueError(f"isplib_amd: `{name}` ({rows} rows at a pitch of {pitch} floats) is outside the attention kernels' domain: "
                             f"rows < 2^31 and rows * pitch * 4 <= {cabi.DENSE_BYTES_MAX} bytes (3.5 GiB, one buffer descriptor)")
    if not x.is_cuda or not y.is_cuda:
        raise TypeError("isplib_amd: `x` and `y` must be GPU tensors -- there is no CPU path")
    if x.device != y.device or st._rowptr.device != x.device:
        raise ValueError("isplib_amd: `x`, `y` and the sparse matrix must be on one device")
    p = float(scale) if scale is not None else 1.0 / float(k) ** 0.5
    return torch.ops.isplib.attention_spmm(st._rowptr, st._col, st.colptr(), st.row_t(), x, y, p)


def gat_matmul(src, y: torch.Tensor, a_dst: torch.Tensor, a_src: torch.Tensor, heads: int = 1, negative_slope: float = 0.2,
               a_edge: Optional[torch.Tensor] = None, dropout: float = 0.0, training: bool = True, seed: Optional[int] = None) -> torch.Tensor:
    """GAT attention aggregation over the stored entries of `src`, all heads in one launch (include/isplib_hip.h, isplib_gat_csr_hip):
    ``z[i, head h] = sum_j softmax_j(leaky_relu(a_dst[i, h] + a_src[j, h])) y[j, head h]`` over the entries (i, j) of row i -- the
    aggregation of GATConv, with its autograd backward in `y`, `a_dst` and `a_src` (torch.ops.isplib.gat_spmm).  `y` [N, heads * d]
    (head h owns the columns [h*d, (h+1)*d)), `a_dst` [M, heads], `a_src` [N, heads] float32 GPU tensors; with ``heads == 1`` the two
    scores may be 1-D [rows].  On a square graph the same tensor may be passed for both scores: its gradient receives both parts.
    The stored values of `src` are not read; an empty row gives 0.  The backward keeps y, the scores, z and one scalar per row and
    head -- nothing per edge.  fp32 only by default (bf16 / fp16 operands raise TypeError); there is no fallback route: outside
    isplib_gat_serves (heads * d <= 512; heads == 1 or d a power of two >= 4) the call raises ValueError.  GATv2 is not this operator.
    A bf16 / fp16 `y` is opt-in: with ISPLIB_HALF_GAT=convert|native|auto set it goes where gat16_route says -- the 16-bit operator
    (torch.ops.isplib.gat_spmm16, which keeps y, the scores and lse for its backward and no z) where BOTH gathered operands are admitted
    (y with its rows, the gradient with M rows at pitch K), else `y.float()` -> this function -> `.to(dtype)`, which raises only what the
    fp32 call raises.  Each score may then be float32 or of y's dtype (a 16-bit score is widened by `.float()`, which is exact, and its
    gradient returns in its own dtype through that cast); the result and y's gradient have y's dtype.  fp32 calls do not read the
    variable.
    `a_edge` (GATConv's ``edge_dim``; None: the call above, unchanged) adds a per-edge, per-head score term with its gradient
    (torch.ops.isplib.gat_edge_spmm): ``u = (a_dst[i, h] + a_src[j, h]) + a_edge[e, h]`` before the leaky_relu -- two fp32 adds in this
    order, the slope branch taken on that fp32 u.  It is a float32 GPU tensor [nnz, heads] ([nnz] with one head; a non-contiguous one
    is copied) with ONE ROW PER STORED ENTRY IN THE STORAGE'S ENTRY ORDER: the order of ``storage.col()`` / ``storage.value()``, i.e.
    CSR positions (sorted by row; inside a row, the order the entries were stored in).  Duplicates (i, j) are separate entries with a
    row each.  A caller who built the matrix from unsorted COO passes ``value=torch.arange(nnz)`` once: ``storage.value()`` is then
    the COO index of every entry, by which the edge attributes are permuted.  Outside isplib_gat_edge_serves (nnz < 2^31 and
    nnz * heads * 4 <= 3.5 GiB) the call raises ValueError: pass fewer heads per call, on column views of `y`.  With a 16-bit `y`
    and ISPLIB_HALF_GAT set (to any value) the call takes the conversion route -- there is no 16-bit edge kernel; `a_edge` may then
    be float32 or of y's dtype.
    `dropout` (GATConv's ``dropout``; a Python float or int in [0, 1)) drops attention coefficients AFTER the softmax, per stored entry
    and per head, and scales the kept ones by ``float32(1 / (1 - dropout))`` (torch.ops.isplib.gat_drop_spmm): the softmax still runs
    over every stored entry.  ``dropout == 0`` or ``training=False`` is the call above, unchanged, bit for bit.  The mask is a pure
    function of (`seed`, the entry's position in ``storage.col()``, head) -- include/isplib_hip.h states it, `gat_dropout_mask`
    returns it -- which the backward recomputes: nothing per edge is stored and no RNG state is kept.  ``seed=None`` draws one int64 in
    [0, 2^63) from torch's default CPU generator (reproducible under ``torch.manual_seed``, no device sync); an explicit `seed` is an
    int in [0, 2^63).  The seed is a kernel ARGUMENT: a captured graph replays ONE mask -- draw the seed outside the capture and
    re-capture, or do not capture a training step that needs fresh masks.  A caller who splits the heads over several calls (column
    views of `y`) gets heads numbered from 0 in each call: pass a different seed per call, or the calls share masks.  With `a_edge` both
    apply.  A 16-bit `y` under ISPLIB_HALF_GAT takes the conversion route, as with `a_edge`."""
    drop = _gat_dropout_args(dropout, training, seed)
    if drop is not None:
        return _gat_drop_matmul(src, y, a_dst, a_src, a_edge, heads, negative_slope, *drop)
    if a_edge is not None:
        return _gat_edge_matmul(src, y, a_dst, a_src, a_edge, heads, negative_slope)
    from . import cabi
    half = isinstance(y, torch.Tensor) and y.dtype in HALF_DTYPES and os.environ.get("ISPLIB_HALF_GAT") is not None
    for name, t in (("y", y), ("a_dst", a_dst), ("a_src", a_src)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"isplib_amd: `{name}` must be a tensor, got {type(t).__name__}")
        if half and name != "y" and t.dtype not in (torch.float32, y.dtype):
            raise TypeError(f"isplib_amd: `{name}` must be float32 or of `y`'s dtype ({y.dtype}), got {t.dtype}")
        if not half and t.dtype != torch.float32:
            raise TypeError(f"isplib_amd: `{name}` must be float32, got {t.dtype} (the attention operator is fp32 only)")
    if half:
        return _gat_matmul16(src, y, a_dst, a_src, heads, negative_slope)
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"isplib_amd: `heads` must be a positive int, got {heads!r}")
    if y.dim() != 2:
        raise ValueError(f"isplib_amd: `y` must be 2-D [rows, heads * d], got shape {tuple(y.shape)}")
    st = _storage_of(src, y)
    m_rows, n_cols = st._rowptr.numel() - 1, st._sparse_sizes[1]
    if y.size(0) != n_cols:
        raise ValueError(f"isplib_amd: `y` must have one row per column of the sparse matrix ({n_cols}), got {y.size(0)}")
    k = y.size(1)
    if k % heads:
        raise ValueError(f"isplib_amd: the width of `y` ({k}) must be heads * d, got heads = {heads}")
    d = k // heads
    if heads == 1:
        a_dst = a_dst.unsqueeze(1) if a_dst.dim() == 1 else a_dst
        a_src = a_src.unsqueeze(1) if a_src.dim() == 1 else a_src
    for name, t, rows, what in (("a_dst", a_dst, m_rows, "row"), ("a_src", a_src, n_cols, "column")):
        if t.dim() != 2 or t.size(0) != rows or t.size(1) != heads:
            raise ValueError(f"isplib_amd: `{name}` must be [{rows}, {heads}] (one entry per {what} of the sparse matrix and head), got "
                             f"shape {tuple(t.shape)}")
    if not (1 <= k <= cabi.GAT_K_MAX) or (heads > 1 and (d < 4 or d & (d - 1))):
        raise ValueError(f"isplib_amd: gat_matmul serves 1 <= heads * d <= {cabi.GAT_K_MAX} with heads == 1 or d a power of two >= 4 (a head "
                         f"is an aligned group of lanes), got heads = {heads}, d = {d}")
    pitch = y.stride(0) if n_cols > 1 and y.stride(1) == 1 and y.stride(0) >= k else k
    for rows, ld, what in ((n_cols, pitch, "`y`"), (m_rows, k, "the gradient of the result")):   # y: forward, rows; g: the columns kernel
        if not cabi.gat_serves(rows, heads, d, ld):
            raise ValueError(f"isplib_amd: {what} ({rows} rows at a pitch of {ld} floats) is outside the GAT kernels' domain: "
                             f"rows < 2^31 and rows * pitch * 4 <= {cabi.DENSE_BYTES_MAX} bytes (3.5 GiB, one buffer descriptor)")
    if not y.is_cuda or not a_dst.is_cuda or not a_src.is_cuda:
        raise TypeError("isplib_amd: `y`, `a_dst` and `a_src` must be GPU tensors -- there is no CPU path")
    if a_dst.device != y.device or a_src.device != y.device or st._rowptr.device != y.device:
        raise ValueError("isplib_amd: `y`, `a_dst`, `a_src` and the sparse matrix must be on one device")
    return torch.ops.isplib.gat_spmm(st._rowptr, st._col, st.colptr(), st.row_t(), y, a_dst, a_src, heads, float(negative_slope))


def _gat_edge_matmul(src, y, a_dst, a_src, a_edge, heads, negative_slope):
    """gat_matmul with the per-edge score term: every check of gat_matmul, `a_edge` and its domain, all before anything touches a
    device; then torch.ops.isplib.gat_edge_spmm.  There is no fallback route."""
    from . import cabi
    half = isinstance(y, torch.Tensor) and y.dtype in HALF_DTYPES and os.environ.get("ISPLIB_HALF_GAT") is not None
    for name, t in (("y", y), ("a_dst", a_dst), ("a_src", a_src), ("a_edge", a_edge)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"isplib_amd: `{name}` must be a tensor, got {type(t).__name__}")
        if half and name != "y" and t.dtype not in (torch.float32, y.dtype):
            raise TypeError(f"isplib_amd: `{name}` must be float32 or of `y`'s dtype ({y.dtype}), got {t.dtype}")
        if not half and t.dtype != torch.float32:
            raise TypeError(f"isplib_amd: `{name}` must be float32, got {t.dtype} (the attention operator is fp32 only)")
    if half:        # the conversion route (no 16-bit edge kernel): .float() is exact, and every gradient returns in its own dtype through the cast
        return _gat_edge_matmul(src, y.float(), a_dst.float(), a_src.float(), a_edge.float(), heads, negative_slope).to(y.dtype)
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"isplib_amd: `heads` must be a positive int, got {heads!r}")
    if y.dim() != 2:
        raise ValueError(f"isplib_amd: `y` must be 2-D [rows, heads * d], got shape {tuple(y.shape)}")
    st = _storage_of(src, y)
    m_rows, n_cols, nnz = st._rowptr.numel() - 1, st._sparse_sizes[1], st._col.numel()
    if y.size(0) != n_cols:
        raise ValueError(f"isplib_amd: `y` must have one row per column of the sparse matrix ({n_cols}), got {y.size(0)}")
    k = y.size(1)
    if k % heads:
        raise ValueError(f"isplib_amd: the width of `y` ({k}) must be heads * d, got heads = {heads}")
    d = k // heads
    if heads == 1:
        a_dst = a_dst.unsqueeze(1) if a_dst.dim() == 1 else a_dst
        a_src = a_src.unsqueeze(1) if a_src.dim() == 1 else a_src
        a_edge = a_edge.unsqueeze(1) if a_edge.dim() == 1 else a_edge
    for name, t, rows, what in (("a_dst", a_dst, m_rows, "row"), ("a_src", a_src, n_cols, "column"), ("a_edge", a_edge, nnz, "stored entry")):
        if t.dim() != 2 or t.size(0) != rows or t.size(1) != heads:
            raise ValueError(f"isplib_amd: `{name}` must be [{rows}, {heads}] (one entry per {what} of the sparse matrix and head), got "
                             f"shape {tuple(t.shape)}")
    if not (1 <= k <= cabi.GAT_K_MAX) or (heads > 1 and (d < 4 or d & (d - 1))):
        raise ValueError(f"isplib_amd: gat_matmul serves 1 <= heads * d <= {cabi.GAT_K_MAX} with heads == 1 or d a power of two >= 4 (a head "
                         f"is an aligned group of lanes), got heads = {heads}, d = {d}")
    pitch = y.stride(0) if n_cols > 1 and y.stride(1) == 1 and y.stride(0) >= k else k
    for rows, ld, what in ((n_cols, pitch, "`y`"), (m_rows, k, "the gradient of the result")):   # y: forward, rows; g: the columns kernel
        if not cabi.gat_serves(rows, heads, d, ld):
            raise ValueError(f"isplib_amd: {what} ({rows} rows at a pitch of {ld} floats) is outside the GAT kernels' domain: "
                             f"rows < 2^31 and rows * pitch * 4 <= {cabi.DENSE_BYTES_MAX} bytes (3.5 GiB, one buffer descriptor)")
    if not cabi.gat_edge_serves(nnz, heads):
        raise ValueError(f"isplib_amd: `a_edge` ({nnz} stored entries x {heads} heads) is outside the GAT edge kernels' domain "
                         f"(isplib_gat_edge_serves): nnz < 2^31 and nnz * heads * 4 <= {cabi.DENSE_BYTES_MAX} bytes (3.5 GiB, one buffer "
                         f"descriptor); pass fewer heads per call, on column views of `y`")
    if not y.is_cuda or not a_dst.is_cuda or not a_src.is_cuda or not a_edge.is_cuda:
        raise TypeError("isplib_amd: `y`, `a_dst`, `a_src` and `a_edge` must be GPU tensors -- there is no CPU path")
    if a_dst.device != y.device or a_src.device != y.device or a_edge.device != y.device or st._rowptr.device != y.device:
        raise ValueError("isplib_amd: `y`, `a_dst`, `a_src`, `a_edge` and the sparse matrix must be on one device")
    if not a_edge.is_contiguous():
        a_edge = a_edge.contiguous()
    return torch.ops.isplib.gat_edge_spmm(st._rowptr, st._col, st.colptr(), st.row_t(), st.csr2csc(), y, a_dst, a_src, a_edge, heads,
                                          float(negative_slope))


def _gat_dropout_args(dropout, training, seed):
    """The dropout arguments of gat_matmul, checked before anything touches a device.  -> None (no dropout: `dropout == 0` or not
    training) or (p, seed) with the seed drawn from torch's default CPU generator where none was given."""
    if isinstance(dropout, bool) or not isinstance(dropout, (int, float)):
        raise TypeError(f"isplib_amd: `dropout` must be a Python float or int in [0, 1), got {type(dropout).__name__}")
    p = float(dropout)
    if not 0.0 <= p < 1.0:                                              # NaN fails both comparisons
        raise ValueError(f"isplib_amd: `dropout` must lie in [0, 1), got {dropout!r}")
    if seed is not None:
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise TypeError(f"isplib_amd: `seed` must be an int in [0, 2^63) or None, got {type(seed).__name__}")
        if not 0 <= seed < 2 ** 63:
            raise ValueError(f"isplib_amd: `seed` must lie in [0, 2^63), got {seed!r}")
    if p == 0.0 or not training:
        return None
    if seed is None:                                                    # one int64 from the default CPU generator: no device sync
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    return p, seed


def _gat_drop_matmul(src, y, a_dst, a_src, a_edge, heads, negative_slope, p, seed):
    """gat_matmul with attention dropout, with or without the per-edge term: every check of gat_matmul (and of `a_edge` and its domain),
    all before anything touches a device; then torch.ops.isplib.gat_drop_spmm.  There is no fallback route."""
    from . import cabi
    edge = a_edge is not None
    half = isinstance(y, torch.Tensor) and y.dtype in HALF_DTYPES and os.environ.get("ISPLIB_HALF_GAT") is not None
    for name, t in (("y", y), ("a_dst", a_dst), ("a_src", a_src)) + ((("a_edge", a_edge),) if edge else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"isplib_amd: `{name}` must be a tensor, got {type(t).__name__}")
        if half and name != "y" and t.dtype not in (torch.float32, y.dtype):
            raise TypeError(f"isplib_amd: `{name}` must be float32 or of `y`'s dtype ({y.dtype}), got {t.dtype}")
        if not half and t.dtype != torch.float32:
            raise TypeError(f"isplib_amd: `{name}` must be float32, got {t.dtype} (the attention operator is fp32 only)")
    if half:        # the conversion route (no 16-bit dropout kernel): .float() is exact, and every gradient returns in its own dtype through the cast
        return _gat_drop_matmul(src, y.float(), a_dst.float(), a_src.float(), a_edge.float() if edge else None, heads, negative_slope, p,
                                seed).to(y.dtype)
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"isplib_amd: `heads` must be a positive int, got {heads!r}")
    if y.dim() != 2:
        raise ValueError(f"isplib_amd: `y` must be 2-D [rows, heads * d], got shape {tuple(y.shape)}")
    st = _storage_of(src, y)
    m_rows, n_cols, nnz = st._rowptr.numel() - 1, st._sparse_sizes[1], st._col.numel()
    if y.size(0) != n_cols:
        raise ValueError(f"isplib_amd: `y` must have one row per column of the sparse matrix ({n_cols}), got {y.size(0)}")
    k = y.size(1)
    if k % heads:
        raise ValueError(f"isplib_amd: the width of `y` ({k}) must be heads * d, got heads = {heads}")
    d = k // heads
    if heads == 1:
        a_dst = a_dst.unsqueeze(1) if a_dst.dim() == 1 else a_dst
        a_src = a_src.unsqueeze(1) if a_src.dim() == 1 else a_src
        a_edge = a_edge.unsqueeze(1) if edge and a_edge.dim() == 1 else a_edge
    for name, t, rows, what in (("a_dst", a_dst, m_rows, "row"), ("a_src", a_src, n_cols, "column")) + \
            ((("a_edge", a_edge, nnz, "stored entry"),) if edge else ()):
        if t.dim() != 2 or t.size(0) != rows or t.size(1) != heads:
            raise ValueError(f"isplib_amd: `{name}` must be [{rows}, {heads}] (one entry per {what} of the sparse matrix and head), got "
                             f"shape {tuple(t.shape)}")
    if not (1 <= k <= cabi.GAT_K_MAX) or (heads > 1 and (d < 4 or d & (d - 1))):
        raise ValueError(f"isplib_amd: gat_matmul serves 1 <= heads * d <= {cabi.GAT_K_MAX} with heads == 1 or d a power of two >= 4 (a head "
                         f"is an aligned group of lanes), got heads = {heads}, d = {d}")
    pitch = y.stride(0) if n_cols > 1 and y.stride(1) == 1 and y.stride(0) >= k else k
    for rows, ld, what in ((n_cols, pitch, "`y`"), (m_rows, k, "the gradient of the result")):   # y: forward, rows; g: the columns kernel
        if not cabi.gat_serves(rows, heads, d, ld):
            raise ValueError(f"isplib_amd: {what} ({rows} rows at a pitch of {ld} floats) is outside the GAT kernels' domain: "
                             f"rows < 2^31 and rows * pitch * 4 <= {cabi.DENSE_BYTES_MAX} bytes (3.5 GiB, one buffer descriptor)")
    if nnz >= 2 ** 31:
        raise ValueError(f"isplib_amd: the dropout keep bit is defined for fewer than 2^31 stored entries, got {nnz}")
    if edge and not cabi.gat_edge_serves(nnz, heads):
        raise ValueError(f"isplib_amd: `a_edge` ({nnz} stored entries x {heads} heads) is outside the GAT edge kernels' domain "
                         f"(isplib_gat_edge_serves): nnz < 2^31 and nnz * heads * 4 <= {cabi.DENSE_BYTES_MAX} bytes (3.5 GiB, one buffer "
                         f"descriptor); pass fewer heads per call, on column views of `y`")
    operands = (y, a_dst, a_src) + ((a_edge,) if edge else ())
    if not all(t.is_cuda for t in operands):
        raise TypeError("isplib_amd: `y`, `a_dst`, `a_src` and `a_edge` must be GPU tensors -- there is no CPU path")
    if any(t.device != y.device for t in operands) or st._rowptr.device != y.device:
        raise ValueError("isplib_amd: `y`, `a_dst`, `a_src`, `a_edge` and the sparse matrix must be on one device")
    if edge and not a_edge.is_contiguous():
        a_edge = a_edge.contiguous()
    return torch.ops.isplib.gat_drop_spmm(st._rowptr, st._col, st.colptr(), st.row_t(), st.csr2csc(), y, a_dst, a_src, a_edge, heads,
                                          float(negative_slope), p, seed)


_MASK32 = 0xFFFFFFFF


def _mul32(x: torch.Tensor, c: int) -> torch.Tensor:
    """(x * c) mod 2^32 for an int64 tensor of 32-bit values, through 16-bit halves: no intermediate reaches 2^63."""
    return ((x & 0xFFFF) * c + ((((x >> 16) * c) & 0xFFFF) << 16)) & _MASK32


def _fmix32(x: torch.Tensor) -> torch.Tensor:
    x = x ^ (x >> 16)
    x = _mul32(x, 0x85EBCA6B)
    x = x ^ (x >> 13)
    x = _mul32(x, 0xC2B2AE35)
    return x ^ (x >> 16)


def gat_dropout_mask(adj_or_nnz, heads: int, dropout: float, seed: int, device=None) -> torch.Tensor:
    """The keep mask of ``gat_matmul(..., dropout=dropout, seed=seed)`` and of ``gatv2_matmul(..., dropout=dropout, seed=seed)`` -- one
    function serves both operators, and ``mha_matmul(..., dropout=dropout, seed=seed)`` as well, whose keep bit is the same: a bool tensor [nnz, heads], row e belonging to the stored entry ``storage.col()[e]``; True = kept.  The realised coefficients are ``mask * a / (1 - dropout)``.  `adj_or_nnz` is the sparse matrix
    (the mask is built on its device) or the number of stored entries (on `device`, the CPU by default).  Written with torch integer
    operations on int64 values masked to 32 bits -- the function of include/isplib_hip.h:
        word(seed, pos, h) = fmix32(fmix32(uint32(pos) ^ uint32(seed)) + uint32(h) * 0x9E3779B9 + uint32(seed >> 32)),  keep = word >= T(p)
    """
    from . import cabi
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"isplib_amd: `heads` must be a positive int, got {heads!r}")
    if isinstance(dropout, bool) or not isinstance(dropout, (int, float)) or not 0.0 <= float(dropout) < 1.0:
        raise ValueError(f"isplib_amd: `dropout` must be a Python float or int in [0, 1), got {dropout!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
        raise ValueError(f"isplib_amd: `seed` must be an int in [0, 2^63), got {seed!r}")
    if isinstance(adj_or_nnz, int) and not isinstance(adj_or_nnz, bool):
        nnz = adj_or_nnz
    else:
        st = adj_or_nnz.storage if hasattr(adj_or_nnz, "storage") else adj_or_nnz
        nnz = st._col.numel()
        device = st._col.device if device is None else device
    if not 0 <= nnz < 2 ** 31:
        raise ValueError(f"isplib_amd: the keep bit is defined for 0 <= nnz < 2^31 stored entries, got {nnz}")
    pos = torch.arange(nnz, dtype=torch.int64, device=device)
    entry = _fmix32(pos ^ (seed & _MASK32))
    headk = torch.tensor([(h * 0x9E3779B9 + (seed >> 32)) & _MASK32 for h in range(heads)], dtype=torch.int64, device=device)
    word = _fmix32((entry[:, None] + headk[None, :]) & _MASK32)
    return word >= cabi.gat_drop_threshold_py(float(dropout))


def gatv2_matmul(src, x: torch.Tensor, att: torch.Tensor, y: Optional[torch.Tensor] = None, heads: int = 1,
                 negative_slope: float = 0.2, dropout: float = 0.0, training: bool = True, seed: Optional[int] = None) -> torch.Tensor:
    """GATv2 attention aggregation over the stored entries of `src`, all heads in one launch (include/isplib_hip.h,
    isplib_gatv2_csr_hip): ``z[i, head h] = sum_j softmax_j(sum_c att[h, c] leaky_relu(x[i, c] + y[j, c])) y[j, head h]`` over the
    entries (i, j) of row i, c over the columns of head h -- the aggregation of GATv2Conv, with its autograd backward in `x`, `y` and
    `att` (torch.ops.isplib.gatv2_spmm).  `x` [M, heads * d] is the target side (PyG's ``lin_r(x)``), `y` [N, heads * d] the source
    side (``lin_l(x)``: gathered, and what is aggregated), head h in the columns [h*d, (h+1)*d); `att` is [heads, d], or [d] / [K] with
    one head.  ``y=None`` means ``y = x`` (``share_weights=True``) and needs a square `src`; the one tensor's gradient then receives
    both parts.  The stored values of `src` are not read; an empty row gives 0.  The backward keeps x, y, att, z and one scalar per row
    and head -- nothing per edge.  fp32 only by default (bf16 / fp16 operands raise TypeError); there is no fallback route: outside
    isplib_gatv2_serves (= isplib_gat_serves: heads * d <= 512; heads == 1 or d a power of two >= 4) the call raises ValueError.
    bf16 / fp16 `x` and `y` (both of one dtype) are opt-in through the GATv2 variable of the module docstring (convert|native|auto):
    once it is set the call goes where gatv2_16_route says -- the 16-bit operator (torch.ops.isplib.gatv2_spmm16, which keeps x, y,
    att and lse for its backward and no z) where ALL three gathered operands are admitted (y with its rows, x with its rows, the
    gradient with M rows at pitch K), else `x.float()`, `y.float()` -> this function -> `.to(dtype)`, which raises only what the fp32
    call raises.  `att` may then be float32 or of that dtype (a 16-bit `att` is widened by `.float()`, which is exact, and its gradient
    returns in its own dtype through that cast); the result and the gradients of `x` and `y` have their dtype.  fp32 calls do not read
    the variable.
    `dropout` (GATv2Conv's ``dropout``; a Python float or int in [0, 1)) drops attention coefficients AFTER the softmax, per stored entry
    and per head, and scales the kept ones by ``float32(1 / (1 - dropout))`` (torch.ops.isplib.gatv2_drop_spmm): the softmax still runs
    over every stored entry.  ``dropout == 0`` or ``training=False`` is the call above, unchanged, bit for bit.  The mask is the one of
    `gat_matmul` -- a pure function of (`seed`, the entry's position in ``storage.col()``, head), which `gat_dropout_mask` returns and
    the backward recomputes: nothing per edge is stored and no RNG state is kept.  ``seed=None`` draws one int64 in [0, 2^63) from
    torch's default CPU generator (reproducible under ``torch.manual_seed``, no device sync); an explicit `seed` is an int in [0, 2^63).
    The seed is a kernel ARGUMENT: a captured graph replays ONE mask -- draw the seed outside the capture and re-capture, or do not
    capture a training step that needs fresh masks.  There is no 16-bit dropout kernel: with 16-bit `x` / `y` and the GATv2 variable
    set (to any value) a call with active dropout converts -- ``.float()`` -> the fp32 dropout operator -> ``.to(dtype)``, every
    gradient returning in its own dtype through the casts; with the variable unset it raises the TypeError above."""
    from . import cabi
    drop = _gat_dropout_args(dropout, training, seed)
    shared = y is None
    if shared:
        y = x
    half = (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and (x.dtype in HALF_DTYPES or y.dtype in HALF_DTYPES) and
            os.environ.get("ISPLIB_HALF_GATV2") is not None)
    for name, t in (("x", x), ("y", y), ("att", att)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"isplib_amd: `{name}` must be a tensor, got {type(t).__name__}")
        if half and name != "att" and (t.dtype not in HALF_DTYPES or t.dtype != x.dtype):
            raise TypeError(f"isplib_amd: `x` and `y` must share one 16-bit dtype, got {x.dtype} and {y.dtype}")
        if half and name == "att" and t.dtype not in (torch.float32, x.dtype):
            raise TypeError(f"isplib_amd: `att` must be float32 or of `x`'s dtype ({x.dtype}), got {t.dtype}")
        if not half and t.dtype != torch.float32:
            raise TypeError(f"isplib_amd: `{name}` must be float32, got {t.dtype} (the GATv2 operator is fp32 only)")
    if half and drop is not None:         # the conversion route whatever the variable says: .float() is exact
        return gatv2_matmul(src, x.float(), att.float(), None if shared else y.float(), heads, negative_slope, drop[0], True,
                            drop[1]).to(x.dtype)
    if half:
        return _gatv2_matmul16(src, x, att, None if shared else y, heads, negative_slope)
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"isplib_amd: `heads` must be a positive int, got {heads!r}")
    if x.dim() != 2 or y.dim() != 2:
        raise ValueError(f"isplib_amd: `x` and `y` must be 2-D [rows, heads * d], got shapes {tuple(x.shape)} and {tuple(y.shape)}")
    st = _storage_of(src, y)
    m_rows, n_cols = st._rowptr.numel() - 1, st._sparse_sizes[1]
    if shared and m_rows != n_cols:
        raise ValueError(f"isplib_amd: `y=None` (y = x) needs a square sparse matrix, got {m_rows} x {n_cols}")
    if x.size(0) != m_rows:
        raise ValueError(f"isplib_amd: `x` must have one row per row of the sparse matrix ({m_rows}), got {x.size(0)}")
    if y.size(0) != n_cols:
        raise ValueError(f"isplib_amd: `y` must have one row per column of the sparse matrix ({n_cols}), got {y.size(0)}")
    k = y.size(1)
    if x.size(1) != k:
        raise ValueError(f"isplib_amd: `x` and `y` must have the same width, got {x.size(1)} and {k}")
    if k % heads:
        raise ValueError(f"isplib_amd: the width of `y` ({k}) must be heads * d, got heads = {heads}")
    d = k // heads
    if heads == 1 and att.dim() == 1:
        att = att.unsqueeze(0)
    if att.dim() != 2 or att.size(0) != heads or att.size(1) != d:
        raise ValueError(f"isplib_amd: `att` must be [{heads}, {d}] (heads x d; [d] with one head), got shape {tuple(att.shape)}")
    if not (1 <= k <= cabi.GAT_K_MAX) or (heads > 1 and (d < 4 or d & (d - 1))):
        raise ValueError(f"isplib_amd: gatv2_matmul serves 1 <= heads * d <= {cabi.GAT_K_MAX} with heads == 1 or d a power of two >= 4 (a "
                         f"head is an aligned group of lanes), got heads = {heads}, d = {d}")
    pitch_y = y.stride(0) if n_cols > 1 and y.stride(1) == 1 and y.stride(0) >= k else k
    pitch_x = x.stride(0) if m_rows > 1 and x.stride(1) == 1 and x.stride(0) >= k else k
    for rows, ld, what in ((n_cols, pitch_y, "`y`"), (m_rows, pitch_x, "`x`"), (m_rows, k, "the gradient of the result")):
        if not cabi.gatv2_serves(rows, heads, d, ld):              # y: forward, rows; x and g: the columns kernel
            raise ValueError(f"isplib_amd: {what} ({rows} rows at a pitch of {ld} floats) is outside the GATv2 kernels' domain: "
                             f"rows < 2^31 and rows * pitch * 4 <= {cabi.DENSE_BYTES_MAX} bytes (3.5 GiB, one buffer descriptor)")
    if not x.is_cuda or not y.is_cuda or not att.is_cuda:
        raise TypeError("isplib_amd: `x`, `y` and `att` must be GPU tensors -- there is no CPU path")
    if x.device != y.device or att.device != y.device or st._rowptr.device != y.device:
        raise ValueError("isplib_amd: `x`, `y`, `att` and the sparse matrix must be on one device")
    if drop is not None:
        if st._col.numel() >= 2 ** 31:
            raise ValueError(f"isplib_amd: the dropout keep bit is defined for fewer than 2^31 stored entries, got {st._col.numel()}")
        return torch.ops.isplib.gatv2_drop_spmm(st._rowptr, st._col, st.colptr(), st.row_t(), st.csr2csc(), x, y, att, heads,
                                                float(negative_slope), *drop)
    return torch.ops.isplib.gatv2_spmm(st._rowptr, st._col, st.colptr(), st.row_t(), x, y, att, heads, float(negative_slope))


def mha_matmul(src, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int = 1, scale: Optional[float] = None,
               dropout: float = 0.0, training: bool = True, seed: Optional[int] = None) -> torch.Tensor:
    """Sparse multi-head dot-product attention with separate keys and values over the stored entries of `src`, all heads in one launch
    (include/isplib_hip_mha.h, isplib_mha_csr_hip): ``z[i, head h] = sum_j softmax_j(scale * <q[i], k[j]>_h) v[j, head h]`` over the
    entries (i, j) of row i -- the aggregation of TransformerConv and of the local attention of sparse graph transformers, with its
    autograd backward in `q`, `k` and `v` (torch.ops.isplib.mha_spmm).  `q` [M, heads * d] is the target side, `k` and `v`
    [N, heads * d] the source side, head h in the columns [h*d, (h+1)*d); ``scale=None`` means ``1 / sqrt(d)`` -- the HEAD width.  The
    three may be column views of one fused ``[rows, 3 * K]`` projection: operands with unit column stride go in at their own pitch,
    without a copy.  ``k is v`` is allowed; the one tensor's gradient receives both parts.  The stored values of `src` are not read;
    every stored entry is its own edge; an empty row gives 0.  The backward keeps q, k, v, z and one scalar per row and head -- nothing
    per edge.  fp32 only by default (bf16 / fp16 operands raise TypeError) and there is no fallback route: outside isplib_mha_serves
    (= isplib_gat_serves: heads * d <= 512; heads == 1 or d a power of two >= 4) the call raises ValueError.  Not part of the operator:
    TransformerConv's edge features, its root weight and its beta gate (dense operations outside the aggregation).
    bf16 / fp16 `q`, `k` and `v` (all three of one dtype) are opt-in through the multi-head variable of the module docstring
    (convert|native|auto): once it is set the call goes where mha16_route says -- the 16-bit operator (torch.ops.isplib.mha_spmm16,
    which keeps q, k, v and lse for its backward and no z; column views of one fused 16-bit projection go in at their own even pitch)
    where ALL four gathered operands are admitted (k and v with their rows, q with its rows, the gradient with M rows at pitch K), else
    `.float()` -> this function -> `.to(dtype)`, which raises only what the fp32 call raises.  ``k is v`` works on both routes.  fp32
    calls do not read the variable.
    `dropout` (TransformerConv's ``dropout``, a graph transformer's ``attn_dropout``; a Python float or int in [0, 1)) drops attention
    coefficients AFTER the softmax, per stored entry and per head, and scales the kept ones by ``float32(1 / (1 - dropout))``
    (torch.ops.isplib.mha_drop_spmm, autograd in `q`, `k` and `v`): the softmax still runs over every stored entry.  ``dropout == 0`` or
    ``training=False`` is the call above, unchanged, bit for bit; it draws no seed.  The mask is the one of `gat_matmul` and
    `gatv2_matmul` -- a pure function of (`seed`, the entry's position in ``storage.col()``, head), which `gat_dropout_mask` returns and
    the backward recomputes: nothing per edge is stored and no RNG state is kept.  ``seed=None`` draws one int64 in [0, 2^63) from
    torch's default CPU generator (reproducible under ``torch.manual_seed``, no device sync); an explicit `seed` is an int in [0, 2^63).
    The seed is a kernel ARGUMENT: a captured graph replays ONE mask -- draw the seed outside the capture and re-capture, or do not
    capture a training step that needs fresh masks.  With 16-bit `q`, `k`, `v`, the multi-head variable set and active dropout, the
    call goes where mha16_drop_route says: with ISPLIB_HALF_MHA_DROP unset no 16-bit dropout kernel runs: the call converts --
    ``.float()`` -> the fp32 dropout operator -> ``.to(dtype)``, every gradient returning in its own dtype through the casts,
    ``k is v`` preserved -- whatever the multi-head variable says; with ISPLIB_HALF_MHA_DROP=native (or auto, where
    cabi.mha16_drop_native_pays says the class pays) and ALL four gathered operands admitted as above it takes the 16-bit dropout
    operator (torch.ops.isplib.mha_drop_spmm16: the DROP kernels of mha16.hip, the same keep bit, q, k, v and lse kept for the
    backward and no z), else it converts as before and nothing raises.  With the multi-head variable unset the call raises the
    TypeError above and ISPLIB_HALF_MHA_DROP is not read."""
    from . import cabi
    drop = _gat_dropout_args(dropout, training, seed)
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"isplib_amd: `{name}` must be a tensor, got {type(t).__name__}")
    half = any(t.dtype in HALF_DTYPES for t in (q, k, v)) and os.environ.get("ISPLIB_HALF_MHA") is not None
    for name, t in (("q", q), ("k", k), ("v", v)):
        if half and (t.dtype not in HALF_DTYPES or t.dtype != q.dtype):
            raise TypeError(f"isplib_amd: `q`, `k` and `v` must share one 16-bit dtype, got {q.dtype}, {k.dtype} and {v.dtype}")
        if not half and t.dtype != torch.float32:
            raise TypeError(f"isplib_amd: `{name}` must be float32, got {t.dtype} (the multi-head attention operator is fp32 only)")
    if half:
        return _mha_matmul16(src, q, k, v, heads, scale, drop)
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"isplib_amd: `heads` must be a positive int, got {heads!r}")
    if q.dim() != 2 or k.dim() != 2 or v.dim() != 2:
        raise ValueError(f"isplib_amd: `q`, `k` and `v` must be 2-D [rows, heads * d], got shapes {tuple(q.shape)}, {tuple(k.shape)} and "
                         f"{tuple(v.shape)}")
    st = _storage_of(src, k)
    m_rows, n_cols = st._rowptr.numel() - 1, st._sparse_sizes[1]
    if q.size(0) != m_rows:
        raise ValueError(f"isplib_amd: `q` must have one row per row of the sparse matrix ({m_rows}), got {q.size(0)}")
    for name, t in (("k", k), ("v", v)):
        if t.size(0) != n_cols:
            raise ValueError(f"isplib_amd: `{name}` must have one row per column of the sparse matrix ({n_cols}), got {t.size(0)}")
    kk = q.size(1)
    if k.size(1) != kk or v.size(1) != kk:
        raise ValueError(f"isplib_amd: `q`, `k` and `v` must have the same width, got {kk}, {k.size(1)} and {v.size(1)}")
    if kk % heads:
        raise ValueError(f"isplib_amd: the width of `q` ({kk}) must be heads * d, got heads = {heads}")
    d = kk // heads
    if not (1 <= kk <= cabi.GAT_K_MAX) or (heads > 1 and (d < 4 or d & (d - 1))):
        raise ValueError(f"isplib_amd: mha_matmul serves 1 <= heads * d <= {cabi.GAT_K_MAX} with heads == 1 or d a power of two >= 4 (a "
                         f"head is an aligned group of lanes), got heads = {heads}, d = {d}")
    if scale is not None and (isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale)):
        raise ValueError(f"isplib_amd: `scale` must be a finite Python number or None (1 / sqrt(d)), got {scale!r}")

    def pitch(t, rows):
        return t.stride(0) if rows > 1 and t.stride(1) == 1 and t.stride(0) >= kk else kk

    for rows, ld, what in ((n_cols, pitch(k, n_cols), "`k`"), (n_cols, pitch(v, n_cols), "`v`"), (m_rows, pitch(q, m_rows), "`q`"),
                           (m_rows, kk, "the gradient of the result")):
        if not cabi.mha_serves(rows, heads, d, ld):                # k, v: forward, rows; q and g: the columns kernel
            raise ValueError(f"isplib_amd: {what} ({rows} rows at a pitch of {ld} floats) is outside the multi-head attention kernels' "
                             f"domain: rows < 2^31 and rows * pitch * 4 <= {cabi.DENSE_BYTES_MAX} bytes (3.5 GiB, one buffer descriptor)")
    if not q.is_cuda or not k.is_cuda or not v.is_cuda:
        raise TypeError("isplib_amd: `q`, `k` and `v` must be GPU tensors -- there is no CPU path")
    if k.device != q.device or v.device != q.device or st._rowptr.device != q.device:
        raise ValueError("isplib_amd: `q`, `k`, `v` and the sparse matrix must be on one device")
    p = float(scale) if scale is not None else 1.0 / math.sqrt(d)
    if drop is not None:
        if st._col.numel() >= 2 ** 31:
            raise ValueError(f"isplib_amd: the dropout keep bit is defined for fewer than 2^31 stored entries, got {st._col.numel()}")
        return torch.ops.isplib.mha_drop_spmm(st._rowptr, st._col, st.colptr(), st.row_t(), st.csr2csc(), q, k, v, heads, p, *drop)
    return torch.ops.isplib.mha_spmm(st._rowptr, st._col, st.colptr(), st.row_t(), q, k, v, heads, p)


def _mha_matmul16(src, q, k, v, heads, scale, drop=None):
    """mha_matmul for bf16 / fp16 `q`, `k` and `v` under ISPLIB_HALF_MHA: the 16-bit operator where mha16_route admits ALL four gathered
    operands (k and v by the forward and the rows kernel; q and the gradient -- M rows, packed -- by the columns kernel), else the
    conversion route.  `k is v`: on both routes the one tensor's gradient receives dk + dv.  `drop` = (p, seed) of an active dropout:
    the same with mha16_drop_route and the 16-bit dropout operator; its conversion route is the fp32 dropout operator (.float() is
    exact)."""
    route, want = (mha16_route, "mha16") if drop is None else (mha16_drop_route, "mha16drop")
    native = False
    if (isinstance(heads, int) and not isinstance(heads, bool) and heads >= 1 and q.dim() == 2 and k.dim() == 2 and v.dim() == 2 and
            k.size(1) == q.size(1) and v.size(1) == q.size(1) and q.size(1) % heads == 0 and q.is_cuda and k.is_cuda and v.is_cuda and
            (scale is None or (not isinstance(scale, bool) and isinstance(scale, (int, float)) and math.isfinite(scale)))):
        st = _storage_of(src, k)
        m_rows, n_cols, kk = st._rowptr.numel() - 1, st._sparse_sizes[1], q.size(1)
        d = kk // heads

        def pitch(t, rows):
            return t.stride(0) if rows > 1 and t.stride(1) == 1 and t.stride(0) >= kk else kk

        native = (q.size(0) == m_rows and k.size(0) == n_cols and v.size(0) == n_cols and
                  all(route(q.dtype, heads, d, ld, rows) == want
                      for rows, ld in ((n_cols, pitch(k, n_cols)), (n_cols, pitch(v, n_cols)), (m_rows, pitch(q, m_rows)), (m_rows, kk))))
    if drop is not None and native and st._col.numel() >= 2 ** 31:
        native = False                                   # the fp32 call raises what it always raised
    if not native:
        kf = k.float()
        if drop is not None:
            return mha_matmul(src, q.float(), kf, kf if v is k else v.float(), heads, scale, drop[0], True, drop[1]).to(q.dtype)
        return mha_matmul(src, q.float(), kf, kf if v is k else v.float(), heads, scale).to(q.dtype)
    if k.device != q.device or v.device != q.device or st._rowptr.device != q.device:
        raise ValueError("isplib_amd: `q`, `k`, `v` and the sparse matrix must be on one device")
    p = float(scale) if scale is not None else 1.0 / math.sqrt(d)
    if drop is not None:
        return torch.ops.isplib.mha_drop_spmm16(st._rowptr, st._col, st.colptr(), st.row_t(), st.csr2csc(), q, k, v, heads, p, *drop)
    return torch.ops.isplib.mha_spmm16(st._rowptr, st._col, st.colptr(), st.row_t(), q, k, v, heads, p)


def _gatv2_matmul16(src, x, att, y, heads, negative_slope):
    """gatv2_matmul for bf16 / fp16 `x` and `y` under ISPLIB_HALF_GATV2: the 16-bit operator where gatv2_16_route admits ALL three
    gathered operands (y by the forward and the rows kernel; x and the gradient -- M rows, packed -- by the columns kernel), else the
    conversion route.  `y` None: y = x, on both routes the one tensor's gradient receives dx + dy."""
    att = att.float()                                 # exact, and no copy of an fp32 att; a gradient returns through the cast
    shared = y is None
    yy = x if shared else y
    native = False
    if (isinstance(heads, int) and not isinstance(heads, bool) and heads >= 1 and x.dim() == 2 and yy.dim() == 2 and
            x.size(1) == yy.size(1) and x.size(1) % heads == 0 and x.is_cuda and yy.is_cuda and att.is_cuda):
        st = _storage_of(src, yy)
        m_rows, n_cols, k = st._rowptr.numel() - 1, st._sparse_sizes[1], yy.size(1)
        d = k // heads
        pitch_y = yy.stride(0) if n_cols > 1 and yy.stride(1) == 1 and yy.stride(0) >= k else k
        pitch_x = x.stride(0) if m_rows > 1 and x.stride(1) == 1 and x.stride(0) >= k else k
        native = (yy.size(0) == n_cols and x.size(0) == m_rows and
                  all(gatv2_16_route(x.dtype, heads, d, ld, rows) == "gatv2_16"
                      for rows, ld in ((n_cols, pitch_y), (m_rows, pitch_x), (m_rows, k))))
    if not native:
        return gatv2_matmul(src, x.float(), att, None if shared else y.float(), heads, negative_slope).to(x.dtype)
    if heads == 1 and att.dim() == 1:
        att = att.unsqueeze(0)
    if att.dim() != 2 or att.size(0) != heads or att.size(1) != d:
        raise ValueError(f"isplib_amd: `att` must be [{heads}, {d}] (heads x d; [d] with one head), got shape {tuple(att.shape)}")
    if x.device != yy.device or att.device != yy.device or st._rowptr.device != yy.device:
        raise ValueError("isplib_amd: `x`, `y`, `att` and the sparse matrix must be on one device")
    return torch.ops.isplib.gatv2_spmm16(st._rowptr, st._col, st.colptr(), st.row_t(), x, yy, att, heads, float(negative_slope))


def _gat_matmul16(src, y, a_dst, a_src, heads, negative_slope):
    """gat_matmul for a bf16 / fp16 `y` under ISPLIB_HALF_GAT: the 16-bit operator where gat16_route admits BOTH gathered operands (y by
    the forward and the rows kernel, the gradient -- M rows, packed -- by the columns kernel), else the conversion route."""
    a_dst, a_src = a_dst.float(), a_src.float()       # exact, and no copy of an fp32 score; a gradient returns through the cast
    native = False
    if isinstance(heads, int) and not isinstance(heads, bool) and heads >= 1 and y.dim() == 2 and y.size(1) % heads == 0 and y.is_cuda:
        st = _storage_of(src, y)
        m_rows, n_cols, k = st._rowptr.numel() - 1, st._sparse_sizes[1], y.size(1)
        d = k // heads
        pitch = y.stride(0) if n_cols > 1 and y.stride(1) == 1 and y.stride(0) >= k else k
        native = (y.size(0) == n_cols and a_dst.is_cuda and a_src.is_cuda and
                  gat16_route(y.dtype, heads, d, pitch, n_cols) == "gat16" and gat16_route(y.dtype, heads, d, k, m_rows) == "gat16")
    if not native:
        return gat_matmul(src, y.float(), a_dst, a_src, heads, negative_slope).to(y.dtype)
    if heads == 1:
        a_dst = a_dst.unsqueeze(1) if a_dst.dim() == 1 else a_dst
        a_src = a_src.unsqueeze(1) if a_src.dim() == 1 else a_src
    for name, t, rows, what in (("a_dst", a_dst, m_rows, "row"), ("a_src", a_src, n_cols, "column")):
        if t.dim() != 2 or t.size(0) != rows or t.size(1) != heads:
            raise ValueError(f"isplib_amd: `{name}` must be [{rows}, {heads}] (one entry per {what} of the sparse matrix and head), got "
                             f"shape {tuple(t.shape)}")
    if a_dst.device != y.device or a_src.device != y.device or st._rowptr.device != y.device:
        raise ValueError("isplib_amd: `y`, `a_dst`, `a_src` and the sparse matrix must be on one device")
    return torch.ops.isplib.gat_spmm16(st._rowptr, st._col, st.colptr(), st.row_t(), y, a_dst, a_src, heads, float(negative_slope))


def gcn_norm_matmul(src, other: torch.Tensor, bias: Optional[torch.Tensor] = None, relu: bool = False) -> torch.Tensor:
    """relu(D^-1/2 (A + I) D^-1/2 @ other + bias) for an UNWEIGHTED square graph, without materialising the
    normalised edge weights: the SpMM runs on the unit-weight fast path, the self loop, the left D^-1/2, bias
    and ReLU are applied inside the fold kernel (include/isplib_hip.h: isplib_epilogue).  This is what a
    GCNConv(normalize=True) layer aggregates (callers: tests/dist/gcn/pyg-sparse.py:61-62); differentiable in
    `other` and `bias`.  Not part of the reference's surface."""
    half = isinstance(other, torch.Tensor) and other.dtype in HALF_DTYPES and os.environ.get("ISPLIB_HALF_GCN") is not None
    if not other.is_cuda or (other.dtype != torch.float32 and not half) or other.dim() != 2:
        raise RuntimeError("isplib_amd: gcn_norm_matmul needs a float32 GPU matrix [N, K] -- there is no CPU path")
    s = _storage_of(src, other)
    if half:
        # bf16 / fp16 features, opt-in (ISPLIB_HALF_GCN): the 16-bit row kernel with the fused epilogue where rows16_gcn_route says so
        # (the plan for A, and for A^T when a gradient can be asked for), else the conversion route
        if s._value is not None:
            raise ValueError("gcn_norm_matmul is defined for unweighted graphs (value=None)")
        if s._sparse_sizes[0] != s._sparse_sizes[1]:
            raise ValueError("gcn_norm_matmul needs a square adjacency")
        n, k = other.size(0), other.size(1)
        pitch = other.stride(0) if n > 1 and other.stride(1) == 1 else k
        plan = _rows16_plan_where(lambda ordered: rows16_gcn_route(other.dtype, k, pitch, n, ordered) == "rows16", s, False, k, other.device)
        if plan is None:
            bias32 = bias.float() if bias is not None and bias.dtype in HALF_DTYPES else bias
            out = gcn_norm_matmul(src, other.float(), bias32, relu)
            s._last_schedule = ("convert",)
            return out.to(other.dtype)
        colptr = row_t = None
        plan_t = []
        if torch.is_grad_enabled() and (other.requires_grad or (bias is not None and bias.requires_grad)):
            colptr, row_t = s.colptr(), s.row_t()
            # dZ: [n, k] packed; the order of A^T's rows is put to the same route, and where it says no the backward keeps index order
            plan_t = _rows16_plan_where(lambda ordered: rows16_gcn_route(other.dtype, k, k, n, ordered) == "rows16", s, True, k, other.device)
            if plan_t is None:
                plan_t = [torch.empty(0, dtype=torch.int32, device=other.device), _ROWS16_MARK]
        s._last_schedule = ("rows16gcn",) + (("ordered",) if plan[0].numel() > 0 else ())
        return torch.ops.isplib.gcn_norm_spmm(s._rowptr, s._col, other, s.gcn_dinv(), colptr, row_t, plan, plan_t, bias, relu)
    if s._value is not None:
        raise ValueError("gcn_norm_matmul is defined for unweighted graphs (value=None)")
    if s._sparse_sizes[0] != s._sparse_sizes[1]:
        raise ValueError("gcn_norm_matmul needs a square adjacency")
    k = other.size(1)
    n = other.size(0)
    needs_grad = torch.is_grad_enabled() and other.requires_grad
    # the same schedule rule as matmul: stream plans (unit weights; the kernel applies the epilogue when it writes a
    # finished row) where isplib_suggest_stream accepts the shape, else the task list
    geom = choose_stream(s, n, n, k)
    plan = s.stream_plan(False, geom) if geom is not None else None
    n_sl = None
    if plan is None:
        n_sl = choose_slices(s, n, k)
        plan = s.plan(n_sl)
    colptr = row_t = None
    plan_t = []
    if needs_grad:
        colptr, row_t = s.colptr(), s.row_t()
        plan_t = s.stream_plan(True, geom, "sum") if geom is not None else None
        if plan_t is None:
            plan_t = s.plan_t(choose_slices(s, n, k, transposed=True) if n_sl is None else n_sl)
    return torch.ops.isplib.gcn_norm_spmm(s._rowptr, s._col, other, s.gcn_dinv(), colptr, row_t, plan, plan_t, bias, relu)


class iSpLibPlugin:
    backup = []          # LIFO of (torch_sparse.matmul | None, torch.sparse.mm, WITH_PT2, WITH_PT20)

    @classmethod
    def patch_pyg(cls) -> None:
        saved_flags = (None, None)
        if _pyg_typing is not None:                                  # :159-171
            saved_flags = (getattr(_pyg_typing, "WITH_PT2", None), getattr(_pyg_typing, "WITH_PT20", None))
            _pyg_typing.WITH_PT2 = False
            _pyg_typing.WITH_PT20 = False
        original_mm = torch.sparse.mm

        def sparse_mm(src, other, reduce: str = "sum"):
            if hasattr(src, "csr") and hasattr(src, "storage"):
                return spmm_autotuned(src, other, reduce)
            return original_mm(src, other) if reduce == "sum" else original_mm(src, other, reduce)

        cls.backup.append((None if _torch_sparse is None else _torch_sparse.matmul, original_mm) + saved_flags)  # :173-174
        if _torch_sparse is not None:
            _torch_sparse.matmul = spmm_autotuned                    # :177
        torch.sparse.mm = sparse_mm                                  # :178

    @classmethod
    def unpatch_pyg(cls) -> None:
        if not cls.backup:                                           # :190
            return
        ts_matmul, sparse_mm, pt2, pt20 = cls.backup.pop()
        torch.sparse.mm = sparse_mm                                  # :194
        if _torch_sparse is not None and ts_matmul is not None:
            _torch_sparse.matmul = ts_matmul                         # :195
        if _pyg_typing is not None:                                  # :197-201
            if pt2 is not None:
                _pyg_typing.WITH_PT2 = pt2
            if pt20 is not None:
                _pyg_typing.WITH_PT20 = pt20

    @classmethod
    def autotune(cls, src, k: int, reduce: str = "sum", candidates=(0, 2, 4, 6, 8, 12, 16, 24), reps: int = 3, other_rows=None,
                 stream_slices=(0.5, 0.75, 1.0, 1.25, 1.5), stream_chunk=(0.5, 2.0)):
        """Times the SpMM of `src` at width `k` on every candidate SCHEDULE AND GEOMETRY on the actual graph and keeps the
        fastest for every later call (the heir of the reference's tuning scripts: autotuner/findbestk.py:34-38 sweeps K and
        prints a table, gpu/kernels/codegen.py:30-41 sweeps a launch parameter).  Candidates, each actually forced:
          ("stream", streams, slices, chunk)  the stream schedule where its rule accepts the shape: the rule's column-slice
                                              count x `stream_slices`, and the rule's hub-row chunk x `stream_chunk`
          ("tasks", slices)                   the task list at every non-zero slice count of `candidates`
          ("plain",)                          the row-per-wave kernel (a 0 in `candidates`)
        A candidate only counts if the call really ran on it (a plan builder that declines falls back to another
        schedule: that measurement is dropped).  Returns {choice: milliseconds}; the winner lives on the graph's storage
        and in the table `save_tuning` writes.  Costs one plan build per candidate; the losers' stream plans are freed."""
        rowptr, col, value = src.csr()
        x = torch.zeros((other_rows or src.sparse_sizes()[1], k), dtype=torch.float32, device=col.device)
        s = _storage_of(src, x)
        minmax = reduce in ("max", "min")
        key = (x.size(0), k, minmax)
        m_rows = rowptr.numel() - 1
        before = s._tuned.pop(key, None)
        rule = stream_minmax_rule(s, m_rows, x.size(0), k) if minmax else stream_rule(s, m_rows, x.size(0), k, s._value is not None)
        stream_off = os.environ.get("ISPLIB_STREAM", "1") == "0" or os.environ.get("ISPLIB_SLICES") is not None
        cands = []
        if rule is not None and not stream_off:
            st, sl, ch = rule
            for f in stream_slices:
                cands.append(("stream", st, max(1, min(512, int(sl * f + 0.5))), ch))
            for f in stream_chunk:
                cands.append(("stream", st, sl, max(256, int(ch * f))))
        for c in candidates:
            cands.append(("tasks", int(c)) if int(c) > 0 else ("plain",))
        cands = list(dict.fromkeys(cands))                         # the rule's own geometry appears once
        times = {}
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        built = set(s._streams)
        for cand in cands:
            s._tuned[key] = cand
            try:
                spmm_autotuned(src, x, reduce)                     # builds the plan, warms up
                if s._last_schedule != cand:                       # the builder declined: this is another schedule's time
                    continue
                start.record()
                for _ in range(reps):
                    spmm_autotuned(src, x, reduce)
                stop.record()
                torch.cuda.synchronize()
                times[cand] = start.elapsed_time(stop) / reps
            except RuntimeError:
                continue
        if times:
            best = s._tuned[key] = min(times, key=times.get)
            _tuning_db.setdefault(graph_signature(s), {})[f"{key[0]}:{k}:{int(minmax)}"] = list(best)
        elif before is not None:
            s._tuned[key] = before
        else:
            s._tuned.pop(key, None)
        keep = s._tuned.get(key)
        for pkey in [p_ for p_ in s._streams if p_ not in built]:      # stream plans of the losing geometries: 4-12 B per edge each
            if not (keep is not None and keep[0] == "stream" and pkey[1:4] == tuple(keep[1:])):
                s._streams.pop(pkey, None)
                for vkey in [v_ for v_ in s._stream_vals if v_[:len(pkey)] == pkey]:
                    s._stream_vals.pop(vkey, None)
        return times

    @classmethod
    def save_tuning(cls, path) -> None:
        """Writes every choice `autotune` has measured (merged over what the file already holds) as JSON."""
        merged = {}
        if os.path.exists(path):
            with open(path) as f:
                merged = json.load(f)
        for sig, table in _tuning_db.items():
            merged.setdefault(sig, {}).update(table)
        with open(path, "w") as f:
            json.dump(merged, f, indent=1, sort_keys=True)

    @classmethod
    def load_tuning(cls, path) -> int:
        """Merges a file written by `save_tuning`; returns the number of graphs it describes."""
        with open(path) as f:
            table = json.load(f)
        for sig, entries in table.items():
            _tuning_db.setdefault(sig, {}).update({k: list(_as_choice(v)) for k, v in entries.items()})
        return len(table)

    @classmethod
    def is_patched(cls) -> bool:
        return bool(cls.backup)

    @classmethod
    def clear_cache(cls) -> None:
        _foreign.clear()
        _tuning_db.clear()


def isplib_autotune(fn):
    """Decorator: run ``fn`` with the patch applied (isplib/__init__.py:204-210);
    unlike the reference, the patch is removed even when ``fn`` raises."""

    def wrapper(*args, **kwargs):
        iSpLibPlugin.patch_pyg()
        try:
            return fn(*args, **kwargs)
        finally:
            iSpLibPlugin.unpatch_pyg()

    wrapper.__name__ = getattr(fn, "__name__", "wrapper")
    wrapper.__doc__ = getattr(fn, "__doc__", None)
    return wrapper


if os.environ.get("ISPLIB_TUNE_FILE") and os.path.exists(os.environ["ISPLIB_TUNE_FILE"]):
    iSpLibPlugin.load_tuning(os.environ["ISPLIB_TUNE_FILE"])
