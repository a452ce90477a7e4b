"""ctypes view of the C ABI (include/isplib_hip.h) for device tensors.

This is the binding a non-torch host (the reference's own launcher,
csrc/fusedmm.cpp:198) would use; here it lets the GPU parity tests and
``bench.py`` call the library exactly at the drop-in boundary, bypassing the
torch operator layer.  Torch is used only to own device memory and name the
stream.  Every function raises ``RuntimeError`` on a non-zero status.
"""
from __future__ import annotations

import ctypes
import math
import os
import struct
from typing import Optional

import torch

from . import _lib

# values of include/isplib_hip.h
MSG_SPMM_SUM = 0x2 | 0x00 | 0x100 | 0x1000 | 0x10000
MSG_SPMM_MEAN = 0x2 | 0x00 | 0x100 | 0x3000 | 0x10000
MSG_SPMM_MAX = 0x2 | 0x00 | 0x100 | 0x1000 | 0x20000
MSG_SPMM_MIN = 0x2 | 0x00 | 0x100 | 0x1000 | 0x30000
MESSAGE = {"sum": MSG_SPMM_SUM, "add": MSG_SPMM_SUM, "mean": MSG_SPMM_MEAN, "max": MSG_SPMM_MAX, "min": MSG_SPMM_MIN}

# status codes (csrc/fusedMM.h:105-114 of the reference + one for HIP runtime errors), under the header's names and short ones
SUCCESS, FAIL, NOT_ENOUGH_MEM, NO_OPT_IMPL, HIP_ERROR = 0, 1, -1, 128, 256
UNDEFINED_USER_FUNCTION = 64
ISPLIB_SUCCESS, ISPLIB_FAIL, ISPLIB_NOT_ENOUGH_MEM, ISPLIB_NO_OPT_IMPL, ISPLIB_HIP_ERROR = SUCCESS, FAIL, NOT_ENOUGH_MEM, NO_OPT_IMPL, HIP_ERROR

# the address domains of the kernel families (the header's section of that name is the contract; tests/test_host.py compares)
DENSE_BYTES_MAX = 7 * 2 ** 29           # n * ldy * 4 of a dense operand read through one buffer descriptor: 3.5 GiB
DENSE_OOB_OFFSET = 15 * 2 ** 28         # a byte offset such a descriptor answers with 0
STREAM_N_END = 2 ** 24                  # the stream schedules: n <, ldy <, nnz <
STREAM_LDY_END = 2 ** 22
STREAM_NNZ_END = 2 ** 31
STREAM_MINMAX_BYTES_END = 2 ** 31       # max / min on the stream schedule: n * ldy * 4 < 2 GiB
K_MIN = 4                               # every entry that takes a plan
SDDMM_TASKS_K_MAX = 1024
MINMAX_BW_PAIRS_END = 2 ** 32 - 2       # the sort-based max / min backward: m * k pairs <
MINMAX_BW_KEYS_MAX = 2 ** 32 - 2        # ... and n * k + 1 < 2^32 sort keys
OWNER_WORLD_MAX = 64                    # ranks of the owner-bucketed exchange
DTYPE_BF16, DTYPE_F16 = 1, 2            # ISPLIB_DTYPE_*: element types of fusedMM_csr_stream16_hip


def stream16_serves(n: int, k: int, ldy: int, ldz: int, nnz: int) -> bool:
    """isplib_stream16_serves of the header: the 16-bit stream entry (bf16 / fp16 operands, sum / mean) serves an n x k operand at
    leading dimension ldy (elements), output pitch ldz, on a graph of nnz entries."""
    return (k >= K_MIN and n < STREAM_N_END and ldy < STREAM_LDY_END and nnz < STREAM_NNZ_END and
            (n <= 0 or n * ldy * 2 <= DENSE_BYTES_MAX) and k % 2 == 0 and ldy % 2 == 0 and ldz % 2 == 0)


def stream16_native_pays(streams: int, weighted: bool) -> bool:
    """isplib_stream16_native_pays of the header: the classes of calls (slot width x weighted plan) in which every native 16-bit run
    measured faster than every run of the conversion route (profiles/stream16_ab.txt: none does); tests/test_half_host.py compares
    the two."""
    return False


ROWS16_K_MIN, ROWS16_K_END = 8, 2 ** 24   # the 16-bit row entry: eight columns per 16-byte gather; a masked lane's offset must not wrap


def rows16_serves(n: int, k: int, ldy: int, ldz: int) -> bool:
    """isplib_rows16_serves of the header: the 16-bit row entry (fusedMM_csr_rows16_hip: bf16 / fp16 operands on the plain
    row-per-wave schedule, sum / mean) serves an n x k operand at leading dimension ldy (elements) and output pitch ldz."""
    return (ROWS16_K_MIN <= k < ROWS16_K_END and n < 2 ** 31 and (n <= 0 or n * ldy * 2 <= DENSE_BYTES_MAX) and
            k % 2 == 0 and ldy % 2 == 0 and ldz % 2 == 0)


def rows16_native_pays(n: int, ldy: int, ordered: bool, weighted: bool) -> bool:
    """isplib_rows16_native_pays of the header: the classes of calls -- (operand beyond 256 MiB at 2 bytes per element or not) x
    (rows in a community order or not) x (weighted or not) -- in which every native run measured faster than every run of the
    conversion route (profiles/rows16_ab.txt: every measured class does; operand inside 256 MiB AND a community order was not
    measured and stays on convert); tests/test_rows16_host.py compares the two."""
    beyond = n > 0 and ldy > 0 and n * ldy * 2 > (256 << 20)
    return bool(beyond or not ordered)


def rows16_minmax_native_pays(n: int, ldy: int, ordered: bool, weighted: bool, want_arg: bool) -> bool:
    """isplib_rows16_minmax_native_pays of the header: the classes of calls -- those of rows16_native_pays x (positions wanted or
    not) -- in which every run of the 16-bit max / min row kernel measured faster than every run of the conversion route
    (profiles/rows16_minmax_ab.txt: every class beyond 256 MiB does; inside 256 MiB the index-order class loses on one measured shape
    and the community-order class was not measured, so both stay on convert); tests/test_rows16_minmax_host.py compares the two."""
    return bool(n > 0 and ldy > 0 and n * ldy * 2 > (256 << 20))


def rows16_colscale_native_pays(n: int, ldy: int, ordered: bool) -> bool:
    """isplib_rows16_colscale_native_pays of the header: the classes of unit-weight mean backwards -- (dY beyond 256 MiB at 2 bytes
    per element or not) x (rows of A^T in a community order or not) -- in which every run on the column-scaled 16-bit row kernel
    measured faster than every run of the conversion route (profiles/rows16_colscale_ab.txt: every measured class does; dY inside
    256 MiB AND a community order was not measured and stays on convert); tests/test_rows16_colscale_host.py compares the two."""
    beyond = n > 0 and ldy > 0 and n * ldy * 2 > (256 << 20)
    return bool(beyond or not ordered)


def rows16_gcn_native_pays(n: int, ldy: int, ordered: bool) -> bool:
    """isplib_rows16_gcn_native_pays of the header: the classes of fused GCN layers (forward + backward) on 16-bit features -- (X beyond
    256 MiB at 2 bytes per element or not) x (rows in a community order or not) -- in which every native run measured faster than every
    run of the conversion route (profiles/rows16_gcn_ab.txt: both classes beyond 256 MiB do; inside 256 MiB the index-order class loses
    on the Reddit shape, where the conversion route's fp32 layer runs on the stream schedule, and the community-order class was not
    measured, so both stay on convert); tests/test_rows16_gcn_host.py compares the two."""
    return bool(n > 0 and ldy > 0 and n * ldy * 2 > (256 << 20))


def sddmm_rows16_serves(n: int, k: int, ldy: int, ldg: int) -> bool:
    """isplib_sddmm_rows16_serves of the header: the 16-bit SDDMM row entry (isplib_sddmm_csr_rows16_hip) serves y [n, k] at leading
    dimension ldy and g at leading dimension ldg -- the 16-bit row entry's domain, and k <= 1024 (g[row, :] sits in registers)."""
    return k <= SDDMM_TASKS_K_MAX and rows16_serves(n, k, ldy, ldg)


def sddmm_rows16_native_pays(n: int, ldy: int, ordered: bool) -> bool:
    """isplib_sddmm_rows16_native_pays of the header: the classes of calls -- (y beyond 256 MiB at 2 bytes per element or not) x
    (rows in a community order or not) -- in which every run of the 16-bit SDDMM row kernel measured faster than every run of the
    conversion route (profiles/sddmm_rows16_ab.txt: both classes beyond 256 MiB do; inside 256 MiB the index-order class loses one
    run on one measured shape and the community-order class was not measured, so both stay on convert);
    tests/test_sddmm_rows16_host.py compares the two."""
    return bool(n > 0 and ldy > 0 and n * ldy * 2 > (256 << 20))


ATTENTION_K_MAX = 512                   # the attention entries hold a row in registers, two 16-byte chunks per lane


def attention_serves(rows_gathered: int, k: int, ld: int) -> bool:
    """isplib_attention_serves of the header: the attention entries (isplib_attention_csr_hip and its two backward entries) gather
    `rows_gathered` rows of k floats at leading dimension ld through one buffer descriptor."""
    return (1 <= k <= ATTENTION_K_MAX and ld >= k and rows_gathered < 2 ** 31 and
            (rows_gathered <= 0 or rows_gathered * ld * 4 <= DENSE_BYTES_MAX))


GAT_K_MAX = 512                         # the GAT entries: heads * d, a row in registers, two 16-byte chunks per lane


def gat_serves(rows_gathered: int, heads: int, d: int, ld: int) -> bool:
    """isplib_gat_serves of the header: the GAT entries (isplib_gat_csr_hip and its two backward entries) gather `rows_gathered` rows of
    heads * d floats at leading dimension ld through one buffer descriptor; with more than one head, d is a power of two >= 4 (a head
    is an aligned group of lanes and a lane's four columns never straddle heads)."""
    if heads < 1 or d < 1 or heads * d > GAT_K_MAX:
        return False
    if heads > 1 and (d < 4 or d & (d - 1)):
        return False
    return ld >= heads * d and rows_gathered < 2 ** 31 and (rows_gathered <= 0 or rows_gathered * ld * 4 <= DENSE_BYTES_MAX)


def gat_edge_serves(nnz: int, heads: int) -> bool:
    """isplib_gat_edge_serves of the header: the per-edge score term a_edge [nnz, heads] of the isplib_gat_edge_* entries sits behind one
    buffer descriptor and an entry's CSR position is a 32-bit int."""
    return heads >= 1 and 0 <= nnz < 2 ** 31 and nnz * heads * 4 <= DENSE_BYTES_MAX


def gatv2_serves(rows_gathered: int, heads: int, d: int, ld: int) -> bool:
    """isplib_gatv2_serves of the header: the GATv2 entries' domain IS isplib_gat_serves -- stated once."""
    return gat_serves(rows_gathered, heads, d, ld)


def mha_serves(rows_gathered: int, heads: int, d: int, ld: int) -> bool:
    """isplib_mha_serves of include/isplib_hip_mha.h: the multi-head dot-product entries' domain IS isplib_gat_serves, asked of every
    gathered operand (key, v; q, g in the columns entry) at its own row count and pitch; tests/test_mha_host.py compares the two."""
    return gat_serves(rows_gathered, heads, d, ld)


ATTENTION16_K_MIN, ATTENTION16_K_MAX = 8, 512   # the 16-bit attention entries: eight columns per lane, one 16-byte chunk per lane


def attention16_serves(rows_gathered: int, k: int, ld: int) -> bool:
    """isplib_attention16_serves of the header: the 16-bit attention entries (isplib_attention16_csr_hip and its two backward entries)
    gather `rows_gathered` rows of k 2-byte elements at leading dimension ld through one buffer descriptor."""
    return (ATTENTION16_K_MIN <= k <= ATTENTION16_K_MAX and k % 2 == 0 and ld % 2 == 0 and ld >= k and rows_gathered < 2 ** 31 and
            (rows_gathered <= 0 or rows_gathered * ld * 2 <= DENSE_BYTES_MAX))


def attention16_native_pays(rows_gathered: int, ld: int) -> bool:
    """isplib_attention16_native_pays of the header: the classes of calls (the gathered operand beyond 256 MiB at 2 bytes per element or
    not) in which every native run of the 16-bit attention operator (forward + backward) measured faster than every run of the
    conversion route (profiles/attention16_ab.txt: both classes do -- the Reddit shape at K = 64 / 128 inside 256 MiB, the ogbn-products
    shape at K = 128 beyond it); tests/test_attention16_host.py compares the two."""
    return bool(rows_gathered > 0 and ld > 0)


GAT16_K_MIN, GAT16_K_MAX = 8, 512      # the 16-bit GAT entries: heads * d, eight columns per lane, one 16-byte chunk per lane


def gat16_serves(rows_gathered: int, heads: int, d: int, ld: int) -> bool:
    """isplib_gat16_serves of the header: the 16-bit GAT entries (isplib_gat16_csr_hip and its two backward entries) gather
    `rows_gathered` rows of heads * d 2-byte elements at leading dimension ld through one buffer descriptor; with one head d is even,
    with more d is a power of two >= 8 (a head is an aligned group of d / 8 lanes and a lane's eight columns never straddle heads)."""
    if heads < 1 or d < 1 or not GAT16_K_MIN <= heads * d <= GAT16_K_MAX:
        return False
    if (d % 2) if heads == 1 else (d < 8 or d & (d - 1)):
        return False
    return (ld % 2 == 0 and ld >= heads * d and rows_gathered < 2 ** 31 and
            (rows_gathered <= 0 or rows_gathered * ld * 2 <= DENSE_BYTES_MAX))


def gat16_native_pays(rows_gathered: int, ld: int) -> bool:
    """isplib_gat16_native_pays of the header: the classes of calls (the gathered operand beyond 256 MiB at 2 bytes per element or not)
    in which every native run of the 16-bit GAT operator (forward + backward) measured faster than every run of the conversion route
    (profiles/gat16_ab.txt: both classes do -- the Reddit shape at (H, d) = (8, 8) / (8, 16) inside 256 MiB, the ogbn-products shape at
    (8, 16) beyond it); tests/test_gat16_host.py compares the two."""
    return bool(rows_gathered > 0 and ld > 0)


def gatv2_16_serves(rows_gathered: int, heads: int, d: int, ld: int) -> bool:
    """isplib_gatv2_16_serves of the header: the 16-bit GATv2 entries' domain IS isplib_gat16_serves -- stated once.  It is asked of
    every gathered wide operand: y with its rows (forward, rows kernel), x and the gradient with theirs (columns kernel)."""
    return gat16_serves(rows_gathered, heads, d, ld)


def gatv2_16_native_pays(rows_gathered: int, ld: int) -> bool:
    """isplib_gatv2_16_native_pays of the header: the classes of calls (the gathered operand beyond 256 MiB at 2 bytes per element or
    not) in which every native run of the 16-bit GATv2 operator (forward + backward) measured faster than every run of the conversion
    route (profiles/gatv2_16_ab.txt: both classes do -- the Reddit shape at (H, d) = (8, 8) / (8, 16) inside 256 MiB, 0.715-0.754 of the
    conversion route's time; the ogbn-products shape at (8, 16) beyond it, 0.825); tests/test_gatv2_16_host.py compares the two."""
    return bool(rows_gathered > 0 and ld > 0)


def mha16_serves(rows_gathered: int, heads: int, d: int, ld: int) -> bool:
    """isplib_qkv16_serves of include/isplib_hip_mha16.h: the 16-bit multi-head attention entries' domain IS isplib_gat16_serves --
    stated once.  It is asked of every gathered wide operand at its own row count and pitch: key and v (forward, rows kernel), q and
    the gradient (columns kernel)."""
    return gat16_serves(rows_gathered, heads, d, ld)


def mha16_native_pays(rows_gathered: int, ld: int) -> bool:
    """isplib_qkv16_native_pays of the header: the classes of calls (the gathered operand beyond 256 MiB at 2 bytes per element or
    not) in which every native run of the 16-bit multi-head attention operator (forward + backward) measured faster than every run of
    the conversion route (profiles/mha16_ab.txt: both classes do -- the Reddit shape at (H, d) = (8, 8) / (8, 16) inside 256 MiB, 0.541-0.565 of the
    conversion route's time; the ogbn-products shape at (8, 16) beyond it, 0.518); tests/test_mha16_host.py compares the two."""
    return bool(rows_gathered > 0 and ld > 0)


def mha16_drop_native_pays(rows_gathered: int, ld: int) -> bool:
    """isplib_qkv_half_drop_native_pays of include/isplib_hip_mha16_drop.h: the classes of calls (the gathered operand beyond 256 MiB
    at 2 bytes per element or not) in which every native run of the 16-bit multi-head attention operator WITH dropout (forward +
    backward through mha_matmul) measured faster than every run of the conversion route (profiles/mha16_dropout_ab.txt: both classes
    do -- the Reddit shape at (H, d) = (8, 8) / (8, 16) inside 256 MiB, 0.562-0.564 of the conversion route's time; the ogbn-products
    shape at (8, 16) beyond it, 0.494); tests/test_mha16_dropout_host.py compares the two."""
    return bool(rows_gathered > 0 and ld > 0)


def owner_exchange_serves(m: int, k: int, world: int, cuts) -> bool:
    """isplib_owner_exchange_serves of the header: m x k winners split for `world` owners at the row boundaries `cuts`."""
    if not 1 <= world <= OWNER_WORLD_MAX or m < 0 or k < 0 or m * k >= MINMAX_BW_PAIRS_END:
        return False
    return all(cuts[p + 1] >= cuts[p] and (cuts[p + 1] - cuts[p]) * k <= MINMAX_BW_KEYS_MAX for p in range(world))


def scatter_keys_serves(total: int, n: int, k: int) -> bool:
    """The domain of isplib_scatter_keys_det_hip: the same two bounds for `total` pairs into an n x k block."""
    return 0 <= total < MINMAX_BW_PAIRS_END and n >= 0 and k >= 0 and n * k <= MINMAX_BW_KEYS_MAX

# FusedMM stage flags (csrc/fusedMM.h:18-74) and the built-in SOP_UDEF menu (enum isplib_sop_udef)
VOP = {"copy_lhs": 0x1, "copy_rhs": 0x2, "add": 0x3, "subl": 0x4, "subr": 0x5, "max": 0x6, "min": 0x7, "udef": 0xF}
ROP = {"noop": 0x00, "dot": 0x10, "add_lhs": 0x20, "add_rhs": 0x30, "norml": 0x40, "normr": 0x50, "udef": 0xF0}
SOP = {"noop": 0x000, "copy": 0x100, "udef": 0xF00}
VSC = {"noop": 0x0000, "mul": 0x1000, "add": 0x2000, "mean": 0x3000, "udef": 0xF000}
AOP = {"add": 0x10000, "max": 0x20000, "min": 0x30000, "udef": 0xF0000}
SOP_UDEF = {"none": 0, "sigmoid": 1, "one_minus_sigmoid": 2, "tdist": 3, "scale": 4, "exp": 5, "leaky_exp": 6}
# the FusedMM paper's named patterns as message words (+ the menu entry their SOP_UDEF stands for)
PATTERNS = {
    "spmm": (MSG_SPMM_SUM, "none"),
    "sigmoid_embedding": (VOP["copy_rhs"] | ROP["dot"] | SOP["udef"] | VSC["mul"] | AOP["add"], "sigmoid"),
    "tdist_embedding": (VOP["subr"] | ROP["normr"] | SOP["udef"] | VSC["mul"] | AOP["add"], "tdist"),
    "attention_sum": (VOP["copy_rhs"] | ROP["dot"] | SOP["udef"] | VSC["mul"] | AOP["add"], "leaky_exp"),
}

EXPORTS = (
    "isplib_hip_abi_version", "isplib_hip_last_error", "isplib_hip_set_empty_row", "isplib_hip_get_empty_row", "fusedMM_csr_hip", "performDummySpMM_hip",
    "isplib_spmm_minmax_bw_hip", "isplib_sddmm_csr_hip", "isplib_csr_row_ids_hip",
    "isplib_csr2csc_workspace_bytes", "isplib_csr2csc_hip",
    "isplib_spmm_slices_bytes", "isplib_spmm_slices_build_hip", "isplib_spmm_sliced_workspace_bytes",
    "fusedMM_csr_sliced_hip", "fusedMM_csr_sliced_phase_hip", "isplib_hip_tune",
    "isplib_spmm_tasks_workspace_bytes", "fusedMM_csr_tasks_hip",
    "isplib_spmm_tasks_plan_workspace_bytes", "isplib_spmm_tasks_count_hip", "isplib_spmm_tasks_fill_hip",
    "isplib_sddmm_csr_tasks_hip", "fusedMM_csr_tasks_epilogue_hip", "fusedMM_csr_udef_hip", "fusedMM_csr_udef_tasks_hip", "isplib_pack_indices_hip",
    "isplib_suggest_slices", "isplib_graph_create", "isplib_graph_set_slices", "isplib_graph_set_values", "isplib_graph_spmm", "isplib_graph_spmm_backward",
    "isplib_graph_destroy", "isplib_suggest_slices_whole_rows", "isplib_graph_sddmm",
    "fusedMM_csr_stream_hip", "isplib_spmm_stream_workspace_bytes", "isplib_spmm_stream_geometry", "isplib_suggest_stream", "isplib_suggest_stream_weighted", "isplib_stream_plan_build_hip", "isplib_stream_plan_build_caps_hip", "isplib_stream_capacities_hip", "isplib_stream_plan_build_minmax_hip", "fusedMM_csr_stream_minmax_hip", "isplib_spmm_stream_minmax_geometry", "isplib_suggest_stream_minmax", "isplib_spmm_stream_minmax_workspace_bytes", "isplib_stream_plan_set_values_hip", "isplib_stream_plan_free", "isplib_stream_packed_dwords", "isplib_stream_pack_hip", "isplib_spmm_minmax_bw_det_hip", "isplib_spmm_minmax_bw_workspace_bytes", "isplib_scatter_rows_det_hip",
    "isplib_minmax_bw_bucket_workspace_bytes", "isplib_minmax_bw_bucket_hip", "isplib_scatter_keys_workspace_bytes", "isplib_scatter_keys_det_hip",
    "isplib_fusedmm_stream_geometry", "isplib_suggest_fusedmm_stream", "isplib_stream_plan_build_fusedmm_hip", "fusedMM_csr_udef_stream_hip",
    "isplib_row_scale_hip", "isplib_masked_scale_colsum_hip", "isplib_masked_scale_colsum_workspace_bytes",
    "fusedMM_csr_ordered_hip", "isplib_community_order_hip", "isplib_community_order_workspace_bytes", "isplib_order_locality_hip",
    "isplib_graph_set_row_order", "isplib_plain_panels",
    "fusedMM_csr_stream16_hip", "isplib_stream16_auto",
    "fusedMM_csr_rows16_hip", "isplib_rows16_auto", "isplib_rows16_domain",
    "fusedMM_csr_rows16_minmax_hip", "isplib_rows16_minmax_auto",
    "fusedMM_csr_rows16_colscale_hip", "isplib_rows16_colscale_auto",
    "fusedMM_csr_rows16_epilogue_hip", "isplib_rows16_gcn_auto", "isplib_masked_colsum16_hip", "isplib_masked_colsum16_workspace_bytes",
    "isplib_sddmm_csr_rows16_hip", "isplib_sddmm_rows16_auto",
    "isplib_attention_csr_hip", "isplib_attention_bw_rows_hip", "isplib_attention_bw_cols_hip", "isplib_attention_domain",
    "isplib_attention16_csr_hip", "isplib_attention16_bw_rows_hip", "isplib_attention16_bw_cols_hip", "isplib_attention16_domain",
    "isplib_attention16_auto",
    "isplib_gat_csr_hip", "isplib_gat_bw_rows_hip", "isplib_gat_bw_cols_hip", "isplib_gat_domain",
    "isplib_gat_edge_csr_hip", "isplib_gat_edge_bw_rows_hip", "isplib_gat_edge_bw_cols_hip", "isplib_gat_edge_domain",
    "isplib_gat_drop_csr_hip", "isplib_gat_drop_bw_rows_hip", "isplib_gat_drop_bw_cols_hip",
    "isplib_gat16_csr_hip", "isplib_gat16_bw_rows_hip", "isplib_gat16_bw_cols_hip", "isplib_gat16_domain", "isplib_gat16_auto",
    "isplib_gatv2_csr_hip", "isplib_gatv2_bw_rows_hip", "isplib_gatv2_bw_rows_workspace_bytes", "isplib_gatv2_bw_cols_hip",
    "isplib_gatv2_domain",
)

# include/isplib_hip_gatv2_16.h (which isplib_hip.h includes; the same library): the 16-bit GATv2 entries, listed apart because EXPORTS
# is what isplib_hip.h itself declares; tests/test_gatv2_16_host.py compares this list with that header and the library's symbols
GATV2_16_EXPORTS = (
    "isplib_gatv2_16_csr_hip", "isplib_gatv2_16_bw_rows_hip", "isplib_gatv2_16_bw_rows_workspace_bytes", "isplib_gatv2_16_bw_cols_hip",
    "isplib_gatv2_16_domain", "isplib_gatv2_16_auto",
)

# include/isplib_hip_gatv2_drop.h (which isplib_hip.h includes; the same library): the GATv2 entries with attention dropout, listed
# apart for the reason the 16-bit GATv2 entries are -- EXPORTS is what isplib_hip.h itself declares, and its GATv2 names are pinned
GATV2_DROP_EXPORTS = ("isplib_gatv2_drop_csr_hip", "isplib_gatv2_drop_bw_rows_hip", "isplib_gatv2_drop_bw_cols_hip")

# include/isplib_hip_mha.h (which isplib_hip.h includes; the same library): multi-head dot-product attention with separate keys and
# values, listed apart for the same reason; tests/test_mha_host.py compares this list with that header and the library's symbols
MHA_EXPORTS = ("isplib_mha_csr_hip", "isplib_mha_bw_rows_hip", "isplib_mha_bw_cols_hip", "isplib_mha_domain")

# include/isplib_hip_mha16.h (which isplib_hip.h includes; the same library): the 16-bit multi-head attention entries.  Their prefix is
# isplib_qkv16_ because the symbols that start with isplib_mha are pinned to MHA_EXPORTS; tests/test_mha16_host.py compares this list
# with that header and the library's symbols
# include/isplib_hip_mha_drop.h (which isplib_hip.h includes; the same library): the fp32 multi-head attention entries with attention
# dropout.  Their prefix is isplib_qkv_drop_ because the symbols that start with isplib_mha and isplib_qkv16 are pinned to the two lists
# around this one; tests/test_mha_dropout_host.py compares this list with the header and the library
MHA_DROP_EXPORTS = ("isplib_qkv_drop_csr_hip", "isplib_qkv_drop_bw_rows_hip", "isplib_qkv_drop_bw_cols_hip")

# include/isplib_hip_mha16_drop.h (which isplib_hip.h includes; the same library): the 16-bit multi-head attention entries with attention
# dropout.  Their prefix is isplib_qkv_half_drop_ because the symbols that start with isplib_mha, isplib_qkv16 and isplib_qkv_drop are
# pinned to the three lists above; tests/test_mha16_dropout_host.py compares this list with the header and the library
MHA16_DROP_EXPORTS = ("isplib_qkv_half_drop_csr_hip", "isplib_qkv_half_drop_bw_rows_hip", "isplib_qkv_half_drop_bw_cols_hip",
                      "isplib_qkv_half_drop_auto")

MHA16_EXPORTS = ("isplib_qkv16_csr_hip", "isplib_qkv16_bw_rows_hip", "isplib_qkv16_bw_cols_hip", "isplib_qkv16_domain", "isplib_qkv16_auto")

# the two host functions of the dropout keep bit (isplib_hip.h declares them; they return uint32_t, not a status, and are listed apart)
GAT_DROP_HOST_EXPORTS = ("isplib_gat_drop_threshold", "isplib_gat_drop_word")

# include/isplib_hip_experimental.h (libisplib_hip_exp.so): forms measured slower than the defaults; tests and experiment scripts only
EXP_EXPORTS = ("fusedMM_csr_sweep_hip", "isplib_spmm_sweep_workspace_bytes", "isplib_spmm_sweep_resident_waves",
               "fusedMM_csr_hybrid_hip", "isplib_spmm_hybrid_geometry", "isplib_spmm_hybrid_workspace_bytes", "isplib_sddmm_stream_hip",
               "isplib_hip_tune_experimental")

_i64, _f32, _vp, _i32 = ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_int32


class Epilogue(ctypes.Structure):          # isplib_epilogue
    _fields_ = [("row_scale", ctypes.c_void_p), ("self", ctypes.c_void_p), ("ld_self", ctypes.c_int64),
                ("bias", ctypes.c_void_p), ("relu", ctypes.c_int)]


class TaskPlanInfo(ctypes.Structure):      # isplib_task_plan_info
    _fields_ = [("n_tasks", ctypes.c_int64), ("lane_off", ctypes.c_int64 * 9), ("slices", ctypes.c_int32),
                ("chunk", ctypes.c_int32), ("short_row", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class SweepPlanStruct(ctypes.Structure):   # isplib_sweep_plan
    _fields_ = [("rows", ctypes.c_int64), ("slices", ctypes.c_int32), ("gens", ctypes.c_int32),
                ("waves_per_gen", ctypes.c_int32), ("rows_per_wave", ctypes.c_int32), ("n_tasks", ctypes.c_int64),
                ("n_parts", ctypes.c_int64), ("n_hub", ctypes.c_int64), ("wave_row", ctypes.c_void_p),
                ("wave_part", ctypes.c_void_p), ("wave_task_off", ctypes.c_void_p), ("task_b", ctypes.c_void_p),
                ("task_meta", ctypes.c_void_p), ("hub_row", ctypes.c_void_p), ("hub_off", ctypes.c_void_p)]


class StreamPlanStruct(ctypes.Structure):  # isplib_stream_plan
    _fields_ = [("rows", ctypes.c_int64), ("cols", ctypes.c_int64), ("slices", ctypes.c_int32), ("gens", ctypes.c_int32),
                ("waves_per_gen", ctypes.c_int32), ("rows_per_wave", ctypes.c_int32), ("streams", ctypes.c_int32),
                ("chunk", ctypes.c_int32), ("n_steps", ctypes.c_int64), ("n_parts", ctypes.c_int64), ("n_hub", ctypes.c_int64),
                ("words", ctypes.c_void_p), ("vals", ctypes.c_void_p), ("wave_step_off", ctypes.c_void_p),
                ("wave_row", ctypes.c_void_p), ("wave_part", ctypes.c_void_p),
                ("hub_row", ctypes.c_void_p), ("hub_off", ctypes.c_void_p), ("perm", ctypes.c_void_p),
                ("packed", ctypes.c_void_p), ("has_packed", ctypes.c_int32)]      # the packed word stream (None / 0: none)


class HybridPlanStruct(ctypes.Structure):  # isplib_hybrid_plan
    _fields_ = [("cold", StreamPlanStruct), ("table_rows", ctypes.c_int32), ("hot_cap", ctypes.c_int32), ("n_hot_steps", ctypes.c_int64),
                ("hot_rows", ctypes.c_void_p), ("hot_words", ctypes.c_void_p), ("hot_step_off", ctypes.c_void_p),
                ("hot_perm", ctypes.c_void_p)]


_sigs_set = False


def lib() -> ctypes.CDLL:
    global _sigs_set
    L = _lib.cdll()
    if not _sigs_set:
        L.isplib_hip_abi_version.restype = ctypes.c_int
        L.isplib_hip_last_error.restype = ctypes.c_char_p
        L.fusedMM_csr_hip.restype = ctypes.c_int
        L.fusedMM_csr_hip.argtypes = [_i32, _i64, _i64, _i64, _f32, _i64, _i64, _i64, _vp, _vp, _vp, _vp,
                                      _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp]
        L.fusedMM_csr_udef_hip.restype = ctypes.c_int
        L.fusedMM_csr_udef_hip.argtypes = [_i32, _i64, _i64, _i64, _f32, _i64, _i64, _i64, _vp, _vp, _vp, _vp,
                                           _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, ctypes.c_int, _f32, _vp]
        L.fusedMM_csr_udef_tasks_hip.restype = ctypes.c_int
        L.fusedMM_csr_udef_tasks_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp,
                                                 _vp, _vp, ctypes.c_int, _vp, _vp, _i64, _vp, _i64, _vp, ctypes.c_int, _f32,
                                                 _vp, ctypes.c_size_t, _vp]
        L.performDummySpMM_hip.restype = None
        L.performDummySpMM_hip.argtypes = [_i64, _vp]
        L.isplib_spmm_minmax_bw_hip.restype = ctypes.c_int
        L.isplib_spmm_minmax_bw_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        L.isplib_sddmm_csr_hip.restype = ctypes.c_int
        L.isplib_sddmm_csr_hip.argtypes = [_i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, ctypes.c_int, _vp, _vp]
        L.isplib_csr_row_ids_hip.restype = ctypes.c_int
        L.isplib_csr_row_ids_hip.argtypes = [_i64, _i64, _vp, _vp, _vp]
        L.isplib_csr2csc_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_csr2csc_workspace_bytes.argtypes = [_i64, _i64, _i64]
        L.isplib_csr2csc_hip.restype = ctypes.c_int
        L.isplib_csr2csc_hip.argtypes = [_i64, _i64, _i64, _vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp,
                                         _vp, ctypes.c_size_t, _vp]
        L.isplib_spmm_slices_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_slices_bytes.argtypes = [_i64, ctypes.c_int]
        L.isplib_spmm_slices_build_hip.restype = ctypes.c_int
        L.isplib_spmm_slices_build_hip.argtypes = [_i64, _i64, _i64, _vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp]
        L.isplib_spmm_sliced_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_sliced_workspace_bytes.argtypes = [_i32, _i64, _i64, ctypes.c_int]
        L.fusedMM_csr_sliced_hip.restype = ctypes.c_int
        L.fusedMM_csr_sliced_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
                                             _vp, _i64, _vp, _i64, _vp, _vp, ctypes.c_size_t, _vp]
        L.fusedMM_csr_sliced_phase_hip.restype = ctypes.c_int
        L.fusedMM_csr_sliced_phase_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _i64, _vp, _i64, _vp,
                                                   _vp, ctypes.c_size_t, _vp]
        L.isplib_spmm_tasks_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_tasks_workspace_bytes.argtypes = [_i32, _i64, _i64]
        L.fusedMM_csr_tasks_hip.restype = ctypes.c_int
        L.isplib_pack_indices_hip.restype = ctypes.c_int
        L.isplib_pack_indices_hip.argtypes = [_i64, _vp, _vp, _vp]
        L.fusedMM_csr_tasks_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp,
                                            ctypes.c_int, _vp, _vp, _i64, _vp, _i64, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_spmm_tasks_plan_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_tasks_plan_workspace_bytes.argtypes = [_i64, ctypes.c_int]
        L.isplib_spmm_tasks_count_hip.restype = ctypes.c_int
        L.isplib_spmm_tasks_count_hip.argtypes = [_i64, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp,
                                                  ctypes.c_size_t, ctypes.POINTER(TaskPlanInfo), _vp]
        L.isplib_spmm_tasks_fill_hip.restype = ctypes.c_int
        L.isplib_spmm_tasks_fill_hip.argtypes = [_i64, _vp, _vp, _vp, ctypes.POINTER(TaskPlanInfo), _vp, _vp, _vp, _vp, _vp]
        L.isplib_sddmm_csr_tasks_hip.restype = ctypes.c_int
        L.isplib_sddmm_csr_tasks_hip.argtypes = [_i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp,
                                                 _i64, ctypes.c_int, _vp, _vp]
        L.fusedMM_csr_tasks_epilogue_hip.restype = ctypes.c_int
        L.fusedMM_csr_tasks_epilogue_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp,
                                                     ctypes.c_int, _vp, _vp, _i64, _vp, _i64, _vp, ctypes.c_size_t,
                                                     ctypes.POINTER(Epilogue), _vp]
        L.isplib_suggest_slices.restype = ctypes.c_int
        L.isplib_suggest_slices.argtypes = [_i64, _i64, _i64, _i64, ctypes.c_int]
        L.isplib_graph_create.restype = ctypes.c_int
        L.isplib_graph_create.argtypes = [_i64, _i64, _i64, _vp, _vp, _vp, ctypes.POINTER(_vp)]
        L.isplib_graph_set_slices.restype = ctypes.c_int
        L.isplib_graph_set_slices.argtypes = [_vp, ctypes.c_int]
        L.isplib_graph_set_values.restype = ctypes.c_int
        L.isplib_graph_set_values.argtypes = [_vp, _vp]
        L.isplib_graph_spmm.restype = ctypes.c_int
        L.isplib_graph_spmm.argtypes = [_vp, _i32, _i64, _vp, _i64, _vp, _i64, _vp, _vp]
        L.isplib_graph_spmm_backward.restype = ctypes.c_int
        L.isplib_graph_spmm_backward.argtypes = [_vp, ctypes.c_int, _i64, _vp, _i64, _vp, _i64, _vp]
        L.isplib_suggest_slices_whole_rows.restype = ctypes.c_int
        L.isplib_suggest_slices_whole_rows.argtypes = [_i64, _i64, _i64, _i64]
        L.isplib_graph_sddmm.restype = ctypes.c_int
        L.isplib_graph_sddmm.argtypes = [_vp, ctypes.c_int, _i64, _vp, _i64, _vp, _i64, _vp, _vp]
        L.isplib_graph_destroy.restype = None
        L.isplib_graph_destroy.argtypes = [_vp]
        L.isplib_hip_tune.restype = ctypes.c_int
        L.isplib_hip_tune.argtypes = [ctypes.c_int, ctypes.c_int]
        L.isplib_spmm_minmax_bw_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_minmax_bw_workspace_bytes.argtypes = [_i64, _i64, _i64]
        L.isplib_spmm_minmax_bw_det_hip.restype = ctypes.c_int
        L.isplib_spmm_minmax_bw_det_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_fusedmm_stream_geometry.restype = ctypes.c_int
        L.isplib_fusedmm_stream_geometry.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.isplib_suggest_fusedmm_stream.restype = ctypes.c_int
        L.isplib_suggest_fusedmm_stream.argtypes = [_i32, _i64, _i64, _i64, _i64] + [ctypes.POINTER(ctypes.c_int)] * 3
        L.isplib_stream_plan_build_fusedmm_hip.restype = ctypes.c_int
        L.isplib_stream_plan_build_fusedmm_hip.argtypes = [_i64, _i64, _i64, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                           ctypes.POINTER(StreamPlanStruct), _vp]
        L.fusedMM_csr_udef_stream_hip.restype = ctypes.c_int
        L.fusedMM_csr_udef_stream_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, ctypes.POINTER(StreamPlanStruct), _vp, _i64, _vp, _i64,
                                                  _vp, _i64, ctypes.c_int, _f32, _vp, ctypes.c_size_t, _vp]
        L.isplib_row_scale_hip.restype = ctypes.c_int
        L.isplib_row_scale_hip.argtypes = [_i64, _i64, _vp, _i64, _vp, _vp, _i64, _vp]
        L.isplib_masked_scale_colsum_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_masked_scale_colsum_workspace_bytes.argtypes = [_i64, _i64]
        L.isplib_masked_scale_colsum_hip.restype = ctypes.c_int
        L.isplib_masked_scale_colsum_hip.argtypes = [_i64, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_scatter_rows_det_hip.restype = ctypes.c_int
        L.isplib_scatter_rows_det_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_minmax_bw_bucket_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_minmax_bw_bucket_workspace_bytes.argtypes = [_i64, _i64, ctypes.c_int]
        L.isplib_minmax_bw_bucket_hip.restype = ctypes.c_int
        L.isplib_minmax_bw_bucket_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.POINTER(_i64), _vp, _vp, _vp,
                                                  _vp, ctypes.c_size_t, _vp]
        L.isplib_scatter_keys_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_scatter_keys_workspace_bytes.argtypes = [_i64, _i64, _i64]
        L.isplib_scatter_keys_det_hip.restype = ctypes.c_int
        L.isplib_scatter_keys_det_hip.argtypes = [_i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_stream_plan_build_hip.restype = ctypes.c_int
        L.isplib_stream_plan_build_hip.argtypes = [_i64, _i64, _i64, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                   ctypes.POINTER(StreamPlanStruct), _vp]
        L.isplib_stream_plan_build_caps_hip.restype = ctypes.c_int
        L.isplib_stream_plan_build_caps_hip.argtypes = [_i64, _i64, _i64, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                        _vp, ctypes.POINTER(StreamPlanStruct), _vp]
        L.isplib_stream_capacities_hip.restype = ctypes.c_int
        L.isplib_stream_capacities_hip.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64, _vp, ctypes.POINTER(ctypes.c_int), _vp]
        L.isplib_stream_packed_dwords.restype = ctypes.c_size_t
        L.isplib_stream_packed_dwords.argtypes = [ctypes.POINTER(StreamPlanStruct)]
        L.isplib_stream_pack_hip.restype = ctypes.c_int
        L.isplib_stream_pack_hip.argtypes = [ctypes.POINTER(StreamPlanStruct), _vp, _i64, ctypes.POINTER(ctypes.c_int), _vp]
        L.isplib_stream_pack_set.restype = ctypes.c_int
        L.isplib_stream_pack_set.argtypes = [ctypes.c_int]
        L.isplib_stream_pack_last.restype = ctypes.c_int
        L.isplib_stream_pack_last.argtypes = []
        L.isplib_stream_level_set.restype = ctypes.c_int
        L.isplib_stream_level_set.argtypes = [ctypes.c_int]
        L.isplib_stream_plan_build_minmax_hip.restype = ctypes.c_int
        L.isplib_stream_plan_build_minmax_hip.argtypes = [_i64, _i64, _i64, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                          ctypes.POINTER(StreamPlanStruct), _vp]
        L.isplib_spmm_stream_minmax_geometry.restype = ctypes.c_int
        L.isplib_spmm_stream_minmax_geometry.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.isplib_suggest_stream_minmax.restype = ctypes.c_int
        L.isplib_suggest_stream_minmax.argtypes = [_i64, _i64, _i64, _i64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.isplib_spmm_stream_minmax_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_stream_minmax_workspace_bytes.argtypes = [ctypes.POINTER(StreamPlanStruct)]
        L.fusedMM_csr_stream_minmax_hip.restype = ctypes.c_int
        L.fusedMM_csr_stream_minmax_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, ctypes.POINTER(StreamPlanStruct), _vp, _i64,
                                                    _vp, _i64, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_stream_plan_set_values_hip.restype = ctypes.c_int
        L.isplib_stream_plan_set_values_hip.argtypes = [ctypes.POINTER(StreamPlanStruct), _vp, _vp]
        L.isplib_stream_plan_free.restype = None
        L.isplib_stream_plan_free.argtypes = [ctypes.POINTER(StreamPlanStruct)]
        L.isplib_community_order_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_community_order_workspace_bytes.argtypes = [_i64, _i64]
        L.isplib_community_order_hip.restype = ctypes.c_int
        L.isplib_community_order_hip.argtypes = [_i64, _i64, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.POINTER(ctypes.c_int), _vp,
                                                 ctypes.c_size_t, _vp]
        L.isplib_order_locality_hip.restype = ctypes.c_int
        L.isplib_order_locality_hip.argtypes = [_i64, _i64, _vp, _vp, _vp, _i64, ctypes.POINTER(ctypes.c_double), _vp, ctypes.c_size_t, _vp]
        L.isplib_graph_set_row_order.restype = ctypes.c_int
        L.isplib_graph_set_row_order.argtypes = [_vp, _vp, _vp]
        L.fusedMM_csr_ordered_hip.restype = ctypes.c_int
        L.fusedMM_csr_ordered_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]
        L.isplib_plain_panels.restype = ctypes.c_int
        L.isplib_plain_panels.argtypes = [_i64, _i64]
        L.isplib_suggest_stream.restype = ctypes.c_int
        L.isplib_suggest_stream.argtypes = [_i64, _i64, _i64, _i64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.isplib_suggest_stream_weighted.restype = ctypes.c_int
        L.isplib_suggest_stream_weighted.argtypes = [_i64, _i64, _i64, _i64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.isplib_spmm_stream_geometry.restype = ctypes.c_int
        L.isplib_spmm_stream_geometry.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.isplib_spmm_stream_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_stream_workspace_bytes.argtypes = [ctypes.POINTER(StreamPlanStruct)]
        L.fusedMM_csr_stream_hip.restype = ctypes.c_int
        L.fusedMM_csr_stream_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, ctypes.POINTER(StreamPlanStruct), _vp, _i64,
                                             _vp, _i64, _vp, ctypes.c_size_t, ctypes.POINTER(Epilogue), _vp]
        L.fusedMM_csr_stream16_hip.restype = ctypes.c_int
        L.fusedMM_csr_stream16_hip.argtypes = [_i32, ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, ctypes.POINTER(StreamPlanStruct), _vp, _i64,
                                               _vp, _i64, _vp, ctypes.c_size_t, _vp]
        L.isplib_stream16_auto.restype = ctypes.c_int
        L.isplib_stream16_auto.argtypes = [ctypes.c_int, ctypes.c_int]
        L.fusedMM_csr_rows16_hip.restype = ctypes.c_int
        L.fusedMM_csr_rows16_hip.argtypes = [_i32, ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]
        L.isplib_rows16_auto.restype = ctypes.c_int
        L.isplib_rows16_auto.argtypes = [_i64, _i64, ctypes.c_int, ctypes.c_int]
        L.isplib_rows16_domain.restype = ctypes.c_int
        L.isplib_rows16_domain.argtypes = [_i64, _i64, _i64, _i64]
        L.fusedMM_csr_rows16_minmax_hip.restype = ctypes.c_int
        L.fusedMM_csr_rows16_minmax_hip.argtypes = [_i32, ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]
        L.isplib_rows16_minmax_auto.restype = ctypes.c_int
        L.isplib_rows16_minmax_auto.argtypes = [_i64, _i64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        L.fusedMM_csr_rows16_colscale_hip.restype = ctypes.c_int
        L.fusedMM_csr_rows16_colscale_hip.argtypes = [_i32, ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]
        L.isplib_rows16_colscale_auto.restype = ctypes.c_int
        L.isplib_rows16_colscale_auto.argtypes = [_i64, _i64, ctypes.c_int]
        L.fusedMM_csr_rows16_epilogue_hip.restype = ctypes.c_int
        L.fusedMM_csr_rows16_epilogue_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp]
        L.isplib_rows16_gcn_auto.restype = ctypes.c_int
        L.isplib_rows16_gcn_auto.argtypes = [_i64, _i64, ctypes.c_int]
        L.isplib_masked_colsum16_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_masked_colsum16_workspace_bytes.argtypes = [_i64, _i64]
        L.isplib_masked_colsum16_hip.restype = ctypes.c_int
        L.isplib_masked_colsum16_hip.argtypes = [ctypes.c_int, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_sddmm_csr_rows16_hip.restype = ctypes.c_int
        L.isplib_sddmm_csr_rows16_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, ctypes.c_int, _vp, _vp]
        L.isplib_sddmm_rows16_auto.restype = ctypes.c_int
        L.isplib_sddmm_rows16_auto.argtypes = [_i64, _i64, ctypes.c_int]
        L.isplib_attention_domain.restype = ctypes.c_int
        L.isplib_attention_domain.argtypes = [_i64, _i64, _i64]
        L.isplib_attention_csr_hip.restype = ctypes.c_int
        L.isplib_attention_csr_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp]
        L.isplib_attention_bw_rows_hip.restype = ctypes.c_int
        L.isplib_attention_bw_rows_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _i64, _vp,
                                                   _vp, _i64, _vp, _vp]
        L.isplib_attention_bw_cols_hip.restype = ctypes.c_int
        L.isplib_attention_bw_cols_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp, _vp,
                                                   _i64, _vp]
        L.isplib_gat_domain.restype = ctypes.c_int
        L.isplib_gat_domain.argtypes = [_i64, _i64, _i64, _i64]
        L.isplib_gat_csr_hip.restype = ctypes.c_int
        L.isplib_gat_csr_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp]
        L.isplib_gat_bw_rows_hip.restype = ctypes.c_int
        L.isplib_gat_bw_rows_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _i64, _vp,
                                             _vp, _vp, _vp]
        L.isplib_gat_bw_cols_hip.restype = ctypes.c_int
        L.isplib_gat_bw_cols_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp, _vp,
                                             _i64, _vp, _vp]
        L.isplib_gat_edge_domain.restype = ctypes.c_int
        L.isplib_gat_edge_domain.argtypes = [_i64, _i64]
        L.isplib_gat_edge_csr_hip.restype = ctypes.c_int          # isplib_gat_csr_hip with a_edge after a_src
        L.isplib_gat_edge_csr_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _f32, _vp, _i64, _vp, _vp]
        L.isplib_gat_edge_bw_rows_hip.restype = ctypes.c_int      # ... and a trailing d_a_edge (after the stream), which may be NULL
        L.isplib_gat_edge_bw_rows_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _f32, _vp, _i64, _vp,
                                                  _i64, _vp, _vp, _vp, _vp, _vp]
        L.isplib_gat_edge_bw_cols_hip.restype = ctypes.c_int      # isplib_gat_bw_cols_hip with csr2csc after cole, a_edge after a_src
        L.isplib_gat_edge_bw_cols_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _f32, _vp, _i64,
                                                  _vp, _vp, _vp, _i64, _vp, _vp]
        # the isplib_gat_edge_* argument lists (a_edge / d_a_edge may be NULL), then threshold, scale, seed
        L.isplib_gat_drop_threshold.restype = ctypes.c_uint32
        L.isplib_gat_drop_threshold.argtypes = [ctypes.c_double]
        L.isplib_gat_drop_word.restype = ctypes.c_uint32
        L.isplib_gat_drop_word.argtypes = [ctypes.c_uint64, _i64, _i64]
        _drop = [ctypes.c_uint32, _f32, ctypes.c_uint64]
        L.isplib_gat_drop_csr_hip.restype = ctypes.c_int
        L.isplib_gat_drop_csr_hip.argtypes = L.isplib_gat_edge_csr_hip.argtypes + _drop
        L.isplib_gat_drop_bw_rows_hip.restype = ctypes.c_int
        L.isplib_gat_drop_bw_rows_hip.argtypes = L.isplib_gat_edge_bw_rows_hip.argtypes + _drop
        L.isplib_gat_drop_bw_cols_hip.restype = ctypes.c_int
        L.isplib_gat_drop_bw_cols_hip.argtypes = L.isplib_gat_edge_bw_cols_hip.argtypes + _drop
        L.isplib_gatv2_domain.restype = ctypes.c_int
        L.isplib_gatv2_domain.argtypes = [_i64, _i64, _i64, _i64]
        L.isplib_gatv2_bw_rows_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_gatv2_bw_rows_workspace_bytes.argtypes = [_i64, _i64]
        L.isplib_gatv2_csr_hip.restype = ctypes.c_int
        L.isplib_gatv2_csr_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp]
        L.isplib_gatv2_bw_rows_hip.restype = ctypes.c_int
        L.isplib_gatv2_bw_rows_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _i64,
                                               _vp, _vp, _i64, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_gatv2_bw_cols_hip.restype = ctypes.c_int
        L.isplib_gatv2_bw_cols_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp,
                                               _vp, _i64, _vp]
        # the isplib_gatv2_* argument lists (the columns entry with csr2csc after cole), then threshold, scale, seed
        L.isplib_gatv2_drop_csr_hip.restype = ctypes.c_int
        L.isplib_gatv2_drop_csr_hip.argtypes = L.isplib_gatv2_csr_hip.argtypes + _drop
        L.isplib_gatv2_drop_bw_rows_hip.restype = ctypes.c_int
        L.isplib_gatv2_drop_bw_rows_hip.argtypes = L.isplib_gatv2_bw_rows_hip.argtypes + _drop
        L.isplib_gatv2_drop_bw_cols_hip.restype = ctypes.c_int
        L.isplib_gatv2_drop_bw_cols_hip.argtypes = (L.isplib_gatv2_bw_cols_hip.argtypes[:7] + [_vp] + L.isplib_gatv2_bw_cols_hip.argtypes[7:] +
                                                    _drop)
        L.isplib_mha_domain.restype = ctypes.c_int
        L.isplib_mha_domain.argtypes = [_i64, _i64, _i64, _i64]
        L.isplib_mha_csr_hip.restype = ctypes.c_int
        L.isplib_mha_csr_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _f32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]
        L.isplib_mha_bw_rows_hip.restype = ctypes.c_int
        L.isplib_mha_bw_rows_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _f32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64,
                                             _vp, _vp, _i64, _vp, _vp]
        L.isplib_mha_bw_cols_hip.restype = ctypes.c_int
        L.isplib_mha_bw_cols_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _f32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64,
                                             _vp, _i64, _vp, _i64, _vp]
        # the isplib_mha_* argument lists behind a dtype; the rows entry takes no z
        L.isplib_qkv16_domain.restype = ctypes.c_int
        L.isplib_qkv16_domain.argtypes = [_i64, _i64, _i64, _i64]
        L.isplib_qkv16_auto.restype = ctypes.c_int
        L.isplib_qkv16_auto.argtypes = [_i64, _i64]
        L.isplib_qkv16_csr_hip.restype = ctypes.c_int
        L.isplib_qkv16_csr_hip.argtypes = [ctypes.c_int] + L.isplib_mha_csr_hip.argtypes
        # the isplib_mha_* argument lists (the columns entry with csr2csc after cole), then threshold, keep_scale, seed
        L.isplib_qkv_drop_csr_hip.restype = ctypes.c_int
        L.isplib_qkv_drop_csr_hip.argtypes = L.isplib_mha_csr_hip.argtypes + _drop
        L.isplib_qkv_drop_bw_rows_hip.restype = ctypes.c_int
        L.isplib_qkv_drop_bw_rows_hip.argtypes = L.isplib_mha_bw_rows_hip.argtypes + _drop
        L.isplib_qkv_drop_bw_cols_hip.restype = ctypes.c_int
        L.isplib_qkv_drop_bw_cols_hip.argtypes = (L.isplib_mha_bw_cols_hip.argtypes[:7] + [_vp] + L.isplib_mha_bw_cols_hip.argtypes[7:] +
                                                  _drop)
        L.isplib_qkv16_bw_rows_hip.restype = ctypes.c_int
        L.isplib_qkv16_bw_rows_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _i64, _f32, _vp, _i64, _vp, _i64, _vp, _i64,
                                               _vp, _i64, _vp, _vp, _i64, _vp, _vp]
        L.isplib_qkv16_bw_cols_hip.restype = ctypes.c_int
        L.isplib_qkv16_bw_cols_hip.argtypes = [ctypes.c_int] + L.isplib_mha_bw_cols_hip.argtypes
        # the isplib_qkv16_* argument lists (the columns entry with csr2csc after cole), then threshold, keep_scale, seed
        L.isplib_qkv_half_drop_auto.restype = ctypes.c_int
        L.isplib_qkv_half_drop_auto.argtypes = [_i64, _i64]
        L.isplib_qkv_half_drop_csr_hip.restype = ctypes.c_int
        L.isplib_qkv_half_drop_csr_hip.argtypes = L.isplib_qkv16_csr_hip.argtypes + _drop
        L.isplib_qkv_half_drop_bw_rows_hip.restype = ctypes.c_int
        L.isplib_qkv_half_drop_bw_rows_hip.argtypes = L.isplib_qkv16_bw_rows_hip.argtypes + _drop
        L.isplib_qkv_half_drop_bw_cols_hip.restype = ctypes.c_int
        L.isplib_qkv_half_drop_bw_cols_hip.argtypes = (L.isplib_qkv16_bw_cols_hip.argtypes[:8] + [_vp] + L.isplib_qkv16_bw_cols_hip.argtypes[8:] +
                                                       _drop)
        L.isplib_gatv2_16_domain.restype = ctypes.c_int
        L.isplib_gatv2_16_domain.argtypes = [_i64, _i64, _i64, _i64]
        L.isplib_gatv2_16_auto.restype = ctypes.c_int
        L.isplib_gatv2_16_auto.argtypes = [_i64, _i64]
        L.isplib_gatv2_16_bw_rows_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_gatv2_16_bw_rows_workspace_bytes.argtypes = [_i64, _i64]
        L.isplib_gatv2_16_csr_hip.restype = ctypes.c_int
        L.isplib_gatv2_16_csr_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _f32, _vp,
                                              _i64, _vp, _vp]
        L.isplib_gatv2_16_bw_rows_hip.restype = ctypes.c_int
        L.isplib_gatv2_16_bw_rows_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _f32,
                                                  _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, ctypes.c_size_t, _vp]
        L.isplib_gatv2_16_bw_cols_hip.restype = ctypes.c_int
        L.isplib_gatv2_16_bw_cols_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _f32,
                                                  _vp, _i64, _vp, _vp, _vp, _i64, _vp]
        L.isplib_gat16_domain.restype = ctypes.c_int
        L.isplib_gat16_domain.argtypes = [_i64, _i64, _i64, _i64]
        L.isplib_gat16_auto.restype = ctypes.c_int
        L.isplib_gat16_auto.argtypes = [_i64, _i64]
        L.isplib_gat16_csr_hip.restype = ctypes.c_int
        L.isplib_gat16_csr_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp]
        L.isplib_gat16_bw_rows_hip.restype = ctypes.c_int
        L.isplib_gat16_bw_rows_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp,
                                               _vp, _vp, _vp]
        L.isplib_gat16_bw_cols_hip.restype = ctypes.c_int
        L.isplib_gat16_bw_cols_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp,
                                               _vp, _vp, _i64, _vp, _vp]
        L.isplib_attention16_domain.restype = ctypes.c_int
        L.isplib_attention16_domain.argtypes = [_i64, _i64, _i64]
        L.isplib_attention16_auto.restype = ctypes.c_int
        L.isplib_attention16_auto.argtypes = [_i64, _i64]
        L.isplib_attention16_csr_hip.restype = ctypes.c_int
        L.isplib_attention16_csr_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp, _vp]
        L.isplib_attention16_bw_rows_hip.restype = ctypes.c_int
        L.isplib_attention16_bw_rows_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp,
                                                     _vp, _i64, _vp, _vp]
        L.isplib_attention16_bw_cols_hip.restype = ctypes.c_int
        L.isplib_attention16_bw_cols_hip.argtypes = [ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _f32, _vp, _i64, _vp,
                                                     _vp, _vp, _i64, _vp]
        _sigs_set = True
    return L


_exp = None


def exp_lib() -> ctypes.CDLL:
    """libisplib_hip_exp.so (include/isplib_hip_experimental.h): the sweep schedule, the LDS hot-row hybrid and the stream-plan
    SDDMM -- built, bit-exact, measured slower than the defaults, kept for tests and experiments.  Loaded on first use."""
    global _exp
    if _exp is None:
        lib()                                     # the default library first: the experimental one links against it
        path = os.path.join(os.path.dirname(_lib.CABI_PATH), "libisplib_hip_exp.so")
        if not os.path.exists(path):
            raise ImportError(f"isplib_amd: '{os.path.basename(path)}' not found; build it with `make -C isplib_amd/csrc`")
        L = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        L.isplib_hip_tune_experimental.restype = ctypes.c_int
        L.isplib_hip_tune_experimental.argtypes = [ctypes.c_int, ctypes.c_int]
        L.isplib_spmm_hybrid_geometry.restype = ctypes.c_int
        L.isplib_spmm_hybrid_geometry.argtypes = [ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 4
        L.isplib_spmm_hybrid_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_hybrid_workspace_bytes.argtypes = [ctypes.POINTER(HybridPlanStruct)]
        L.fusedMM_csr_hybrid_hip.restype = ctypes.c_int
        L.fusedMM_csr_hybrid_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, ctypes.POINTER(HybridPlanStruct), _vp, _i64, _vp, _i64,
                                             _vp, ctypes.c_size_t, _vp, _vp]
        L.isplib_sddmm_stream_hip.restype = ctypes.c_int
        L.isplib_sddmm_stream_hip.argtypes = [_i64, _i64, _i64, _i64, _vp, _vp, ctypes.POINTER(StreamPlanStruct), _vp, _i64, _vp, _i64,
                                              ctypes.c_int, _vp, _vp]
        L.isplib_spmm_sweep_resident_waves.restype = ctypes.c_int
        L.isplib_spmm_sweep_resident_waves.argtypes = [_i32, _i64, ctypes.c_int]
        L.isplib_spmm_sweep_workspace_bytes.restype = ctypes.c_size_t
        L.isplib_spmm_sweep_workspace_bytes.argtypes = [_i32, ctypes.POINTER(SweepPlanStruct), _i64]
        L.fusedMM_csr_sweep_hip.restype = ctypes.c_int
        L.fusedMM_csr_sweep_hip.argtypes = [_i32, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(SweepPlanStruct),
                                            _vp, _i64, _vp, _i64, _vp, _vp, ctypes.c_size_t, ctypes.POINTER(Epilogue), _vp]
        _exp = L
    return _exp


def last_error() -> str:
    return lib().isplib_hip_last_error().decode()


class IsplibError(RuntimeError):
    """A non-zero status of the C ABI (include/isplib_hip.h: ISPLIB_*), with the library's message."""

    def __init__(self, status: int, what: str, message: str):
        super().__init__(f"{what} failed with status {status}: {message}")
        self.status = int(status)


def _check(status: int, what: str) -> None:
    if status != 0:
        raise IsplibError(status, what, last_error())


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _dev(t: torch.Tensor, name: str, dtype) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"isplib_amd: `{name}` must be a GPU tensor -- there is no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"isplib_amd: `{name}` must be {dtype}, got {t.dtype}")
    return t.contiguous()


def fusedMM_csr_hip(imessage: int, rowptr: torch.Tensor, col: torch.Tensor, val: Optional[torch.Tensor],
                    y: torch.Tensor, z: torch.Tensor, z_arg: Optional[torch.Tensor] = None, *, beta: float = 0.0,
                    check: bool = True) -> int:
    """Raw boundary call with the reference's argument pattern (csrc/fusedmm.cpp:198):
    pntrb = rowptr, pntre = rowptr + 1, ldy/ldz = row strides of y/z."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    if val is not None:
        val = _dev(val, "val", torch.float32)
    assert y.is_cuda and z.is_cuda and y.dtype == torch.float32 and z.dtype == torch.float32
    assert y.dim() == 2 and z.dim() == 2 and y.stride(1) == 1 and z.stride(1) == 1
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    assert z.size(0) == m and z.size(1) == k
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_hip(int(imessage), m, n, k, 1.0, col.numel(), m, n, _ptr(val), _ptr(col),
                                   ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), None, k, _ptr(y),
                                   y.stride(0) if n > 1 else max(k, y.stride(0)), beta, _ptr(z),
                                   z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(z_arg), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_hip")
    return st


def community_order(rowptr, col, rounds: int = 8, seed: int = 0):
    """(order int32 [m], labels int32 [m], rounds run) by the library's label propagation (isplib_community_order_hip)."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    m, nnz = rowptr.numel() - 1, col.numel()
    order = torch.empty(m, dtype=torch.int32, device=col.device)
    labels = torch.empty(m, dtype=torch.int32, device=col.device)
    ran = ctypes.c_int(0)
    with torch.cuda.device(col.device):
        ws = torch.empty(lib().isplib_community_order_workspace_bytes(m, nnz), dtype=torch.uint8, device=col.device)
        _check(lib().isplib_community_order_hip(m, nnz, _ptr(rowptr), _ptr(col), int(rounds), int(seed), _ptr(order), _ptr(labels),
                                                ctypes.byref(ran), _ptr(ws), ws.numel(), _stream(col.device)), "isplib_community_order_hip")
    return order, labels, ran.value


def order_locality(rowptr, col, order, window: int = 1024) -> float:
    """Share of the stored entries whose column lies within `window` positions of its row in `order` (None: index order)."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    m = rowptr.numel() - 1
    share = ctypes.c_double(0.0)
    with torch.cuda.device(col.device):
        ws = torch.empty(4 * m + 1024, dtype=torch.uint8, device=col.device)
        _check(lib().isplib_order_locality_hip(m, col.numel(), _ptr(rowptr), _ptr(col), _ptr(order), int(window), ctypes.byref(share),
                                               _ptr(ws), ws.numel(), _stream(col.device)), "isplib_order_locality_hip")
    return share.value


def fusedMM_csr_ordered_hip(imessage: int, rowptr, col, val, order, y, z, z_arg=None, check: bool = True) -> int:
    """The plain kernel with the rows taken in `order` (int32 [m], position -> row; None = fusedMM_csr_hip)."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    if order is not None:
        order = _dev(order, "order", torch.int32)
        assert order.numel() == rowptr.numel() - 1
    assert y.is_cuda and z.is_cuda and y.dtype == torch.float32 and z.dtype == torch.float32 and y.stride(1) == 1 and z.stride(1) == 1
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_ordered_hip(int(imessage), m, n, k, col.numel(), _ptr(val), _ptr(col), ctypes.c_void_p(rp),
                                           ctypes.c_void_p(rp + 8), _ptr(order), _ptr(y), y.stride(0) if n > 1 else max(k, y.stride(0)),
                                           _ptr(z), z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(z_arg), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_ordered_hip")
    return st


def plain_panels(n: int, ldy: int) -> bool:
    """Whether fusedMM_csr_hip in index order runs K > 128 in 128-column panels for an [n, ldy] operand (isplib_plain_panels)."""
    return bool(lib().isplib_plain_panels(int(n), int(ldy)))


def spmm_ordered(rowptr, col, val, order, y, reduce: str = "sum"):
    """Allocate the outputs and call the ordered plain kernel; returns (out, arg|None)."""
    y = y.contiguous()
    m, k = rowptr.numel() - 1, y.size(1)
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    arg = torch.empty((m, k), dtype=torch.int64, device=y.device) if reduce in ("max", "min") else None
    fusedMM_csr_ordered_hip(MESSAGE[reduce], rowptr, col, val, order, y, out, arg)
    return out, arg


def reads_x(imessage: int) -> bool:
    """Whether the generic pipeline reads the left operand x for this word (fusedmm_general.hip: needs_x)."""
    vop, rop = imessage & 0xF, imessage & 0xF0
    return vop != VOP["copy_rhs"] or rop in (ROP["dot"], ROP["add_lhs"], ROP["norml"])


def check_fusedmm_operands(imessage: int, m: int, x, y, plan=None, x_read: Optional[bool] = None) -> None:
    """Shapes of the FusedMM operands, checked before any library call: the kernels read x[i, :k] for every row i < m
    and y[j, :k] for every stored column id j, and the C entries cannot know how many rows either tensor has.  y is
    2-D; x, where the word reads it (`x_read`: the kernel's own rule, default reads_x), is [m, k]; a plan must have been
    built for m rows over y's rows."""
    if y.dim() != 2:
        raise ValueError(f"isplib_amd: `y` must be 2-D [n, k], got shape {tuple(y.shape)}")
    k = y.size(1)
    if x_read is None:
        x_read = reads_x(int(imessage))
    if x is not None and x_read and (x.dim() != 2 or tuple(x.shape) != (m, k)):
        raise ValueError(f"isplib_amd: `x` must be [m, k] = [{m}, {k}] for this message word, got shape {tuple(x.shape)}")
    if plan is not None:
        cols, rows = getattr(plan, "cols", None), getattr(plan, "rows", None)
        if cols is not None and int(cols) != y.size(0):
            raise ValueError(f"isplib_amd: the plan was built for {cols} columns, `y` has {y.size(0)} rows")
        if rows is not None and int(rows) != m:
            raise ValueError(f"isplib_amd: the plan was built for {rows} rows, the graph has {m}")
        seg_off = getattr(plan, "seg_off", None)
        if seg_off is not None and seg_off.numel() != plan.slices * m + 1:
            raise ValueError(f"isplib_amd: the task plan was built for {(seg_off.numel() - 1) // max(plan.slices, 1)} rows, the graph has {m}")


def _fusedmm_out(out, m: int, k: int, y):
    if out is None:
        return torch.empty((m, k), dtype=torch.float32, device=y.device)
    if out.dtype != torch.float32 or out.device != y.device or tuple(out.shape) != (m, k) or not out.is_contiguous():
        raise ValueError(f"isplib_amd: `out` must be a contiguous float32 [{m}, {k}] tensor on {y.device}")
    return out


def fusedmm(imessage: int, rowptr, col, val, x, y, sop_udef="none", sop_param: float = 0.0, check: bool = True, plan=None, out=None):
    """The generic FusedMM pipeline (fusedMM_csr_udef_hip): z[i,:] = AOP_j VSC(SOP(ROP(VOP(x_i, y_j))), .) over the
    stored entries of row i.  `imessage` is a word built from VOP/ROP/SOP/VSC/AOP (or PATTERNS[name][0]);
    `sop_udef` names the built-in function a SOP_UDEF stage stands for.  With `plan` (isplib_amd.plan.TaskPlan) the
    task form runs (fusedMM_csr_udef_tasks_hip).  `out`: a contiguous fp32 [m, k] tensor to write z into (every element is
    written; the tests hand in a NaN-filled one).  Returns (status, z, z_arg | None)."""
    check_fusedmm_operands(imessage, rowptr.numel() - 1, x, y, plan)
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    if val is not None:
        val = _dev(val, "val", torch.float32)
    y = _dev(y, "y", torch.float32)
    if x is not None:
        x = _dev(x, "x", torch.float32)
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    z = _fusedmm_out(out, m, k, y)
    arg = torch.empty((m, k), dtype=torch.int64, device=y.device) if ((imessage >> 16) & 0xF) in (2, 3) else None
    rp = rowptr.data_ptr()
    kind = SOP_UDEF[sop_udef] if isinstance(sop_udef, str) else int(sop_udef)
    with torch.cuda.device(y.device):
        if plan is not None:
            reduce = {1: "sum", 2: "max", 3: "min"}.get((imessage >> 16) & 0xF, "sum")
            work = plan.workspace(reduce, k)
            lane = (ctypes.c_int64 * 9)(*plan.lane_off)
            st = lib().fusedMM_csr_udef_tasks_hip(int(imessage), m, n, k, col.numel(), _ptr(val), _ptr(col), _plan_col32(plan, col),
                                                  ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(x), k, plan.n_tasks,
                                                  _ptr(plan.task_row), _ptr(plan.task_b), _ptr(plan.task_len), _ptr(plan.seg_off),
                                                  plan.slices, lane, _ptr(y), k, _ptr(z), k, _ptr(arg), kind, float(sop_param),
                                                  _ptr(work), work.numel(), _stream(y.device))
        else:
            st = lib().fusedMM_csr_udef_hip(int(imessage), m, n, k, 1.0, col.numel(), m, n, _ptr(val), _ptr(col),
                                            ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(x), k, _ptr(y), k, 0.0,
                                            _ptr(z), k, _ptr(arg), kind, float(sop_param), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_udef_tasks_hip" if plan is not None else "fusedMM_csr_udef_hip")
    return st, z, arg


def suggest_fusedmm_stream(imessage: int, m: int, n: int, nnz: int, k: int):
    """(streams, slices, chunk) when the word should run on the stream front end (isplib_suggest_fusedmm_stream), else None."""
    v = [ctypes.c_int(0) for _ in range(3)]
    if not lib().isplib_suggest_fusedmm_stream(int(imessage), int(m), int(n), int(nnz), int(k), *[ctypes.byref(x) for x in v]):
        return None
    return tuple(int(x.value) for x in v)


def fusedmm_stream_geometry(streams: int = 2):
    rpw, res = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().isplib_fusedmm_stream_geometry(int(streams), ctypes.byref(rpw), ctypes.byref(res)), "isplib_fusedmm_stream_geometry")
    return int(rpw.value), int(res.value)


def fusedmm_stream(imessage: int, rowptr, nnz: int, plan, x, y, sop_udef="none", sop_param: float = 0.0, check: bool = True, out=None):
    """The two SDDMM-fused words on the stream front end (fusedMM_csr_udef_stream_hip); `plan`: a NativeStreamPlan built with
    fusedmm=True; `out` as for fusedmm().  Returns (status, z)."""
    if x is None:
        raise ValueError("isplib_amd: the stream FusedMM words read `x`")
    check_fusedmm_operands(imessage, rowptr.numel() - 1, x, y, plan, x_read=True)   # the kernel loads x[i] of every owned row
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    x, y = _dev(x, "x", torch.float32), _dev(y, "y", torch.float32)
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    z = _fusedmm_out(out, m, k, y)
    kind = SOP_UDEF[sop_udef] if isinstance(sop_udef, str) else int(sop_udef)
    work = plan.workspace()
    rp = rowptr.data_ptr()
    ps = plan.struct()
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_udef_stream_hip(int(imessage), m, n, k, int(nnz), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), ctypes.byref(ps),
                                               _ptr(x), k, _ptr(y), k, _ptr(z), k, kind, float(sop_param), _ptr(work), work.numel(),
                                               _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_udef_stream_hip")
    return st, z


def spmm(rowptr, col, val, y, reduce: str = "sum"):
    """Allocate outputs and call the boundary; returns (out, arg|None)."""
    m, k = rowptr.numel() - 1, y.size(1)
    y = y.contiguous()
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    arg = torch.empty((m, k), dtype=torch.int64, device=y.device) if reduce in ("max", "min") else None
    fusedMM_csr_hip(MESSAGE[reduce], rowptr, col, val, y, out, arg)
    return out, arg


def perform_dummy_spmm(flag: int = 0) -> None:
    lib().performDummySpMM_hip(int(flag), _stream(None))


def spmm_minmax_bw(col, val, mat, arg, grad_out, need_mat=True, need_val=True, deterministic=False):
    """(grad_val, grad_mat) of SpMM-max/min; deterministic=True: the atomic-free form (isplib_spmm_minmax_bw_det_hip)."""
    col = _dev(col, "col", torch.int64)
    mat = _dev(mat, "mat", torch.float32)
    arg = _dev(arg, "arg", torch.int64)
    grad_out = _dev(grad_out, "grad_out", torch.float32)
    if val is not None:
        val = _dev(val, "val", torch.float32)
    m, k = arg.shape
    n, nnz = mat.size(0), col.numel()
    grad_mat = torch.empty_like(mat) if need_mat else None
    grad_val = torch.empty(nnz, dtype=torch.float32, device=mat.device) if need_val else None
    with torch.cuda.device(mat.device):
        if deterministic:
            ws = lib().isplib_spmm_minmax_bw_workspace_bytes(m, n, k)
            work = torch.empty(max(ws, 256), dtype=torch.uint8, device=mat.device)
            st = lib().isplib_spmm_minmax_bw_det_hip(m, n, k, nnz, _ptr(col), _ptr(val), _ptr(mat), _ptr(arg), _ptr(grad_out),
                                                     _ptr(grad_mat), _ptr(grad_val), _ptr(work), work.numel(), _stream(mat.device))
            _check(st, "isplib_spmm_minmax_bw_det_hip")
            return grad_val, grad_mat
        st = lib().isplib_spmm_minmax_bw_hip(m, n, k, nnz, _ptr(col), _ptr(val), _ptr(mat), _ptr(arg), _ptr(grad_out),
                                             _ptr(grad_mat), _ptr(grad_val), _stream(mat.device))
    _check(st, "isplib_spmm_minmax_bw_hip")
    return grad_val, grad_mat


def row_scale(x: torch.Tensor, scale: torch.Tensor, pitch: Optional[int] = None) -> torch.Tensor:
    """y = scale[:, None] * x through isplib_row_scale_hip; `pitch` > k: a [n, k] view of an [n, pitch] buffer (padding 0)."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    scale = _dev(scale, "scale", torch.float32)
    n, k = x.shape
    ld = k if pitch is None else int(pitch)
    buf = torch.empty((n, ld), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().isplib_row_scale_hip(n, k, _ptr(x), x.stride(0) if n > 1 else max(k, x.stride(0)), _ptr(scale), _ptr(buf), ld,
                                          _stream(x.device)), "isplib_row_scale_hip")
    return buf[:, :k]


def masked_scale_colsum(dz: torch.Tensor, out: Optional[torch.Tensor], scale: Optional[torch.Tensor], want_gy: bool = True,
                        want_bias: bool = True, pitch: Optional[int] = None):
    """(gy, grad_bias) of isplib_masked_scale_colsum_hip: g = dz * (out > 0), gy = g * scale[:, None], grad_bias = g.sum(0)."""
    dz = _dev(dz, "dz", torch.float32)
    out = None if out is None else _dev(out, "out", torch.float32)
    scale = None if scale is None else _dev(scale, "scale", torch.float32)
    n, k = dz.shape
    ld = k if pitch is None else int(pitch)
    gy = torch.empty((n, ld), dtype=torch.float32, device=dz.device) if want_gy else None
    gb = torch.empty(k, dtype=torch.float32, device=dz.device) if want_bias else None
    with torch.cuda.device(dz.device):
        ws = lib().isplib_masked_scale_colsum_workspace_bytes(n, k)
        work = torch.empty(max(ws, 256), dtype=torch.uint8, device=dz.device)
        _check(lib().isplib_masked_scale_colsum_hip(n, k, _ptr(dz), k, _ptr(out), k, _ptr(scale), _ptr(gy), ld, _ptr(gb), _ptr(work),
                                                    work.numel(), _stream(dz.device)), "isplib_masked_scale_colsum_hip")
    return (None if gy is None else gy[:, :k]), gb


def set_empty_row(mode: str = "zero") -> None:
    """What an EMPTY row of max / min holds from now on, every schedule: "zero" (default) or "init" (-FLT_MAX / +FLT_MAX, the
    reference launcher's pre-fill left untouched; include/isplib_hip.h: isplib_hip_set_empty_row).  Positions stay nnz."""
    if mode not in ("zero", "init"):
        raise ValueError("empty-row mode: 'zero' or 'init'")
    _check(lib().isplib_hip_set_empty_row(1 if mode == "init" else 0), "isplib_hip_set_empty_row")


def get_empty_row() -> str:
    return "init" if lib().isplib_hip_get_empty_row() else "zero"


def scatter_rows_det(dest: torch.Tensor, gval: torch.Tensor, lo: int, n: int) -> torch.Tensor:
    """grad[d - lo, c] = sum over i (ascending) of gval[i, c] where dest[i, c] == d, for d in [lo, lo + n)
    (isplib_scatter_rows_det_hip: the local half of the row-partitioned max / min backward)."""
    dest = _dev(dest, "dest", torch.int32)
    gval = _dev(gval, "gval", torch.float32)
    assert dest.shape == gval.shape and dest.dim() == 2
    m, k = dest.shape
    out = torch.empty((n, k), dtype=torch.float32, device=gval.device)
    with torch.cuda.device(gval.device):
        ws = lib().isplib_spmm_minmax_bw_workspace_bytes(m, n, k)
        if ws == 0 and m * k > 0 and n > 0:
            # beyond the sort's 32-bit keys (n * k or m * k >= 2^32): torch's atomic scatter on the same pairs -- correct, not
            # bitwise reproducible (the one place of the partitioned backward that is not; no shape of BASELINE.json gets here)
            d = dest.to(torch.int64) - int(lo)
            mine = (dest >= 0) & (d >= 0) & (d < n)
            rows, cols = mine.nonzero(as_tuple=True)
            out.zero_()
            out.index_put_((d[rows, cols], cols), gval[rows, cols], accumulate=True)
            return out
        work = torch.empty(max(ws, 256), dtype=torch.uint8, device=gval.device)
        _check(lib().isplib_scatter_rows_det_hip(m, n, k, int(lo), _ptr(dest), _ptr(gval), _ptr(out), _ptr(work), work.numel(),
                                                 _stream(gval.device)), "isplib_scatter_rows_det_hip")
    return out


def _operand(t, name: str, dtype, dims: int) -> None:
    """Shape, dtype and layout of one operand of the owner-exchange entries; they take the tensors as they are (fixed buffers
    of a captured graph), so nothing is converted or copied on the caller's behalf."""
    if not isinstance(t, torch.Tensor) or t.dim() != dims:
        raise ValueError(f"isplib_amd: `{name}` must be a {dims}-D tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"isplib_amd: `{name}` must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"isplib_amd: `{name}` must be contiguous")


def _same_gpu(tensors) -> None:
    first = None
    for name, t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"isplib_amd: `{name}` must be a GPU tensor -- there is no CPU path")
        if first is None:
            first = t.device
        elif t.device != first:
            raise ValueError(f"isplib_amd: `{name}` is on {t.device}, the other operands on {first}")


def minmax_bw_bucket(arg, edge0: int, col, val, grad_out, cuts, out=None, workspace=None):
    """The sender's half of the owner-bucketed max / min backward (isplib_minmax_bw_bucket_hip): this rank's [m, k] winners
    `arg` (CSR positions; position - edge0 indexes `col` / `val`, anything outside [0, nnz) is no winner) and gradients,
    split by the owner of the destination row `col[.]` at the row boundaries `cuts` (world + 1, ascending).  Returns
    (keys, vals, seg_off): owner p's pairs are [seg_off[p], seg_off[p + 1]) of keys (uint32 as int32 storage:
    (row - cuts[p]) * k + feature) and vals, in ascending (row, feature) of this rank; seg_off is a device int64 tensor.
    `out` = (keys, vals, seg_off) and `workspace` let a caller reuse fixed buffers (graph capture)."""
    _operand(arg, "arg", torch.int64, 2)
    _operand(grad_out, "grad_out", torch.float32, 2)
    if arg.shape != grad_out.shape:
        raise ValueError(f"isplib_amd: `arg` {tuple(arg.shape)} and `grad_out` {tuple(grad_out.shape)} must have one shape [m, k]")
    _operand(col, "col", torch.int64, 1)
    if val is not None:
        _operand(val, "val", torch.float32, 1)
        if val.numel() != col.numel():
            raise ValueError(f"isplib_amd: `val` has {val.numel()} entries, `col` {col.numel()}")
    cuts = [int(c) for c in cuts]
    world = len(cuts) - 1
    if not 1 <= world <= OWNER_WORLD_MAX:
        raise ValueError(f"isplib_amd: `cuts` must hold world + 1 boundaries for 1..{OWNER_WORLD_MAX} owners, got {len(cuts)}")
    if any(cuts[p + 1] < cuts[p] for p in range(world)):
        raise ValueError("isplib_amd: `cuts` must ascend")
    m, k = arg.shape
    if not owner_exchange_serves(m, k, world, cuts):
        raise ValueError(f"isplib_amd: {m} x {k} winners over these cuts are outside the owner exchange's 32-bit keys (owner_exchange_serves)")
    total = m * k
    if out is not None:
        keys, vals, seg_off = out
        _operand(keys, "keys", torch.int32, 1)
        _operand(vals, "vals", torch.float32, 1)
        _operand(seg_off, "seg_off", torch.int64, 1)
        if keys.numel() < total or vals.numel() < total or seg_off.numel() != world + 1:
            raise ValueError(f"isplib_amd: `out` must hold {total} keys, {total} values and {world + 1} offsets")
    _same_gpu((("arg", arg), ("grad_out", grad_out), ("col", col), ("val", val)) +
              ((("keys", out[0]), ("vals", out[1]), ("seg_off", out[2])) if out is not None else ()))
    dev = grad_out.device
    if out is None:
        keys = torch.empty(total, dtype=torch.int32, device=dev)
        vals = torch.empty(total, dtype=torch.float32, device=dev)
        seg_off = torch.empty(world + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ws = lib().isplib_minmax_bw_bucket_workspace_bytes(m, k, world)
        if workspace is None:
            workspace = torch.empty(max(ws, 256), dtype=torch.uint8, device=dev)
        _check(lib().isplib_minmax_bw_bucket_hip(m, k, col.numel(), int(edge0), _ptr(arg), _ptr(col), _ptr(val), _ptr(grad_out), world,
                                                 (_i64 * (world + 1))(*cuts), _ptr(keys), _ptr(vals), _ptr(seg_off), _ptr(workspace),
                                                 workspace.numel(), _stream(dev)), "isplib_minmax_bw_bucket_hip")
    return keys, vals, seg_off


def scatter_keys_det(keys, vals, n: int, k: int, out=None, workspace=None):
    """The receiver's half (isplib_scatter_keys_det_hip): grad[key // k, key % k] = sum of vals over equal keys in the order
    given; keys >= n * k are ignored.  keys: int32 storage of uint32 keys, as `minmax_bw_bucket` returns them."""
    _operand(keys, "keys", torch.int32, 1)
    _operand(vals, "vals", torch.float32, 1)
    if keys.numel() != vals.numel():
        raise ValueError(f"isplib_amd: {keys.numel()} keys for {vals.numel()} values")
    n, k, total = int(n), int(k), keys.numel()
    if not scatter_keys_serves(total, n, k):
        raise ValueError(f"isplib_amd: {total} pairs into {n} x {k} are outside the sort's 32-bit keys (scatter_keys_serves)")
    if out is not None:
        _operand(out, "out", torch.float32, 2)
        if tuple(out.shape) != (n, k):
            raise ValueError(f"isplib_amd: `out` must be [{n}, {k}], got {tuple(out.shape)}")
    _same_gpu((("keys", keys), ("vals", vals), ("out", out)))
    dev = vals.device
    if out is None:
        out = torch.empty((n, k), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = lib().isplib_scatter_keys_workspace_bytes(total, n, k)
        if workspace is None:
            workspace = torch.empty(max(ws, 256), dtype=torch.uint8, device=dev)
        _check(lib().isplib_scatter_keys_det_hip(total, n, k, _ptr(keys), _ptr(vals), _ptr(out), _ptr(workspace), workspace.numel(),
                                                 _stream(dev)), "isplib_scatter_keys_det_hip")
    return out


def _sddmm_operands(rowptr, col, y, g, out, check: bool, min_rows: int = 0, what: str = "the plan"):
    """The operand checks of sddmm, sddmm_tasks and GraphHandle.sddmm, made BEFORE the call -- the entries cannot know how many rows
    either dense operand has, so a mis-shaped one is an out-of-bounds device read: `y` [n, k] and `g` [m, k] (m = rowptr.numel() - 1)
    float32 with unit inner stride (row-strided views keep their pitch), rowptr / col int64, everything on one GPU, n at least
    `min_rows` (the column count `what` was built for), `out` (allocated when None) a contiguous float32 tensor of at least nnz
    entries, and -- `check` -- every column id inside [0, n).  Returns (rowptr, col, out, ldy, ldg)."""
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, k]")
    if y.dtype != torch.float32:
        raise TypeError(f"isplib_amd: `y` must be float32, got {y.dtype} (bfloat16 / float16: sddmm_rows16)")
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1 or not isinstance(col, torch.Tensor) or col.dim() != 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) and `col` must be 1-D tensors")
    if rowptr.dtype != torch.int64 or col.dtype != torch.int64:
        raise TypeError(f"isplib_amd: `rowptr` and `col` must be int64, got {rowptr.dtype} and {col.dtype}")
    m, nnz = rowptr.numel() - 1, col.numel()
    n, k = y.size(0), y.size(1)
    if not isinstance(g, torch.Tensor) or g.dim() != 2 or tuple(g.shape) != (m, k):
        raise ValueError(f"isplib_amd: `g` must be a 2-D tensor [{m}, {k}] (one row per row of the sparse operand, y's width), got "
                         f"{tuple(g.shape) if isinstance(g, torch.Tensor) else type(g).__name__}")
    if g.dtype != torch.float32:
        raise TypeError(f"isplib_amd: `g` must be float32, got {g.dtype}")
    if k > 0 and ((n > 0 and y.stride(1) != 1) or (m > 0 and g.stride(1) != 1)):
        raise ValueError("isplib_amd: `y` and `g` must have unit inner stride")
    ldy = y.stride(0) if n > 1 else max(k, y.stride(0))
    ldg = g.stride(0) if m > 1 else max(k, g.stride(0))
    if ldy < k or ldg < k:
        raise ValueError(f"isplib_amd: the rows of `y` (pitch {ldy}) and `g` (pitch {ldg}) must not overlap: k = {k}")
    if n < min_rows:
        raise ValueError(f"isplib_amd: {what} was built for {min_rows} columns, `y` has {n} rows")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 1 or out.numel() < nnz or
                            not out.is_contiguous()):
        raise ValueError(f"isplib_amd: `out` must be a contiguous float32 tensor of at least {nnz} entries")
    if check and nnz > 0 and (int(col.min()) < 0 or int(col.max()) >= n):
        raise ValueError(f"isplib_amd: column ids must lie in [0, {n}): `y` must hold a row for every column of the sparse operand")
    _same_gpu((("y", y), ("g", g), ("rowptr", rowptr), ("col", col), ("out", out)))
    rowptr, col = rowptr.contiguous(), col.contiguous()
    if out is None:
        out = torch.empty(nnz, dtype=torch.float32, device=y.device)
    return rowptr, col, out, ldy, ldg


def sddmm(rowptr, col, y, g, mean: bool = False, *, out=None, check: bool = True):
    """dA of SpMM-sum / SpMM-mean on the row kernel (isplib_sddmm_csr_hip): returns `out`, float32 in CSR order (allocated with
    col.numel() entries when not given; a given one of at least that many is written in place), out[e] = <y[col[e], :], g[i, :]>
    (`mean`: / max(deg_i, 1)) for the edges e of row i.  Row-strided views of `y` and `g` keep their pitch.  The operands are
    checked before the call (_sddmm_operands; `check`: the column ids too -- two reductions over `col` and a synchronisation, so a
    timed loop over a graph already checked passes check=False)."""
    rowptr, col, out, ldy, ldg = _sddmm_operands(rowptr, col, y, g, out, check)
    m, k = rowptr.numel() - 1, y.size(1)
    if col.numel() == 0:                                        # no edge, nothing to write (and an empty tensor has no address to hand over)
        return out
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_sddmm_csr_hip(m, k, _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(y), ldy,
                                        _ptr(g), ldg, int(bool(mean)), _ptr(out), _stream(y.device))
    _check(st, "isplib_sddmm_csr_hip")
    return out


def csr_row_ids(rowptr, nnz: int):
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    row = torch.empty(nnz, dtype=torch.int64, device=rowptr.device)
    with torch.cuda.device(rowptr.device):
        st = lib().isplib_csr_row_ids_hip(rowptr.numel() - 1, nnz, _ptr(rowptr), _ptr(row), _stream(rowptr.device))
    _check(st, "isplib_csr_row_ids_hip")
    return row


def csr2csc(rowptr, col, val, ncols: int, *, mean_scale: bool = False, want_perm: bool = True,
            want_row: bool = True, want_val: bool = True):
    """Device CSR -> CSC operands: (colptr, csr2csc|None, row_t|None, val_t|None)."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    if val is not None:
        val = _dev(val, "val", torch.float32)
    dev = col.device
    m, nnz = rowptr.numel() - 1, col.numel()
    colptr = torch.empty(ncols + 1, dtype=torch.int64, device=dev)
    perm = torch.empty(nnz, dtype=torch.int64, device=dev) if want_perm else None
    row_t = torch.empty(nnz, dtype=torch.int64, device=dev) if want_row else None
    val_t = torch.empty(nnz, dtype=torch.float32, device=dev) if want_val else None
    with torch.cuda.device(dev):
        ws = lib().isplib_csr2csc_workspace_bytes(m, ncols, nnz)
        if ws == 0:
            raise RuntimeError("isplib_csr2csc_workspace_bytes failed: " + last_error())
        work = torch.empty(ws, dtype=torch.uint8, device=dev)
        st = lib().isplib_csr2csc_hip(m, ncols, nnz, _ptr(rowptr), _ptr(col), _ptr(val), int(bool(mean_scale)),
                                      _ptr(colptr), _ptr(perm), _ptr(row_t), _ptr(val_t), _ptr(work), ws, _stream(dev))
    _check(st, "isplib_csr2csc_hip")
    return colptr, perm, row_t, val_t


def spmm_slices(rowptr, col, ncols: int, slices: int = 8, check_sorted: bool = True):
    """Per-graph slice table for fusedMM_csr_sliced_hip: (sliceptr[m*(slices+1)], rows_sorted).
    ``rows_sorted`` is False when some row's columns are not ascending (table unusable);
    reading it synchronises once -- this runs once per graph, never per SpMM."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    dev = col.device
    m = rowptr.numel() - 1
    sliceptr = torch.empty(m * (slices + 1), dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if check_sorted else None
    rp = rowptr.data_ptr()
    with torch.cuda.device(dev):
        st = lib().isplib_spmm_slices_build_hip(m, ncols, col.numel(), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                                _ptr(col), slices, _ptr(sliceptr), _ptr(flag), _stream(dev))
    _check(st, "isplib_spmm_slices_build_hip")
    return sliceptr, (True if flag is None else int(flag.item()) == 0)


def sliced_workspace(reduce: str, m: int, k: int, slices: int, device) -> torch.Tensor:
    nbytes = lib().isplib_spmm_sliced_workspace_bytes(MESSAGE[reduce], m, k, slices)
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def fusedMM_csr_sliced_hip(imessage: int, rowptr, col, val, sliceptr, slices: int, y, z, z_arg, workspace,
                           check: bool = True) -> int:
    """Raw boundary call of the column-sliced SpMM (operands as fusedMM_csr_hip + slice table + workspace)."""
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_sliced_hip(int(imessage), m, n, k, col.numel(), _ptr(val), _ptr(col),
                                          ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(sliceptr), slices,
                                          _ptr(y), y.stride(0) if n > 1 else max(k, y.stride(0)), _ptr(z),
                                          z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(z_arg),
                                          _ptr(workspace), workspace.numel(), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_sliced_hip")
    return st


def spmm_sliced(rowptr, col, val, sliceptr, slices: int, y, reduce: str = "sum", workspace=None):
    """Allocate outputs (+ workspace) and call the sliced boundary; returns (out, arg|None)."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    if val is not None:
        val = _dev(val, "val", torch.float32)
    y = y.contiguous()
    m, k = rowptr.numel() - 1, y.size(1)
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    arg = torch.empty((m, k), dtype=torch.int64, device=y.device) if reduce in ("max", "min") else None
    if workspace is None:
        workspace = sliced_workspace(reduce, m, k, slices, y.device)
    fusedMM_csr_sliced_hip(MESSAGE[reduce], rowptr, col, val, sliceptr, slices, y, out, arg, workspace)
    return out, arg


def fusedMM_csr_sliced_phase_hip(imessage: int, rowptr, col, val, sliceptr, slices: int, slice_first: int,
                                 slice_count: int, combine: bool, y_ptr: int, n: int, k: int, ldy: int, z, z_arg,
                                 workspace, check: bool = True) -> int:
    """One phase of the column-sliced SpMM (include/isplib_hip.h).  ``y_ptr`` is a raw device address so
    that a phase can read its columns through a base shifted onto a shard of the dense operand."""
    m = rowptr.numel() - 1
    rp = rowptr.data_ptr()
    with torch.cuda.device(z.device):
        st = lib().fusedMM_csr_sliced_phase_hip(
            int(imessage), m, n, k, col.numel(), _ptr(val), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
            _ptr(sliceptr), slices, slice_first, slice_count, int(bool(combine)), ctypes.c_void_p(y_ptr), ldy, _ptr(z),
            z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(z_arg), _ptr(workspace), workspace.numel(),
            _stream(z.device))
    if check:
        _check(st, "fusedMM_csr_sliced_phase_hip")
    return st


def pack_indices(col: torch.Tensor) -> torch.Tensor:
    """int32 copy of the column ids (isplib_pack_indices_hip): what the task kernels stream instead of the int64 array."""
    col = _dev(col, "col", torch.int64)
    out = torch.empty(col.numel(), dtype=torch.int32, device=col.device)
    with torch.cuda.device(col.device):
        _check(lib().isplib_pack_indices_hip(col.numel(), _ptr(col), _ptr(out), _stream(col.device)), "isplib_pack_indices_hip")
    return out


def _plan_col32(plan, col):
    """The plan's packed column ids if it has them and they belong to this `col` (same length), else NULL."""
    c32 = getattr(plan, "col32", None)
    return _ptr(c32) if c32 is not None and c32.numel() == col.numel() and c32.device == col.device else None


def fusedMM_csr_tasks_hip(imessage: int, rowptr, col, val, plan, y, z, z_arg, workspace, check: bool = True) -> int:
    """Raw boundary call of the task-list SpMM; ``plan`` is an isplib_amd.plan.TaskPlan."""
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    rp = rowptr.data_ptr()
    lane = (ctypes.c_int64 * 9)(*plan.lane_off)
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_tasks_hip(int(imessage), m, n, k, col.numel(), _ptr(val), _ptr(col), _plan_col32(plan, col), ctypes.c_void_p(rp),
                                         ctypes.c_void_p(rp + 8), plan.n_tasks, _ptr(plan.task_row), _ptr(plan.task_b),
                                         _ptr(plan.task_len), _ptr(plan.seg_off), plan.slices, lane, _ptr(y),
                                         y.stride(0) if n > 1 else max(k, y.stride(0)), _ptr(z),
                                         z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(z_arg), _ptr(workspace),
                                         workspace.numel(), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_tasks_hip")
    return st


def spmm_tasks(rowptr, col, val, plan, y, reduce: str = "sum", workspace=None):
    """Allocate outputs (+ workspace) and call the task-list boundary; returns (out, arg|None)."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    if val is not None:
        val = _dev(val, "val", torch.float32)
    y = y.contiguous()
    m, k = rowptr.numel() - 1, y.size(1)
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    arg = torch.empty((m, k), dtype=torch.int64, device=y.device) if reduce in ("max", "min") else None
    if workspace is None:
        workspace = plan.workspace(reduce, k)
    fusedMM_csr_tasks_hip(MESSAGE[reduce], rowptr, col, val, plan, y, out, arg, workspace)
    return out, arg


def sddmm_stream(rowptr, nnz: int, plan, y, g, mean: bool = False):
    """dA over the stream plan of the SpMM (isplib_sddmm_stream_hip): dval[e] = <y[col[e]], g[row(e)]> (/ max(deg, 1))."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    y, g = y.contiguous(), g.contiguous()
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    assert g.size(0) == m and g.size(1) == k
    dval = torch.empty(int(nnz), dtype=torch.float32, device=y.device)
    rp = rowptr.data_ptr()
    ps = plan.struct()
    with torch.cuda.device(y.device):
        st = exp_lib().isplib_sddmm_stream_hip(m, n, k, int(nnz), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), ctypes.byref(ps), _ptr(y), k,
                                           _ptr(g), k, int(bool(mean)), _ptr(dval), _stream(y.device))
    _check(st, "isplib_sddmm_stream_hip")
    return dval


def sddmm_tasks(rowptr, col, plan, y, g, mean: bool = False, *, out=None, check: bool = True, col32: bool = True):
    """dA over the task plan of the SpMM (isplib_sddmm_csr_tasks_hip); `out`, `check` and the operand checks as for sddmm, and the
    plan must have been built for this graph's rows and at most y's rows as columns.  `col32=False`: the int64 column ids
    instead of the plan's packed 32-bit copy (indx32 = NULL)."""
    m = rowptr.numel() - 1 if isinstance(rowptr, torch.Tensor) else -1
    seg_off = getattr(plan, "seg_off", None)
    if seg_off is not None and seg_off.numel() != plan.slices * m + 1:
        raise ValueError(f"isplib_amd: the task plan was built for {(seg_off.numel() - 1) // max(plan.slices, 1)} rows, the graph has {m}")
    rowptr, col, out, ldy, ldg = _sddmm_operands(rowptr, col, y, g, out, check, int(getattr(plan, "ncols", None) or 0), "the task plan")
    if plan.n_tasks > 0 and plan.task_row.device != y.device:
        raise ValueError(f"isplib_amd: the task plan is on {plan.task_row.device}, the operands on {y.device}")
    n, k = y.size(0), y.size(1)
    if col.numel() == 0:
        return out
    rp = rowptr.data_ptr()
    lane = (ctypes.c_int64 * 9)(*plan.lane_off)
    with torch.cuda.device(y.device):
        st = lib().isplib_sddmm_csr_tasks_hip(m, n, k, _ptr(col), _plan_col32(plan, col) if col32 else None, ctypes.c_void_p(rp),
                                              ctypes.c_void_p(rp + 8), plan.n_tasks, _ptr(plan.task_row), _ptr(plan.task_b),
                                              _ptr(plan.task_len), lane, _ptr(y), ldy, _ptr(g), ldg, int(bool(mean)), _ptr(out),
                                              _stream(y.device))
    _check(st, "isplib_sddmm_csr_tasks_hip")
    return out


def spmm_tasks_epilogue(rowptr, col, val, plan, y, reduce="sum", row_scale=None, self_term=None, bias=None, relu=False):
    """fusedMM_csr_tasks_epilogue_hip: out = act(row_scale * (reduce + self) + bias), sum / mean only."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    y = y.contiguous()
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    work = plan.workspace(reduce, k)
    ep = Epilogue(None if row_scale is None else row_scale.data_ptr(), None if self_term is None else self_term.data_ptr(),
                  k if self_term is None else self_term.stride(0), None if bias is None else bias.data_ptr(), int(bool(relu)))
    rp = rowptr.data_ptr()
    lane = (ctypes.c_int64 * 9)(*plan.lane_off)
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_tasks_epilogue_hip(MESSAGE[reduce], m, n, k, col.numel(), _ptr(val), _ptr(col), _plan_col32(plan, col), ctypes.c_void_p(rp),
                                                  ctypes.c_void_p(rp + 8), plan.n_tasks, _ptr(plan.task_row), _ptr(plan.task_b),
                                                  _ptr(plan.task_len), _ptr(plan.seg_off), plan.slices, lane, _ptr(y), k, _ptr(out),
                                                  k, _ptr(work), work.numel(), ctypes.byref(ep), _stream(y.device))
    _check(st, "fusedMM_csr_tasks_epilogue_hip")
    return out


def fusedMM_csr_sweep_hip(imessage: int, rowptr, col, val, plan, y, z, z_arg, workspace=None, epilogue=None, check: bool = True) -> int:
    """Raw boundary call of the sweep-schedule SpMM; ``plan`` is an isplib_amd.plan.SweepPlan."""
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    rp = rowptr.data_ptr()
    ps = plan.struct()
    with torch.cuda.device(y.device):
        st = exp_lib().fusedMM_csr_sweep_hip(int(imessage), m, n, k, col.numel(), _ptr(val), _ptr(col), _plan_col32(plan, col),
                                         ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), ctypes.byref(ps), _ptr(y),
                                         y.stride(0) if n > 1 else max(k, y.stride(0)), _ptr(z),
                                         z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(z_arg), _ptr(workspace),
                                         0 if workspace is None else workspace.numel(),
                                         None if epilogue is None else ctypes.byref(epilogue), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_sweep_hip")
    return st


def spmm_sweep(rowptr, col, val, plan, y, reduce: str = "sum", workspace=None, row_scale=None, self_term=None, bias=None,
               relu=False):
    """Allocate outputs (+ workspace) and call the sweep boundary; returns (out, arg|None)."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    if val is not None:
        val = _dev(val, "val", torch.float32)
    y = y.contiguous()
    m, k = rowptr.numel() - 1, y.size(1)
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    arg = torch.empty((m, k), dtype=torch.int64, device=y.device) if reduce in ("max", "min") else None
    if workspace is None:
        workspace = plan.workspace(reduce, k)
    ep = None
    if row_scale is not None or self_term is not None or bias is not None or relu:
        ep = Epilogue(None if row_scale is None else row_scale.data_ptr(), None if self_term is None else self_term.data_ptr(),
                      k if self_term is None else self_term.stride(0), None if bias is None else bias.data_ptr(), int(bool(relu)))
    fusedMM_csr_sweep_hip(MESSAGE[reduce], rowptr, col, val, plan, y, out, arg, workspace, ep)
    return out, arg


def fusedMM_csr_stream_hip(imessage: int, rowptr, nnz: int, plan, y, z, workspace=None, epilogue=None, check: bool = True) -> int:
    """Raw boundary call of the stream-form SpMM (sum / mean); ``plan`` is an isplib_amd.plan.StreamPlan."""
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    rp = rowptr.data_ptr()
    ps = plan.struct()
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_stream_hip(int(imessage), m, n, k, int(nnz), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                          ctypes.byref(ps), _ptr(y), y.stride(0) if n > 1 else max(k, y.stride(0)), _ptr(z),
                                          z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(workspace),
                                          0 if workspace is None else workspace.numel(),
                                          None if epilogue is None else ctypes.byref(epilogue), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_stream_hip")
    return st


def spmm_stream(rowptr, nnz: int, plan, y, reduce: str = "sum", workspace=None, row_scale=None, self_term=None, bias=None,
                relu=False):
    """Allocate the output (+ workspace) and call the stream boundary; returns out."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    y = y.contiguous()
    m, k = rowptr.numel() - 1, y.size(1)
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    if workspace is None:
        workspace = plan.workspace()
    ep = None
    if row_scale is not None or self_term is not None or bias is not None or relu:
        ep = Epilogue(None if row_scale is None else row_scale.data_ptr(), None if self_term is None else self_term.data_ptr(),
                      k if self_term is None else self_term.stride(0), None if bias is None else bias.data_ptr(), int(bool(relu)))
    fusedMM_csr_stream_hip(MESSAGE[reduce], rowptr, nnz, plan, y, out, workspace, ep)
    return out


HALF_DTYPES = {torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_F16}


def fusedMM_csr_stream16_hip(imessage: int, rowptr, nnz: int, plan, y, z, workspace=None, check: bool = True, dtype=None, k=None,
                             ldy=None, ldz=None) -> int:
    """Raw boundary call of the 16-bit stream SpMM (sum / mean), for operands the entry may refuse: it hands over what it is given
    (`dtype`, `k`, `ldy`, `ldz`: override what the tensors say -- refusal tests; the entry refuses before it reads anything).
    Callers that want their operands checked use spmm_stream16."""
    m, n = rowptr.numel() - 1, y.size(0)
    k = y.size(1) if k is None else int(k)
    code = HALF_DTYPES.get(y.dtype, 0) if dtype is None else int(dtype)
    rp = rowptr.data_ptr()
    ps = plan.struct()
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_stream16_hip(int(imessage), code, m, n, k, int(nnz), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                            ctypes.byref(ps), _ptr(y), (y.stride(0) if n > 1 else max(k, y.stride(0))) if ldy is None else int(ldy),
                                            _ptr(z), (z.stride(0) if m > 1 else max(k, z.stride(0))) if ldz is None else int(ldz),
                                            _ptr(workspace), 0 if workspace is None else workspace.numel(), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_stream16_hip")
    return st


def spmm_stream16(rowptr, nnz: int, plan, y, reduce: str = "sum", workspace=None, out=None):
    """The 16-bit stream SpMM (sum / mean) of a bf16 / fp16 `y` [n, k] on a sum plan: returns `out` [m, k] of y's dtype (allocated
    when not given; a row-strided view is written at its own pitch).  Every operand is checked BEFORE the call -- a mis-shaped one is
    an out-of-bounds device read: y 2-D on the GPU with unit inner stride and one row per column of the plan, rowptr with one entry
    per row of the plan (+ 1), the shape inside isplib_stream16_serves, `out` [m, k] of the same dtype at an even pitch."""
    if reduce not in ("sum", "add", "mean"):
        raise ValueError(f"isplib_amd: spmm_stream16 serves sum / mean, got '{reduce}'")
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    if not isinstance(y, torch.Tensor) or not y.is_cuda or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D GPU tensor [n, k]")
    if y.dtype not in HALF_DTYPES:
        raise TypeError(f"isplib_amd: `y` must be bfloat16 or float16, got {y.dtype} (float32: spmm_stream)")
    n, k = y.size(0), y.size(1)
    m = rowptr.numel() - 1
    if k > 0 and y.stride(1) != 1:
        raise ValueError("isplib_amd: `y` must have unit inner stride")
    if n != plan.cols or m != plan.rows:
        raise ValueError(f"isplib_amd: the plan was built for a {plan.rows} x {plan.cols} graph, got rowptr of {m} rows and y of {n} rows")
    if rowptr.device != y.device:
        raise ValueError("isplib_amd: rowptr and y are on different devices")
    ldy = y.stride(0) if n > 1 else max(k, y.stride(0))
    if out is None:
        out = torch.empty((m, k), dtype=y.dtype, device=y.device)
    elif not isinstance(out, torch.Tensor) or out.device != y.device or tuple(out.shape) != (m, k) or out.dtype != y.dtype or (k > 0 and out.stride(1) != 1):
        raise ValueError(f"isplib_amd: `out` must be a [{m}, {k}] {y.dtype} tensor on {y.device} with unit inner stride")
    ldz = out.stride(0) if m > 1 else max(k, out.stride(0))
    if m > 0 and k > 0:
        if ldy < k or ldz < k or not stream16_serves(n, k, ldy, ldz, int(nnz)):
            raise ValueError(f"isplib_amd: outside the 16-bit stream entry's domain (isplib_stream16_serves: n={n}, k={k}, ldy={ldy}, ldz={ldz}, nnz={int(nnz)})")
        if (y.data_ptr() | out.data_ptr()) & 3:
            raise ValueError("isplib_amd: `y` and `out` must be 4-byte aligned")
    if workspace is None:
        workspace = plan.workspace()
    fusedMM_csr_stream16_hip(MESSAGE[reduce], rowptr, nnz, plan, y, out, workspace)
    return out


def _rows16_raw(symbol: str, imessage: int, rowptr, col, val, order, y, z, check, dtype, k, ldy, ldz, *tail) -> int:
    """The raw boundary call shared by the three entries of the 16-bit row family (`tail`: an entry's own trailing arguments)."""
    m, n = rowptr.numel() - 1, y.size(0)
    k = y.size(1) if k is None else int(k)
    code = HALF_DTYPES.get(y.dtype, 0) if dtype is None else int(dtype)
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = getattr(lib(), symbol)(int(imessage), code, m, n, k, col.numel(), _ptr(val), _ptr(col), ctypes.c_void_p(rp),
                                    ctypes.c_void_p(rp + 8), _ptr(order),
                                    _ptr(y), (y.stride(0) if n > 1 else max(k, y.stride(0))) if ldy is None else int(ldy),
                                    _ptr(z), (z.stride(0) if m > 1 else max(k, z.stride(0))) if ldz is None else int(ldz), *tail,
                                    _stream(y.device))
    if check:
        _check(st, symbol)
    return st


def fusedMM_csr_rows16_hip(imessage: int, rowptr, col, val, order, y, z, check: bool = True, dtype=None, k=None, ldy=None, ldz=None) -> int:
    """Raw boundary call of the 16-bit row SpMM (sum / mean), for operands the entry may refuse: it hands over what it is given
    (`dtype`, `k`, `ldy`, `ldz`: override what the tensors say -- refusal tests; the entry refuses before it reads anything).
    Callers that want their operands checked use spmm_rows16."""
    return _rows16_raw("fusedMM_csr_rows16_hip", imessage, rowptr, col, val, order, y, z, check, dtype, k, ldy, ldz)


def spmm_rows16(rowptr, col, val, y, reduce: str = "sum", order=None, out=None):
    """The 16-bit row SpMM (sum / mean) of a bf16 / fp16 `y` [n, k]: returns `out` [m, k] of y's dtype (allocated when not given; a
    row-strided view is written at its own pitch).  `val`: fp32 weights or None; `order`: int32 [m], position -> row, or None.
    Every operand is checked BEFORE the call -- a mis-shaped one is an out-of-bounds device read: rowptr / col int64 on y's device,
    rowptr ascending from 0 to col.numel(), every column id inside [0, n), the shape inside isplib_rows16_serves, `out` [m, k] of
    the same dtype at an even pitch, `order` a permutation's length."""
    if reduce not in ("sum", "add", "mean"):
        raise ValueError(f"isplib_amd: spmm_rows16 serves sum / mean, got '{reduce}'")
    rowptr, col, val, order, out, _ = _rows16_operands(rowptr, col, val, False, y, order, out)
    fusedMM_csr_rows16_hip(MESSAGE[reduce], rowptr, col, val, order, y, out)
    return out


def _rows16_operands(rowptr, col, val, per_column: bool, y, order, out, arg=None, want_arg: bool = False):
    """The operand checks of spmm_rows16, spmm_rows16_minmax and spmm_rows16_colscale (`per_column`: `val` is the n-entry table, not nnz weights);
    returns (rowptr, col, val, order, out, arg) as the entries take them.  The max / min wrapper also hands over its positions tensor
    `arg` (allocated when `want_arg` and not given), checked in its place among the others, and gets it back; the others get None."""
    if not isinstance(y, torch.Tensor) or not y.is_cuda or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D GPU tensor [n, k]")
    if y.dtype not in HALF_DTYPES:
        raise TypeError(f"isplib_amd: `y` must be bfloat16 or float16, got {y.dtype} (float32: spmm)")
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    n, k = y.size(0), y.size(1)
    m = rowptr.numel() - 1
    if m < 0 or rowptr.device != y.device or col.device != y.device:
        raise ValueError("isplib_amd: rowptr (m + 1 entries), col and y must be on one device")
    if k > 0 and y.stride(1) != 1:
        raise ValueError("isplib_amd: `y` must have unit inner stride")
    if per_column:
        if val is None:
            raise ValueError("isplib_amd: `scale` must be given (unit weights: spmm_rows16 with val=None)")
        val = _dev(val, "scale", torch.float32)
        if val.numel() != n or val.device != y.device:
            raise ValueError("isplib_amd: `scale` must hold one float32 factor per row of `y`, on y's device")
    elif val is not None:
        val = _dev(val, "val", torch.float32)
        if val.numel() != col.numel() or val.device != y.device:
            raise ValueError("isplib_amd: `val` must hold one float32 weight per entry of `col`, on y's device")
    if order is not None:
        order = _dev(order, "order", torch.int32)
        if order.numel() != m or order.device != y.device or (m > 0 and (int(order.min()) < 0 or int(order.max()) >= m)):
            raise ValueError("isplib_amd: `order` must hold one int32 row in [0, m) per position, on y's device")
    if m > 0 and (int(rowptr[0]) != 0 or int(rowptr[-1]) != col.numel() or bool((rowptr[1:] < rowptr[:-1]).any())):
        raise ValueError("isplib_amd: rowptr must ascend from 0 to col.numel()")
    if col.numel() > 0 and (int(col.min()) < 0 or int(col.max()) >= n):
        raise ValueError(f"isplib_amd: column ids must lie in [0, {n})")
    ldy = y.stride(0) if n > 1 else max(k, y.stride(0))
    if out is None:
        out = torch.empty((m, k), dtype=y.dtype, device=y.device)
    elif not isinstance(out, torch.Tensor) or out.device != y.device or tuple(out.shape) != (m, k) or out.dtype != y.dtype or (k > 0 and out.stride(1) != 1):
        raise ValueError(f"isplib_amd: `out` must be a [{m}, {k}] {y.dtype} tensor on {y.device} with unit inner stride")
    if arg is None:
        arg = torch.empty((m, k), dtype=torch.int64, device=y.device) if want_arg else None
    elif not isinstance(arg, torch.Tensor) or arg.device != y.device or tuple(arg.shape) != (m, k) or arg.dtype != torch.int64 or (k > 0 and arg.stride(1) != 1):
        raise ValueError(f"isplib_amd: `arg` must be a [{m}, {k}] int64 tensor on {y.device} with unit inner stride")
    ldz = out.stride(0) if m > 1 else max(k, out.stride(0))
    if m > 0 and k > 0:
        if ldy < k or ldz < k or not rows16_serves(n, k, ldy, ldz):
            raise ValueError(f"isplib_amd: outside the 16-bit row entry's domain (isplib_rows16_serves: n={n}, k={k}, ldy={ldy}, ldz={ldz})")
        if arg is not None and m > 1 and arg.stride(0) < k:
            raise ValueError("isplib_amd: `arg` rows must not overlap")
        if (y.data_ptr() | out.data_ptr()) & 3:
            raise ValueError("isplib_amd: `y` and `out` must be 4-byte aligned")
    return rowptr, col, val, order, out, arg


def fusedMM_csr_rows16_colscale_hip(imessage: int, rowptr, col, scale, order, y, z, check: bool = True, dtype=None, k=None, ldy=None,
                                    ldz=None) -> int:
    """Raw boundary call of the column-scaled 16-bit row SpMM (sum / mean), for operands the entry may refuse: it hands over what
    it is given (`dtype`, `k`, `ldy`, `ldz`: override what the tensors say -- refusal tests; the entry refuses before it reads
    anything).  Callers that want their operands checked use spmm_rows16_colscale."""
    return _rows16_raw("fusedMM_csr_rows16_colscale_hip", imessage, rowptr, col, scale, order, y, z, check, dtype, k, ldy, ldz)


def spmm_rows16_colscale(rowptr, col, scale, y, reduce: str = "sum", order=None, out=None):
    """spmm_rows16 with one fp32 factor per column of the sparse operand, `scale` [n], in place of per-edge weights: the bits of
    spmm_rows16(rowptr, col, scale[col], y, ...) without the nnz-long weight array.  The same operand checks BEFORE the call."""
    if reduce not in ("sum", "add", "mean"):
        raise ValueError(f"isplib_amd: spmm_rows16_colscale serves sum / mean, got '{reduce}'")
    rowptr, col, scale, order, out, _ = _rows16_operands(rowptr, col, scale, True, y, order, out)
    fusedMM_csr_rows16_colscale_hip(MESSAGE[reduce], rowptr, col, scale, order, y, out)
    return out


class Epilogue16(ctypes.Structure):
    """isplib_epilogue16 of the header."""
    _fields_ = [("row_scale", ctypes.c_void_p), ("self_scale", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("relu", ctypes.c_int)]


def fusedMM_csr_rows16_epilogue_hip(rowptr, col, col_scale, order, y, z, row_scale=None, self_scale=None, bias=None, relu: bool = False,
                                    null_epilogue: bool = False, check: bool = True, dtype=None, m=None, k=None, ldy=None, ldz=None) -> int:
    """Raw boundary call of the 16-bit row SpMM with an epilogue, for operands the entry may refuse: it hands over what it is given
    (`dtype`, `m`, `k`, `ldy`, `ldz`: override what the tensors say -- refusal tests; the entry refuses before it reads anything;
    `null_epilogue`: pass ep = NULL instead of a struct).  Callers that want their operands checked use spmm_rows16_epilogue."""
    m = rowptr.numel() - 1 if m is None else int(m)
    n = y.size(0)
    k = y.size(1) if k is None else int(k)
    code = HALF_DTYPES.get(y.dtype, 0) if dtype is None else int(dtype)
    ep = Epilogue16(None if row_scale is None else row_scale.data_ptr(), None if self_scale is None else self_scale.data_ptr(),
                    None if bias is None else bias.data_ptr(), int(bool(relu)))
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_rows16_epilogue_hip(code, m, n, k, col.numel(), _ptr(col_scale), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                                   _ptr(order), _ptr(y), (y.stride(0) if n > 1 else max(k, y.stride(0))) if ldy is None else int(ldy),
                                                   _ptr(z), (z.stride(0) if z.size(0) > 1 else max(k, z.stride(0))) if ldz is None else int(ldz),
                                                   None if null_epilogue else ctypes.cast(ctypes.pointer(ep), ctypes.c_void_p), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_rows16_epilogue_hip")
    return st


def spmm_rows16_epilogue(rowptr, col, col_scale, y, row_scale=None, self_scale=None, bias=None, relu: bool = False, order=None, out=None):
    """out[i] = round16(act(row_scale[i] * (sum_e col_scale[col[e]] * y[col[e]] + self_scale[i] * y[i]) + bias)) of a bf16 / fp16 `y`
    [n, k] on the 16-bit row kernel (fusedMM_csr_rows16_epilogue_hip): every table is float32 and optional (`col_scale` None: unit
    weights; `self_scale` needs a square operand).  The operand checks of spmm_rows16 and the tables' lengths, dtypes and devices are
    checked BEFORE the call."""
    if col_scale is None:
        rowptr, col, _, order, out, _ = _rows16_operands(rowptr, col, None, False, y, order, out)
    else:
        rowptr, col, col_scale, order, out, _ = _rows16_operands(rowptr, col, col_scale, True, y, order, out)
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    tables = {}
    for name, t, length in (("row_scale", row_scale, m), ("self_scale", self_scale, m), ("bias", bias, k)):
        if t is not None:
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"isplib_amd: `{name}` must be a float32 GPU tensor")
            t = _dev(t, name, torch.float32)
            if t.numel() != length or t.device != y.device:
                raise ValueError(f"isplib_amd: `{name}` must hold {length} float32 values on y's device")
        tables[name] = t
    if self_scale is not None and m != n:
        raise ValueError(f"isplib_amd: `self_scale` needs a square operand (the self row of i is y[i]); m={m}, n={n}")
    fusedMM_csr_rows16_epilogue_hip(rowptr, col, col_scale, order, y, out, tables["row_scale"], tables["self_scale"], tables["bias"], relu)
    return out


def masked_colsum16(dz: torch.Tensor, out: Optional[torch.Tensor], want_g: bool = True, want_bias: bool = True):
    """(g, grad_bias) of isplib_masked_colsum16_hip for bf16 / fp16 `dz` [n, k] (row-strided views keep their pitch): g = dz where
    out > 0 else +0 (a bit select; `out` None: no mask), grad_bias = g.float().sum(0) in fp32.  Either may be left out."""
    if not isinstance(dz, torch.Tensor) or not dz.is_cuda or dz.dim() != 2 or dz.dtype not in HALF_DTYPES:
        raise TypeError("isplib_amd: `dz` must be a 2-D bfloat16 / float16 GPU tensor")
    n, k = dz.shape
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != dz.dtype or out.device != dz.device or tuple(out.shape) != (n, k)):
        raise ValueError("isplib_amd: `out` must have dz's shape, dtype and device")
    pitches = []
    for name, t in (("dz", dz), ("out", out)):
        if t is not None and k > 0:
            ld = t.stride(0) if n > 1 else max(k, t.stride(0))
            if t.stride(1) != 1 or ld < k or ld % 2 or t.data_ptr() & 3:
                raise ValueError(f"isplib_amd: `{name}` must have unit inner stride, an even pitch >= k and a 4-byte aligned base")
            pitches.append(ld)
    if k % 2:
        raise ValueError("isplib_amd: k must be even")
    g = torch.empty((n, k), dtype=dz.dtype, device=dz.device) if want_g else None
    gb = torch.empty(k, dtype=torch.float32, device=dz.device) if want_bias else None
    with torch.cuda.device(dz.device):
        ws = lib().isplib_masked_colsum16_workspace_bytes(n, k)
        work = torch.empty(max(ws, 256), dtype=torch.uint8, device=dz.device)
        _check(lib().isplib_masked_colsum16_hip(HALF_DTYPES[dz.dtype], n, k, _ptr(dz), pitches[0] if pitches else k, _ptr(out),
                                                pitches[1] if len(pitches) > 1 else k, _ptr(g), k, _ptr(gb), _ptr(work), work.numel(),
                                                _stream(dz.device)), "isplib_masked_colsum16_hip")
    return g, gb


def isplib_sddmm_csr_rows16_hip(rowptr, col, order, y, g, dval, mean: bool = False, check: bool = True, dtype=None, k=None, ldy=None,
                                ldg=None) -> int:
    """Raw boundary call of the 16-bit SDDMM row entry, for operands the entry may refuse: it hands over what it is given (`dtype`,
    `k`, `ldy`, `ldg`: override what the tensors say; `y`, `g`, `dval` may be None -- refusal tests; the entry refuses before it
    reads anything).  Callers that want their operands checked use sddmm_rows16."""
    some = y if y is not None else g
    m, n = rowptr.numel() - 1, some.size(0) if y is None else y.size(0)
    k = some.size(1) if k is None else int(k)
    code = HALF_DTYPES.get(some.dtype, 0) if dtype is None else int(dtype)
    rp = rowptr.data_ptr()
    if ldy is None:
        ldy = k if y is None else (y.stride(0) if n > 1 else max(k, y.stride(0)))
    if ldg is None:
        ldg = k if g is None else (g.stride(0) if m > 1 else max(k, g.stride(0)))
    with torch.cuda.device(rowptr.device):
        st = lib().isplib_sddmm_csr_rows16_hip(code, m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(order),
                                               _ptr(y), int(ldy), _ptr(g), int(ldg), 1 if mean else 0, _ptr(dval), _stream(rowptr.device))
    if check:
        _check(st, "isplib_sddmm_csr_rows16_hip")
    return st


def sddmm_rows16(rowptr, col, y, g, mean: bool = False, order=None, out=None):
    """The value gradient of SpMM-sum / SpMM-mean for bf16 / fp16 operands, neither widened in memory: returns `out`, float32
    [col.numel()] in CSR order (allocated when not given), out[j] = <y[col[j], :], g[i, :]> (`mean`: / max(deg_i, 1)) for the
    entries j of row i.  `y` [n, k] and `g` [m, k] of one 16-bit dtype, row-strided views keep their pitch; `order`: int32 [m],
    position -> row, or None.  Every operand is checked BEFORE the call -- a mis-shaped one is an out-of-bounds device read: shapes
    and dtypes, unit inner strides, rowptr / col int64 on y's device, rowptr ascending from 0 to col.numel(), every column id inside
    [0, n), the shape inside isplib_sddmm_rows16_serves, 4-byte aligned bases, `order` a permutation's length."""
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, k]")
    if y.dtype not in HALF_DTYPES:
        raise TypeError(f"isplib_amd: `y` must be bfloat16 or float16, got {y.dtype} (float32: sddmm)")
    m = rowptr.numel() - 1
    n, k = y.size(0), y.size(1)
    if not isinstance(g, torch.Tensor) or g.dim() != 2 or tuple(g.shape) != (m, k):
        raise ValueError(f"isplib_amd: `g` must be a 2-D tensor [{m}, {k}] (one row per row of the sparse operand, y's width)")
    if g.dtype != y.dtype:
        raise TypeError(f"isplib_amd: `g` must have y's dtype {y.dtype}, got {g.dtype}")
    if k > 0 and (y.stride(1) != 1 or g.stride(1) != 1):
        raise ValueError("isplib_amd: `y` and `g` must have unit inner stride")
    if not y.is_cuda or g.device != y.device:
        raise ValueError("isplib_amd: `y` and `g` must be GPU tensors on one device -- there is no CPU path")
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    col = _dev(col, "col", torch.int64)
    if m < 0 or rowptr.device != y.device or col.device != y.device:
        raise ValueError("isplib_amd: rowptr (m + 1 entries), col and y must be on one device")
    if order is not None:
        order = _dev(order, "order", torch.int32)
        if order.numel() != m or order.device != y.device or (m > 0 and (int(order.min()) < 0 or int(order.max()) >= m)):
            raise ValueError("isplib_amd: `order` must hold one int32 row in [0, m) per position, on y's device")
    if m > 0 and (int(rowptr[0]) != 0 or int(rowptr[-1]) != col.numel() or bool((rowptr[1:] < rowptr[:-1]).any())):
        raise ValueError("isplib_amd: rowptr must ascend from 0 to col.numel()")
    if col.numel() > 0 and (int(col.min()) < 0 or int(col.max()) >= n):
        raise ValueError(f"isplib_amd: column ids must lie in [0, {n}): `y` must hold a row for every column of the sparse operand")
    if out is None:
        out = torch.empty(col.numel(), dtype=torch.float32, device=y.device)
    elif not isinstance(out, torch.Tensor) or out.device != y.device or out.dtype != torch.float32 or out.dim() != 1 or \
            out.numel() < col.numel() or not out.is_contiguous():
        raise ValueError(f"isplib_amd: `out` must be a contiguous float32 tensor of at least {col.numel()} entries on {y.device}")
    ldy = y.stride(0) if n > 1 else max(k, y.stride(0))
    ldg = g.stride(0) if m > 1 else max(k, g.stride(0))
    if m > 0 and k > 0 and col.numel() > 0:
        if ldy < k or ldg < k or not sddmm_rows16_serves(n, k, ldy, ldg):
            raise ValueError(f"isplib_amd: outside the 16-bit SDDMM row entry's domain (isplib_sddmm_rows16_serves: n={n}, k={k}, ldy={ldy}, ldg={ldg})")
        if (y.data_ptr() | g.data_ptr()) & 3:
            raise ValueError("isplib_amd: `y` and `g` must be 4-byte aligned")
    isplib_sddmm_csr_rows16_hip(rowptr, col, order, y, g, out, mean)
    return out


def _attn_dense(t, name: str, rows: int, k: Optional[int], what: str) -> int:
    """One dense operand of the attention entries: 2-D float32 [rows, k] on the GPU with unit inner stride; a row-strided view keeps its
    pitch (head views of one [N, H*d] tensor go in without a copy).  Returns the pitch in elements."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"isplib_amd: `{name}` must be a 2-D tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"isplib_amd: `{name}` must be float32, got {t.dtype} (the attention operator is fp32 only)")
    if t.size(0) != rows or (k is not None and t.size(1) != k):
        raise ValueError(f"isplib_amd: `{name}` must be [{rows}, {'k' if k is None else k}] ({what}), got {tuple(t.shape)}")
    if t.size(1) > 0 and t.size(0) > 0 and t.stride(1) != 1:
        raise ValueError(f"isplib_amd: `{name}` must have unit inner stride")
    ld = t.stride(0) if t.size(0) > 1 else max(t.size(1), t.stride(0))
    if ld < t.size(1):
        raise ValueError(f"isplib_amd: the rows of `{name}` (pitch {ld}) must not overlap: k = {t.size(1)}")
    return int(ld)


def _attn_vector(t, name: str, rows: int) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != rows or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"isplib_amd: `{name}` must be a contiguous float32 tensor of {rows} entries")


def _attn_structure(ptr, idx, ptr_name: str, idx_name: str, id_end: int, check: bool):
    """rowptr / col (or colptr / row_t): 1-D int64; with `check` (two reductions and a synchronisation -- a timed loop over a graph
    already checked passes check=False) the pointer array ascends from 0 to idx.numel() and every id lies in [0, id_end)."""
    if not isinstance(ptr, torch.Tensor) or ptr.dim() != 1 or ptr.numel() < 1 or not isinstance(idx, torch.Tensor) or idx.dim() != 1:
        raise ValueError(f"isplib_amd: `{ptr_name}` (one entry more than it has ranges) and `{idx_name}` must be 1-D tensors")
    if ptr.dtype != torch.int64 or idx.dtype != torch.int64:
        raise TypeError(f"isplib_amd: `{ptr_name}` and `{idx_name}` must be int64, got {ptr.dtype} and {idx.dtype}")
    if check and ptr.is_cuda and idx.is_cuda:
        if int(ptr[0]) != 0 or int(ptr[-1]) != idx.numel() or bool((ptr[1:] < ptr[:-1]).any()):
            raise ValueError(f"isplib_amd: `{ptr_name}` must ascend from 0 to {idx_name}.numel()")
        if idx.numel() > 0 and (int(idx.min()) < 0 or int(idx.max()) >= id_end):
            raise ValueError(f"isplib_amd: the ids of `{idx_name}` must lie in [0, {id_end}): the gathered operand must hold a row for each")
    return ptr.contiguous(), idx.contiguous()


def _attn_domain(rows_gathered: int, k: int, lds) -> None:
    for ld in lds:
        if k > 0 and not attention_serves(rows_gathered, k, ld):
            raise ValueError(f"isplib_amd: outside the attention entries' domain (isplib_attention_serves: 1 <= k <= {ATTENTION_K_MAX}, "
                             f"gathered rows < 2^31, rows * pitch * 4 <= 3.5 GiB), got rows={rows_gathered}, k={k}, pitch={ld}")


def _attn_scale(scale, k: int) -> float:
    return float(scale) if scale is not None else (1.0 / float(k) ** 0.5 if k > 0 else 1.0)


def attention(rowptr, col, x, y, scale: Optional[float] = None, *, out=None, check: bool = True):
    """Row-softmax attention aggregation (isplib_attention_csr_hip): over the stored entries e = (i, j) of the CSR structure,
    s_e = scale <x_i, y_j>, a_e = softmax of s over the row's entries, z_i = sum_e a_e y_j.  Returns (z [m, k], lse [m]); an empty
    row has z_i = 0 and lse_i = -inf.  `x` [m, k] and `y` [n, k] float32, row-strided views keep their pitch; `scale` None =
    1 / sqrt(k); `out` = (z, lse) to write in place.  Every operand is checked BEFORE the call -- a mis-shaped one is an out-of-bounds
    device read (`check`: also the two checks that read the structure on the device)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    ldx = _attn_dense(x, "x", m, None, "one row per row of the sparse operand")
    k = x.size(1)
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, k]")
    n = y.size(0)
    ldy = _attn_dense(y, "y", n, k, "x's width")
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        z, lse = out
        ldz = _attn_dense(z, "out[0]", m, k, "z")
        _attn_vector(lse, "out[1]", m)
    _attn_domain(n, k, (ldy,))
    _same_gpu((("x", x), ("y", y), ("rowptr", rowptr), ("col", col)) + ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, k), dtype=torch.float32, device=x.device)
        lse = torch.empty(m, dtype=torch.float32, device=x.device)
        ldz = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            lse.fill_(float("-inf"))                            # no column, no score: every row is empty
        return z, lse
    rp = rowptr.data_ptr()
    with torch.cuda.device(x.device):
        st = lib().isplib_attention_csr_hip(m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(x), ldx,
                                            _ptr(y), ldy, _attn_scale(scale, k), _ptr(z), ldz, _ptr(lse), _stream(x.device))
    _check(st, "isplib_attention_csr_hip")
    return z, lse


def attention_bw_rows(rowptr, col, x, y, g, z, lse, scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `attention` over the rows (isplib_attention_bw_rows_hip): for g = dL/dz [m, k] and the forward's z and lse,
    D_i = <g_i, z_i>, ds_e = a_e (<g_i, y_j> - D_i) with a_e = exp(s_e - lse_i) recomputed, dx_i = scale sum_e ds_e y_j.  Returns
    (dx [m, k], D [m]); an empty row has dx_i = 0 and D_i = 0.  `out` = (dx, D); the operand checks are attention's."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    ldx = _attn_dense(x, "x", m, None, "one row per row of the sparse operand")
    k = x.size(1)
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, k]")
    n = y.size(0)
    ldy = _attn_dense(y, "y", n, k, "x's width")
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    ldz = _attn_dense(z, "z", m, k, "the forward's output")
    _attn_vector(lse, "lse", m)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        dx, dsum = out
        lddx = _attn_dense(dx, "out[0]", m, k, "dx")
        _attn_vector(dsum, "out[1]", m)
    _attn_domain(n, k, (ldy,))
    _same_gpu((("x", x), ("y", y), ("g", g), ("z", z), ("lse", lse), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        dx = torch.empty((m, k), dtype=torch.float32, device=x.device)
        dsum = torch.empty(m, dtype=torch.float32, device=x.device)
        lddx = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            dsum.zero_()
        return dx, dsum
    rp = rowptr.data_ptr()
    with torch.cuda.device(x.device):
        st = lib().isplib_attention_bw_rows_hip(m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(x), ldx,
                                                _ptr(y), ldy, _attn_scale(scale, k), _ptr(g), ldg, _ptr(z), ldz, _ptr(lse), _ptr(dx), lddx,
                                                _ptr(dsum), _stream(x.device))
    _check(st, "isplib_attention_bw_rows_hip")
    return dx, dsum


def attention_bw_cols(colptr, row_t, x, y, g, lse, dsum, scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `attention` over the columns (isplib_attention_bw_cols_hip), on the transposed structure (`colptr` [n + 1],
    `row_t`: the row ids of the entries in column-major order, SparseStorage.colptr() / row_t()): dy_j = sum over the entries
    e = (i, j) of column j of a_e g_i + scale ds_e x_i, with `lse` of the forward and `dsum` = D of attention_bw_rows.  Returns
    dy [n, k]; a column no entry points at has dy_j = 0.  `out` = dy; the operand checks are attention's."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    k = y.size(1)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("isplib_amd: `x` must be a 2-D tensor [m, k]")
    m = x.size(0)
    ldx = _attn_dense(x, "x", m, k, "y's width")
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    _attn_vector(lse, "lse", m)
    _attn_vector(dsum, "dsum", m)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    if out is not None:
        lddy = _attn_dense(out, "out", n, k, "dy")
    _attn_domain(m, k, (ldx, ldg))
    _same_gpu((("x", x), ("y", y), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t), ("out", out)))
    if out is None:
        out = torch.empty((n, k), dtype=torch.float32, device=y.device)
        lddy = max(k, 1)
    if n == 0 or k == 0:
        return out
    cp = colptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_attention_bw_cols_hip(m, n, k, row_t.numel(), _ptr(row_t), ctypes.c_void_p(cp), ctypes.c_void_p(cp + 8), _ptr(x), ldx,
                                                _ptr(y), ldy, _attn_scale(scale, k), _ptr(g), ldg, _ptr(lse), _ptr(dsum), _ptr(out), lddy,
                                                _stream(y.device))
    _check(st, "isplib_attention_bw_cols_hip")
    return out


def _gat_heads(heads, k: int) -> int:
    if isinstance(heads, bool) or not isinstance(heads, int) or heads < 1:
        raise ValueError(f"isplib_amd: `heads` must be a positive int, got {heads!r}")
    if k % heads:
        raise ValueError(f"isplib_amd: the width of `y` ({k}) must be heads * d, got heads = {heads}")
    return k // heads


def _gat_table(t, name: str, rows: int, heads: int) -> None:
    """One per-node table of the GAT entries: a dense float32 [rows, heads] tensor."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"isplib_amd: `{name}` must be a 2-D tensor [{rows}, {heads}], got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"isplib_amd: `{name}` must be float32, got {t.dtype} (the attention operator is fp32 only)")
    if t.size(0) != rows or t.size(1) != heads:
        raise ValueError(f"isplib_amd: `{name}` must be [{rows}, {heads}] (one entry per row and head), got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"isplib_amd: `{name}` must be contiguous (the [rows, heads] tables are dense)")


def _gat_domain(rows_gathered: int, heads: int, d: int, ld: int) -> None:
    if d > 0 and not gat_serves(rows_gathered, heads, d, ld):
        raise ValueError(f"isplib_amd: outside the GAT entries' domain (isplib_gat_serves: heads * d <= {GAT_K_MAX}, heads == 1 or d a power "
                         f"of two >= 4, gathered rows < 2^31, rows * pitch * 4 <= 3.5 GiB), got rows={rows_gathered}, heads={heads}, d={d}, "
                         f"pitch={ld}")


def gat(rowptr, col, y, a_dst, a_src, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """GAT attention aggregation, all heads in one launch (isplib_gat_csr_hip): over the stored entries e = (i, j) of the CSR structure
    and every head h, s_e = leaky_relu(a_dst[i,h] + a_src[j,h]), a_e = softmax of s over the row's entries, z_i[head h] = sum_e a_e
    y_j[head h].  Returns (z [m, heads * d], lse [m, heads]); an empty row has z_i = 0 and lse = -inf.  `y` [n, heads * d] float32 (a
    row-strided view keeps its pitch), `a_dst` [m, heads] and `a_src` [n, heads] dense float32; `out` = (z, lse) to write in place.
    Every operand is checked BEFORE the call (`check`: also the two checks that read the structure on the device)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n, k = y.size(0), y.size(1)
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    d = _gat_heads(heads, k)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        z, lse = out
        ldz = _attn_dense(z, "out[0]", m, k, "z")
        _gat_table(lse, "out[1]", m, heads)
    _gat_domain(n, heads, d, ldy)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, k), dtype=torch.float32, device=y.device)
        lse = torch.empty((m, heads), dtype=torch.float32, device=y.device)
        ldz = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_csr_hip(m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(a_dst), _ptr(y), ldy,
                                      _ptr(a_src), heads, float(negative_slope), _ptr(z), ldz, _ptr(lse), _stream(y.device))
    _check(st, "isplib_gat_csr_hip")
    return z, lse


def gat_bw_rows(rowptr, col, y, a_dst, a_src, g, z, lse, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """The backward of `gat` over the rows (isplib_gat_bw_rows_hip): for g = dL/dz [m, heads * d] and the forward's z and lse,
    D[i,h] = <g_i, z_i>_h, du_e = a_e (<g_i, y_j>_h - D[i,h]) * (1 or negative_slope) with a_e recomputed from lse, d a_dst[i,h] =
    sum_e du_e.  Returns (d_a_dst [m, heads], D [m, heads]); an empty row has both 0.  `out` = (d_a_dst, D); the operand checks are
    gat's."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n, k = y.size(0), y.size(1)
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    d = _gat_heads(heads, k)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    ldz = _attn_dense(z, "z", m, k, "the forward's output")
    _gat_table(lse, "lse", m, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        _gat_table(out[0], "out[0]", m, heads)
        _gat_table(out[1], "out[1]", m, heads)
    _gat_domain(n, heads, d, ldy)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("g", g), ("z", z), ("lse", lse), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        out = (torch.empty((m, heads), dtype=torch.float32, device=y.device), torch.empty((m, heads), dtype=torch.float32, device=y.device))
    dadst, dsum = out
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            dadst.zero_()
            dsum.zero_()
        return dadst, dsum
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_bw_rows_hip(m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(a_dst), _ptr(y),
                                          ldy, _ptr(a_src), heads, float(negative_slope), _ptr(g), ldg, _ptr(z), ldz, _ptr(lse), _ptr(dadst),
                                          _ptr(dsum), _stream(y.device))
    _check(st, "isplib_gat_bw_rows_hip")
    return dadst, dsum


def gat_bw_cols(colptr, row_t, y, a_dst, a_src, g, lse, dsum, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """The backward of `gat` over the columns (isplib_gat_bw_cols_hip), on the transposed structure (`colptr` [n + 1], `row_t`: the row
    ids of the entries in column-major order): dy_j[head h] = sum over the entries e = (i, j) of column j of a_e g_i[head h] and
    d a_src[j,h] = sum of du_e, with `lse` of the forward and `dsum` = D of gat_bw_rows.  Returns (dy [n, heads * d], d_a_src
    [n, heads]); a column no entry points at has both 0.  `out` = (dy, d_a_src); the operand checks are gat's."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    k = y.size(1)
    d = _gat_heads(heads, k)
    if not isinstance(g, torch.Tensor) or g.dim() != 2:
        raise ValueError("isplib_amd: `g` must be a 2-D tensor [m, heads * d]")
    m = g.size(0)
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    _gat_table(lse, "lse", m, heads)
    _gat_table(dsum, "dsum", m, heads)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    if out is not None:
        lddy = _attn_dense(out[0], "out[0]", n, k, "dy")
        _gat_table(out[1], "out[1]", n, heads)
    _gat_domain(m, heads, d, ldg)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        out = (torch.empty((n, k), dtype=torch.float32, device=y.device), torch.empty((n, heads), dtype=torch.float32, device=y.device))
        lddy = max(k, 1)
    dy, dasrc = out
    if n == 0 or k == 0:
        if k == 0 and n > 0:
            dasrc.zero_()
        return dy, dasrc
    cp = colptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_bw_cols_hip(m, n, k, row_t.numel(), _ptr(row_t), ctypes.c_void_p(cp), ctypes.c_void_p(cp + 8), _ptr(a_dst),
                                          _ptr(y), ldy, _ptr(a_src), heads, float(negative_slope), _ptr(g), ldg, _ptr(lse), _ptr(dsum),
                                          _ptr(dy), lddy, _ptr(dasrc), _stream(y.device))
    _check(st, "isplib_gat_bw_cols_hip")
    return dy, dasrc


def _gat_edge_domain(nnz: int, heads: int) -> None:
    if not gat_edge_serves(nnz, heads):
        raise ValueError(f"isplib_amd: outside the GAT edge entries' domain (isplib_gat_edge_serves: nnz < 2^31, nnz * heads * 4 <= "
                         f"{DENSE_BYTES_MAX} bytes = 3.5 GiB, `a_edge` behind one buffer descriptor), got nnz={nnz}, heads={heads}; pass fewer "
                         f"heads per call, on column views of `y`")


def _gat_edge_positions(csr2csc, nnz: int, check: bool):
    if not isinstance(csr2csc, torch.Tensor) or csr2csc.dim() != 1 or csr2csc.numel() != nnz:
        raise ValueError(f"isplib_amd: `csr2csc` must be a 1-D tensor of {nnz} entries (the CSR position of every entry of the transposed "
                         f"structure), got {tuple(csr2csc.shape) if isinstance(csr2csc, torch.Tensor) else type(csr2csc).__name__}")
    if csr2csc.dtype != torch.int64:
        raise TypeError(f"isplib_amd: `csr2csc` must be int64, got {csr2csc.dtype}")
    if check and csr2csc.is_cuda and nnz > 0 and (int(csr2csc.min()) < 0 or int(csr2csc.max()) >= nnz):
        raise ValueError(f"isplib_amd: the positions of `csr2csc` must lie in [0, {nnz})")
    return csr2csc.contiguous()


def gat_edge(rowptr, col, y, a_dst, a_src, a_edge, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """`gat` with a per-edge score term (isplib_gat_edge_csr_hip): u_e = (a_dst[i,h] + a_src[j,h]) + a_edge[e,h], two fp32 adds in this
    order; `a_edge` is a dense float32 [nnz, heads], row e belonging to the entry col[e] (CSR position order).  Returns (z, lse); every
    operand, the domain of `a_edge` (gat_edge_serves) included, is checked BEFORE the call."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n, k = y.size(0), y.size(1)
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    d = _gat_heads(heads, k)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    _gat_table(a_edge, "a_edge", col.numel(), heads)
    if out is not None:
        z, lse = out
        ldz = _attn_dense(z, "out[0]", m, k, "z")
        _gat_table(lse, "out[1]", m, heads)
    _gat_domain(n, heads, d, ldy)
    _gat_edge_domain(col.numel(), heads)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("a_edge", a_edge), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, k), dtype=torch.float32, device=y.device)
        lse = torch.empty((m, heads), dtype=torch.float32, device=y.device)
        ldz = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_edge_csr_hip(m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(a_dst), _ptr(y),
                                           ldy, _ptr(a_src), _ptr(a_edge), heads, float(negative_slope), _ptr(z), ldz, _ptr(lse),
                                           _stream(y.device))
    _check(st, "isplib_gat_edge_csr_hip")
    return z, lse


def gat_edge_bw_rows(rowptr, col, y, a_dst, a_src, a_edge, g, z, lse, heads: int = 1, negative_slope: float = 0.2, *, out=None,
                     want_edge: bool = True, check: bool = True):
    """The backward of `gat_edge` over the rows (isplib_gat_edge_bw_rows_hip): `gat_bw_rows` with the per-edge term, and d a_edge[e,h] =
    du_e written once per entry.  Returns (d_a_dst [m, heads], D [m, heads], d_a_edge [nnz, heads]); with want_edge=False nothing per
    edge is allocated or written and the third result is None.  `out` = (d_a_dst, D, d_a_edge or None)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n, k = y.size(0), y.size(1)
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    d = _gat_heads(heads, k)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    ldz = _attn_dense(z, "z", m, k, "the forward's output")
    _gat_table(lse, "lse", m, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    nnz = col.numel()
    _gat_table(a_edge, "a_edge", nnz, heads)
    if out is not None:
        _gat_table(out[0], "out[0]", m, heads)
        _gat_table(out[1], "out[1]", m, heads)
        if out[2] is not None:
            _gat_table(out[2], "out[2]", nnz, heads)
    _gat_domain(n, heads, d, ldy)
    _gat_edge_domain(nnz, heads)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("a_edge", a_edge), ("g", g), ("z", z), ("lse", lse), ("rowptr", rowptr),
               ("col", col)) + ((("out[0]", out[0]), ("out[1]", out[1]), ("out[2]", out[2])) if out is not None else ()))
    if out is None:
        out = (torch.empty((m, heads), dtype=torch.float32, device=y.device), torch.empty((m, heads), dtype=torch.float32, device=y.device),
               torch.empty((nnz, heads), dtype=torch.float32, device=y.device) if want_edge else None)
    dadst, dsum, dedge = out
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            dadst.zero_()
            dsum.zero_()
            if dedge is not None:
                dedge.zero_()
        return dadst, dsum, dedge
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_edge_bw_rows_hip(m, n, k, nnz, _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(a_dst), _ptr(y), ldy,
                                               _ptr(a_src), _ptr(a_edge), heads, float(negative_slope), _ptr(g), ldg, _ptr(z), ldz, _ptr(lse),
                                               _ptr(dadst), _ptr(dsum), _stream(y.device), _ptr(dedge) if nnz > 0 else None)
    _check(st, "isplib_gat_edge_bw_rows_hip")
    return dadst, dsum, dedge


def gat_edge_bw_cols(colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, g, lse, dsum, heads: int = 1, negative_slope: float = 0.2, *, out=None,
                     check: bool = True):
    """The backward of `gat_edge` over the columns (isplib_gat_edge_bw_cols_hip): `gat_bw_cols` with the per-edge term; `csr2csc`
    (int64 [nnz], what `csr2csc` returns and SparseStorage.csr2csc() caches) is the CSR position of every entry of the transposed
    structure, by which `a_edge` is gathered.  Returns (dy, d_a_src)."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    k = y.size(1)
    d = _gat_heads(heads, k)
    if not isinstance(g, torch.Tensor) or g.dim() != 2:
        raise ValueError("isplib_amd: `g` must be a 2-D tensor [m, heads * d]")
    m = g.size(0)
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    _gat_table(lse, "lse", m, heads)
    _gat_table(dsum, "dsum", m, heads)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    nnz = row_t.numel()
    csr2csc = _gat_edge_positions(csr2csc, nnz, check)
    _gat_table(a_edge, "a_edge", nnz, heads)
    if out is not None:
        lddy = _attn_dense(out[0], "out[0]", n, k, "dy")
        _gat_table(out[1], "out[1]", n, heads)
    _gat_domain(m, heads, d, ldg)
    _gat_edge_domain(nnz, heads)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("a_edge", a_edge), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr),
               ("row_t", row_t), ("csr2csc", csr2csc)) + ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        out = (torch.empty((n, k), dtype=torch.float32, device=y.device), torch.empty((n, heads), dtype=torch.float32, device=y.device))
        lddy = max(k, 1)
    dy, dasrc = out
    if n == 0 or k == 0:
        if k == 0 and n > 0:
            dasrc.zero_()
        return dy, dasrc
    cp = colptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_edge_bw_cols_hip(m, n, k, nnz, _ptr(row_t), ctypes.c_void_p(cp), ctypes.c_void_p(cp + 8), _ptr(csr2csc),
                                               _ptr(a_dst), _ptr(y), ldy, _ptr(a_src), _ptr(a_edge), heads, float(negative_slope), _ptr(g),
                                               ldg, _ptr(lse), _ptr(dsum), _ptr(dy), lddy, _ptr(dasrc), _stream(y.device))
    _check(st, "isplib_gat_edge_bw_cols_hip")
    return dy, dasrc


SEED_END = 2 ** 63                      # a dropout seed: a non-negative int64


def gat_drop_threshold_py(p: float) -> int:
    """T(p) = min(2^32 - 1, floor(p * 2^32)), the pure-Python mirror of isplib_gat_drop_threshold (p * 2^32 is exact in double)."""
    v = math.floor(float(p) * 4294967296.0) if p == p and p > 0 else 0
    return min(2 ** 32 - 1, max(0, int(v)))


def gat_drop_threshold(p: float) -> int:
    """isplib_gat_drop_threshold: the uint32 T(p) of the dropout keep bit, keep = word >= T."""
    return int(lib().isplib_gat_drop_threshold(float(p)))


def gat_drop_word(seed: int, pos: int, head: int) -> int:
    """isplib_gat_drop_word: the 32-bit word of (seed, CSR position, head) the kernels compare with T(p) (csrc/gat_dropout.h)."""
    return int(lib().isplib_gat_drop_word(int(seed), int(pos), int(head)))


def gat_drop_scale(p: float) -> float:
    """c = float32(1 / (1 - p)), as a Python float."""
    return struct.unpack("f", struct.pack("f", 1.0 / (1.0 - float(p))))[0]


def _gat_drop_args(threshold, scale, seed):
    if isinstance(threshold, bool) or not isinstance(threshold, int) or not 0 <= threshold < 2 ** 32:
        raise ValueError(f"isplib_amd: `threshold` must be an int in [0, 2^32), got {threshold!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < SEED_END:
        raise ValueError(f"isplib_amd: `seed` must be an int in [0, 2^63), got {seed!r}")
    scale = float(scale)
    if not (0.0 < scale < float("inf")):
        raise ValueError(f"isplib_amd: `scale` must be a positive finite number, got {scale!r}")
    return threshold, scale, seed


def gat_drop(rowptr, col, y, a_dst, a_src, a_edge, threshold: int, scale: float, seed: int, heads: int = 1, negative_slope: float = 0.2, *,
             out=None, check: bool = True):
    """`gat` / `gat_edge` (a_edge None or [nnz, heads]) with attention dropout (isplib_gat_drop_csr_hip): entry e and head h are kept where
    gat_drop_word(seed, e, h) >= threshold, and z is scaled by `scale`; lse is that of the call without dropout.  Returns (z, lse)."""
    threshold, scale, seed = _gat_drop_args(threshold, scale, seed)
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n, k = y.size(0), y.size(1)
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    d = _gat_heads(heads, k)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if a_edge is not None:
        _gat_table(a_edge, "a_edge", col.numel(), heads)
    if out is not None:
        z, lse = out
        ldz = _attn_dense(z, "out[0]", m, k, "z")
        _gat_table(lse, "out[1]", m, heads)
    _gat_domain(n, heads, d, ldy)
    if a_edge is not None:
        _gat_edge_domain(col.numel(), heads)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("rowptr", rowptr), ("col", col)) +
              ((("a_edge", a_edge),) if a_edge is not None else ()) + ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, k), dtype=torch.float32, device=y.device)
        lse = torch.empty((m, heads), dtype=torch.float32, device=y.device)
        ldz = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_drop_csr_hip(m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(a_dst), _ptr(y),
                                           ldy, _ptr(a_src), _ptr(a_edge) if a_edge is not None and col.numel() > 0 else None, heads,
                                           float(negative_slope), _ptr(z), ldz, _ptr(lse), _stream(y.device), threshold, scale, seed)
    _check(st, "isplib_gat_drop_csr_hip")
    return z, lse


def gat_drop_bw_rows(rowptr, col, y, a_dst, a_src, a_edge, g, z, lse, threshold: int, scale: float, seed: int, heads: int = 1,
                     negative_slope: float = 0.2, *, out=None, want_edge: bool = True, check: bool = True):
    """The backward of `gat_drop` over the rows (isplib_gat_drop_bw_rows_hip), with the mask of the same (threshold, seed).  Returns
    (d_a_dst, D, d_a_edge); d_a_edge is None without `a_edge` or with want_edge=False.  `out` = (d_a_dst, D, d_a_edge or None)."""
    threshold, scale, seed = _gat_drop_args(threshold, scale, seed)
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n, k = y.size(0), y.size(1)
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    d = _gat_heads(heads, k)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    ldz = _attn_dense(z, "z", m, k, "the forward's output")
    _gat_table(lse, "lse", m, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    nnz = col.numel()
    want_edge = want_edge and a_edge is not None
    if a_edge is not None:
        _gat_table(a_edge, "a_edge", nnz, heads)
    if out is not None:
        _gat_table(out[0], "out[0]", m, heads)
        _gat_table(out[1], "out[1]", m, heads)
        if out[2] is not None:
            if a_edge is None:
                raise ValueError("isplib_amd: `out[2]` (d_a_edge) needs `a_edge`")
            _gat_table(out[2], "out[2]", nnz, heads)
    _gat_domain(n, heads, d, ldy)
    if a_edge is not None:
        _gat_edge_domain(nnz, heads)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("g", g), ("z", z), ("lse", lse), ("rowptr", rowptr), ("col", col)) +
              ((("a_edge", a_edge),) if a_edge is not None else ()) +
              ((("out[0]", out[0]), ("out[1]", out[1]), ("out[2]", out[2])) if out is not None else ()))
    if out is None:
        out = (torch.empty((m, heads), dtype=torch.float32, device=y.device), torch.empty((m, heads), dtype=torch.float32, device=y.device),
               torch.empty((nnz, heads), dtype=torch.float32, device=y.device) if want_edge else None)
    dadst, dsum, dedge = out
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            dadst.zero_()
            dsum.zero_()
            if dedge is not None:
                dedge.zero_()
        return dadst, dsum, dedge
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_drop_bw_rows_hip(m, n, k, nnz, _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(a_dst), _ptr(y), ldy,
                                               _ptr(a_src), _ptr(a_edge) if a_edge is not None and nnz > 0 else None, heads,
                                               float(negative_slope), _ptr(g), ldg, _ptr(z), ldz, _ptr(lse), _ptr(dadst), _ptr(dsum),
                                               _stream(y.device), _ptr(dedge) if dedge is not None and nnz > 0 else None, threshold, scale,
                                               seed)
    _check(st, "isplib_gat_drop_bw_rows_hip")
    return dadst, dsum, dedge


def gat_drop_bw_cols(colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, g, lse, dsum, threshold: int, scale: float, seed: int, heads: int = 1,
                     negative_slope: float = 0.2, *, out=None, check: bool = True):
    """The backward of `gat_drop` over the columns (isplib_gat_drop_bw_cols_hip); `csr2csc` is required with or without `a_edge`: the
    keep bit is a function of the entry's CSR position.  Returns (dy, d_a_src)."""
    threshold, scale, seed = _gat_drop_args(threshold, scale, seed)
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    k = y.size(1)
    d = _gat_heads(heads, k)
    if not isinstance(g, torch.Tensor) or g.dim() != 2:
        raise ValueError("isplib_amd: `g` must be a 2-D tensor [m, heads * d]")
    m = g.size(0)
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    _gat_table(lse, "lse", m, heads)
    _gat_table(dsum, "dsum", m, heads)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    nnz = row_t.numel()
    csr2csc = _gat_edge_positions(csr2csc, nnz, check)
    if a_edge is not None:
        _gat_table(a_edge, "a_edge", nnz, heads)
    if out is not None:
        lddy = _attn_dense(out[0], "out[0]", n, k, "dy")
        _gat_table(out[1], "out[1]", n, heads)
    _gat_domain(m, heads, d, ldg)
    if a_edge is not None:
        _gat_edge_domain(nnz, heads)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t),
               ("csr2csc", csr2csc)) + ((("a_edge", a_edge),) if a_edge is not None else ()) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        out = (torch.empty((n, k), dtype=torch.float32, device=y.device), torch.empty((n, heads), dtype=torch.float32, device=y.device))
        lddy = max(k, 1)
    dy, dasrc = out
    if n == 0 or k == 0:
        if k == 0 and n > 0:
            dasrc.zero_()
        return dy, dasrc
    cp = colptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat_drop_bw_cols_hip(m, n, k, nnz, _ptr(row_t), ctypes.c_void_p(cp), ctypes.c_void_p(cp + 8), _ptr(csr2csc),
                                               _ptr(a_dst), _ptr(y), ldy, _ptr(a_src), _ptr(a_edge) if a_edge is not None and nnz > 0 else None,
                                               heads, float(negative_slope), _ptr(g), ldg, _ptr(lse), _ptr(dsum), _ptr(dy), lddy, _ptr(dasrc),
                                               _stream(y.device), threshold, scale, seed)
    _check(st, "isplib_gat_drop_bw_cols_hip")
    return dy, dasrc


def _gatv2_att(att, name: str, heads: int, d: int) -> None:
    """The attention vector of the GATv2 entries: a contiguous float32 [heads, d] tensor (k floats)."""
    if not isinstance(att, torch.Tensor) or att.dim() != 2:
        raise ValueError(f"isplib_amd: `{name}` must be a 2-D tensor [{heads}, {d}], got "
                         f"{tuple(att.shape) if isinstance(att, torch.Tensor) else type(att).__name__}")
    if att.dtype != torch.float32:
        raise TypeError(f"isplib_amd: `{name}` must be float32, got {att.dtype} (the attention operator is fp32 only)")
    if att.size(0) != heads or att.size(1) != d:
        raise ValueError(f"isplib_amd: `{name}` must be [{heads}, {d}] (heads x d), got {tuple(att.shape)}")
    if not att.is_contiguous():
        raise ValueError(f"isplib_amd: `{name}` must be contiguous (k floats)")


def _gatv2_domain(rows_gathered: int, heads: int, d: int, lds) -> None:
    for ld in lds:
        if d > 0 and not gatv2_serves(rows_gathered, heads, d, ld):
            raise ValueError(f"isplib_amd: outside the GATv2 entries' domain (isplib_gatv2_serves = isplib_gat_serves: heads * d <= {GAT_K_MAX}, "
                             f"heads == 1 or d a power of two >= 4, gathered rows < 2^31, rows * pitch * 4 <= 3.5 GiB), got "
                             f"rows={rows_gathered}, heads={heads}, d={d}, pitch={ld}")


def gatv2_bw_rows_workspace_bytes(m: int, k: int) -> int:
    """isplib_gatv2_bw_rows_workspace_bytes: what `gatv2_bw_rows` needs behind `workspace` when `datt` is asked for."""
    return int(lib().isplib_gatv2_bw_rows_workspace_bytes(int(m), int(k)))


def gatv2(rowptr, col, x, y, att, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """GATv2 attention aggregation, all heads in one launch (isplib_gatv2_csr_hip): over the stored entries e = (i, j) of the CSR
    structure and every head h, s_e = sum over the head's columns of att_c leaky_relu(x_ic + y_jc), a_e = softmax of s over the row's
    entries, z_i[head h] = sum_e a_e y_j[head h].  Returns (z [m, heads * d], lse [m, heads]); an empty row has z_i = 0 and lse = -inf.
    `x` [m, heads * d] and `y` [n, heads * d] float32 (row-strided views keep their pitch), `att` [heads, d] contiguous float32; `out` =
    (z, lse) to write in place.  Every operand is checked BEFORE the call (`check`: also the two checks that read the structure on the
    device)."""
    return _gatv2_forward(rowptr, col, x, y, att, heads, negative_slope, out, check, None)


def _gatv2_nnz(nnz: int) -> None:
    if nnz >= 2 ** 31:
        raise ValueError(f"isplib_amd: the dropout keep bit is defined for fewer than 2^31 stored entries, got {nnz}")


def _gatv2_forward(rowptr, col, x, y, att, heads, negative_slope, out, check, drop):
    """`gatv2` (drop None) and `gatv2_drop` (drop = (threshold, scale, seed), checked): one set of operand checks, all before the call."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    ldx = _attn_dense(x, "x", m, None, "one row per row of the sparse operand")
    k = x.size(1)
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n = y.size(0)
    ldy = _attn_dense(y, "y", n, k, "one row per column of the sparse operand, x's width")
    d = _gat_heads(heads, k)
    _gatv2_att(att, "att", heads, d)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if drop is not None:
        _gatv2_nnz(col.numel())
    if out is not None:
        z, lse = out
        ldz = _attn_dense(z, "out[0]", m, k, "z")
        _gat_table(lse, "out[1]", m, heads)
    _gatv2_domain(n, heads, d, (ldy,))
    _same_gpu((("x", x), ("y", y), ("att", att), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, k), dtype=torch.float32, device=x.device)
        lse = torch.empty((m, heads), dtype=torch.float32, device=x.device)
        ldz = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    entry = "isplib_gatv2_csr_hip" if drop is None else "isplib_gatv2_drop_csr_hip"
    with torch.cuda.device(x.device):
        st = getattr(lib(), entry)(m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(x), ldx, _ptr(y), ldy,
                                   _ptr(att), heads, float(negative_slope), _ptr(z), ldz, _ptr(lse), _stream(x.device), *(drop or ()))
    _check(st, entry)
    return z, lse


def gatv2_drop(rowptr, col, x, y, att, threshold: int, scale: float, seed: int, heads: int = 1, negative_slope: float = 0.2, *, out=None,
               check: bool = True):
    """`gatv2` with attention dropout (isplib_gatv2_drop_csr_hip): entry e (its position in `col`) and head h are kept where
    gat_drop_word(seed, e, h) >= threshold -- the keep bit of `gat_drop` -- and z is scaled by `scale`; lse is that of the call without
    dropout.  Returns (z, lse); the operand checks are gatv2's, and nnz < 2^31."""
    return _gatv2_forward(rowptr, col, x, y, att, heads, negative_slope, out, check, _gat_drop_args(threshold, scale, seed))


def gatv2_bw_rows(rowptr, col, x, y, att, g, z, lse, heads: int = 1, negative_slope: float = 0.2, *, want_datt: bool = True, out=None,
                  workspace=None, check: bool = True):
    """The backward of `gatv2` over the rows (isplib_gatv2_bw_rows_hip): for g = dL/dz [m, heads * d] and the forward's z and lse,
    D[i,h] = <g_i, z_i>_h, ds_e = a_e (<g_i, y_j>_h - D[i,h]) with a_e recomputed from lse, dx_ic = sum_e ds_e att_c sl_ec and, with
    `want_datt`, datt_c = sum over every edge of ds_e v_ec.  Returns (dx [m, heads * d], D [m, heads], datt [heads, d] or None); an empty
    row has dx_i = 0 and D = 0.  `out` = (dx, D, datt or None); `workspace`: a uint8 GPU tensor of at least
    gatv2_bw_rows_workspace_bytes(m, k) bytes (allocated when None); the operand checks are gatv2's."""
    return _gatv2_backward_rows(rowptr, col, x, y, att, g, z, lse, heads, negative_slope, want_datt, out, workspace, check, None)


def _gatv2_backward_rows(rowptr, col, x, y, att, g, z, lse, heads, negative_slope, want_datt, out, workspace, check, drop):
    """`gatv2_bw_rows` (drop None) and `gatv2_drop_bw_rows` (drop = (threshold, scale, seed), checked)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    ldx = _attn_dense(x, "x", m, None, "one row per row of the sparse operand")
    k = x.size(1)
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n = y.size(0)
    ldy = _attn_dense(y, "y", n, k, "one row per column of the sparse operand, x's width")
    d = _gat_heads(heads, k)
    _gatv2_att(att, "att", heads, d)
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    ldz = _attn_dense(z, "z", m, k, "the forward's output")
    _gat_table(lse, "lse", m, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if drop is not None:
        _gatv2_nnz(col.numel())
    if out is not None:
        if len(out) != 3:
            raise ValueError("isplib_amd: `out` must be (dx, D, datt or None)")
        lddx = _attn_dense(out[0], "out[0]", m, k, "dx")
        _gat_table(out[1], "out[1]", m, heads)
        if (out[2] is not None) != bool(want_datt):
            raise ValueError("isplib_amd: `out[2]` (datt) must be given exactly when `want_datt`")
        if out[2] is not None:
            _gatv2_att(out[2], "out[2]", heads, d)
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
            raise ValueError("isplib_amd: `workspace` must be a contiguous 1-D uint8 tensor")
    _gatv2_domain(n, heads, d, (ldy,))
    _same_gpu((("x", x), ("y", y), ("att", att), ("g", g), ("z", z), ("lse", lse), ("rowptr", rowptr), ("col", col), ("workspace", workspace)) +
              ((("out[0]", out[0]), ("out[1]", out[1]), ("out[2]", out[2])) if out is not None else ()))
    if out is None:
        out = (torch.empty((m, k), dtype=torch.float32, device=x.device), torch.empty((m, heads), dtype=torch.float32, device=x.device),
               torch.empty((heads, d), dtype=torch.float32, device=x.device) if want_datt else None)
        lddx = max(k, 1)
    dx, dsum, datt = out
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            dsum.zero_()
        if datt is not None:
            datt.zero_()
        return dx, dsum, datt
    rp = rowptr.data_ptr()
    entry = "isplib_gatv2_bw_rows_hip" if drop is None else "isplib_gatv2_drop_bw_rows_hip"
    with torch.cuda.device(x.device):
        if datt is not None:
            need = gatv2_bw_rows_workspace_bytes(m, k)
            if workspace is None:
                workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=x.device)
            elif workspace.numel() < need:
                raise ValueError(f"isplib_amd: `workspace` holds {workspace.numel()} bytes, isplib_gatv2_bw_rows_workspace_bytes asks for {need}")
        st = getattr(lib(), entry)(m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), _ptr(x), ldx, _ptr(y), ldy,
                                   _ptr(att), heads, float(negative_slope), _ptr(g), ldg, _ptr(z), ldz, _ptr(lse), _ptr(dx), lddx, _ptr(dsum),
                                   _ptr(datt), _ptr(workspace) if datt is not None else None,
                                   workspace.numel() if datt is not None else 0, _stream(x.device), *(drop or ()))
    _check(st, entry)
    return dx, dsum, datt


def gatv2_drop_bw_rows(rowptr, col, x, y, att, g, z, lse, threshold: int, scale: float, seed: int, heads: int = 1,
                       negative_slope: float = 0.2, *, want_datt: bool = True, out=None, workspace=None, check: bool = True):
    """The backward of `gatv2_drop` over the rows (isplib_gatv2_drop_bw_rows_hip), with the mask of the same (threshold, seed):
    t_e = q_e scale <g_i, y_j>_h, everything else as `gatv2_bw_rows` (z is the forward's, under the mask).  Returns (dx, D, datt or None)."""
    return _gatv2_backward_rows(rowptr, col, x, y, att, g, z, lse, heads, negative_slope, want_datt, out, workspace, check,
                                _gat_drop_args(threshold, scale, seed))


def gatv2_bw_cols(colptr, row_t, x, y, att, g, lse, dsum, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """The backward of `gatv2` over the columns (isplib_gatv2_bw_cols_hip), on the transposed structure (`colptr` [n + 1], `row_t`: the
    row ids of the entries in column-major order): dy_jc = sum over the entries e = (i, j) of column j of a_e g_ic + ds_e att_c sl_ec,
    with `lse` of the forward and `dsum` = D of gatv2_bw_rows.  Returns dy [n, heads * d]; a column no entry points at has 0.  `out` =
    dy; the operand checks are gatv2's."""
    return _gatv2_backward_cols(colptr, row_t, None, x, y, att, g, lse, dsum, heads, negative_slope, out, check, None)


def _gatv2_backward_cols(colptr, row_t, csr2csc, x, y, att, g, lse, dsum, heads, negative_slope, out, check, drop):
    """`gatv2_bw_cols` (drop None, no csr2csc) and `gatv2_drop_bw_cols` (drop = (threshold, scale, seed), checked; csr2csc required)."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldy = _attn_dense(y, "y", n, None, "one row per column of the sparse operand")
    k = y.size(1)
    d = _gat_heads(heads, k)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("isplib_amd: `x` must be a 2-D tensor [m, heads * d]")
    m = x.size(0)
    ldx = _attn_dense(x, "x", m, k, "one row per row of the sparse operand, y's width")
    ldg = _attn_dense(g, "g", m, k, "the gradient of z")
    _gatv2_att(att, "att", heads, d)
    _gat_table(lse, "lse", m, heads)
    _gat_table(dsum, "dsum", m, heads)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    if drop is not None:
        _gatv2_nnz(row_t.numel())
        csr2csc = _gat_edge_positions(csr2csc, row_t.numel(), check)
    if out is not None:
        lddy = _attn_dense(out, "out", n, k, "dy")
    _gatv2_domain(m, heads, d, (ldx, ldg))
    _same_gpu((("x", x), ("y", y), ("att", att), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t), ("out", out)) +
              ((("csr2csc", csr2csc),) if drop is not None else ()))
    if out is None:
        out = torch.empty((n, k), dtype=torch.float32, device=y.device)
        lddy = max(k, 1)
    if n == 0 or k == 0:
        return out
    cp = colptr.data_ptr()
    entry = "isplib_gatv2_bw_cols_hip" if drop is None else "isplib_gatv2_drop_bw_cols_hip"
    with torch.cuda.device(y.device):
        st = getattr(lib(), entry)(m, n, k, row_t.numel(), _ptr(row_t), ctypes.c_void_p(cp), ctypes.c_void_p(cp + 8),
                                   *((_ptr(csr2csc),) if drop is not None else ()), _ptr(x), ldx, _ptr(y), ldy, _ptr(att), heads,
                                   float(negative_slope), _ptr(g), ldg, _ptr(lse), _ptr(dsum), _ptr(out), lddy, _stream(y.device),
                                   *(drop or ()))
    _check(st, entry)
    return out


def gatv2_drop_bw_cols(colptr, row_t, csr2csc, x, y, att, g, lse, dsum, threshold: int, scale: float, seed: int, heads: int = 1,
                       negative_slope: float = 0.2, *, out=None, check: bool = True):
    """The backward of `gatv2_drop` over the columns (isplib_gatv2_drop_bw_cols_hip): dy_jc = sum over the entries of column j of
    q_e scale a_e g_ic + r_ec.  `csr2csc` [nnz] int64 is required: the keep bit is a function of the entry's CSR position, and this
    entry walks the transposed structure.  Returns dy."""
    return _gatv2_backward_cols(colptr, row_t, csr2csc, x, y, att, g, lse, dsum, heads, negative_slope, out, check,
                                _gat_drop_args(threshold, scale, seed))


def _mha_domain(rows_gathered: int, heads: int, d: int, lds) -> None:
    for ld in lds:
        if d > 0 and not mha_serves(rows_gathered, heads, d, ld):
            raise ValueError(f"isplib_amd: outside the multi-head attention entries' domain (isplib_mha_serves = isplib_gat_serves: heads * d <= "
                             f"{GAT_K_MAX}, heads == 1 or d a power of two >= 4, gathered rows < 2^31, rows * pitch * 4 <= 3.5 GiB), got "
                             f"rows={rows_gathered}, heads={heads}, d={d}, pitch={ld}")


def _mha_scale(scale, d: int) -> float:
    """The scale of the scores: a finite Python number, or None for 1 / sqrt(d) -- the HEAD width, not k."""
    if scale is None:
        return 1.0 / float(d) ** 0.5 if d > 0 else 1.0
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
        raise ValueError(f"isplib_amd: `scale` must be a finite number or None, got {scale!r}")
    return float(scale)


def _mha_qkv(m: int, q, k, v):
    """q [m, K] and k, v [n, K] of the multi-head entries; returns (n, K, ldq, ldk, ldv)."""
    ldq = _attn_dense(q, "q", m, None, "one row per row of the sparse operand")
    kk = q.size(1)
    if not isinstance(k, torch.Tensor) or k.dim() != 2:
        raise ValueError("isplib_amd: `k` must be a 2-D tensor [n, heads * d]")
    n = k.size(0)
    ldk = _attn_dense(k, "k", n, kk, "one row per column of the sparse operand, q's width")
    ldv = _attn_dense(v, "v", n, kk, "one row per column of the sparse operand, q's width")
    return n, kk, ldq, ldk, ldv


def mha(rowptr, col, q, k, v, heads: int = 1, scale: Optional[float] = None, *, out=None, check: bool = True):
    """Sparse multi-head dot-product attention with separate keys and values, all heads in one launch (isplib_mha_csr_hip): over the
    stored entries e = (i, j) of the CSR structure and every head h, s_e = scale <q_i, k_j>_h, a_e = softmax of s over the row's entries,
    z_i[head h] = sum_e a_e v_j[head h].  Returns (z [m, heads * d], lse [m, heads]); an empty row has z_i = 0 and lse = -inf.  `q`
    [m, heads * d], `k` and `v` [n, heads * d] float32 (row-strided views keep their pitch: column views of one fused projection go in
    without a copy); `scale` None: 1 / sqrt(d); `out` = (z, lse) to write in place.  Every operand is checked BEFORE the call
    (`check`: also the two checks that read the structure on the device)."""
    return _mha_forward(rowptr, col, q, k, v, heads, scale, out, check, None)


def _mha_drop_args(threshold, keep_scale, seed):
    """(threshold, keep_scale, seed) of the isplib_qkv_drop_* entries, checked: the ranges of `_gat_drop_args`, under this family's names."""
    if isinstance(keep_scale, bool) or not isinstance(keep_scale, (int, float)) or not 0.0 < float(keep_scale) < float("inf"):
        raise ValueError(f"isplib_amd: `keep_scale` must be a positive finite number, got {keep_scale!r}")
    return _gat_drop_args(threshold, keep_scale, seed)


def _mha_forward(rowptr, col, q, k, v, heads, scale, out, check, drop):
    """`mha` (drop None) and `mha_drop` (drop = (threshold, keep_scale, seed), checked): one set of operand checks, all before the call."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    n, kk, ldq, ldk, ldv = _mha_qkv(m, q, k, v)
    d = _gat_heads(heads, kk)
    p = _mha_scale(scale, d)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if drop is not None:
        _gatv2_nnz(col.numel())
    if out is not None:
        z, lse = out
        ldz = _attn_dense(z, "out[0]", m, kk, "z")
        _gat_table(lse, "out[1]", m, heads)
    _mha_domain(n, heads, d, (ldk, ldv))
    _same_gpu((("q", q), ("k", k), ("v", v), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, kk), dtype=torch.float32, device=q.device)
        lse = torch.empty((m, heads), dtype=torch.float32, device=q.device)
        ldz = max(kk, 1)
    if m == 0 or kk == 0:
        if kk == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    entry = "isplib_mha_csr_hip" if drop is None else "isplib_qkv_drop_csr_hip"
    with torch.cuda.device(q.device):
        st = getattr(lib(), entry)(m, n, kk, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), heads, p, _ptr(q), ldq,
                                   _ptr(k), ldk, _ptr(v), ldv, _ptr(z), ldz, _ptr(lse), _stream(q.device), *(drop or ()))
    _check(st, entry)
    return z, lse


def mha_drop(rowptr, col, q, k, v, threshold: int, keep_scale: float, seed: int, heads: int = 1, scale: Optional[float] = None, *,
             out=None, check: bool = True):
    """`mha` with attention dropout (isplib_qkv_drop_csr_hip): entry e (its position in `col`) and head h are kept where
    gat_drop_word(seed, e, h) >= threshold -- the keep bit of `gat_drop` and `gatv2_drop` -- and z is scaled by `keep_scale`; lse is
    that of the call without dropout.  Returns (z, lse); the operand checks are mha's, and nnz < 2^31."""
    return _mha_forward(rowptr, col, q, k, v, heads, scale, out, check, _mha_drop_args(threshold, keep_scale, seed))


def mha_bw_rows(rowptr, col, q, k, v, g, z, lse, heads: int = 1, scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `mha` over the rows (isplib_mha_bw_rows_hip): for g = dL/dz [m, heads * d] and the forward's z and lse,
    D[i,h] = <g_i, z_i>_h, ds_e = a_e (<g_i, v_j>_h - D[i,h]) with a_e recomputed from lse, dq_i[head h] = scale sum_e ds_e k_j[head h].
    Returns (dq [m, heads * d], D [m, heads]); an empty row has dq_i = 0 and D = 0.  `out` = (dq, D); the operand checks are mha's."""
    return _mha_backward_rows(rowptr, col, q, k, v, g, z, lse, heads, scale, out, check, None)


def _mha_backward_rows(rowptr, col, q, k, v, g, z, lse, heads, scale, out, check, drop):
    """`mha_bw_rows` (drop None) and `mha_drop_bw_rows` (drop = (threshold, keep_scale, seed), checked)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    n, kk, ldq, ldk, ldv = _mha_qkv(m, q, k, v)
    d = _gat_heads(heads, kk)
    p = _mha_scale(scale, d)
    ldg = _attn_dense(g, "g", m, kk, "the gradient of z")
    ldz = _attn_dense(z, "z", m, kk, "the forward's output")
    _gat_table(lse, "lse", m, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if drop is not None:
        _gatv2_nnz(col.numel())
    if out is not None:
        if len(out) != 2:
            raise ValueError("isplib_amd: `out` must be (dq, D)")
        lddq = _attn_dense(out[0], "out[0]", m, kk, "dq")
        _gat_table(out[1], "out[1]", m, heads)
    _mha_domain(n, heads, d, (ldk, ldv))
    _same_gpu((("q", q), ("k", k), ("v", v), ("g", g), ("z", z), ("lse", lse), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        out = (torch.empty((m, kk), dtype=torch.float32, device=q.device), torch.empty((m, heads), dtype=torch.float32, device=q.device))
        lddq = max(kk, 1)
    dq, dsum = out
    if m == 0 or kk == 0:
        if kk == 0 and m > 0:
            dsum.zero_()
        return dq, dsum
    rp = rowptr.data_ptr()
    entry = "isplib_mha_bw_rows_hip" if drop is None else "isplib_qkv_drop_bw_rows_hip"
    with torch.cuda.device(q.device):
        st = getattr(lib(), entry)(m, n, kk, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8), heads, p, _ptr(q), ldq,
                                   _ptr(k), ldk, _ptr(v), ldv, _ptr(g), ldg, _ptr(z), ldz, _ptr(lse), _ptr(dq), lddq, _ptr(dsum),
                                   _stream(q.device), *(drop or ()))
    _check(st, entry)
    return dq, dsum


def mha_drop_bw_rows(rowptr, col, q, k, v, g, z, lse, threshold: int, keep_scale: float, seed: int, heads: int = 1,
                     scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `mha_drop` over the rows (isplib_qkv_drop_bw_rows_hip), with the mask of the same (threshold, seed):
    t_e = q_e keep_scale <g_i, v_j>_h, everything else as `mha_bw_rows` (z is the forward's, under the mask).  Returns (dq, D)."""
    return _mha_backward_rows(rowptr, col, q, k, v, g, z, lse, heads, scale, out, check, _mha_drop_args(threshold, keep_scale, seed))


def mha_bw_cols(colptr, row_t, q, k, v, g, lse, dsum, heads: int = 1, scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `mha` over the columns (isplib_mha_bw_cols_hip), on the transposed structure (`colptr` [n + 1], `row_t`: the row
    ids of the entries in column-major order): dk_j[head h] = scale sum over the entries e = (i, j) of column j of ds_e q_i[head h] and
    dv_j[head h] = sum of a_e g_i[head h], with `lse` of the forward and `dsum` = D of mha_bw_rows.  Returns (dk, dv), both
    [n, heads * d]; a column no entry points at has 0 in both.  `out` = (dk, dv); the operand checks are mha's."""
    return _mha_backward_cols(colptr, row_t, None, q, k, v, g, lse, dsum, heads, scale, out, check, None)


def _mha_backward_cols(colptr, row_t, csr2csc, q, k, v, g, lse, dsum, heads, scale, out, check, drop):
    """`mha_bw_cols` (drop None, no csr2csc) and `mha_drop_bw_cols` (drop = (threshold, keep_scale, seed), checked; csr2csc required)."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldk = _attn_dense(k, "k", n, None, "one row per column of the sparse operand")
    kk = k.size(1)
    ldv = _attn_dense(v, "v", n, kk, "one row per column of the sparse operand, k's width")
    d = _gat_heads(heads, kk)
    p = _mha_scale(scale, d)
    if not isinstance(q, torch.Tensor) or q.dim() != 2:
        raise ValueError("isplib_amd: `q` must be a 2-D tensor [m, heads * d]")
    m = q.size(0)
    ldq = _attn_dense(q, "q", m, kk, "one row per row of the sparse operand, k's width")
    ldg = _attn_dense(g, "g", m, kk, "the gradient of z")
    _gat_table(lse, "lse", m, heads)
    _gat_table(dsum, "dsum", m, heads)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    if drop is not None:
        _gatv2_nnz(row_t.numel())
        csr2csc = _gat_edge_positions(csr2csc, row_t.numel(), check)
    if out is not None:
        if len(out) != 2:
            raise ValueError("isplib_amd: `out` must be (dk, dv)")
        lddk = _attn_dense(out[0], "out[0]", n, kk, "dk")
        lddv = _attn_dense(out[1], "out[1]", n, kk, "dv")
    _mha_domain(m, heads, d, (ldq, ldg))
    _same_gpu((("q", q), ("k", k), ("v", v), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()) + ((("csr2csc", csr2csc),) if drop is not None else ()))
    if out is None:
        out = (torch.empty((n, kk), dtype=torch.float32, device=k.device), torch.empty((n, kk), dtype=torch.float32, device=k.device))
        lddk = lddv = max(kk, 1)
    dk, dv = out
    if n == 0 or kk == 0:
        return dk, dv
    cp = colptr.data_ptr()
    entry = "isplib_mha_bw_cols_hip" if drop is None else "isplib_qkv_drop_bw_cols_hip"
    with torch.cuda.device(k.device):
        st = getattr(lib(), entry)(m, n, kk, row_t.numel(), _ptr(row_t), ctypes.c_void_p(cp), ctypes.c_void_p(cp + 8),
                                   *((_ptr(csr2csc),) if drop is not None else ()), heads, p, _ptr(q), ldq, _ptr(g), ldg, _ptr(lse),
                                   _ptr(dsum), _ptr(k), ldk, _ptr(v), ldv, _ptr(dk), lddk, _ptr(dv), lddv, _stream(k.device),
                                   *(drop or ()))
    _check(st, entry)
    return dk, dv


def mha_drop_bw_cols(colptr, row_t, csr2csc, q, k, v, g, lse, dsum, threshold: int, keep_scale: float, seed: int, heads: int = 1,
                     scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `mha_drop` over the columns (isplib_qkv_drop_bw_cols_hip): dk as `mha_bw_cols` with t_e under the mask, dv_j[head h]
    = sum over the entries of column j of q_e keep_scale a_e g_i[head h].  `csr2csc` [nnz] int64 is required: the keep bit is a function of
    the entry's CSR position, and this entry walks the transposed structure.  Returns (dk, dv)."""
    return _mha_backward_cols(colptr, row_t, csr2csc, q, k, v, g, lse, dsum, heads, scale, out, check,
                              _mha_drop_args(threshold, keep_scale, seed))


def _attn16_dense(t, name: str, rows: int, k: Optional[int], what: str, dtype=None) -> int:
    """One dense operand of the 16-bit attention entries: 2-D bf16 / fp16 [rows, k] (of `dtype` when given: every operand of a call
    has x's) on the GPU with unit inner stride, an even pitch and a 4-byte aligned base; a row-strided view keeps its pitch.  Returns
    the pitch in elements."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"isplib_amd: `{name}` must be a 2-D tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dtype not in HALF_DTYPES or (dtype is not None and t.dtype != dtype):
        raise TypeError(f"isplib_amd: `{name}` must be {dtype or 'bfloat16 or float16'}, got {t.dtype} (float32 operands: cabi.attention)")
    if t.size(0) != rows or (k is not None and t.size(1) != k):
        raise ValueError(f"isplib_amd: `{name}` must be [{rows}, {'k' if k is None else k}] ({what}), got {tuple(t.shape)}")
    if t.size(1) > 0 and t.size(0) > 0 and t.stride(1) != 1:
        raise ValueError(f"isplib_amd: `{name}` must have unit inner stride")
    ld = t.stride(0) if t.size(0) > 1 else max(t.size(1), t.stride(0))
    if ld < t.size(1):
        raise ValueError(f"isplib_amd: the rows of `{name}` (pitch {ld}) must not overlap: k = {t.size(1)}")
    if t.numel() > 0 and (ld % 2 or t.data_ptr() % 4):
        raise ValueError(f"isplib_amd: `{name}` needs an even pitch (got {ld}) and a 4-byte aligned base (the 16-bit attention entries)")
    return int(ld)


def _attn16_domain(rows_gathered: int, k: int, lds) -> None:
    for ld in lds:
        if k > 0 and not attention16_serves(rows_gathered, k, ld):
            raise ValueError(f"isplib_amd: outside the 16-bit attention entries' domain (isplib_attention16_serves: {ATTENTION16_K_MIN} <= k <= "
                             f"{ATTENTION16_K_MAX}, k and the pitch even, gathered rows < 2^31, rows * pitch * 2 <= 3.5 GiB), got "
                             f"rows={rows_gathered}, k={k}, pitch={ld}")


def attention16(rowptr, col, x, y, scale: Optional[float] = None, *, out=None, check: bool = True):
    """`attention` for bf16 / fp16 operands (isplib_attention16_csr_hip): x [m, k] and y [n, k] of one 16-bit dtype go in as they lie,
    every product, sum and exponential is fp32, z is rounded once to the operands' dtype.  Returns (z [m, k] 16-bit, lse [m] fp32);
    `out` = (z, lse).  The operand checks are attention's, with the 16-bit family's (even k and pitches, 4-byte aligned bases)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    ldx = _attn16_dense(x, "x", m, None, "one row per row of the sparse operand")
    k = x.size(1)
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, k]")
    n = y.size(0)
    ldy = _attn16_dense(y, "y", n, k, "x's width", x.dtype)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        z, lse = out
        ldz = _attn16_dense(z, "out[0]", m, k, "z", x.dtype)
        _attn_vector(lse, "out[1]", m)
    _attn16_domain(n, k, (ldy,))
    _same_gpu((("x", x), ("y", y), ("rowptr", rowptr), ("col", col)) + ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, k), dtype=x.dtype, device=x.device)
        lse = torch.empty(m, dtype=torch.float32, device=x.device)
        ldz = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    with torch.cuda.device(x.device):
        st = lib().isplib_attention16_csr_hip(HALF_DTYPES[x.dtype], m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                              _ptr(x), ldx, _ptr(y), ldy, _attn_scale(scale, k), _ptr(z), ldz, _ptr(lse), _stream(x.device))
    _check(st, "isplib_attention16_csr_hip")
    return z, lse


def attention16_bw_rows(rowptr, col, x, y, g, lse, scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `attention16` over the rows (isplib_attention16_bw_rows_hip): for g = dL/dz [m, k] (the operands' dtype) and the
    forward's lse -- z is NOT read: D_i = sum_e a_e <g_i, y_j> is formed in fp32 from the row's edges -- returns (dx [m, k] 16-bit,
    D [m] fp32).  `out` = (dx, D); the operand checks are attention16's."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    ldx = _attn16_dense(x, "x", m, None, "one row per row of the sparse operand")
    k = x.size(1)
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, k]")
    n = y.size(0)
    ldy = _attn16_dense(y, "y", n, k, "x's width", x.dtype)
    ldg = _attn16_dense(g, "g", m, k, "the gradient of z", x.dtype)
    _attn_vector(lse, "lse", m)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        dx, dsum = out
        lddx = _attn16_dense(dx, "out[0]", m, k, "dx", x.dtype)
        _attn_vector(dsum, "out[1]", m)
    _attn16_domain(n, k, (ldy,))
    _same_gpu((("x", x), ("y", y), ("g", g), ("lse", lse), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        dx = torch.empty((m, k), dtype=x.dtype, device=x.device)
        dsum = torch.empty(m, dtype=torch.float32, device=x.device)
        lddx = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            dsum.zero_()
        return dx, dsum
    rp = rowptr.data_ptr()
    with torch.cuda.device(x.device):
        st = lib().isplib_attention16_bw_rows_hip(HALF_DTYPES[x.dtype], m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp),
                                                  ctypes.c_void_p(rp + 8), _ptr(x), ldx, _ptr(y), ldy, _attn_scale(scale, k), _ptr(g), ldg,
                                                  _ptr(lse), _ptr(dx), lddx, _ptr(dsum), _stream(x.device))
    _check(st, "isplib_attention16_bw_rows_hip")
    return dx, dsum


def attention16_bw_cols(colptr, row_t, x, y, g, lse, dsum, scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `attention16` over the columns (isplib_attention16_bw_cols_hip), on the transposed structure: dy_j = sum over the
    entries e = (i, j) of column j of a_e g_i + scale ds_e x_i, with `lse` of the forward and `dsum` = D of attention16_bw_rows (both
    fp32).  Returns dy [n, k] in the operands' dtype; `out` = dy; the operand checks are attention16's."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldy = _attn16_dense(y, "y", n, None, "one row per column of the sparse operand")
    k = y.size(1)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("isplib_amd: `x` must be a 2-D tensor [m, k]")
    m = x.size(0)
    ldx = _attn16_dense(x, "x", m, k, "y's width", y.dtype)
    ldg = _attn16_dense(g, "g", m, k, "the gradient of z", y.dtype)
    _attn_vector(lse, "lse", m)
    _attn_vector(dsum, "dsum", m)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    if out is not None:
        lddy = _attn16_dense(out, "out", n, k, "dy", y.dtype)
    _attn16_domain(m, k, (ldx, ldg))
    _same_gpu((("x", x), ("y", y), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t), ("out", out)))
    if out is None:
        out = torch.empty((n, k), dtype=y.dtype, device=y.device)
        lddy = max(k, 1)
    if n == 0 or k == 0:
        return out
    cp = colptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_attention16_bw_cols_hip(HALF_DTYPES[y.dtype], m, n, k, row_t.numel(), _ptr(row_t), ctypes.c_void_p(cp),
                                                  ctypes.c_void_p(cp + 8), _ptr(x), ldx, _ptr(y), ldy, _attn_scale(scale, k), _ptr(g), ldg,
                                                  _ptr(lse), _ptr(dsum), _ptr(out), lddy, _stream(y.device))
    _check(st, "isplib_attention16_bw_cols_hip")
    return out


def _gat16_domain(rows_gathered: int, heads: int, d: int, ld: int) -> None:
    if d > 0 and not gat16_serves(rows_gathered, heads, d, ld):
        raise ValueError(f"isplib_amd: outside the 16-bit GAT entries' domain (isplib_gat16_serves: {GAT16_K_MIN} <= heads * d <= {GAT16_K_MAX}, "
                         f"heads == 1 with d even or d a power of two >= 8, the pitch even, gathered rows < 2^31, rows * pitch * 2 <= 3.5 GiB), "
                         f"got rows={rows_gathered}, heads={heads}, d={d}, pitch={ld}")


def gat16_forward(rowptr, col, y, a_dst, a_src, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """`gat` for a bf16 / fp16 `y` (isplib_gat16_csr_hip): y [n, heads * d] goes in as it lies, the scores a_dst [m, heads] and a_src
    [n, heads] are dense float32 as in `gat`, every product, sum and exponential is fp32, z is rounded once to y's dtype.  Returns
    (z [m, heads * d] 16-bit, lse [m, heads] fp32); `out` = (z, lse).  The operand checks are gat's, with the 16-bit family's (even
    pitches, 4-byte aligned bases)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n, k = y.size(0), y.size(1)
    ldy = _attn16_dense(y, "y", n, None, "one row per column of the sparse operand")
    d = _gat_heads(heads, k)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        z, lse = out
        ldz = _attn16_dense(z, "out[0]", m, k, "z", y.dtype)
        _gat_table(lse, "out[1]", m, heads)
    _gat16_domain(n, heads, d, ldy)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, k), dtype=y.dtype, device=y.device)
        lse = torch.empty((m, heads), dtype=torch.float32, device=y.device)
        ldz = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat16_csr_hip(HALF_DTYPES[y.dtype], m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                        _ptr(a_dst), _ptr(y), ldy, _ptr(a_src), heads, float(negative_slope), _ptr(z), ldz, _ptr(lse),
                                        _stream(y.device))
    _check(st, "isplib_gat16_csr_hip")
    return z, lse


def gat16_backward_rows(rowptr, col, y, a_dst, a_src, g, lse, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """The backward of `gat16_forward` over the rows (isplib_gat16_bw_rows_hip): for g = dL/dz [m, heads * d] (y's dtype) and the
    forward's lse -- z is NOT read: D[i,h] = sum_e a_e <g_i, y_j>_h is formed in fp32 from the row's edges, in the same pass as
    d a_dst = P - D Q.  Returns (d_a_dst [m, heads], D [m, heads]), both fp32; an empty row has both 0.  `out` = (d_a_dst, D)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n, k = y.size(0), y.size(1)
    ldy = _attn16_dense(y, "y", n, None, "one row per column of the sparse operand")
    d = _gat_heads(heads, k)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    ldg = _attn16_dense(g, "g", m, k, "the gradient of z", y.dtype)
    _gat_table(lse, "lse", m, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        _gat_table(out[0], "out[0]", m, heads)
        _gat_table(out[1], "out[1]", m, heads)
    _gat16_domain(n, heads, d, ldy)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("g", g), ("lse", lse), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        out = (torch.empty((m, heads), dtype=torch.float32, device=y.device), torch.empty((m, heads), dtype=torch.float32, device=y.device))
    dadst, dsum = out
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            dadst.zero_()
            dsum.zero_()
        return dadst, dsum
    rp = rowptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat16_bw_rows_hip(HALF_DTYPES[y.dtype], m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                            _ptr(a_dst), _ptr(y), ldy, _ptr(a_src), heads, float(negative_slope), _ptr(g), ldg, _ptr(lse),
                                            _ptr(dadst), _ptr(dsum), _stream(y.device))
    _check(st, "isplib_gat16_bw_rows_hip")
    return dadst, dsum


def gat16_backward_cols(colptr, row_t, y, a_dst, a_src, g, lse, dsum, heads: int = 1, negative_slope: float = 0.2, *, out=None,
                        check: bool = True):
    """The backward of `gat16_forward` over the columns (isplib_gat16_bw_cols_hip), on the transposed structure: dy_j[head h] = sum over
    the entries e = (i, j) of column j of a_e g_i[head h], rounded once to y's dtype, and d a_src[j,h] = sum of du_e (fp32), with `lse`
    of the forward and `dsum` = D of gat16_backward_rows.  Returns (dy [n, heads * d] 16-bit, d_a_src [n, heads] fp32); `out` = (dy,
    d_a_src)."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldy = _attn16_dense(y, "y", n, None, "one row per column of the sparse operand")
    k = y.size(1)
    d = _gat_heads(heads, k)
    if not isinstance(g, torch.Tensor) or g.dim() != 2:
        raise ValueError("isplib_amd: `g` must be a 2-D tensor [m, heads * d]")
    m = g.size(0)
    ldg = _attn16_dense(g, "g", m, k, "the gradient of z", y.dtype)
    _gat_table(a_dst, "a_dst", m, heads)
    _gat_table(a_src, "a_src", n, heads)
    _gat_table(lse, "lse", m, heads)
    _gat_table(dsum, "dsum", m, heads)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    if out is not None:
        lddy = _attn16_dense(out[0], "out[0]", n, k, "dy", y.dtype)
        _gat_table(out[1], "out[1]", n, heads)
    _gat16_domain(m, heads, d, ldg)
    _same_gpu((("y", y), ("a_dst", a_dst), ("a_src", a_src), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        out = (torch.empty((n, k), dtype=y.dtype, device=y.device), torch.empty((n, heads), dtype=torch.float32, device=y.device))
        lddy = max(k, 1)
    dy, dasrc = out
    if n == 0 or k == 0:
        if k == 0 and n > 0:
            dasrc.zero_()
        return dy, dasrc
    cp = colptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gat16_bw_cols_hip(HALF_DTYPES[y.dtype], m, n, k, row_t.numel(), _ptr(row_t), ctypes.c_void_p(cp),
                                            ctypes.c_void_p(cp + 8), _ptr(a_dst), _ptr(y), ldy, _ptr(a_src), heads, float(negative_slope),
                                            _ptr(g), ldg, _ptr(lse), _ptr(dsum), _ptr(dy), lddy, _ptr(dasrc), _stream(y.device))
    _check(st, "isplib_gat16_bw_cols_hip")
    return dy, dasrc


def _gatv2_16_domain(rows_gathered: int, heads: int, d: int, lds) -> None:
    for ld in lds:
        if d > 0 and not gatv2_16_serves(rows_gathered, heads, d, ld):
            raise ValueError(f"isplib_amd: outside the 16-bit GATv2 entries' domain (isplib_gatv2_16_serves = isplib_gat16_serves: "
                             f"{GAT16_K_MIN} <= heads * d <= {GAT16_K_MAX}, heads == 1 with d even or d a power of two >= 8, the pitch even, "
                             f"gathered rows < 2^31, rows * pitch * 2 <= 3.5 GiB), got rows={rows_gathered}, heads={heads}, d={d}, pitch={ld}")


def gatv2_16_bw_rows_workspace_bytes(m: int, k: int) -> int:
    """isplib_gatv2_16_bw_rows_workspace_bytes: what `gatv2_16_backward_rows` needs behind `workspace` when `datt` is asked for."""
    return int(lib().isplib_gatv2_16_bw_rows_workspace_bytes(int(m), int(k)))


def gatv2_16_forward(rowptr, col, x, y, att, heads: int = 1, negative_slope: float = 0.2, *, out=None, check: bool = True):
    """`gatv2` for bf16 / fp16 `x` and `y` of one dtype (isplib_gatv2_16_csr_hip): x [m, heads * d] and y [n, heads * d] go in as they
    lie, att [heads, d] is contiguous float32 as in `gatv2`, every sum, product and exponential is fp32, z is rounded once to the
    operands' dtype.  Returns (z [m, heads * d] 16-bit, lse [m, heads] fp32); `out` = (z, lse).  The operand checks are gatv2's, with
    the 16-bit family's (even pitches, 4-byte aligned bases)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    ldx = _attn16_dense(x, "x", m, None, "one row per row of the sparse operand")
    k = x.size(1)
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n = y.size(0)
    ldy = _attn16_dense(y, "y", n, k, "one row per column of the sparse operand, x's width", x.dtype)
    d = _gat_heads(heads, k)
    _gatv2_att(att, "att", heads, d)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        z, lse = out
        ldz = _attn16_dense(z, "out[0]", m, k, "z", x.dtype)
        _gat_table(lse, "out[1]", m, heads)
    _gatv2_16_domain(n, heads, d, (ldy,))
    _same_gpu((("x", x), ("y", y), ("att", att), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, k), dtype=x.dtype, device=x.device)
        lse = torch.empty((m, heads), dtype=torch.float32, device=x.device)
        ldz = max(k, 1)
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    with torch.cuda.device(x.device):
        st = lib().isplib_gatv2_16_csr_hip(HALF_DTYPES[x.dtype], m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                           _ptr(x), ldx, _ptr(y), ldy, _ptr(att), heads, float(negative_slope), _ptr(z), ldz, _ptr(lse),
                                           _stream(x.device))
    _check(st, "isplib_gatv2_16_csr_hip")
    return z, lse


def gatv2_16_backward_rows(rowptr, col, x, y, att, g, lse, heads: int = 1, negative_slope: float = 0.2, *, want_datt: bool = True, out=None,
                           workspace=None, check: bool = True):
    """The backward of `gatv2_16_forward` over the rows (isplib_gatv2_16_bw_rows_hip): for g = dL/dz [m, heads * d] (x's dtype) and the
    forward's lse -- z is NOT read: D[i,h] = sum_e a_e <g_i, y_j>_h is formed in fp32 from the row's edges, in the same pass as
    dx_ic = att_c (P_c - D Q_c) and, with `want_datt`, the row's part R_c - D S_c of datt_c.  Returns (dx [m, heads * d] 16-bit,
    D [m, heads] fp32, datt [heads, d] fp32 or None); an empty row has dx_i = 0 and D = 0.  `out` = (dx, D, datt or None);
    `workspace`: a uint8 GPU tensor of at least gatv2_16_bw_rows_workspace_bytes(m, k) bytes (allocated when None)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    ldx = _attn16_dense(x, "x", m, None, "one row per row of the sparse operand")
    k = x.size(1)
    if not isinstance(y, torch.Tensor) or y.dim() != 2:
        raise ValueError("isplib_amd: `y` must be a 2-D tensor [n, heads * d]")
    n = y.size(0)
    ldy = _attn16_dense(y, "y", n, k, "one row per column of the sparse operand, x's width", x.dtype)
    d = _gat_heads(heads, k)
    _gatv2_att(att, "att", heads, d)
    ldg = _attn16_dense(g, "g", m, k, "the gradient of z", x.dtype)
    _gat_table(lse, "lse", m, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if out is not None:
        if len(out) != 3:
            raise ValueError("isplib_amd: `out` must be (dx, D, datt or None)")
        lddx = _attn16_dense(out[0], "out[0]", m, k, "dx", x.dtype)
        _gat_table(out[1], "out[1]", m, heads)
        if (out[2] is not None) != bool(want_datt):
            raise ValueError("isplib_amd: `out[2]` (datt) must be given exactly when `want_datt`")
        if out[2] is not None:
            _gatv2_att(out[2], "out[2]", heads, d)
    if workspace is not None:
        if not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1 or not workspace.is_contiguous():
            raise ValueError("isplib_amd: `workspace` must be a contiguous 1-D uint8 tensor")
    _gatv2_16_domain(n, heads, d, (ldy,))
    _same_gpu((("x", x), ("y", y), ("att", att), ("g", g), ("lse", lse), ("rowptr", rowptr), ("col", col), ("workspace", workspace)) +
              ((("out[0]", out[0]), ("out[1]", out[1]), ("out[2]", out[2])) if out is not None else ()))
    if out is None:
        out = (torch.empty((m, k), dtype=x.dtype, device=x.device), torch.empty((m, heads), dtype=torch.float32, device=x.device),
               torch.empty((heads, d), dtype=torch.float32, device=x.device) if want_datt else None)
        lddx = max(k, 1)
    dx, dsum, datt = out
    if m == 0 or k == 0:
        if k == 0 and m > 0:
            dsum.zero_()
        if datt is not None:
            datt.zero_()
        return dx, dsum, datt
    rp = rowptr.data_ptr()
    with torch.cuda.device(x.device):
        if datt is not None:
            need = gatv2_16_bw_rows_workspace_bytes(m, k)
            if workspace is None:
                workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=x.device)
            elif workspace.numel() < need:
                raise ValueError(f"isplib_amd: `workspace` holds {workspace.numel()} bytes, isplib_gatv2_16_bw_rows_workspace_bytes asks for {need}")
        st = lib().isplib_gatv2_16_bw_rows_hip(HALF_DTYPES[x.dtype], m, n, k, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                               _ptr(x), ldx, _ptr(y), ldy, _ptr(att), heads, float(negative_slope), _ptr(g), ldg, _ptr(lse),
                                               _ptr(dx), lddx, _ptr(dsum), _ptr(datt), _ptr(workspace) if datt is not None else None,
                                               workspace.numel() if datt is not None else 0, _stream(x.device))
    _check(st, "isplib_gatv2_16_bw_rows_hip")
    return dx, dsum, datt


def gatv2_16_backward_cols(colptr, row_t, x, y, att, g, lse, dsum, heads: int = 1, negative_slope: float = 0.2, *, out=None,
                           check: bool = True):
    """The backward of `gatv2_16_forward` over the columns (isplib_gatv2_16_bw_cols_hip), on the transposed structure: dy_jc = sum over
    the entries e = (i, j) of column j of a_e g_ic + ds_e att_c sl_ec, rounded once to the operands' dtype, with `lse` of the forward
    and `dsum` = D of gatv2_16_backward_rows.  Returns dy [n, heads * d] 16-bit; a column no entry points at has 0.  `out` = dy."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldy = _attn16_dense(y, "y", n, None, "one row per column of the sparse operand")
    k = y.size(1)
    d = _gat_heads(heads, k)
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("isplib_amd: `x` must be a 2-D tensor [m, heads * d]")
    m = x.size(0)
    ldx = _attn16_dense(x, "x", m, k, "one row per row of the sparse operand, y's width", y.dtype)
    ldg = _attn16_dense(g, "g", m, k, "the gradient of z", y.dtype)
    _gatv2_att(att, "att", heads, d)
    _gat_table(lse, "lse", m, heads)
    _gat_table(dsum, "dsum", m, heads)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    if out is not None:
        lddy = _attn16_dense(out, "out", n, k, "dy", y.dtype)
    _gatv2_16_domain(m, heads, d, (ldx, ldg))
    _same_gpu((("x", x), ("y", y), ("att", att), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t), ("out", out)))
    if out is None:
        out = torch.empty((n, k), dtype=y.dtype, device=y.device)
        lddy = max(k, 1)
    if n == 0 or k == 0:
        return out
    cp = colptr.data_ptr()
    with torch.cuda.device(y.device):
        st = lib().isplib_gatv2_16_bw_cols_hip(HALF_DTYPES[y.dtype], m, n, k, row_t.numel(), _ptr(row_t), ctypes.c_void_p(cp),
                                               ctypes.c_void_p(cp + 8), _ptr(x), ldx, _ptr(y), ldy, _ptr(att), heads, float(negative_slope),
                                               _ptr(g), ldg, _ptr(lse), _ptr(dsum), _ptr(out), lddy, _stream(y.device))
    _check(st, "isplib_gatv2_16_bw_cols_hip")
    return out


def _mha16_domain(rows_gathered: int, heads: int, d: int, lds) -> None:
    for ld in lds:
        if d > 0 and not mha16_serves(rows_gathered, heads, d, ld):
            raise ValueError(f"isplib_amd: outside the 16-bit multi-head attention entries' domain (isplib_qkv16_serves = isplib_gat16_serves: "
                             f"{GAT16_K_MIN} <= heads * d <= {GAT16_K_MAX}, heads == 1 with d even or d a power of two >= 8, the pitch even, "
                             f"gathered rows < 2^31, rows * pitch * 2 <= 3.5 GiB), got rows={rows_gathered}, heads={heads}, d={d}, pitch={ld}")


def _mha16_qkv(m: int, q, k, v):
    """q [m, K] and k, v [n, K] of the 16-bit multi-head entries, all of q's dtype; returns (n, K, ldq, ldk, ldv)."""
    ldq = _attn16_dense(q, "q", m, None, "one row per row of the sparse operand")
    kk = q.size(1)
    if not isinstance(k, torch.Tensor) or k.dim() != 2:
        raise ValueError("isplib_amd: `k` must be a 2-D tensor [n, heads * d]")
    n = k.size(0)
    ldk = _attn16_dense(k, "k", n, kk, "one row per column of the sparse operand, q's width", q.dtype)
    ldv = _attn16_dense(v, "v", n, kk, "one row per column of the sparse operand, q's width", q.dtype)
    return n, kk, ldq, ldk, ldv


def mha16_forward(rowptr, col, q, k, v, heads: int = 1, scale: Optional[float] = None, *, out=None, check: bool = True):
    """`mha` for bf16 / fp16 `q`, `k` and `v` of one dtype (isplib_qkv16_csr_hip): q [m, heads * d], k and v [n, heads * d] go in as
    they lie (row-strided views keep their even pitch: column views of one fused 16-bit projection go in without a copy), every
    product, sum and exponential is fp32, z is rounded once to the operands' dtype.  Returns (z [m, heads * d] 16-bit, lse [m, heads]
    fp32); `out` = (z, lse); `scale` None: 1 / sqrt(d).  The operand checks are mha's, with the 16-bit family's (even pitches, 4-byte
    aligned bases)."""
    return _mha16_forward(rowptr, col, q, k, v, heads, scale, out, check, None)


def mha16_drop_forward(rowptr, col, q, k, v, threshold: int, keep_scale: float, seed: int, heads: int = 1, scale: Optional[float] = None,
                       *, out=None, check: bool = True):
    """`mha16_forward` with attention dropout (isplib_qkv_half_drop_csr_hip): the keep bit and the keep scale of `mha_drop`, the 16-bit
    family's contract -- the finished row times `keep_scale`, then the one rounding; lse is that of the call without dropout.  Returns
    (z 16-bit, lse fp32); the operand checks are mha16_forward's, and nnz < 2^31."""
    return _mha16_forward(rowptr, col, q, k, v, heads, scale, out, check, _mha_drop_args(threshold, keep_scale, seed))


def _mha16_forward(rowptr, col, q, k, v, heads, scale, out, check, drop):
    """`mha16_forward` (drop None) and `mha16_drop_forward` (drop = (threshold, keep_scale, seed), checked)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    n, kk, ldq, ldk, ldv = _mha16_qkv(m, q, k, v)
    d = _gat_heads(heads, kk)
    p = _mha_scale(scale, d)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if drop is not None:
        _gatv2_nnz(col.numel())
    if out is not None:
        z, lse = out
        ldz = _attn16_dense(z, "out[0]", m, kk, "z", q.dtype)
        _gat_table(lse, "out[1]", m, heads)
    _mha16_domain(n, heads, d, (ldk, ldv))
    _same_gpu((("q", q), ("k", k), ("v", v), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        z = torch.empty((m, kk), dtype=q.dtype, device=q.device)
        lse = torch.empty((m, heads), dtype=torch.float32, device=q.device)
        ldz = max(kk, 1)
    if m == 0 or kk == 0:
        if kk == 0 and m > 0:
            lse.fill_(float("-inf"))
        return z, lse
    rp = rowptr.data_ptr()
    entry = "isplib_qkv16_csr_hip" if drop is None else "isplib_qkv_half_drop_csr_hip"
    with torch.cuda.device(q.device):
        st = getattr(lib(), entry)(HALF_DTYPES[q.dtype], m, n, kk, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                   heads, p, _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(z), ldz, _ptr(lse), _stream(q.device),
                                   *(drop or ()))
    _check(st, entry)
    return z, lse


def mha16_backward_rows(rowptr, col, q, k, v, g, lse, heads: int = 1, scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `mha16_forward` over the rows (isplib_qkv16_bw_rows_hip): for g = dL/dz [m, heads * d] (q's dtype) and the
    forward's lse -- z is NOT read: D[i,h] = sum_e a_e <g_i, v_j>_h is formed in fp32 from the row's edges, in the same pass as
    dq_ic = scale (P_c - D Q_c).  Returns (dq [m, heads * d] 16-bit, D [m, heads] fp32); an empty row has dq_i = 0 and D = 0.
    `out` = (dq, D)."""
    return _mha16_backward_rows(rowptr, col, q, k, v, g, lse, heads, scale, out, check, None)


def mha16_drop_backward_rows(rowptr, col, q, k, v, g, lse, threshold: int, keep_scale: float, seed: int, heads: int = 1,
                             scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `mha16_drop_forward` over the rows (isplib_qkv_half_drop_bw_rows_hip), with the mask of the same (threshold,
    seed): t_e = q_e keep_scale <g_i, v_j>_h, D = sum_e a_e t_e from the row's edges (z is not read), everything else as
    `mha16_backward_rows`.  Returns (dq 16-bit, D fp32)."""
    return _mha16_backward_rows(rowptr, col, q, k, v, g, lse, heads, scale, out, check, _mha_drop_args(threshold, keep_scale, seed))


def _mha16_backward_rows(rowptr, col, q, k, v, g, lse, heads, scale, out, check, drop):
    """`mha16_backward_rows` (drop None) and `mha16_drop_backward_rows` (drop = (threshold, keep_scale, seed), checked)."""
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise ValueError("isplib_amd: `rowptr` (m + 1 entries) must be a 1-D tensor")
    m = rowptr.numel() - 1
    n, kk, ldq, ldk, ldv = _mha16_qkv(m, q, k, v)
    d = _gat_heads(heads, kk)
    p = _mha_scale(scale, d)
    ldg = _attn16_dense(g, "g", m, kk, "the gradient of z", q.dtype)
    _gat_table(lse, "lse", m, heads)
    rowptr, col = _attn_structure(rowptr, col, "rowptr", "col", n, check)
    if drop is not None:
        _gatv2_nnz(col.numel())
    if out is not None:
        if len(out) != 2:
            raise ValueError("isplib_amd: `out` must be (dq, D)")
        lddq = _attn16_dense(out[0], "out[0]", m, kk, "dq", q.dtype)
        _gat_table(out[1], "out[1]", m, heads)
    _mha16_domain(n, heads, d, (ldk, ldv))
    _same_gpu((("q", q), ("k", k), ("v", v), ("g", g), ("lse", lse), ("rowptr", rowptr), ("col", col)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()))
    if out is None:
        out = (torch.empty((m, kk), dtype=q.dtype, device=q.device), torch.empty((m, heads), dtype=torch.float32, device=q.device))
        lddq = max(kk, 1)
    dq, dsum = out
    if m == 0 or kk == 0:
        if kk == 0 and m > 0:
            dsum.zero_()
        return dq, dsum
    rp = rowptr.data_ptr()
    entry = "isplib_qkv16_bw_rows_hip" if drop is None else "isplib_qkv_half_drop_bw_rows_hip"
    with torch.cuda.device(q.device):
        st = getattr(lib(), entry)(HALF_DTYPES[q.dtype], m, n, kk, col.numel(), _ptr(col), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                   heads, p, _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv, _ptr(g), ldg, _ptr(lse), _ptr(dq), lddq,
                                   _ptr(dsum), _stream(q.device), *(drop or ()))
    _check(st, entry)
    return dq, dsum


def mha16_backward_cols(colptr, row_t, q, k, v, g, lse, dsum, heads: int = 1, scale: Optional[float] = None, *, out=None,
                        check: bool = True):
    """The backward of `mha16_forward` over the columns (isplib_qkv16_bw_cols_hip), on the transposed structure: dk_j[head h] = scale
    sum over the entries e = (i, j) of column j of ds_e q_i[head h] and dv_j[head h] = sum of a_e g_i[head h], each rounded once to the
    operands' dtype, with `lse` of the forward and `dsum` = D of mha16_backward_rows.  Returns (dk, dv), both [n, heads * d] 16-bit; a
    column no entry points at has 0 in both.  `out` = (dk, dv)."""
    return _mha16_backward_cols(colptr, row_t, None, q, k, v, g, lse, dsum, heads, scale, out, check, None)


def mha16_drop_backward_cols(colptr, row_t, csr2csc, q, k, v, g, lse, dsum, threshold: int, keep_scale: float, seed: int, heads: int = 1,
                             scale: Optional[float] = None, *, out=None, check: bool = True):
    """The backward of `mha16_drop_forward` over the columns (isplib_qkv_half_drop_bw_cols_hip): dk as `mha16_backward_cols` with t_e
    under the mask, dv_j[head h] = sum over the entries of column j of q_e keep_scale a_e g_i[head h], each rounded once.  `csr2csc`
    [nnz] int64 is required: the keep bit is a function of the entry's CSR position.  Returns (dk, dv)."""
    return _mha16_backward_cols(colptr, row_t, csr2csc, q, k, v, g, lse, dsum, heads, scale, out, check,
                                _mha_drop_args(threshold, keep_scale, seed))


def _mha16_backward_cols(colptr, row_t, csr2csc, q, k, v, g, lse, dsum, heads, scale, out, check, drop):
    """`mha16_backward_cols` (drop None, no csr2csc) and `mha16_drop_backward_cols` (drop = (threshold, keep_scale, seed), checked;
    csr2csc required)."""
    if not isinstance(colptr, torch.Tensor) or colptr.dim() != 1 or colptr.numel() < 1:
        raise ValueError("isplib_amd: `colptr` (n + 1 entries) must be a 1-D tensor")
    n = colptr.numel() - 1
    ldk = _attn16_dense(k, "k", n, None, "one row per column of the sparse operand")
    kk = k.size(1)
    ldv = _attn16_dense(v, "v", n, kk, "one row per column of the sparse operand, k's width", k.dtype)
    d = _gat_heads(heads, kk)
    p = _mha_scale(scale, d)
    if not isinstance(q, torch.Tensor) or q.dim() != 2:
        raise ValueError("isplib_amd: `q` must be a 2-D tensor [m, heads * d]")
    m = q.size(0)
    ldq = _attn16_dense(q, "q", m, kk, "one row per row of the sparse operand, k's width", k.dtype)
    ldg = _attn16_dense(g, "g", m, kk, "the gradient of z", k.dtype)
    _gat_table(lse, "lse", m, heads)
    _gat_table(dsum, "dsum", m, heads)
    colptr, row_t = _attn_structure(colptr, row_t, "colptr", "row_t", m, check)
    if drop is not None:
        _gatv2_nnz(row_t.numel())
        csr2csc = _gat_edge_positions(csr2csc, row_t.numel(), check)
    if out is not None:
        if len(out) != 2:
            raise ValueError("isplib_amd: `out` must be (dk, dv)")
        lddk = _attn16_dense(out[0], "out[0]", n, kk, "dk", k.dtype)
        lddv = _attn16_dense(out[1], "out[1]", n, kk, "dv", k.dtype)
    _mha16_domain(m, heads, d, (ldq, ldg))
    _same_gpu((("q", q), ("k", k), ("v", v), ("g", g), ("lse", lse), ("dsum", dsum), ("colptr", colptr), ("row_t", row_t)) +
              ((("out[0]", out[0]), ("out[1]", out[1])) if out is not None else ()) + ((("csr2csc", csr2csc),) if drop is not None else ()))
    if out is None:
        out = (torch.empty((n, kk), dtype=k.dtype, device=k.device), torch.empty((n, kk), dtype=k.dtype, device=k.device))
        lddk = lddv = max(kk, 1)
    dk, dv = out
    if n == 0 or kk == 0:
        return dk, dv
    cp = colptr.data_ptr()
    entry = "isplib_qkv16_bw_cols_hip" if drop is None else "isplib_qkv_half_drop_bw_cols_hip"
    with torch.cuda.device(k.device):
        st = getattr(lib(), entry)(HALF_DTYPES[k.dtype], m, n, kk, row_t.numel(), _ptr(row_t), ctypes.c_void_p(cp), ctypes.c_void_p(cp + 8),
                                   *((_ptr(csr2csc),) if drop is not None else ()), heads, p, _ptr(q), ldq, _ptr(g), ldg, _ptr(lse),
                                   _ptr(dsum), _ptr(k), ldk, _ptr(v), ldv, _ptr(dk), lddk, _ptr(dv), lddv, _stream(k.device),
                                   *(drop or ()))
    _check(st, entry)
    return dk, dv


def fusedMM_csr_rows16_minmax_hip(imessage: int, rowptr, col, val, order, y, z, z_arg=None, check: bool = True, dtype=None, k=None, ldy=None,
                                  ldz=None, ldarg=None) -> int:
    """Raw boundary call of the 16-bit row SpMM for max / min, for operands the entry may refuse: it hands over what it is given
    (`dtype`, `k`, `ldy`, `ldz`, `ldarg`: override what the tensors say -- refusal tests; the entry refuses before it reads anything).
    `z_arg` None is the values-only launch.  Callers that want their operands checked use spmm_rows16_minmax."""
    if ldarg is None:
        m, kk = rowptr.numel() - 1, y.size(1) if k is None else int(k)
        ldarg = 0 if z_arg is None else (z_arg.stride(0) if m > 1 else max(kk, z_arg.stride(0)))
    return _rows16_raw("fusedMM_csr_rows16_minmax_hip", imessage, rowptr, col, val, order, y, z, check, dtype, k, ldy, ldz, _ptr(z_arg), int(ldarg))


def spmm_rows16_minmax(rowptr, col, val, y, reduce: str = "max", order=None, out=None, arg=None, want_arg: bool = True):
    """The 16-bit row SpMM for max / min of a bf16 / fp16 `y` [n, k]: returns (out, arg) -- `out` [m, k] of y's dtype and `arg` int64
    [m, k], the CSR position of each winner (col.numel() where nothing won); both allocated when not given, row-strided views are
    written at their own pitch.  want_arg=False (and no `arg`): the values-only launch, returns (out, None) with the same value bits.
    `val`: fp32 weights or None; `order`: int32 [m], position -> row, or None.  Values and positions are bit-equal to the fp32 kernel's
    on the widened operand, rounded once.  Every operand is checked BEFORE the call -- a mis-shaped one is an out-of-bounds device
    read: rowptr / col int64 on y's device, rowptr ascending from 0 to col.numel(), every column id inside [0, n), the shape inside
    isplib_rows16_serves, `out` [m, k] of the same dtype at an even pitch, `arg` int64 [m, k], `order` a permutation's length."""
    if reduce not in ("max", "min"):
        raise ValueError(f"isplib_amd: spmm_rows16_minmax serves max / min, got '{reduce}' (sum / mean: spmm_rows16)")
    rowptr, col, val, order, out, arg = _rows16_operands(rowptr, col, val, False, y, order, out, arg, want_arg)
    fusedMM_csr_rows16_minmax_hip(MESSAGE[reduce], rowptr, col, val, order, y, out, arg)
    return out, arg


def fusedMM_csr_stream_minmax_hip(imessage: int, rowptr, nnz: int, plan, y, z, z_arg=None, workspace=None, check: bool = True) -> int:
    """Raw boundary call of the stream-form SpMM for max / min; ``plan`` must be built for stream_minmax_geometry()."""
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    rp = rowptr.data_ptr()
    ps = plan.struct()
    with torch.cuda.device(y.device):
        st = lib().fusedMM_csr_stream_minmax_hip(int(imessage), m, n, k, int(nnz), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                                 ctypes.byref(ps), _ptr(y), y.stride(0) if n > 1 else max(k, y.stride(0)), _ptr(z),
                                                 z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(z_arg), _ptr(workspace),
                                                 0 if workspace is None else workspace.numel(), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_stream_minmax_hip")
    return st


def spmm_stream_minmax(rowptr, nnz: int, plan, y, reduce: str = "max", workspace=None, want_arg: bool = True):
    """Allocate the outputs (+ workspace) and call the max / min stream boundary; returns (out, arg)."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    y = y.contiguous()
    m, k = rowptr.numel() - 1, y.size(1)
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    arg = torch.empty((m, k), dtype=torch.int64, device=y.device) if want_arg else None
    if workspace is None:
        workspace = plan.workspace(minmax=True)
    fusedMM_csr_stream_minmax_hip(MESSAGE[reduce], rowptr, nnz, plan, y, out, arg, workspace)
    return out, arg


def suggest_stream_minmax(m: int, n: int, nnz: int, k: int):
    """(streams, slices, chunk) when the stream schedule is expected to win for max / min on this shape, else None."""
    st, sl, ch = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if not lib().isplib_suggest_stream_minmax(int(m), int(n), int(nnz), int(k), ctypes.byref(st), ctypes.byref(sl), ctypes.byref(ch)):
        return None
    return st.value, sl.value, ch.value


def stream_minmax_geometry(streams: int = 4):
    """(rows per wave, resident waves) of the max / min stream kernel for `streams` = 4 (64-column slots) or 8 (32-column)."""
    rpw, res = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().isplib_spmm_stream_minmax_geometry(int(streams), ctypes.byref(rpw), ctypes.byref(res)), "isplib_spmm_stream_minmax_geometry")
    return rpw.value, res.value


def hybrid_geometry(streams: int = 4):
    """(rows per wave, resident waves, table rows, hot-step cap per wave and slice) of the hybrid kernel (isplib_spmm_hybrid_geometry)."""
    v = [ctypes.c_int(0) for _ in range(4)]
    _check(exp_lib().isplib_spmm_hybrid_geometry(int(streams), *[ctypes.byref(x) for x in v]), "isplib_spmm_hybrid_geometry")
    return tuple(x.value for x in v)


def fusedMM_csr_hybrid_hip(imessage: int, rowptr, nnz: int, plan, y, z, workspace=None, epilogue=None, check: bool = True) -> int:
    """Raw boundary call of the hybrid-form SpMM (sum / mean, unit weights); ``plan`` is an isplib_amd.plan.HybridPlan."""
    assert y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1
    m, n, k = rowptr.numel() - 1, y.size(0), y.size(1)
    rp = rowptr.data_ptr()
    ps = plan.struct()
    with torch.cuda.device(y.device):
        st = exp_lib().fusedMM_csr_hybrid_hip(int(imessage), m, n, k, int(nnz), ctypes.c_void_p(rp), ctypes.c_void_p(rp + 8),
                                          ctypes.byref(ps), _ptr(y), y.stride(0) if n > 1 else max(k, y.stride(0)), _ptr(z),
                                          z.stride(0) if m > 1 else max(k, z.stride(0)), _ptr(workspace),
                                          0 if workspace is None else workspace.numel(),
                                          None if epilogue is None else ctypes.byref(epilogue), _stream(y.device))
    if check:
        _check(st, "fusedMM_csr_hybrid_hip")
    return st


def spmm_hybrid(rowptr, nnz: int, plan, y, reduce: str = "sum", workspace=None, row_scale=None, self_term=None, bias=None, relu=False):
    """Allocate the output (+ workspace) and call the hybrid boundary; returns out."""
    rowptr = _dev(rowptr, "rowptr", torch.int64)
    y = y.contiguous()
    m, k = rowptr.numel() - 1, y.size(1)
    out = torch.empty((m, k), dtype=torch.float32, device=y.device)
    if workspace is None:
        workspace = plan.workspace()
    ep = None
    if row_scale is not None or self_term is not None or bias is not None or relu:
        ep = Epilogue(None if row_scale is None else row_scale.data_ptr(), None if self_term is None else self_term.data_ptr(),
                      k if self_term is None else self_term.stride(0), None if bias is None else bias.data_ptr(), int(bool(relu)))
    fusedMM_csr_hybrid_hip(MESSAGE[reduce], rowptr, nnz, plan, y, out, workspace, ep)
    return out


def suggest_stream(m: int, n: int, nnz: int, k: int, weighted: bool = False):
    """(streams, slices, chunk) when the stream schedule is expected to win for this shape, else None
    (isplib_suggest_stream_weighted; `weighted`: the plan will carry edge weights)."""
    st, sl, ch = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if not lib().isplib_suggest_stream_weighted(int(m), int(n), int(nnz), int(k), int(bool(weighted)), ctypes.byref(st), ctypes.byref(sl), ctypes.byref(ch)):
        return None
    return st.value, sl.value, ch.value


class _DevView:
    """A device array the C library owns, seen through __cuda_array_interface__ (no copy).  `owner` is the object whose
    destructor frees the array: torch.as_tensor keeps THIS object alive for as long as the tensor's storage lives (its
    deleter holds the reference), so holding the owner here ties the library's memory to every tensor that looks at it
    -- including the copies autograd saves for a backward that runs after the graph object is gone."""

    def __init__(self, ptr: int, count: int, typestr: str, owner=None):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2}
        self._owner = owner


class NativeStreamPlan:
    """A stream plan built by the C library (isplib_stream_plan_build_hip) -- the torch-free host's counterpart of
    isplib_amd.plan.build_stream_plan; same interface as plan.StreamPlan for the boundary wrappers."""

    def __init__(self, rowptr, col, val, ncols: int, streams: int, slices: int, chunk: int, waves_per_gen: int = 0,
                 minmax: bool = False, fusedmm: bool = False, capacities=None):
        """capacities (sum / mean plans): the levelled deal with the caller's capacities, one per wave of a generation
        (isplib_stream_plan_build_caps_hip); None: the library's own (isplib_stream_plan_build_hip)."""
        assert capacities is None or not (minmax or fusedmm), "max / min and FusedMM plans keep equal capacities"
        self._s = StreamPlanStruct()
        self.device = col.device
        m = rowptr.numel() - 1
        with torch.cuda.device(col.device):
            if fusedmm:       # the generic FusedMM kernel's geometry (isplib_fusedmm_stream_geometry); no weights in the plan
                _check(lib().isplib_stream_plan_build_fusedmm_hip(m, int(ncols), col.numel(), _ptr(rowptr), _ptr(col), int(streams), int(slices),
                                                                  int(chunk), int(waves_per_gen), ctypes.byref(self._s), _stream(col.device)),
                       "isplib_stream_plan_build_fusedmm_hip")
            elif minmax:
                _check(lib().isplib_stream_plan_build_minmax_hip(m, int(ncols), col.numel(), _ptr(rowptr), _ptr(col), _ptr(val),
                                                                 int(streams), int(slices), int(chunk), int(waves_per_gen), ctypes.byref(self._s),
                                                                 _stream(col.device)), "isplib_stream_plan_build_minmax_hip")
            elif capacities is not None:
                caps = (ctypes.c_uint32 * len(capacities))(*[int(c) for c in capacities])
                rpw, resident = stream_geometry(streams)
                if len(caps) != (int(waves_per_gen) if waves_per_gen > 0 else resident):
                    raise ValueError("one capacity per wave of a generation")
                _check(lib().isplib_stream_plan_build_caps_hip(m, int(ncols), col.numel(), _ptr(rowptr), _ptr(col), _ptr(val), int(streams),
                                                               int(slices), int(chunk), int(waves_per_gen), ctypes.cast(caps, _vp),
                                                               ctypes.byref(self._s), _stream(col.device)), "isplib_stream_plan_build_caps_hip")
            else:
                _check(lib().isplib_stream_plan_build_hip(m, int(ncols), col.numel(), _ptr(rowptr), _ptr(col), _ptr(val), int(streams),
                                                          int(slices), int(chunk), int(waves_per_gen), ctypes.byref(self._s),
                                                          _stream(col.device)), "isplib_stream_plan_build_hip")
        for name in ("rows", "cols", "slices", "gens", "waves_per_gen", "rows_per_wave", "streams", "n_steps", "n_parts", "n_hub"):
            setattr(self, name, int(getattr(self._s, name)))

    def struct(self):
        return self._s

    def packed_dwords(self) -> int:
        """Dwords of the plan's packed word stream (the bit pattern of uint32 in an int32 view); 0: the plan has none."""
        return int(lib().isplib_stream_packed_dwords(ctypes.byref(self._s))) if self._s.has_packed else 0

    def workspace(self, minmax: bool = False):
        L = lib()
        nbytes = (L.isplib_spmm_stream_minmax_workspace_bytes if minmax else L.isplib_spmm_stream_workspace_bytes)(ctypes.byref(self._s))
        return torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def set_values(self, val):
        with torch.cuda.device(self.device):
            _check(lib().isplib_stream_plan_set_values_hip(ctypes.byref(self._s), _ptr(val), _stream(self.device)), "isplib_stream_plan_set_values_hip")

    def array(self, name: str) -> torch.Tensor:
        """A copy of one of the plan's device arrays as a tensor."""
        nw = self.gens * self.waves_per_gen
        count, typestr = {"words": (self.n_steps * self.streams, "<i4"), "perm": (self.n_steps * self.streams, "<i4"),
                          "vals": (self.n_steps * self.streams, "<f4"), "wave_step_off": (nw + 1, "<i8"),
                          "wave_row": (nw * self.rows_per_wave, "<i4"), "wave_part": (nw * self.rows_per_wave, "<i4"),
                          "hub_row": (self.n_hub, "<i4"), "hub_off": (self.n_hub + 1, "<i4"),
                          "packed": (self.packed_dwords(), "<i4")}[name]
        ptr = getattr(self._s, name)
        if not ptr or count == 0:
            return torch.empty(0, device=self.device)
        return torch.as_tensor(_DevView(ptr, count, typestr), device=self.device).clone()

    def view(self, name: str, dtype: torch.dtype) -> torch.Tensor:
        """One of the plan's device arrays as a tensor WITHOUT a copy.  The memory belongs to this plan object; the tensor
        holds a reference to it (through its _DevView), so the arrays are freed only when the last tensor looking at them
        is gone -- never under a backward pass that still has them saved.  (close() is for owners that hand out no views.)"""
        nw = self.gens * self.waves_per_gen
        count, typestr = {"words": (self.n_steps * self.streams, "<i4"), "perm": (self.n_steps * self.streams, "<i4"),
                          "wave_step_off": (nw + 1, "<i8"), "wave_row": (nw * self.rows_per_wave, "<i4"),
                          "wave_part": (nw * self.rows_per_wave, "<i4"), "hub_row": (self.n_hub, "<i4"),
                          "hub_off": (self.n_hub + 1, "<i4"), "packed": (self.packed_dwords(), "<i4")}[name]
        ptr = getattr(self._s, name)
        if not ptr or count == 0:
            return torch.empty(0, dtype=dtype, device=self.device)
        t = torch.as_tensor(_DevView(ptr, count, typestr, owner=self), device=self.device)
        assert t.dtype == dtype and t.data_ptr() == ptr, "zero-copy view of a library array"
        return t

    def close(self):
        if self._s.words or self._s.wave_row:
            lib().isplib_stream_plan_free(ctypes.byref(self._s))

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


STREAM_CAP_ONE = 4096          # ISPLIB_STREAM_CAP_ONE: the nominal capacity of the levelled deal


def stream_capacities(device, streams: int, waves_per_gen: int, nnz: int):
    """The capacities of the levelled deal for a sum / mean plan of this geometry on `device` (isplib_stream_capacities_hip: the
    library's rule and its once-per-process calibration): a list of waves_per_gen integers, or None where the deal stays
    unlevelled (ISPLIB_STREAM_LEVEL=0, another waves_per_gen than the resident waves, a small graph under auto)."""
    device = torch.device(device)
    if device.type != "cuda":
        return None
    _, resident = stream_geometry(streams)
    wpg = int(waves_per_gen) if waves_per_gen > 0 else resident
    caps = (ctypes.c_uint32 * wpg)()
    levelled = ctypes.c_int(0)
    with torch.cuda.device(device):
        _check(lib().isplib_stream_capacities_hip(-1, int(streams), wpg, int(nnz), ctypes.cast(caps, _vp), ctypes.byref(levelled),
                                                  _stream(device)), "isplib_stream_capacities_hip")
    return list(caps) if levelled.value else None


def stream_pack(plan) -> Optional[torch.Tensor]:
    """The packed word stream of a plan whose arrays are torch tensors (isplib_stream_pack_hip: the library's packing pass over
    `plan.words`): an int32 tensor holding the uint32 dwords, or None where the plan is not representable (include/isplib_hip.h)."""
    ps = plan.struct()
    ps.packed, ps.has_packed = None, 0
    dwords = int(lib().isplib_stream_packed_dwords(ctypes.byref(ps)))
    if dwords <= 0 or not plan.words.is_cuda:
        return None
    out = torch.empty(dwords, dtype=torch.int32, device=plan.words.device)
    ok = ctypes.c_int(0)
    with torch.cuda.device(out.device):
        _check(lib().isplib_stream_pack_hip(ctypes.byref(ps), _ptr(out), dwords, ctypes.byref(ok), _stream(out.device)), "isplib_stream_pack_hip")
    return out if ok.value else None


def stream_pack_set(mode: int) -> None:
    """A/B runs and tests: 0 off, 1 every plan that has a packed stream, 2 auto (overrides ISPLIB_STREAM_PACK)."""
    _check(lib().isplib_stream_pack_set(int(mode)), "isplib_stream_pack_set")


def stream_pack_last() -> bool:
    """Whether the last fusedMM_csr_stream_hip of this thread read the plan's packed word stream."""
    return bool(lib().isplib_stream_pack_last())


def stream_level_set(mode: int) -> None:
    """A/B runs and tests: 0 off, 1 on, 2 auto (overrides ISPLIB_STREAM_LEVEL; plans built afterwards)."""
    _check(lib().isplib_stream_level_set(int(mode)), "isplib_stream_level_set")


def stream_geometry(streams: int = 4):
    """(rows per wave, resident waves) of the stream kernel for `streams` slots per wave (isplib_spmm_stream_geometry)."""
    rpw, res = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().isplib_spmm_stream_geometry(int(streams), ctypes.byref(rpw), ctypes.byref(res)), "isplib_spmm_stream_geometry")
    return rpw.value, res.value


def sweep_resident_waves(reduce: str, k: int, rows_per_wave: int = 16) -> int:
    return int(exp_lib().isplib_spmm_sweep_resident_waves(MESSAGE[reduce], int(k), int(rows_per_wave)))


class GraphHandle:
    """ctypes view of `isplib_graph` (include/isplib_hip.h): the torch-free host's per-graph object.  torch only
    supplies the device buffers here; plans, packed ids, CSC operands and workspace live inside the library."""

    def __init__(self, rowptr, col, val, ncols: int):
        self.rowptr = _dev(rowptr, "rowptr", torch.int64)       # borrowed by the handle: keep them alive
        self.col = _dev(col, "col", torch.int64)
        self.val = None if val is None else _dev(val, "val", torch.float32)
        self.m, self.n = self.rowptr.numel() - 1, int(ncols)
        self._cols_ok = None                                    # sddmm's column-id check, made once
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.col.device):
            _check(lib().isplib_graph_create(self.m, self.n, self.col.numel(), _ptr(self.rowptr), _ptr(self.col),
                                             _ptr(self.val), ctypes.byref(self._h)), "isplib_graph_create")

    def set_slices(self, slices: int) -> None:
        _check(lib().isplib_graph_set_slices(self._h, int(slices)), "isplib_graph_set_slices")

    def set_row_order(self, order, order_t=None) -> None:
        """The plain kernel's row order of A / of A^T (int32, position -> row; None = index order, and no search for one)."""
        self.order = None if order is None else _dev(order, "order", torch.int32)           # borrowed by the handle: keep them alive
        self.order_t = None if order_t is None else _dev(order_t, "order_t", torch.int32)
        assert self.order is None or self.order.numel() == self.m
        assert self.order_t is None or self.order_t.numel() == self.n
        _check(lib().isplib_graph_set_row_order(self._h, _ptr(self.order), _ptr(self.order_t)), "isplib_graph_set_row_order")

    def set_values(self, val) -> None:
        """New weights for the same structure (another array, the same one edited in place, or None = unit weights)."""
        self.val = None if val is None else _dev(val, "val", torch.float32)
        assert self.val is None or self.val.numel() == self.col.numel()
        _check(lib().isplib_graph_set_values(self._h, _ptr(self.val)), "isplib_graph_set_values")

    def spmm(self, y: torch.Tensor, reduce: str = "sum"):
        """y: [n, k] with unit column stride; a row stride > k (a column block of a wider matrix) is passed on as ldy."""
        if not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.stride(1) == 1 and y.stride(0) >= y.size(1)):
            y = _dev(y, "y", torch.float32)
        k = y.size(1)
        ldy = y.stride(0) if y.size(0) > 1 else max(k, y.stride(0))
        out = torch.empty((self.m, k), dtype=torch.float32, device=y.device)
        arg = torch.empty((self.m, k), dtype=torch.int64, device=y.device) if reduce in ("max", "min") else None
        with torch.cuda.device(y.device):
            _check(lib().isplib_graph_spmm(self._h, MESSAGE[reduce], k, _ptr(y), ldy, _ptr(out), k, _ptr(arg), _stream(y.device)),
                   "isplib_graph_spmm")
        return out, arg

    def spmm_backward(self, dy: torch.Tensor, mean: bool = False) -> torch.Tensor:
        dy = _dev(dy, "dy", torch.float32)
        k = dy.size(1)
        dx = torch.empty((self.n, k), dtype=torch.float32, device=dy.device)
        with torch.cuda.device(dy.device):
            _check(lib().isplib_graph_spmm_backward(self._h, int(bool(mean)), k, _ptr(dy), k, _ptr(dx), k, _stream(dy.device)),
                   "isplib_graph_spmm_backward")
        return dx

    def sddmm(self, y: torch.Tensor, g: torch.Tensor, mean: bool = False, *, out=None, check: bool = True) -> torch.Tensor:
        """dA through isplib_graph_sddmm (the task plan of the handle's slice count, else the row kernel); `out` and the operand
        checks as for cabi.sddmm, `y` holding at least the handle's column count of rows.  `check`: the handle's column ids lie in
        [0, ncols) -- looked at once per handle (its graph is fixed), so a timed loop pays for it in its first call only."""
        _, _, out, ldy, ldg = _sddmm_operands(self.rowptr, self.col, y, g, out, False, self.n, "the handle")
        if check and self._cols_ok is None:
            self._cols_ok = self.col.numel() == 0 or (int(self.col.min()) >= 0 and int(self.col.max()) < self.n)
        if check and not self._cols_ok:
            raise ValueError(f"isplib_amd: the handle's column ids must lie in [0, {self.n})")
        k = y.size(1)
        with torch.cuda.device(y.device):
            _check(lib().isplib_graph_sddmm(self._h, int(bool(mean)), k, _ptr(y), ldy, _ptr(g), ldg, _ptr(out), _stream(y.device)),
                   "isplib_graph_sddmm")
        return out

    def close(self) -> None:
        if self._h:
            lib().isplib_graph_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass
