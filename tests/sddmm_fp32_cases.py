"""Inputs shared by tests/test_gpu_sddmm_fp32.py and the census and emulation of them in tests/test_sddmm_fp32_host.py, for the fp32
value gradient dval[e] = <y[col[e], :], g[row(e), :]> (mean: / max(deg, 1)) in its three forms: sddmm_csr_kernel, sddmm_task_kernel
(isplib_amd/csrc/backward.hip) and the route through isplib_graph_sddmm (graph_runtime.hip).  The kernels' constants and selection
rules are restated here; the host test holds them against the source."""
import numpy as np

from tests import cases

N = 200                                        # columns of both graphs
LONG_ROW = 4096                                # sddmm_csr_kernel: rows with more edges are split across a workgroup's four waves
U = 4                                          # gathers per slot and step, both kernels
K_MIN, TASKS_K_MAX = 4, 1024                   # the task entry's widths (ISPLIB_K_MIN, ISPLIB_SDDMM_TASKS_K_MAX)

# float4 form: the four LPRs at their first and last width, the second 256-column trip of <4, 64> partial (260) and whole (1024)
ROW_WIDTHS_VEC4 = (4, 32, 36, 64, 68, 128, 132, 256, 260, 1024)
# scalar form (32: reached by misalignment): the three scalar instantiations at both ends, a second trip at 65
ROW_WIDTHS_SCALAR = (1, 3, 16, 17, 31, 32, 33, 41, 65, 130)
ROW_WIDTHS = tuple((k, True) for k in ROW_WIDTHS_VEC4) + tuple((k, False) for k in ROW_WIDTHS_SCALAR)
# all six instantiations whole and ragged, vfirst of 1, 2 and 3, the ragged vector in the second (258, 259) and fourth (1021)
# chunk of the NCH = 2 and 4 forms and in the third (514)
TASK_WIDTHS = (4, 5, 7, 32, 33, 41, 64, 66, 128, 130, 256, 258, 259, 512, 514, 1021, 1024)
ROW_LENGTH_WIDTHS = ((32, True), (64, True), (128, True), (256, True), (16, False), (31, False), (41, False))
TASK_LENGTH_WIDTHS = (32, 64, 128, 256, 512, 1024)
REAL_WIDTHS = (41, 64, 130, 260, 1024)
TRAP_WIDTHS = (5, 41, 66, 130, 259, 1021)
PANEL_TRAP_WIDTH, PANEL_COLS, PANEL_PITCH = 129, 64, 160       # 64-column panels: the last is columns 64..128, 65 wide and ragged

LENGTH_PLAN = (1, 4096, 0)                     # (slices, chunk, short_row): a row of at most 4096 edges is one task
HUB_PLAN = (3, 64, 16)                         # slice pieces of at most 64 edges that begin off 64-edge boundaries


def row_slot(k, vec4):
    """(VEC, LPR) of isplib_sddmm_csr_hip; `vec4`: k % 4 == 0, both pitches multiples of 4 and both bases 16-byte aligned."""
    if vec4:
        assert k % 4 == 0
        w = k // 4
        return 4, (8 if w <= 8 else 16 if w <= 16 else 32 if w <= 32 else 64)
    return 1, (16 if k <= 16 else 32 if k <= 32 else 64)


def task_slot(k):
    """(LPR, NCH) of isplib_sddmm_csr_tasks_hip: lanes per row slot and 4-column chunks per lane."""
    w = (k + 3) // 4
    for lpr in (8, 16, 32, 64):
        if w <= lpr:
            return lpr, 1
    return (64, 2) if w <= 128 else (64, 4)


def task_lane_columns(k):
    """Per (lane of a slot, chunk): (first column gathered, vfirst) by sddmm_task_kernel's column rule, or None beyond the row."""
    lpr, nch = task_slot(k)
    out = {}
    for lc in range(lpr):
        for j in range(nch):
            c = (j * lpr + lc) * 4
            if c >= k:
                out[lc, j] = None
            elif c + 4 > k:
                out[lc, j] = (k - 4, c + 4 - k)
            else:
                out[lc, j] = (c, 0)
    return out


def duplicated_columns(k):
    """The columns the task form's shifted last vector gathers a second time: [k - 4, 4 * (k // 4)), empty when k % 4 == 0."""
    return list(range(k - 4, 4 * (k // 4))) if k % 4 else []


def hub_graph():
    """300 rows over N columns, three of them empty, duplicates in every row, and a hub longer than long_row."""
    return cases.random_csr(300, N, 12, 31, empty_rows=(0, 150, 299), hub=(7, 5000), duplicates=True)


def edge_degrees():
    deg = {0, 1, 63, 64, 65, 127, 128, 129, LONG_ROW - 1, LONG_ROW, LONG_ROW + 1, 4160, 12293}
    for g in (8, 4, 2, 1):                     # G = 64 / LPR edges per gather, G * U per step
        deg |= {g - 1, g, g + 1, g * U - 1, g * U, g * U + 1}
    return sorted(deg)


def length_degrees():
    deg = edge_degrees()
    return deg + deg[::-1]                     # every length in two different wave positions of a four-row workgroup


def length_graph():
    return cases.csr_of_degrees(length_degrees(), N, 17)


def trap_rows():
    """(rows of y that hold Inf, their signs)."""
    rows = np.arange(0, N, 3)
    return rows, np.where((rows // 3) % 2 == 0, np.float32(1.0), np.float32(-1.0))


def ragged_trap(m, k, seed=43, dup=None):
    """(y [N, k], g [m, k]) for the trap of a ragged K: y holds Inf -- one sign per row, in every third row -- in exactly the columns
    the task form's shifted last vector gathers a second time (`dup`, default duplicated_columns(k)), g is finite and at least 0.5
    there, everything else is uniform.  An edge touching such a row of y is Inf of that sign; a kernel that zeroes g's duplicates
    but multiplies y's makes it Inf * 0 = NaN."""
    dup = duplicated_columns(k) if dup is None else list(dup)
    assert dup
    y, g = cases.dense(N, k, seed, "uniform"), cases.dense(m, k, seed + 1, "uniform")
    g[:, dup] = np.abs(g[:, dup]) + np.float32(0.5)
    rows, signs = trap_rows()
    for r, s in zip(rows, signs):
        y[r, dup] = s * np.float32(np.inf)
    return y, g


def subnormal_operands(m, k, seed=47):
    """y of magnitude up to 3e-38, g uniform in [-1, 1]: the products lie at the bottom of the normal range and below, and their
    partial sums in the subnormal range."""
    return cases.dense(N, k, seed, "denormal"), cases.dense(m, k, seed + 1, "uniform")


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _flushed(x):
    x = np.array(x, np.float32)
    x[np.abs(x) < np.float32(2.0 ** -126)] = 0
    return x


def emulate(rowptr, col, y, g, mean=False, form="task", flush=False, zero_times_dup=False):
    """The kernels' summation order in numpy fp32.  One rounding per fused multiply-add (formed in double -- the product of two
    floats is exact there -- and rounded once), then the pairwise tree of reduce_transposed over the slot's lanes, widest partner
    first, then the mean's fp32 1.0f / deg and one multiply.  Per lane:
      "task"  sddmm_task_kernel: its chunks in ascending order, a chunk's four columns in ascending order, one fma each (the
              duplicated components of a shifted vector contribute nothing);
      "row4"  sddmm_csr_kernel<4, LPR>: per trip of LPR * 4 columns dot_chunk<4> -- the product of the vector's LAST column, then
              an fma for each earlier one -- and one add of the chunk to the lane's accumulator;
      "row1"  sddmm_csr_kernel<1, LPR>: columns lc, lc + LPR, ...: acc += y * g, contracted to one fma.
    The two broken copies the host test needs: `flush` flushes every subnormal operand and result to zero; `zero_times_dup` (task
    form) multiplies the gathered duplicates of y by g's zeroed registers, as the kernel did before it masked y."""
    y, g = np.asarray(y, np.float32), np.asarray(g, np.float32)
    k = y.shape[1]
    deg = np.diff(rowptr)
    erow = np.repeat(np.arange(deg.size), deg)
    if flush:
        y, g = _flushed(y), _flushed(g)
    yy, gg = y[col].astype(np.float64), g[erow].astype(np.float64)
    rnd = (lambda x: _flushed(_f32(x))) if flush else _f32

    def fma(a, b, c):
        with np.errstate(invalid="ignore", over="ignore"):
            return rnd(a * b + c.astype(np.float64))

    if form == "task":
        lpr, nch = task_slot(k)
        cols = task_lane_columns(k)
        part = np.zeros((lpr, col.size), np.float32)
        for lc in range(lpr):
            for j in range(nch):
                if cols[lc, j] is None:
                    continue
                first, vfirst = cols[lc, j]
                for c in range(first, first + 4):
                    if c >= first + vfirst:
                        part[lc] = fma(yy[:, c], gg[:, c], part[lc])
                    elif zero_times_dup:
                        part[lc] = fma(yy[:, c], np.float64(0.0), part[lc])
    elif form in ("row4", "row1"):
        vec, lpr = row_slot(k, form == "row4")
        part = np.zeros((lpr, col.size), np.float32)
        for lc in range(lpr):
            for c in range(lc * vec, k, lpr * vec):
                if vec == 1:
                    part[lc] = fma(yy[:, c], gg[:, c], part[lc])
                else:
                    with np.errstate(invalid="ignore", over="ignore"):
                        chunk = rnd(yy[:, c + 3] * gg[:, c + 3])
                        for v in (2, 1, 0):
                            chunk = fma(yy[:, c + v], gg[:, c + v], chunk)
                        part[lc] = rnd(part[lc].astype(np.float64) + chunk)
    else:
        raise ValueError(form)
    with np.errstate(invalid="ignore", over="ignore"):
        while part.shape[0] > 1:               # the butterfly: halves of the slot, widest first
            h = part.shape[0] // 2
            part = rnd(part[:h].astype(np.float64) + part[h:])
        out = part[0]
        if mean:
            out = rnd(out.astype(np.float64) * (np.float32(1.0) / np.maximum(deg, 1).astype(np.float32))[erow])
    return out
