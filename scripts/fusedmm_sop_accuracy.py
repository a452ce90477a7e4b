#!/usr/bin/env python3
"""What the scalar stage of the FusedMM kernels achieves on this part: the single-edge probe of tests/fusedmm_cases.py (row i
holds the one edge (i, i); on the dot word x_i = (1, 0, ...), y_j = (s_j, 1, 0, ...), so z[i, 1] is the device's f(s_j) with
nothing else rounded; on the norm word y_j = (a_j, 0, ...), s = a_j^2 exactly and z[i, 0] = f(s) a_j) over 4096 values of s,
against the fp64 menu of tests/fusedmm_ref.py, in units of the model error of tests/fusedmm_bound.py (sop_model).

Row form (fusedmm_general.hip) and stream form at 8 streams (fusedmm_stream.hip); the task form shares sop_apply with the row
form and is asserted to give the same bits.  Prints, per menu entry, word and form, the largest ratio and where it occurs, then
C_f = four times the largest ratio of a kernel file, rounded up to a power of two: the constants of tests/fusedmm_bound.py and
the table of DESIGN.md 4.6a.  The committed output is profiles/fusedmm_sop_accuracy.txt:

    python3 scripts/fusedmm_sop_accuracy.py --out profiles/fusedmm_sop_accuracy.txt
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from isplib_amd import cabi  # noqa: E402
from isplib_amd.plan import build_task_plan  # noqa: E402
from tests import fusedmm_bound as fb  # noqa: E402
from tests import fusedmm_cases as fc  # noqa: E402

NPTS, K, STREAMS = 4096, 8, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    to = lambda a: torch.from_numpy(a).to(dev)                                     # noqa: E731
    rowptr, col = fc.probe_graph(NPTS)
    d_rowptr, d_col = to(rowptr), to(col)
    tasks = build_task_plan(d_rowptr, d_col, NPTS, 4, 256, 16)
    stream = cabi.NativeStreamPlan(d_rowptr, d_col, None, NPTS, STREAMS, 1, 64, 4, fusedmm=True)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# scripts/fusedmm_sop_accuracy.py on {arch}: {NPTS} single-edge rows, k = {K}, menu parameter {fc.PARAM}",
             "# ratio = max over the grid of (|f_device - f_fp64| - floor) / df(s), df = tests/fusedmm_bound.py: sop_model",
             f"# {'entry':<18} {'word':<5} {'form':<7} {'max ratio':>10}   at s"]
    worst = {"general": {}, "stream": {}}
    for fn in fc.MENU:
        kind = fb.KINDS[fn]
        for word_name, word in (("dot", fc.DOT_WORD), ("norm", fc.NORM_WORD)):
            if word_name == "dot":
                s = fc.probe_grid(fn, NPTS)
                x, y = fc.probe_dot(s, K)
                column, factor = 1, None
            else:
                a = fc.probe_norm_args(fn, NPTS)
                s = a.astype(np.float64) ** 2
                x, y = fc.probe_norm(a, K)
                column, factor = 0, a
            d_x, d_y = to(x), to(y)
            outs = {}
            for form in ("row", "task", "stream"):
                nan = torch.full((NPTS, K), float("nan"), device=dev)
                if form == "stream":
                    cabi.fusedmm_stream(word, d_rowptr, col.size, stream, d_x, d_y, sop_udef=fn, sop_param=fc.PARAM, out=nan)
                else:
                    cabi.fusedmm(word, d_rowptr, d_col, None, d_x, d_y, sop_udef=fn, sop_param=fc.PARAM, plan=tasks if form == "task" else None, out=nan)
                outs[form] = nan.cpu().numpy()
            assert np.array_equal(outs["row"], outs["task"], equal_nan=True), (fn, word_name, "task form differs from the row form")
            for form, file in (("row", "general"), ("stream", "stream")):
                got = outs[form][:, column]
                assert not np.any(np.isnan(got)), (fn, word_name, form)
                excess, df = fb.probe_excess(kind, fc.PARAM, s, got, factor)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(df > 0, excess / df, np.where(excess > 0, np.inf, 0.0))
                w = int(np.argmax(ratio))
                worst[file][kind] = max(worst[file].get(kind, 0.0), float(ratio[w]))
                lines.append(f"  {fn:<18} {word_name:<5} {form:<7} {ratio[w]:>10.3f}   {float(s[w]):.9g}")
    lines.append("#")
    lines.append("# C_f = 4 x the largest ratio of the kernel file, rounded up to a power of two (at least 1)")
    lines.append(f"# {'entry':<18} {'general max':>12} {'C_f':>6} {'stream max':>12} {'C_f':>6}")
    for fn in fc.MENU:
        kind = fb.KINDS[fn]
        cell = []
        for file in ("general", "stream"):
            mx = worst[file][kind]
            cf = 2.0 ** max(0, math.ceil(math.log2(4.0 * mx))) if mx > 0 else 1.0
            cell.append(f"{mx:>12.3f} {cf:>6g}")
        lines.append(f"  {fn:<18} {cell[0]} {cell[1]}")
    stream.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
