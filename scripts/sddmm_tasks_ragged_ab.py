#!/usr/bin/env python3
"""dA through the task plan (isplib_graph_sddmm with the whole-row slice rule) on the reddit-like benchmark graph at the ragged
widths k = 41 and 130 and, as a control, at k = 128: one JSON line of HIP-event times per process.

    python scripts/sddmm_tasks_ragged_ab.py LABEL [--out FILE]

A process loads one build of libisplib_hip.so, so an A/B of two commits is three processes in one sitting -- parent, this commit,
parent again -- with the library beside the package replaced between them (profiles/sddmm_tasks_ragged_ab.txt).  Per width: 3 warm-up
launches, then 7 batches of 10 launches; median, min and max of the batch means in ms per launch.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from isplib_amd import cabi, synth  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("label")
    p.add_argument("--out", default="", help="append the JSON line to this file as well")
    args = p.parse_args()
    dev = torch.device("cuda:0")
    rowptr, col, n = synth.dataset_like("reddit", device=dev)
    h = cabi.GraphHandle(rowptr, col, None, n)
    res = {"label": args.label, "n": n, "nnz": int(col.numel())}
    for k in (41, 130, 128):
        xs, gs = synth.features(n, k, device=dev), synth.features(n, k, seed=5, device=dev)
        for _ in range(3):
            h.sddmm(xs, gs)
        torch.cuda.synchronize()
        batches = []
        for _ in range(7):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(10):
                h.sddmm(xs, gs)
            e.record()
            torch.cuda.synchronize()
            batches.append(s.elapsed_time(e) / 10)
        res[f"k{k}_ms_median"] = round(statistics.median(batches), 4)
        res[f"k{k}_ms_min"] = round(min(batches), 4)
        res[f"k{k}_ms_max"] = round(max(batches), 4)
        res[f"k{k}_slices"] = int(cabi.lib().isplib_suggest_slices_whole_rows(n, n, int(col.numel()), k))
        del xs, gs
    h.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
