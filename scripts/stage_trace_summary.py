"""Helpers of scripts/stage_ab.sh.
  stage_trace_summary.py <rocprofv3 output dir>   per-dispatch times of one kernel trace: the stream kernel by its position among a
                                                   call's four dispatches, the staging copy, the hub fold (first fifth dropped: warm-up)
  stage_trace_summary.py --record <outdir>        the table of profiles/stream_stage_panels.txt from the runs stage_ab.sh left there,
                                                   with the gain criterion worked out"""
import csv
import glob
import json
import os
import statistics
import sys


def trace(path):
    rows = []
    for f in glob.glob(path + "/**/*kernel_trace.csv", recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    seq, pos = {}, 0
    for s, e, n in rows:
        if "stream_stage_copy" in n:
            seq.setdefault("stage copy (before dispatch %d)" % (pos % 4 + 1), []).append((e - s) / 1e6)
        elif "sweep_hub_fold" in n:
            seq.setdefault("hub fold", []).append((e - s) / 1e6)
        elif "spmm_stream_kernel" in n:
            seq.setdefault("stream dispatch %d" % (pos % 4 + 1), []).append((e - s) / 1e6)
            pos += 1
    for k in sorted(seq):
        v = seq[k][len(seq[k]) // 5:]
        print("%-34s n=%3d  median %.4f ms  min %.4f  max %.4f" % (k, len(v), statistics.median(v), min(v), max(v)))


def record(d):
    def load(name):
        j = json.loads(open(os.path.join(d, name + ".json")).read().strip().splitlines()[-1])
        return j["roofline"]["kernel_avg_ms"], j["ms_per_step"]
    P = [load("parent_%d" % i) for i in range(1, 6)]
    N = [load("new_%d" % i) for i in range(1, 6)]
    print("run   parent: kernel_avg_ms  ms_per_step     this change: kernel_avg_ms  ms_per_step")
    for i in range(5):
        print("%3d   %21.4f  %11.4f     %26.4f  %11.4f" % (i + 1, P[i][0], P[i][1], N[i][0], N[i][1]))
    for col, name in ((0, "kernel_avg_ms"), (1, "ms_per_step")):
        p, n = [x[col] for x in P], [x[col] for x in N]
        spread, md = max(p) - min(p), statistics.median(p) - statistics.median(n)
        print("%s: parent %.4f .. %.4f (median %.4f, spread %.4f); this change %.4f .. %.4f (median %.4f); every new run below every "
              "parent run: %s; median difference %.4f = %.1f x the parent's spread (criterion: >= 3)"
              % (name, min(p), max(p), statistics.median(p), spread, min(n), max(n), statistics.median(n), max(n) < min(p), md,
                 md / spread if spread else float("inf")))
    for name in ("new_off", "new_force", "new_auto_again"):
        if os.path.exists(os.path.join(d, name + ".json")):
            print("%s: kernel_avg_ms %.4f  ms_per_step %.4f" % ((name,) + load(name)))


if __name__ == "__main__":
    record(sys.argv[2]) if sys.argv[1] == "--record" else trace(sys.argv[1])
