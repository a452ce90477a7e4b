#!/bin/bash
# The A/B of the levelled deal (include/isplib_hip.h, isplib_stream_capacities_hip) that profiles/stream_level_ab.txt records: the
# default `python3 bench.py` of a PARENT tree (a built checkout of the commit before the change) against this tree, alternating,
# five runs each; this tree once more with ISPLIB_STREAM_LEVEL=0; `bench.py --dump-outputs` of both, compared bit for bit; then
# one rocprofv3 kernel trace of each, summarised per dispatch by scripts/stage_trace_summary.py; last the other stream configurations
# (mean K=64 weighted, sum K=128 weighted, sum K=64 / 32 / 41 / 256), three alternating runs each, and the 16-bit kernel on a
# levelled against an unlevelled plan (scripts/half_ab.py, twice each).
# usage: scripts/level_ab.sh <parent tree> [outdir]     (both trees built; run from this tree's root; outdir: level_ab_out)
# Every GPU step runs under its own timeout and the first failure ends the script: nothing is started on a card after a fault.
set -o pipefail
parent=$(realpath "$1"); root=$(pwd); out=$(realpath -m "${2:-level_ab_out}")
[ -f "$parent/bench.py" ] || { echo "usage: scripts/level_ab.sh <parent tree> [outdir]" >&2; exit 2; }
mkdir -p "$out"
py=$(command -v python3)
bench() {  # bench <tree> <name> [VAR=value ...] [-- bench.py arguments]
  local dir=$1 of=$out/$2.json; shift 2
  local envs=() args=()
  while [ $# -gt 0 ] && [ "$1" != "--" ]; do envs+=("$1"); shift; done
  [ "$1" = "--" ] && shift; args=("$@")
  ( cd "$dir" && env "${envs[@]}" timeout -k 10 300 "$py" bench.py "${args[@]}" > "$of" 2> "$of.err" ) || { rc=$?; echo "FAILED rc=$rc: bench in $dir"; tail -5 "$of.err"; exit $rc; }
  "$py" -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[2], 'kernel_avg_ms', d['roofline']['kernel_avg_ms'], 'ms_per_step', d['ms_per_step'])" "$of" "$(basename "$of")"
}
for i in 1 2 3 4 5; do
  bench "$parent" parent_$i || exit $?
  bench "$root" new_$i || exit $?
done
bench "$root" new_off ISPLIB_STREAM_LEVEL=0 || exit $?
"$py" - "$out" <<'PY'
import json, statistics, sys
out = sys.argv[1]
def runs(name, key):
    return [(lambda d: d["roofline"]["kernel_avg_ms"] if key == "kernel_avg_ms" else d[key])(json.loads(open(f"{out}/{name}_{i}.json").read().strip().splitlines()[-1])) for i in range(1, 6)]
for key in ("kernel_avg_ms", "ms_per_step"):
    p, n = runs("parent", key), runs("new", key)
    spread = max(p) - min(p)
    diff = statistics.median(p) - statistics.median(n)
    print(f"{key}: parent {min(p):.4f} .. {max(p):.4f} (median {statistics.median(p):.4f}, spread {spread:.4f}); this change {min(n):.4f} .. {max(n):.4f} "
          f"(median {statistics.median(n):.4f}); every new run below every parent run: {max(n) < min(p)}; median difference {diff:.4f} = {diff / spread:.1f} x the parent's spread")
PY
bench "$parent" dump_parent -- --dump-outputs "$out/dump_parent" || exit $?
bench "$root" dump_new -- --dump-outputs "$out/dump_new" || exit $?
"$py" - "$out" <<'PY'
import glob, os, sys
import numpy as np
out = sys.argv[1]
names = sorted(os.path.basename(p) for p in glob.glob(f"{out}/dump_parent/*.npy"))
assert names, "no outputs dumped"
for n in names:
    a, b = np.load(f"{out}/dump_parent/{n}"), np.load(f"{out}/dump_new/{n}")
    print(f"--dump-outputs {n}: shape {a.shape}, bitwise equal: {a.shape == b.shape and a.tobytes() == b.tobytes()}")
PY
rm -r "$out/dump_parent" "$out/dump_new"                  # 48 MB each
trace() {  # trace <tree> <name> [VAR=value ...]
  local dir=$1 name=$2; shift 2
  ( cd "$dir" && env "$@" timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/kt_$name" -- "$py" bench.py --steps 20 --warmup 5 \
      > "$out/kt_$name.json" 2> "$out/kt_$name.log" ) || { rc=$?; echo "FAILED rc=$rc: trace $name"; tail -5 "$out/kt_$name.log"; exit $rc; }
  echo "-- $name"; "$py" "$root/scripts/stage_trace_summary.py" "$out/kt_$name" | tee "$out/kt_$name.summary.txt"
}
trace "$parent" parent || exit $?
trace "$root" new || exit $?
for cfg in "mean64w:--reduce mean --k 64 --weighted" "sum128w:--weighted" "sum64:--k 64" "sum32:--k 32" "sum41:--k 41" "sum256:--k 256"; do
  name=${cfg%%:*}; flags=${cfg#*:}
  for i in 1 2 3; do
    bench "$parent" ${name}_parent_$i -- --no-extra --no-cpu-baseline $flags || exit $?
    bench "$root" ${name}_new_$i -- --no-extra --no-cpu-baseline $flags || exit $?
  done
done
for i in 1 2; do
  ISPLIB_STREAM_LEVEL=0 timeout -k 10 300 "$py" scripts/half_ab.py --runs 3 --out "$out/half_unlevelled_$i.txt" > /dev/null 2> "$out/half.err" || { rc=$?; echo "FAILED rc=$rc: half_ab"; tail -5 "$out/half.err"; exit $rc; }
  timeout -k 10 300 "$py" scripts/half_ab.py --runs 3 --out "$out/half_levelled_$i.txt" > /dev/null 2> "$out/half.err" || { rc=$?; echo "FAILED rc=$rc: half_ab"; tail -5 "$out/half.err"; exit $rc; }
done
grep -H native "$out"/half_*levelled_*.txt
