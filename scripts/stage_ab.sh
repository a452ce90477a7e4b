#!/bin/bash
# The A/B of the staged column panels (include/isplib_hip.h, isplib_stream_stage_panel) that profiles/stream_stage_panels.txt
# records: the default `python3 bench.py` of a PARENT tree (a built checkout of the commit before the change) against this
# tree, alternating, five runs each; this tree once more with ISPLIB_STREAM_STAGE=0 / 1 / auto; then one rocprofv3 kernel
# trace of the parent, of auto and of forced staging, each summarised per dispatch by scripts/stage_trace_summary.py.
# usage: scripts/stage_ab.sh <parent tree> [outdir]     (both trees built; run from this tree's root; outdir: stage_ab_out)
# Every GPU step runs under its own timeout and the first failure ends the script: nothing is started on a card after a fault.
set -o pipefail
parent=$(realpath "$1"); root=$(pwd); out=$(realpath -m "${2:-stage_ab_out}")
[ -f "$parent/bench.py" ] || { echo "usage: scripts/stage_ab.sh <parent tree> [outdir]" >&2; exit 2; }
mkdir -p "$out"
py=$(command -v python3)
bench() {  # bench <tree> <name> [VAR=value ...]
  local dir=$1 of=$out/$2.json; shift 2
  ( cd "$dir" && env "$@" timeout -k 10 300 "$py" bench.py > "$of" 2> "$of.err" ) || { rc=$?; echo "FAILED rc=$rc: bench in $dir"; tail -5 "$of.err"; exit $rc; }
  "$py" -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[2], 'kernel_avg_ms', d['roofline']['kernel_avg_ms'], 'ms_per_step', d['ms_per_step'])" "$of" "$(basename "$of")"
}
for i in 1 2 3 4 5; do
  bench "$parent" parent_$i || exit $?
  bench "$root" new_$i || exit $?
done
bench "$root" new_off ISPLIB_STREAM_STAGE=0 || exit $?
bench "$root" new_force ISPLIB_STREAM_STAGE=1 || exit $?
bench "$root" new_auto_again ISPLIB_STREAM_STAGE=auto || exit $?
trace() {  # trace <tree> <name> [VAR=value ...]
  local dir=$1 name=$2; shift 2
  ( cd "$dir" && env "$@" timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/kt_$name" -- "$py" bench.py --steps 20 --warmup 5 \
      > "$out/kt_$name.json" 2> "$out/kt_$name.log" ) || { rc=$?; echo "FAILED rc=$rc: trace $name"; tail -5 "$out/kt_$name.log"; exit $rc; }
  "$py" "$root/scripts/stage_trace_summary.py" "$out/kt_$name" | tee "$out/kt_$name.summary.txt"
}
trace "$parent" parent || exit $?
trace "$root" new_auto ISPLIB_STREAM_STAGE=auto || exit $?
trace "$root" new_force ISPLIB_STREAM_STAGE=1 || exit $?
"$py" "$root/scripts/stage_trace_summary.py" --record "$out"
