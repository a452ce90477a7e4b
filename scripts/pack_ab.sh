#!/bin/bash
# The A/B of the packed word stream (include/isplib_hip.h, PACKED WORD STREAM) that profiles/stream_packed_words.txt records: the
# default `python3 bench.py` of a PARENT tree (a built checkout of the commit before the change) against this tree, alternating,
# five runs each; this tree once more with ISPLIB_STREAM_PACK=0 / 1 / auto; the other stream configurations the kernel serves
# (K=64 unit, K=64 mean weighted, K=256 unit), three alternating runs each; then one rocprofv3 kernel trace and one FETCH_SIZE
# counter pass (a run of its own) of the parent and of this tree.
# usage: scripts/pack_ab.sh <parent tree> [outdir]     (both trees built; run from this tree's root; outdir: pack_ab_out)
# Every GPU step runs under its own timeout and the first failure ends the script: nothing is started on a card after a fault.
set -o pipefail
parent=$(realpath "$1"); root=$(pwd); out=$(realpath -m "${2:-pack_ab_out}")
[ -f "$parent/bench.py" ] || { echo "usage: scripts/pack_ab.sh <parent tree> [outdir]" >&2; exit 2; }
mkdir -p "$out"
py=$(command -v python3)
bench() {  # bench <tree> <name> [VAR=value ...] [-- bench.py arguments]
  local dir=$1 of=$out/$2.json; shift 2
  local envs=() args=()
  while [ $# -gt 0 ] && [ "$1" != "--" ]; do envs+=("$1"); shift; done
  [ "$1" == "--" ] && shift
  args=("$@")
  ( cd "$dir" && env "${envs[@]}" timeout -k 10 300 "$py" bench.py "${args[@]}" > "$of" 2> "$of.err" ) || { rc=$?; echo "FAILED rc=$rc: bench in $dir"; tail -5 "$of.err"; exit $rc; }
  "$py" -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[2], 'kernel_avg_ms', d['roofline']['kernel_avg_ms'], 'ms_per_step', d['ms_per_step'], 'value', d.get('value'))" "$of" "$(basename "$of")"
}
for i in 1 2 3 4 5; do
  bench "$parent" parent_$i || exit $?
  bench "$root" new_$i || exit $?
done
bench "$root" new_off ISPLIB_STREAM_PACK=0 || exit $?
bench "$root" new_force ISPLIB_STREAM_PACK=1 || exit $?
bench "$root" new_auto_again ISPLIB_STREAM_PACK=auto || exit $?
for cfg in "k64_unit --k 64" "k64_mean_weighted --k 64 --reduce mean --weighted" "k256_unit --k 256"; do
  set -- $cfg; name=$1; shift
  for i in 1 2 3; do
    bench "$parent" ${name}_parent_$i -- "$@" || exit $?
    bench "$root" ${name}_new_$i -- "$@" || exit $?
  done
done
trace() {  # trace <tree> <name>
  local dir=$1 name=$2
  ( cd "$dir" && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$out/kt_$name" -- "$py" bench.py --steps 20 --warmup 5 \
      > "$out/kt_$name.json" 2> "$out/kt_$name.log" ) || { rc=$?; echo "FAILED rc=$rc: trace $name"; tail -5 "$out/kt_$name.log"; exit $rc; }
  "$py" "$root/scripts/stage_trace_summary.py" "$out/kt_$name" | tee "$out/kt_$name.summary.txt"
}
trace "$parent" parent || exit $?
trace "$root" new || exit $?
pmc() {  # pmc <tree> <name>: FETCH_SIZE per dispatch, counters alone in the run
  local dir=$1 name=$2
  ( cd "$dir" && timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$out/pmc_$name" -- "$py" bench.py --steps 5 --warmup 2 \
      > "$out/pmc_$name.json" 2> "$out/pmc_$name.log" ) || { rc=$?; echo "FAILED rc=$rc: pmc $name"; tail -5 "$out/pmc_$name.log"; exit $rc; }
  "$py" "$root/scripts/pmc_summary.py" "$out/pmc_$name" | tee "$out/pmc_$name.summary.txt"
}
pmc "$parent" parent || exit $?
pmc "$root" new || exit $?
"$py" "$root/scripts/stage_trace_summary.py" --record "$out"
"$py" - "$out" <<'EOF'
import json, statistics, sys
out = sys.argv[1]
def load(name):
    j = json.loads(open("%s/%s.json" % (out, name)).read().strip().splitlines()[-1])
    return j["roofline"]["kernel_avg_ms"]
for cfg in ("k64_unit", "k64_mean_weighted", "k256_unit"):
    p = [load("%s_parent_%d" % (cfg, i)) for i in (1, 2, 3)]
    n = [load("%s_new_%d" % (cfg, i)) for i in (1, 2, 3)]
    print("%-18s kernel_avg_ms parent %s  this change %s  every new run below every parent run: %s; medians %.4f -> %.4f"
          % (cfg, " ".join("%.4f" % v for v in p), " ".join("%.4f" % v for v in n), max(n) < min(p), statistics.median(p), statistics.median(n)))
EOF
