#!/bin/bash
# rocprofv3 kernel trace of the default bench line (six chunks; tools/profile_bench.sh
# profiles a one-chunk call): parent library (tools/ab/base.so) in line
# (base) and this tree's library with its default schedule (new).  No counters.
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT_ROOT:-out}/prof_plan_overlap
mkdir -p "$OUT"
FL="--no-sharded --no-neumf --no-eval --no-large --no-cpu-baseline"
for v in ${VARIANTS:-base new}; do
  case $v in
    base) export ACF_ALT_LIB=tools/ab/base.so; X="--no-plan-overlap" ;;
    new) unset ACF_ALT_LIB; X="" ;;
  esac
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -f csv -d "$OUT/$v" -o bench -- python3 tools/bench_lib.py --gpus 1 $FL $X > "$OUT/bench_$v.json" 2> "$OUT/bench_$v.err"
  rc=$?
  if [ $rc -ne 0 ]; then echo "FAILED rc=$rc ($v)"; tail -n 30 "$OUT/bench_$v.err"; exit $rc; fi
  tail -n 1 "$OUT/bench_$v.json" | cut -c1-400
done
unset ACF_ALT_LIB
python3 tools/plan_overlap_trace.py "$OUT"
find "$OUT" -name "*.csv" -size +200k -delete
find "$OUT" -name "*.csv"
