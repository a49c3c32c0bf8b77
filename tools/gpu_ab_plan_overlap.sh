#!/bin/bash
# tests of the new schedule, then a same-box A/B of the headline line:
# base = parent library, in line; new = this tree's library, default schedule;
# newinl = this tree's library, --no-plan-overlap.  RUNS rounds, alternating.
cd "$(dirname "$0")/.." || exit 1  # the repository root
OUT=${OUT_ROOT:-out}/${OUT_TAG:-ab_plan_overlap}
mkdir -p "$OUT"
FL="--no-sharded --no-neumf --no-eval --no-large --no-cpu-baseline"
step() {  # step <seconds> <log> <cmd...>: stop everything at the first failure
  local t=$1 log=$2; shift 2
  timeout -k 10 "$t" "$@" > "$log" 2> "$log.err"
  local rc=$?
  if [ $rc -ne 0 ]; then echo "FAILED rc=$rc: $*"; tail -n 30 "$log"; tail -n 30 "$log.err"; exit $rc; fi
}
if [ "${TESTS:-1}" = 1 ]; then
  step 400 "$OUT/tests.log" python3 -u -m pytest -q -x -m gpu --durations=8 tests/test_gpu_plan_beside_stream.py tests/test_gpu_plan.py
  tail -12 "$OUT/tests.log"
fi
for r in $(seq 1 "${RUNS:-3}"); do
  for v in ${VARIANTS:-base new newinl}; do
    case $v in
      base) export ACF_ALT_LIB=tools/ab/base.so; X="--no-plan-overlap" ;;
      new) unset ACF_ALT_LIB; X="" ;;
      newinl) unset ACF_ALT_LIB; X="--no-plan-overlap" ;;
    esac
    D=""
    if [ "$r" = 1 ]; then D="--dump-outputs $OUT/dump_$v"; fi
    step 200 "$OUT/d_${v}_$r.json" python3 tools/bench_lib.py --gpus 1 $FL $X $D
    if [ "${SHORT:-1}" = 1 ]; then
      step 200 "$OUT/s_${v}_$r.json" python3 tools/bench_lib.py --gpus 1 $FL $X --steps 20 --warmup 5
    fi
    python3 - "$v" "$r" "$OUT" <<'EOF'
import json, sys
v, r, out = sys.argv[1:]
def last(p):
    try:
        return json.loads(open(p).read().strip().splitlines()[-1])
    except Exception:
        return None
d, s = last(f"{out}/d_{v}_{r}.json"), last(f"{out}/s_{v}_{r}.json")
print(v, r, "default", d and (d["value"], d["step_errors"], d["stream_recoveries"]),
      "steps20", s and (s["value"], s["step_errors"], s["stream_recoveries"]), flush=True)
EOF
  done
done
unset ACF_ALT_LIB
python3 - "$OUT" <<'EOF'
import glob, os, sys
import numpy as np
out = sys.argv[1]
for v in ("new", "newinl"):
    for f in sorted(glob.glob(f"{out}/dump_base/*.npy")):
        g = f.replace("dump_base", f"dump_{v}")
        if os.path.exists(g):
            print("bitcmp", v, os.path.basename(f), bool(np.array_equal(np.load(f), np.load(g))))
EOF
rm -rf "$OUT"/dump_*
