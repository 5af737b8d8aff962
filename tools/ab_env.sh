#!/bin/bash
# Interleaved A/B of bench.py under values of one environment variable:  tools/ab_env.sh VAR "v1 v2 ..." [reps=2] [bench args]
# Bench lines (--full, for the gather-GEMM roofline) and their stderr go to $OUT (default runs/).
set -e
VAR=$1; VALS=$2; REPS=${3:-2}; shift 3 || true
OUT=${OUT:-runs}
mkdir -p "$OUT"
for rep in $(seq 1 $REPS); do
  for v in $VALS; do
    F="$OUT/ab_env_${VAR}_$(basename $v)_${rep}"
    env $VAR=$v timeout -k 10 200 python bench.py --steps 300 --warmup 30 --full --no-cpu-baseline --no-extra-paths "$@" > "$F.json" 2> "$F.err"
    python - <<PY
import json
d = json.loads(open("$F.json").read().strip().splitlines()[-1])
print("$VAR=$v rep $rep:", d["value"], d["ms_per_step"], "gg frac", d["roofline"]["frac"], flush=True)
PY
  done
done
