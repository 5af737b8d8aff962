#!/bin/bash
# Interleaved same-box A/B of bench.py between this tree and a second checkout (built beforehand):
#   tools/ab_tree.sh scratch/base [reps=3] [bench args]
# Bench lines (--full, for the gather-GEMM roofline) and their stderr go to $OUT (default runs/).
B=$1; REPS=${2:-3}; shift 2 || true
OUT=${OUT:-runs}
mkdir -p "$OUT"
for rep in $(seq 1 $REPS); do
  for t in "$B" .; do
    F="$OUT/ab_tree_$(basename $t)_${rep}"
    FULL=; grep -q '"--full"' "$t/bench.py" && FULL=--full      # checkouts older than --full print the roofline without it
    ( cd $t && timeout -k 10 200 python bench.py --steps 300 --warmup 30 $FULL --no-cpu-baseline --no-extra-paths "$@" ) > "$F.json" 2> "$F.err" || { echo "bench failed in $t"; tail -3 "$F.err"; exit 1; }
    python - <<PY
import json
d = json.loads(open("$F.json").read().strip().splitlines()[-1])
print("$t rep $rep:", d["value"], d["ms_per_step"], "gg frac", d["roofline"]["frac"], flush=True)
PY
  done
done
