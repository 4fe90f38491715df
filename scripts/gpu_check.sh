#!/bin/bash
# Usage (on a GPU box): bash scripts/gpu_check.sh "cfg2 cfg5" [pytest-args]
# Runs the GPU parity tests, then bench.py --full (with `host_api`) for the named configs; logs under $PYA_OUT (bench_out/).
cd ${GRAFT_REPO_ROOT:-.}
OUT=${PYA_OUT:-bench_out}
mkdir -p $OUT
CFGS=${1:-cfg2}
shift
timeout 1200 python -m pytest tests -m gpu -x -q "$@" 2>&1 > $OUT/gpu_tests.log; grep -E "passed|failed|error" $OUT/gpu_tests.log | tail -5
for c in $CFGS; do
  timeout 600 python bench.py --full --config $c --steps 5 --warmup 2 --no-cpu-baseline --no-other-configs 2>&1 | tail -1 > $OUT/bench_$c.json
  python - <<PY
import json
d = json.load(open("$OUT/bench_$c.json"))
print("$c", "%.3g PSMs/s" % d["value"], "ms/step %.3f" % d["ms_per_step"], {k.replace("pya_","").replace("_kernel",""): round(v,3) for k,v in d["roofline"]["kernel_ms"].items()}, "host_api %.3g" % d["host_api"]["value"])
PY
done
