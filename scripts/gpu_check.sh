#!/bin/bash
# usage (on a GPU machine): [OUT=dir] bash scripts/gpu_check.sh [bench args...]; logs go to $OUT (default check_out/)
OUT=${OUT:-check_out}
mkdir -p "$OUT"
python -m pytest tests -m gpu -q 2>&1 | tail -n 120 > "$OUT/test.log"
grep -E "passed|failed|error" "$OUT/test.log" | tail -3
python bench.py --steps 10 --warmup 3 --full --no-cpu-baseline "$@" > "$OUT/bench.json" 2> "$OUT/bench.err"
OUT="$OUT" python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ["OUT"], "bench.json")))
print("value", round(d["value"]), "ms/step", round(d["ms_per_step"], 3), d["config"]["launch"])
print("roofline", d["roofline"])
print("kernels ms/step", {k: round(v, 3) for k, v in d["kernels_ms_per_step"].items()})
print("kernels GB/s", {k: round(v) for k, v in d["kernels_gbps"].items()})
print("kernels TFLOP/s", {k: round(v, 1) for k, v in d.get("kernels_tflops", {}).items()})
PY
grep -v Warn "$OUT/bench.err" | grep -v amdgpu.ids | tail -5
