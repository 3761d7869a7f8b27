#!/bin/bash
# Scan / select tests + the scan legs of the bench (no encoders' side legs).
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}       # where the outputs go
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout 1500 python -m pytest tests/test_scan_gpu.py tests/test_scan_sweep_gpu.py tests/test_abi_sweeps_gpu.py tests/test_pipeline_gpu.py -m gpu -x -q 2>&1 | tail -15 | tee "$OUT"/pytest_scan.log
timeout 900 python bench.py --full --no-cpu-baseline --no-surface-leg --no-config5-leg --no-fp8-leg --no-reference-leg --no-fp16-leg > "$OUT"/bench_scan.json 2> "$OUT"/bench_scan.err
tail -3 "$OUT"/bench_scan.err
OUT=$OUT python - <<'PY'
import json
import os
j = json.load(open(os.environ["OUT"] + "/bench_scan.json"))
c = j["config"]
print("headline", j["value"], "ms/step", j["ms_per_step"], "stage", j["stage_ms_per_step"])
print("scan_only", {k: v for k, v in c["scan_only"].items() if k != "what"})
print("shard", {k: v for k, v in c["scan_only_shard"].items() if k != "what"})
PY
