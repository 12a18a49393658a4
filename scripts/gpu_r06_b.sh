#!/bin/bash
# r06 call B: new + touched GPU tests, the default bench line (new keys: step_split_ms, default_auto, configs_4), same-box short benches.
set -u
OUT=${1:?usage: gpu_r06_b.sh OUTPUT_DIR}; mkdir -p "$OUT"; export TMPDIR=/tmp
echo "== new + touched tests"; timeout 1800 python -m pytest tests/test_gpu_r06.py tests/test_gpu_debug.py tests/test_gpu_e2e.py -q -m gpu -p no:cacheprovider -s 2>&1 | grep -E "^\[|passed|failed|FAILED|Error|error" | tail -120 | tee $OUT/r06_b_tests.log | tail -60
echo "== bench default"; timeout 900 python bench.py --steps 10 --warmup 3 --full 2>&1 | tail -1 | tee $OUT/r06_b_bench.json | cut -c1-200
python - "$OUT" <<'PY'
import json, sys
d = json.load(open(sys.argv[1] + "/r06_b_bench.json"))
for k in ("value", "step_split_ms", "default_auto", "configs_4", "configs_1", "e2e_host_stream", "latency_ms", "roofline_depthwise_all", "parity"):
    print(k, json.dumps(d.get(k))[:400])
PY
