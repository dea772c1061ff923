#!/bin/bash
# quick GPU check of a contact-law change: parity tests of the contact scenes + the two contact benches.   tools/gpu_parity_quick.sh <output dir>
OUT=${1:?usage: tools/gpu_parity_quick.sh <output dir>}
mkdir -p "$OUT"
python -m pytest tests/test_gpu_parity.py tests/test_gpu_state_parity.py tests/test_gpu_sampler_shards.py -m gpu -q -s 2>&1 | grep -v "^$" > "$OUT/parity.log"
grep "vs fp64\|passed\|failed\|Error\|assert " "$OUT/parity.log" | cut -c1-330 | head -60
for w in boxer_push panda_pick; do python bench.py --full --no-cpu-baseline --workload $w > "$OUT/bench_$w.json"; done
python - "$OUT" <<'PY'
import json, os, sys
for w in ("boxer_push", "panda_pick"):
    d = json.loads(open(os.path.join(sys.argv[1], "bench_%s.json" % w)).read().strip().splitlines()[-1]); print(w, d["value"], d["kernels_ms"], d["config"].get("task_outcome"))
PY
