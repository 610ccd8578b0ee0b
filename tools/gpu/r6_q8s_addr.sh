#!/bin/bash
# round 6: q8s phase probe, the int8 GPU tests and the bench line's int8 side objects.  usage: bash tools/gpu/r6_q8s_addr.sh OUTDIR
O=${1:?usage: bash tools/gpu/r6_q8s_addr.sh OUTDIR}
mkdir -p "$O"
timeout -k 10 200 ./tools/q8s_phase_probe > "$O/q8s_phase_final.txt" 2>&1
timeout -k 10 1500 python -m pytest tests -x -q -m gpu -k "int8 or q8 or headline or batch or reproducible or pipeline_groups" 2>&1 | tail -5 > "$O/tests.log"
timeout -k 10 900 python bench.py --full --no-cpu-baseline > "$O/bench.json" 2> "$O/bench.err"
cat "$O/tests.log"
python - "$O/bench.json" <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print(d['value'], d['int8_decode']['tokens_per_s'], d['int8_decode']['kernels'], d['int8_decode']['pods_batched'])
PY
