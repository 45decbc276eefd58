#!/bin/bash
# small graphs A/B on one box: parity tests, then intel / m3500 / dlr bench lines for a list of environments -> OUT/
# usage: scripts/gpu_small.sh OUT [notests] ; environments in $ENVS (";"-separated, "-" = default)
OUT=$1
mkdir -p "$OUT"
if [ "$2" != "notests" ]; then timeout -k 10 600 python -m pytest tests -m gpu -x -q > "$OUT"/pytest.log 2>&1; tail -3 "$OUT"/pytest.log; fi
IFS=';' read -ra EV <<< "${ENVS:--;RR_PGO_LDS_FLOW=0}"
for W in ${WORKLOADS:-intel m3500 dlr}; do
  for E in "${EV[@]}"; do
    N=$(echo "$E" | tr ' =' '__')
    if [ "$E" = "-" ]; then E=""; fi
    env $E timeout -k 10 120 python bench.py --workload $W --precision ${PREC:-f64} --steps 200 --warmup 20 --full --no-cpu-baseline --no-secondary > "$OUT"/bench_${W}_$N.json 2>"$OUT"/bench_${W}_$N.err || { echo "FAILED $W $E"; tail -3 "$OUT"/bench_${W}_$N.err; continue; }
    python3 -c "
import json; d=json.loads(open('$OUT/bench_${W}_$N.json').read().strip().splitlines()[-1]); print('$W', '[$E]', round(d['value'],1), 'it/s', round(d['ms_per_step']*1000,1), 'us', {k: round(v,1) for k, v in d['roofline']['per_step_us_by_kernel_class'].items() if v}, d['errors'][-1], 'launches', d['launches_per_step'])"
  done
done
