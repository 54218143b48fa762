#!/bin/bash
# A/B of the two routes of the packed all-reduce on a world-size-1 RCCL group (run on the GPU box): alternating processes.
# usage: tools/rccl_ws1_ab.sh <tag> [rounds]   -> $VQ_OUT/<tag>_{torch,direct}_<i>.json (default out/) + a summary
tag=$1; rounds=${2:-3}
cd /root/repo
out=${VQ_OUT:-out}; mkdir -p "$out"      # output directory (default out/ in the repository)
for i in $(seq 1 $rounds); do
  for route in torch direct; do
    VQ_FORCE_EXCHANGE=1 VQHIP_ALLREDUCE=$route timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node=1 --master-addr 127.0.0.1 --master-port $((29520 + i)) bench.py --workload cvq --full --min-seconds 2 --no-cpu-baseline > "$out/${tag}_${route}_$i.json" 2> "$out/${tag}_${route}_$i.err" || echo "$route $i failed"
  done
done
python3 - $tag $rounds "$out" <<'PY'
import json, sys
tag, rounds, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
for route in ('torch', 'direct'):
    rows = []
    for i in range(1, rounds + 1):
        try:
            d = json.loads(open(f'{out}/{tag}_{route}_{i}.json').read().strip().splitlines()[-1])
        except Exception as e:
            print(route, i, 'ERR', e); continue
        c = d['cvq']
        rows.append((c['ms_per_step'], c.get('ms_per_step_graphed'), c['collective_ms'], c['exchange_route']['direct'], c.get('graphed_error')))
    print(route, [tuple(round(v, 4) if isinstance(v, float) else v for v in r) for r in rows])
PY
