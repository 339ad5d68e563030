#!/bin/bash
# In-model A/B of library builds on ONE box: bench.py (no legs, no CPU baseline) alternating between the libraries, N rounds.
#   tools/ab_bench.sh OUT.jsonl libA.so libB.so [...]      (run on the GPU box from the repo root)
OUT=$1; shift
: > $OUT
for round in 1 2 3; do
  for lib in "$@"; do
    IRM_HIP_LIB=$lib python3 bench.py --full --steps 6 --warmup 2 --no-legs --no-cpu-baseline 2>/dev/null | python3 -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print(json.dumps({'lib':'$lib','round':$round,'ms_per_frame':d['ms_per_frame'],'kernels':{k:round(v['ms_per_frame'],3) for k,v in d['kernels'].items()}}))" >> $OUT
  done
done
python3 - $OUT <<'PY'
import json,sys,collections
rows=[json.loads(l) for l in open(sys.argv[1])]
by=collections.defaultdict(list)
for r in rows: by[r['lib']].append(r)
for lib,rs in by.items():
    ms=sorted(r['ms_per_frame'] for r in rs)
    ks={k:sorted(r['kernels'][k] for r in rs)[len(rs)//2] for k in rs[0]['kernels']}
    print(lib, 'ms_per_frame median %.2f min %.2f'%(ms[len(ms)//2],ms[0]), {k:v for k,v in list(ks.items())[:6]})
PY
