#!/bin/bash
# bench.py --full over a few pangenome shapes on the GPU box (one line each: G k-mers/s co-scheduled,
# G k-mers/s with one launch per genome, k_probe ms per launch, roofline frac, table GB)
cd ${GRAFT_REPO_ROOT:-/root/repo}
ERR=$(mktemp)
for A in "" "--k 31" "--genomes 27 --genome-mb 40" "--genomes 64 --genome-mb 20 --k 31 --d 0.005" "--k 25" "--genomes 2 --genome-mb 400" "$@"; do
  echo "== $A"
  timeout 600 python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline $A 2>$ERR | python -c "
import sys,json
d=json.loads(sys.stdin.read())
print(round(d['value']/1e9,1), round(d['config'].get('per_genome_launches_value',0)/1e9,1), round(d['roofline']['avg_launch_ms'],3), d['roofline']['frac'], round(d['config']['table_bytes']/1e9,1))" 2>&1 || tail -3 $ERR
done
rm -f $ERR
