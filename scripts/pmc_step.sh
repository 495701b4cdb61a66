#!/bin/bash
# usage: scripts/pmc_step.sh <tag>  (GPU box; writes under $OUT_DIR, default prof_out) — separate PMC passes for HBM traffic and L2 hit rate
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
out=${OUT_DIR:-prof_out}; mkdir -p $out
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $out/pmc_$1_$c -- python bench.py --steps 6 --warmup 2 --full --no-cpu-baseline > $out/pmc_$1_$c.log 2>&1 || exit 1
done
rocprofv3 --kernel-trace --pmc TCC_HIT_sum TCC_MISS_sum --output-format csv -d $out/pmc_$1_L2 -- python bench.py --steps 6 --warmup 2 --full --no-cpu-baseline > $out/pmc_$1_L2.log 2>&1
echo done
