#!/bin/bash
# (round 5) the DBGK_DEBUG_* / tile-geometry / schedule switches used here exist only in a library built with -DDBGK_EXPERIMENTS:
#   profiles/tools/build_variant.sh exp dbg_assembly_amd/csrc -DDBGK_EXPERIMENTS  &&  export DBGK_LIB=$PWD/dbg_assembly_amd/_variants/exp.so
# level-2 / build overlap granularity: bucket chunks per step (DBGK_OVERLAP_CHUNKS); the finer the chunks, the sooner
# the region build reads the records level 2 has just written (Infinity Cache reuse) -- at the price of more launches
R=${GRAFT_REPO_ROOT:-/root/repo}
for c in ${CHUNKS:-8 16 32 64 128 287}; do
  DBGK_OVERLAP_CHUNKS=$c python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu-baseline 2>/dev/null | python3 -c "
import json,sys
j=json.loads(sys.stdin.read())
print('chunks', $c, 'ms_per_step %.3f' % j['ms_per_step'], 'l1 %.2f' % j['phases_ms_per_step']['insert'], 'l2 %.2f build %.2f wall %.2f' % (j['phases_ms_per_step']['partition'], j['phases_ms_per_step']['build'], j['phases_ms_per_step']['partition_and_build_wall']), 'verified' if j['verified'] else 'UNVERIFIED')
"
done
