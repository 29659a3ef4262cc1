#!/bin/bash
# the pair rows' weight gradient as ONE launch with nothing beside it (one stream, no early part): kernel durations
# tools/ab/wgrad_alone.sh [bench args]
export CLIORA_WAVEFRONT=0 CLIORA_WGRAD_EARLY_STEP=-1
bash tools/trace_step.sh alone "$@" > /dev/null
S=$(find . -path '*/prof/alone_kernel_stats.csv' | head -1)      # where tools/trace_step.sh put the kernel stats
grep -E "tn_gemm_tiles|tn_gemm_dma3x|level_compose_bwd|slab_reduce" "$S" | cut -c1-60,60-400 | awk -F, '{print substr($1,1,70), $2, $3, $4}'
