#!/bin/bash
# Where the time of tconv.hip goes: a scratch library (tools/ab_build.sh) with one part of the loop body removed (SV_TCONVR_DBG
# bits: 1 no MFMA loop, 2 no output stores, 4 no next-image load / staging, 8 no statistics, 16 no LDS fragment reads) or another
# schedule (-DSV_TCONVR_PD=1, -DSV_TCONVR_KL=8, ...), selected with SV_LIB_PATH, the layer timed.
#   GPU box: bash tools/probes/tconvr_ablate.sh "-DSV_TCONVR_DBG=1" ...
R="$(cd "$(dirname "$0")/../.." && pwd)"
n=0
for flags in "$@"; do
  n=$((n + 1))
  LIBV=$(bash "$R/tools/ab_build.sh" tconv.hip "tconvr_$n" $flags) || exit 1
  echo -n "[$flags]  "; SV_LIB_PATH="$LIBV" SV_BENCH_T=1 python3 $R/tools/layer_bench.py 2048 128 8 64 2>&1 | grep "of bf16" | head -1
done
