#!/bin/bash
# Variants of the 16x16 data-gradient kernel of tconv.hip (-DSV_TCONVX16_TP=1, -DSV_TCONVR_PD=1, ...): scratch libraries
# (tools/ab_build.sh) selected with SV_LIB_PATH, the layer timed.  GPU box.
R="$(cd "$(dirname "$0")/../.." && pwd)"
n=0
for flags in "$@"; do
  n=$((n + 1))
  LIBV=$(bash "$R/tools/ab_build.sh" tconv.hip "tconvx16_$n" $flags) || exit 1
  echo -n "[$flags]  "; SV_LIB_PATH="$LIBV" SV_BENCH_S=2 python3 $R/tools/layer_bench.py 2048 32 32 64 2>&1 | grep "dgrad" | head -1
done
