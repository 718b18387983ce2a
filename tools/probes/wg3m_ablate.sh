#!/bin/bash
# Timing ablations of wgrad3x3m_kernel (results wrong by construction): built HERE into scratch libraries
# build/ab/lib_wg3m_<tag>.so (tools/ab_build.sh), selected on the GPU box through SV_LIB_PATH.
#   tools/probes/wg3m_ablate.sh build      (no GPU needed: hipcc cross-compiles)
#   tools/probes/wg3m_ablate.sh run        (on the GPU box)
R="$(cd "$(dirname "$0")/../.." && pwd)"
declare -A V=( [base]="" [nomma]="-DSV_WG3M_NO_MMA" [noxform]="-DSV_WG3M_NO_XFORM" [noload]="-DSV_WG3M_NO_LOAD" [nohst]="-DSV_WG3M_NO_HST" [onlyload]="-DSV_WG3M_NO_MMA -DSV_WG3M_NO_HST" [onlymma]="-DSV_WG3M_NO_LOAD -DSV_WG3M_NO_HST" )
TAGS="base nomma noxform noload nohst onlyload onlymma"
if [ "$1" = "build" ]; then
  for t in $TAGS; do
    bash "$R/tools/ab_build.sh" wgrad3x3.hip "wg3m_$t" ${V[$t]} $SV_WG3M_EXTRA || exit 1
  done
  exit 0
fi
cd "$R"
for t in $TAGS; do
  for shape in "2048 32 32 32" "2048 64 16 64" "2048 128 8 128"; do
    for pb in 512 256; do
      printf "%-9s budget=%d  " $t $pb
      SV_LIB_PATH="$R/build/ab/lib_wg3m_$t.so" SV_BENCH_PERSISTENT_BLOCKS=$pb python tools/layer_bench.py $shape wgrad 2>&1 | grep wgrad | awk '{print $1,$2,$3,$4,$6,"us"}'
    done
  done
done
