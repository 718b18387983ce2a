#!/bin/bash
# Timing ablations / variants of bwd3x3f_kernel (ablated results are wrong by construction): built HERE into scratch libraries
# build/ab/lib_bwdf_<tag>.so (tools/ab_build.sh), selected on the GPU box through SV_LIB_PATH.
#   tools/probes/bwdf_ablate.sh build      (no GPU needed: hipcc cross-compiles)
#   tools/probes/bwdf_ablate.sh run        (on the GPU box)
R="$(cd "$(dirname "$0")/../.." && pwd)"
declare -A V=( [base]="" [nog]="-DSV_BWDF_ABL=1" [nod]="-DSV_BWDF_ABL=2" [noload]="-DSV_BWDF_ABL=4" [nostage]="-DSV_BWDF_ABL=8" [onlymma]="-DSV_BWDF_ABL=12" [noepi]="-DSV_BWDF_ABL=16" [donly]="-DSV_BWDF_ABL=13" [gonly]="-DSV_BWDF_ABL=14" [memonly]="-DSV_BWDF_ABL=3" [wregs1]="-DSV_BWDF_WREGS=1" )
[ -n "$SV_BWDF_TAGS" ] || SV_BWDF_TAGS="base nog nod noload nostage onlymma noepi"
if [ "$1" = "build" ]; then
  for t in $SV_BWDF_TAGS; do
    bash "$R/tools/ab_build.sh" bwd3x3f.hip "bwdf_$t" ${V[$t]} $SV_BWDF_EXTRA || exit 1
  done
  exit 0
fi
cd "$R"
for t in $SV_BWDF_TAGS; do
  printf "%-9s " $t
  SV_LIB_PATH="$R/build/ab/lib_bwdf_$t.so" python tools/bwdf_bench.py ${SV_BWDF_ARGS:-512 32 4 0} 2>&1 | grep fused | awk '{printf "%s %s us   ", $1, $3} END {print ""}'
done
