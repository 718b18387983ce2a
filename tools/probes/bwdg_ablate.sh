#!/bin/bash
# Timing ablations / variants of bwd3x3g_kernel (64 channels; ablated results are wrong by construction): scratch libraries
# build/ab/lib_bwdg_<tag>.so (tools/ab_build.sh), selected on the GPU box through SV_LIB_PATH.   build (no GPU needed) | run (GPU box)
R="$(cd "$(dirname "$0")/../.." && pwd)"
declare -A V=( [base]="" [nog]="-DSV_BWDG_ABL=1" [nod]="-DSV_BWDG_ABL=2" [noload]="-DSV_BWDG_ABL=4" [nostage]="-DSV_BWDG_ABL=8" [onlymma]="-DSV_BWDG_ABL=12" [donly]="-DSV_BWDG_ABL=13" [gonly]="-DSV_BWDG_ABL=14" [memonly]="-DSV_BWDG_ABL=3" [noepi]="-DSV_BWDG_ABL=16" [w0]="-DSV_BWDG_WREG=0" [pd1]="-DSV_BWDG_PD=1" [pd3]="-DSV_BWDG_PD=3" [pd3donly]="-DSV_BWDG_PD=3 -DSV_BWDG_ABL=13" )
[ -n "$SV_BWDG_TAGS" ] || SV_BWDG_TAGS="base nog nod noload nostage onlymma donly gonly memonly noepi"
if [ "$1" = "build" ]; then
  for t in $SV_BWDG_TAGS; do
    bash "$R/tools/ab_build.sh" bwd3x3g.hip "bwdg_$t" ${V[$t]} $SV_BWDG_EXTRA || exit 1
  done
  exit 0
fi
cd "$R"
for t in $SV_BWDG_TAGS; do
  printf "%-9s " $t
  SV_LIB_PATH="$R/build/ab/lib_bwdg_$t.so" python tools/bwdf_bench.py ${SV_BWDG_ARGS:-512 16 4 248 64} 2>&1 | grep fused | awk '{printf "%s %s us   ", $1, $3} END {print ""}'
done
