#!/bin/bash
# A/B builds of ONE kernel file with macro sets, each followed by the per-launch table of the whole step (config 2 and, with
# SV_AB_C4=1, config 4).  The dials left in the sources: SV_C3P_WAVES, SV_C3P_DEPTH, SV_W3_EPD, SV_X3_EPD, SV_X3_CAP, SV_HALOP_OCC*,
# SV_TCONVR_PD, SV_TCONVR_KL, SV_TCONVX16_TP, SV_SCONV_PD, SV_BWDF_WREGS, SV_BWDG_PD, SV_BWDG_WREG*, SV_WG3_LD?_PAD,
# SV_IG_MIN_TILES (or any experiment of the moment).
#   usage: tools/ab.sh igemm.hip "tags-regex" "-DA=1" "-DB=2 -DC=3" ...        ("" = the file as it is)
# Every variant is a scratch library built by tools/ab_build.sh and selected through SV_LIB_PATH (shot_vae_amd/_lib.py): the
# shipped library and its objects are never touched, and a variant that does not build is reported as FAILED and not timed.
R="$(cd "$(dirname "$0")/.." && pwd)"
FILE=$1; TAGS=$2; shift 2
n=0
for v in "$@"; do
  n=$((n + 1))
  echo "== $FILE $v"
  if ! LIBV=$(bash "$R/tools/ab_build.sh" "$FILE" "ab_$n" $v); then
    echo "   FAILED to build: not timed"
    continue
  fi
  (cd "$R" && export SV_LIB_PATH="$LIBV"
   SV_BENCH_TABLE=1 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-extras 2> "$R/build/ab/table" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('config 2:', d['ms_per_step'], 'ms', d['value'])"; grep -E "$TAGS" "$R/build/ab/table" | awk '{printf "   %-30s %8.1f us\n",$2,$6}'
   if [ -n "$SV_AB_C4" ]; then SV_BENCH_TABLE=1 python bench.py --full --net wideresnet-28-10 --classes 100 --batch 256 --steps 10 --warmup 3 --no-cpu-baseline 2> "$R/build/ab/table4" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('config 4:', d['ms_per_step'], 'ms', d['value'])"; grep -E "$TAGS" "$R/build/ab/table4" | awk '{printf "   %-30s %8.1f us\n",$2,$6}'; fi)
done
