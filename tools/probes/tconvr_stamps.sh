#!/bin/bash
# Diagnostic build of tconv.hip with s_memtime stamps (SV_TCONVR_DBG = 32, + extra flags per argument) in a scratch library
# (tools/ab_build.sh), read by tools/probes/tconvr_stamps.py.  GPU box.
R="$(cd "$(dirname "$0")/../.." && pwd)"
n=0
for f in "$@"; do
  n=$((n + 1))
  LIBV=$(bash "$R/tools/ab_build.sh" tconv.hip "tconvr_stamps_$n" -DSV_TCONVR_DBG=32 $f) || exit 1
  echo "== $f"; SV_LIB_PATH="$LIBV" python3 $R/tools/probes/tconvr_stamps.py 2048
done
