#!/bin/bash
# Build variant libraries of conv3x3x.hip for same-box A/Bs (no GPU needed; build/ travels with the tree, git-ignored):
#   bash tools/probes/x3_variants.sh "name:-DFLAG=.. -DFLAG=.." ...      -> build/ab/lib_<name>.so  (tools/ab_build.sh)
# e.g.  "epd2:-DSV_X3_EPD=2" "stamp0c8:-DSV_X3_STAMP=1 -DSV_X3_CAP=8"
# then  bash tools/experiments/x3_epi.sh   (times every build/ab/lib_*.so)   or   bash tools/probes/x3_stamps.sh 512   on the GPU box
R="$(cd "$(dirname "$0")/../.." && pwd)"
for v in "$@"; do
  bash "$R/tools/ab_build.sh" conv3x3x.hip "${v%%:*}" ${v#*:} || exit 1
done
