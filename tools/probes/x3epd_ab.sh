#!/bin/bash
# conv3x3x.hip: residual rows in flight in the epilogue (SV_X3_EPD = 1 / 2 / 3), built into scratch libraries
# (tools/ab_build.sh) and timed on the wide layers.  GPU box.
R="$(cd "$(dirname "$0")/../.." && pwd)"
cd "$R"
for v in 1 2 3; do
  bash tools/ab_build.sh conv3x3x.hip "x3e$v" -DSV_X3_EPD=$v > /dev/null || exit 1
done
for v in 1 2 3; do
  echo "== EPD=$v"
  SV_LIB_PATH="$R/build/ab/lib_x3e$v.so" python tools/layer_bench.py 2>&1 | grep "of bf16" | grep -v wgrad
done
