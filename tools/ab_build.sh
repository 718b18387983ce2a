#!/bin/bash
# Builds ONE variant library for A/B runs and ablations: one kernel file of the Makefile's SRCS compiled with extra flags, linked
# with the shipped objects of every other file of SRCS.  It writes build/ab/<TAG>.o and build/ab/lib_<TAG>.so only -- the shipped
# shot_vae_amd/libshotvae_hip.so and shot_vae_amd/csrc/*.o are built by `make` first and never written with a variant -- and
# prints the library's path (the only line on stdout).  Select it with SV_LIB_PATH (shot_vae_amd/_lib.py).  Needs no GPU.
#   usage: tools/ab_build.sh FILE TAG [FLAGS...]        e.g. tools/ab_build.sh bwd3x3f.hip nog -DSV_BWDF_ABL=1
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R/shot_vae_amd/csrc"
FILE=$1; TAG=$2
[ $# -ge 2 ] && [ -n "$TAG" ] && [ "${TAG//\//}" = "$TAG" ] || { echo "usage: tools/ab_build.sh FILE TAG [FLAGS...]" >&2; exit 2; }
shift 2
mkvar() { make -s --no-print-directory --eval "_ab_var: ; @echo \$($1)" _ab_var; }
SRCS=$(mkvar SRCS); CXXFLAGS=$(mkvar CXXFLAGS); HIPCC=$(mkvar HIPCC); ARCH=$(mkvar ARCH)
case " $SRCS " in *" $FILE "*) ;; *) echo "ab_build: $FILE is not in the Makefile's SRCS ($SRCS)" >&2; exit 2;; esac
make -s -j16 >&2
OBJS=""
for f in $SRCS; do [ "$f" != "$FILE" ] && OBJS="$OBJS ${f%.hip}.o"; done
OUT="$R/build/ab"
mkdir -p "$OUT"
$HIPCC $CXXFLAGS "$@" -c "$FILE" -o "$OUT/$TAG.o" >&2
$HIPCC --offload-arch="$ARCH" -shared -fPIC "$OUT/$TAG.o" $OBJS -o "$OUT/lib_$TAG.so" >&2
echo "$OUT/lib_$TAG.so"
