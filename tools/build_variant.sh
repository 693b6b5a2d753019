#!/bin/bash
# build the library from another source directory into lib/exp/NAME.so (A/B experiments; run
# on the CPU side, the .so travels with the snapshot).  usage: tools/build_variant.sh NAME SRC_DIR [FLAGS...]
# Every SRC_DIR/*.hip with the Makefile's flags for that file, at most 16 compiles at once.
set -e
NAME=$1; SRC=$2; shift 2
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=$ROOT/julia-ocean-modelling_amd
ROCM=${ROCM:-/opt/rocm}
OUT=$(mktemp -d); trap 'rm -rf "$OUT"' EXIT
mkdir -p $PKG/lib/exp
export HIPCC=$ROCM/bin/hipcc OUT SRC
export FLAGS="-O3 -fPIC -std=c++17 --offload-arch=gfx950 -I$ROOT/include -I$SRC -Wall -Wno-unused-function $*"
# the Makefile's NOFMA list: the files compiled with -ffp-contract=off
export NOFMA=" $(sed -n 's/^NOFMA *= *//p' $PKG/Makefile) "
[ "$NOFMA" != "  " ] || { echo "no NOFMA list in $PKG/Makefile" >&2; exit 1; }
ls $SRC/*.hip | xargs -P 16 -I{} bash -c '
  f=$(basename {} .hip); X=""
  case "$NOFMA" in *" $f "*) X="-ffp-contract=off";; esac
  $HIPCC $FLAGS $X -c {} -o $OUT/$f.o'
$HIPCC --offload-arch=gfx950 -shared -o $PKG/lib/exp/$NAME.so $OUT/*.o -L$ROCM/lib -lrccl -Wl,-rpath,$ROCM/lib
ls -la $PKG/lib/exp/$NAME.so
