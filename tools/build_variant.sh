#!/bin/bash
# usage: tools/build_variant.sh <name> "<extra hipcc flags, e.g. -O2>"
# Builds global-motion-estimation_amd/csrc into tools/microbench/libgme_<name>.so (same C ABI as the tree's
# library) for same-box A/B runs with tools/ab.sh.
set -e
cd "$(dirname "$0")/.."
NAME=$1; FLAGS=$2
B=/tmp/gme_variant_$NAME; rm -rf $B; mkdir -p $B
SRC=global-motion-estimation_amd/csrc
CXX="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden -Wno-unused-value $FLAGS"
pids=""
for f in $(sed -n 's/^SRCS *:= *//p' $SRC/Makefile); do      # the library's own source list
  $CXX -c $SRC/$f -o $B/${f%.hip}.o & pids="$pids $!"
done
for p in $pids; do wait $p; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/microbench/libgme_$NAME.so $B/*.o -ldl
ls -la tools/microbench/libgme_$NAME.so
