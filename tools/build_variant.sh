#!/bin/bash
# usage: tools/build_variant.sh <name> "<extra hipcc flags, e.g. -O2 or -DSEA_PHASE_STAMPS>" ["<sources the flags concern>"]
# Builds global-motion-estimation_amd/csrc into tools/microbench/libgme_<name>.so (same C ABI as the tree's
# library) for same-box A/B runs with tools/ab.sh.  With a third argument (e.g. "bbme_sea.hip bbme_sea_mse.hip") only
# those sources are compiled with the extra flags; the others are linked from the tree's own objects (csrc/build, which
# `make -C csrc` must have brought up to date): a macro that only two files read does not pay for two dozen compilations.
set -e
cd "$(dirname "$0")/.."
NAME=$1; FLAGS=$2; ONLY=$3
B=/tmp/gme_variant_$NAME; rm -rf $B; mkdir -p $B
SRC=global-motion-estimation_amd/csrc
CXX="/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -fvisibility=hidden -Wno-unused-value $FLAGS"
pids=""
for f in $(cd $SRC && ls *.hip); do      # every translation unit of the library, as its Makefile takes them
  if [ -n "$ONLY" ] && ! echo " $ONLY " | grep -q " $f "; then
    cp $SRC/build/${f%.hip}.o $B/
  else
    $CXX -Rpass-analysis=kernel-resource-usage -c $SRC/$f -o $B/${f%.hip}.o 2> $B/${f%.hip}.remarks & pids="$pids $!"
  fi
done
for p in $pids; do wait $p || { grep -h -v "remark:" $B/*.remarks; exit 1; }; done
# the compiler's per-kernel resource remarks of what was compiled here, beside the library (tools/sea_phase_stamps.py reads them)
cat $B/*.remarks | grep "remark:" > tools/microbench/libgme_$NAME.remarks || true
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/microbench/libgme_$NAME.so $B/*.o -ldl
ls -la tools/microbench/libgme_$NAME.so
