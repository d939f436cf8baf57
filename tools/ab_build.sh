#!/bin/bash
# Builds a variant of libbrx.so with extra compiler flags for a same-box A/B:
#   tools/ab_build.sh NAME "-DBRX_XCD_ITEMS=0"   ->  br_amd/lib/ab/libbrx_NAME.so   (git-ignored, travels with gpurun)
# (round 8: -DBRX_REV_BLOCK=2 / 4 / 8, the rounds per block of the reverse scans; -DBRX_ONE64_WAVES=6 / 7 / 8)
# and is picked up with BRX_LIB_PATH=br_amd/lib/ab/libbrx_NAME.so python bench.py ...
# Different GPU boxes of the pool differ by up to ~10 % on the same code, so variants are compared inside one call.
set -e
cd "$(dirname "$0")/../br_amd/csrc"
name=$1; shift
bdir=build_ab_$name
mkdir -p $bdir ../lib/ab
# every source of br_amd/csrc/Makefile (and --no-undefined, as there: a library that lacks one does not link)
srcs=$(sed -n 's/^SRCS *= *//p' Makefile | sed 's/\.hip//g')
pids=()
for f in $srcs; do
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 "$@" -c $f.hip -o $bdir/$f.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
objs=""; for f in $srcs; do objs="$objs $bdir/$f.o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/ab/libbrx_$name.so $objs -lpthread -ldl -Wl,-rpath,/opt/rocm/lib -Wl,--no-undefined
rm -rf $bdir
echo "br_amd/lib/ab/libbrx_$name.so"
