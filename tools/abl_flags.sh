#!/bin/bash
# usage: abl_flags.sh <file.hip> name "flags" [name "flags"]...   -> rgbmanip_amd/abl/librgbm_hip_<name>.so (<file.hip> rebuilt with the flags,
# e.g. abl_flags.sh igemm_m32.hip probe "-DM32_RACE_PROBE=1")
cd "$(dirname "$0")/../rgbmanip_amd/csrc"
mkdir -p ../abl
src=$1; shift
while [ $# -gt 1 ]; do
  n=$1; f=$2; shift 2
  ( hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Xclang -target-feature -Xclang -packed-fp32-ops $f -c $src -o /tmp/abl_$n.o 2>&1 | grep -v "recognized feature" | grep -A5 "error"
    objs=$(ls build/*.o | grep -v "build/${src%.hip}.o")
    hipcc --offload-arch=gfx950 -shared -fPIC -o ../abl/librgbm_hip_$n.so $objs /tmp/abl_$n.o ) &
done
wait
ls ../abl
