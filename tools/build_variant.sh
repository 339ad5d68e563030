#!/bin/bash
# usage: tools/build_variant.sh NAME "EXTRA FLAGS" file.hip [file2.hip ...]  -> tools/vbuild/libirm_NAME.so
# Rebuilds the named (edited) kernel files, links them with the product's objects of the others; load the result through
# IRM_HIP_LIB for an A/B.  The sources have no -D switches: EXTRA FLAGS is for compiler options and may be "".
set -e
cd "$(dirname "$0")/../image-restoration-models_amd/csrc"
name=$1; flags=$2; shift 2
mkdir -p ../../tools/vbuild/obj_$name
objs=""
for f in *.hip; do
  o=${f%.hip}.o
  use=$o
  for v in "$@"; do
    if [ "$v" == "$f" ]; then
      /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -fno-slp-vectorize $flags -c $f -o ../../tools/vbuild/obj_$name/$o
      use=../../tools/vbuild/obj_$name/$o
    fi
  done
  objs="$objs $use"
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 $objs -o ../../tools/vbuild/libirm_$name.so
echo built tools/vbuild/libirm_$name.so
