#!/bin/bash
# tools/mkvariant.sh NAME [-DSWITCH ...] : build dd2360-raytracing_amd/variants/lib_NAME.so (the product library with extra -D switches) for tools/ab.sh
# The units and their flags are the Makefile's: this drives it with an object directory of its own, the switches and the output name.
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)/dd2360-raytracing_amd
obj=$(mktemp -d /tmp/rt_variant_XXXX)      # objects outside the tree: only the finished library travels with gpurun
make -C $root -j16 BUILD=$obj EXTRA="$*" LIB=variants/lib_$name.so variants/lib_$name.so > /dev/null
rm -rf $obj
echo "built variants/lib_$name.so"
