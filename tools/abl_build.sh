#!/bin/bash
# build variants of libani_hip.so: tools/abl/libani_<NAME>.so with extra flags on the kernel files of ONE unit, everything else (flags,
# object list, the other objects) taken from the Makefile.  The product sources carry only the stamp switches (-DABLB_STAMPS,
# -DABLB_STAMPS_VM on aev, -DABLF_STAMPS on mlpf); an experiment is a branch, built with this or with plain make.
# usage: tools/abl_build.sh UNIT NAME "FLAGS" [NAME2 "FLAGS2" ...]      UNIT: aev, mlpf, ...: ani_kernels_<UNIT>.hip together with
#   every ani_kernels_<UNIT>_*.hip (aev: ani_kernels_aev_lists.hip, ani_kernels_aev_fast.hip, ani_kernels_aev_generic.hip)
#   e.g. tools/abl_build.sh aev STAMPS "-DABLB_STAMPS"    tools/abl_build.sh mlpf STAMPS "-DABLF_STAMPS"
set -e
unit=$1; shift
cd "$(dirname "$0")/../lammps-ani_amd/csrc"
files=$(ls ani_kernels_$unit.hip ani_kernels_${unit}_*.hip 2>/dev/null || true)
[ -n "$files" ] || { echo "no ani_kernels_$unit.hip or ani_kernels_${unit}_*.hip" >&2; exit 2; }
make -j8
mkvar() { make -s --eval="print-var: ; @echo \$($1)" print-var; }
CXXFLAGS=$(mkvar CXXFLAGS); ROCTX_LIBS=$(mkvar ROCTX_LIBS)
OBJS=$(mkvar OBJS | tr ' ' '\n' | grep -v -e "^ani_kernels_$unit.o$" -e "^ani_kernels_${unit}_.*\.o$")
mkdir -p ../../tools/abl
while [ $# -ge 2 ]; do
  name=$1; flags=$2; shift 2
  ( objs=
    for f in $files; do
      o=../../tools/abl/$(basename $f .hip | sed 's/^ani_kernels_//')_$name.o
      hipcc $CXXFLAGS $flags -c $f -o $o || exit 1
      objs="$objs $o"
    done
    hipcc -shared -fPIC --offload-arch=gfx950 -o ../../tools/abl/libani_$name.so $OBJS $objs $ROCTX_LIBS -ldl && echo built $name ) &
  while [ $(jobs -r | wc -l) -ge 4 ]; do sleep 0.5; done
done
wait
