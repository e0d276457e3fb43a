#!/bin/bash
# Is the device code of the hot kernel files the same as at another commit?  Compiles each file at REV and in the working tree
# with the Makefile's CXXFLAGS plus --cuda-device-only -S and compares the gfx950 assembly, less the lines with the
# per-translation-unit identifier (__hip_cuid_*, which changes with any source edit).  Needs no GPU.  Compiles and diffs only.
# usage: tools/same_device_code.sh [REV (default HEAD)] [file.hip ...]     exit status 0: every file identical
set -euo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
rev=${1:-HEAD}; shift || true
files=${*:-ani_kernels_aev.hip ani_kernels_mlp.hip ani_kernels_mlpf.hip ani_kernels_mlpg.hip}
flags=$(make -s -C "$root/lammps-ani_amd/csrc" --eval='print-cxxflags: ; @echo $(CXXFLAGS)' print-cxxflags)
hipcc=${HIPCC:-hipcc}
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
mkdir -p "$tmp/old" "$tmp/out"
git -C "$root" archive "$rev" lammps-ani_amd/csrc include | tar -x -C "$tmp/old"
for f in $files; do
  for side in old new; do
    dir=$root/lammps-ani_amd/csrc; [ $side = old ] && dir=$tmp/old/lammps-ani_amd/csrc
    ( cd "$dir" && $hipcc $flags --cuda-device-only -S "$f" -o "$tmp/out/$side.$f.s" 2>"$tmp/out/$side.$f.err" &&
      grep -v __hip_cuid_ "$tmp/out/$side.$f.s" >"$tmp/out/$side.$f.flt" ) &
  done
done
wait
status=0
for f in $files; do
  old=$tmp/out/old.$f.flt; new=$tmp/out/new.$f.flt
  if [ ! -s "$old" ] || [ ! -s "$new" ]; then echo "$f: did not compile"; cat "$tmp"/out/*."$f".err; status=1; continue; fi
  n=$(grep -c '^\s*\.amdhsa_kernel ' "$new")
  if cmp -s "$old" "$new"; then echo "$f: identical to $rev ($n kernels, $(wc -l <"$new") lines of assembly)"
  else echo "$f: DIFFERS from $rev ($n kernels now, $(grep -c '^\s*\.amdhsa_kernel ' "$old") then)"; diff "$old" "$new" | head -20 || true; status=1; fi
done
exit $status
