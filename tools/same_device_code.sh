#!/bin/bash
# Is the device code of the hot kernel files the same as at another commit?  Compiles each file at REV and in the working tree
# with the Makefile's CXXFLAGS plus --cuda-device-only -S and compares the gfx950 assembly, less the lines with the
# per-translation-unit identifier (__hip_cuid_*, which changes with any source edit).  Needs no GPU.  Compiles and diffs only.
# usage: tools/same_device_code.sh [REV (default HEAD)] [file.hip ...]     exit status 0: every file identical
#        tools/same_device_code.sh --per-kernel REV old.hip [...] -- new.hip [...]
#   the second form is for kernels that moved between files: the files named before `--` are taken at REV, those behind it from
#   the working tree, and the comparison goes function by function (tools/same_device_code.py).  exit status 0: the same
#   symbols on both sides, every one identical
set -euo pipefail
root=$(cd "$(dirname "$0")/.." && pwd)
per_kernel=0
if [ "${1:-}" = --per-kernel ]; then per_kernel=1; shift; fi
rev=${1:-HEAD}; shift || true
if [ $per_kernel = 1 ]; then
  old_files=(); while [ $# -gt 0 ] && [ "$1" != -- ]; do old_files+=("$1"); shift; done
  shift || true
  new_files=("$@")
  if [ ${#old_files[@]} = 0 ] || [ ${#new_files[@]} = 0 ]; then echo "usage: $0 --per-kernel REV old.hip [...] -- new.hip [...]" >&2; exit 2; fi
else
  files=${*:-ani_kernels_aev_lists.hip ani_kernels_aev_fast.hip ani_kernels_aev_generic.hip ani_kernels_mlp.hip ani_kernels_mlpf.hip ani_kernels_mlpg.hip}
  old_files=($files); new_files=($files)
fi
flags=$(make -s -C "$root/lammps-ani_amd/csrc" --eval='print-cxxflags: ; @echo $(CXXFLAGS)' print-cxxflags)
hipcc=${HIPCC:-hipcc}
tmp=$(mktemp -d); trap 'rm -rf "$tmp"' EXIT
mkdir -p "$tmp/old" "$tmp/out"
git -C "$root" archive "$rev" lammps-ani_amd/csrc include | tar -x -C "$tmp/old"
compile() {   # side file
  local dir=$root/lammps-ani_amd/csrc; [ "$1" = old ] && dir=$tmp/old/lammps-ani_amd/csrc
  ( cd "$dir" && $hipcc $flags --cuda-device-only -S "$2" -o "$tmp/out/$1.$2.s" 2>"$tmp/out/$1.$2.err" &&
    grep -v __hip_cuid_ "$tmp/out/$1.$2.s" >"$tmp/out/$1.$2.flt" ) &
}
for f in "${old_files[@]}"; do compile old "$f"; done
for f in "${new_files[@]}"; do compile new "$f"; done
wait
status=0
if [ $per_kernel = 1 ]; then
  old=(); new=()
  for f in "${old_files[@]}"; do old+=("$tmp/out/old.$f.flt"); done
  for f in "${new_files[@]}"; do new+=("$tmp/out/new.$f.flt"); done
  for s in "${old[@]}" "${new[@]}"; do
    if [ ! -s "$s" ]; then echo "$(basename "$s" .flt): did not compile"; cat "${s%.flt}.err"; status=1; fi
  done
  [ $status = 0 ] || exit $status
  echo "per kernel: ${old_files[*]} at $rev  against  ${new_files[*]} in the working tree"
  python3 "$root/tools/same_device_code.py" "${old[@]}" -- "${new[@]}" || status=1
  exit $status
fi
for f in $files; do
  old=$tmp/out/old.$f.flt; new=$tmp/out/new.$f.flt
  if [ ! -s "$old" ] || [ ! -s "$new" ]; then echo "$f: did not compile"; cat "$tmp"/out/*."$f".err; status=1; continue; fi
  n=$(grep -c '^\s*\.amdhsa_kernel ' "$new")
  if cmp -s "$old" "$new"; then echo "$f: identical to $rev ($n kernels, $(wc -l <"$new") lines of assembly)"
  else echo "$f: DIFFERS from $rev ($n kernels now, $(grep -c '^\s*\.amdhsa_kernel ' "$old") then)"; diff "$old" "$new" | head -20 || true; status=1; fi
done
exit $status
