#!/bin/bash
# Builds one copy of the HIP library per variant of ONE source file of csrc/ (a profiling build, a -D of a kernel under development) into
# build/var_<file>/lib_<name>.so
# tools/lib_variants.sh conv_s16 "base:" "stamp:-DS16_STAMP" ...      (DEQSCI_HIP_LIB=<that .so> selects it)
# A variant's device assembly stays in build/var_<file>/<name>/ (-save-temps); its register and spill counts are printed.
set -e
cd "$(dirname "$0")/.."
SRC=$1; shift
D=build/var_$SRC
mkdir -p $D
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Iinclude -Ideqsci_amd/csrc -Wall -Wno-unused-function -Wno-inline-asm"
OTHERS=""
for path in deqsci_amd/csrc/*.hip; do
  f=$(basename $path .hip)
  [ $f = $SRC ] && continue
  OTHERS="$OTHERS $D/$f.o"
  if [ ! -f $D/$f.o ] || [ $path -nt $D/$f.o ] || [ deqsci_amd/csrc/common.hpp -nt $D/$f.o ]; then
    /opt/rocm/bin/hipcc $FLAGS -c -o $D/$f.o $path 2>/dev/null &
  fi
done
wait
for spec in "$@"; do
  name="${spec%%:*}"; defs="${spec#*:}"
  ( mkdir -p $D/$name &&      # (own directory: the -save-temps files of parallel builds would otherwise overwrite each other)
    /opt/rocm/bin/hipcc $FLAGS $defs -c -save-temps=obj -o $D/$name/$SRC.o deqsci_amd/csrc/$SRC.hip 2>/dev/null &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o $D/lib_$name.so $OTHERS $D/$name/$SRC.o &&
    echo "built $name ($defs) $(grep -h -E 'vgpr_count|vgpr_spill_count' $D/$name/*gfx950.s 2>/dev/null | awk '/spill/ { s += $2; next } $2 > m { m = $2 } END { print "max vgprs " m ", spilled " s }')" ) &
done
wait
