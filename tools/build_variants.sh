#!/bin/bash
# Build variants of libptmi.so with different -D tuning macros HERE (hipcc cross-compiles without a GPU); the .so files
# under opencl_pathtracer_amd/lib/variants/ travel to the GPU box with the snapshot, where tools/run_variants.sh benches
# them one after the other on the same box.  Each variant is the product library as the Makefile defines it (its object list,
# both arithmetic modes), built into a directory of its own with the macros in EXTRA.
# usage: tools/build_variants.sh "name1:-DA=1 -DB=2" "name2:-DA=3" ...       (SRC=<dir> builds another source tree)
set -e
SRC=${SRC:-.}
HERE=$(cd "$(dirname "$0")/.." && pwd)
OUT=$PWD/opencl_pathtracer_amd/lib/variants
mkdir -p $OUT
build_one() {
  name="$1"; defs="$2"; dir=$OUT/build_$name
  if make -f $HERE/Makefile -C $SRC lib LIBDIR=$dir EXTRA="$defs" > $OUT/build_$name.log 2>&1; then
    cp $dir/libptmi.so $OUT/libptmi_$name.so && echo "built $name"
  else
    echo "$name: BUILD FAILED"; tail -5 $OUT/build_$name.log
  fi
  rm -rf $dir
}
for spec in "$@"; do
  name="${spec%%:*}"; defs="${spec#*:}"; [ "$defs" = "$spec" ] && defs=""
  build_one "$name" "$defs"
done
