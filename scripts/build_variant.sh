#!/bin/bash
# build_probe/lib_<name>.so = libr2dm_hip.so with every kernel source compiled with extra -D flags (ablation
# experiments; select with R2DM_HIP_LIB=build_probe/lib_<name>.so).  Usage: scripts/build_variant.sh <name> [-DFLAG ...]
# Sources and per-file flags: r2dm_amd/csrc/sources.sh, as r2dm_amd/csrc/build.sh.
set -e
name=$1; shift
cd "$(dirname "$0")/../r2dm_amd/csrc"
. ./sources.sh
out=../../build_probe/obj_$name
mkdir -p $out
pids=()
for f in $R2DM_SOURCES; do
  hipcc $R2DM_FLAGS $(r2dm_extra_flags $f) "$@" -c $f.hip -o $out/$f.o 2> $out/$f.err &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p || { echo "compile failed:"; head -5 $out/*.err; exit 1; }; done
hipcc --offload-arch=gfx950 -shared -fPIC $out/*.o -o ../../build_probe/lib_$name.so
echo built lib_$name.so
