#!/bin/bash
# Builds libr2dm_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
set -euo pipefail
cd "$(dirname "$0")"
. ./sources.sh
OUT=../libr2dm_hip.so
mkdir -p build
pids=()
for f in $R2DM_SOURCES; do
  stale=0
  for d in $f.hip $R2DM_HEADERS sources.sh; do if [ ! -f build/$f.o ] || [ $d -nt build/$f.o ]; then stale=1; fi; done
  if [ $stale = 1 ]; then
    hipcc $R2DM_FLAGS $(r2dm_extra_flags $f) -c $f.hip -o build/$f.o 2> >(grep -v "packed-fp32-ops' is not a recognized feature" >&2) &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC build/*.o -o $OUT
echo "built $(realpath $OUT)"
