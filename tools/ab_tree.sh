#!/bin/bash
# Build the WORKING TREE's kernels (_lib.SOURCES, compiled where they lie, next to their headers) into
# multitask_hydranet_amd/libhydranet_hip_$1.so (a named variant for HN_TUNING=ab HN_LIB_AB=<that file>); extra hipcc flags
# (e.g. -DSOME_EXPERIMENT=2) may follow the name.
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
T=$(mktemp -d)
objs=""
for f in $(python3 $R/tools/lib_sources.py < $R/multitask_hydranet_amd/_lib.py); do
  while [ $(jobs -rp | wc -l) -ge 16 ]; do wait -n; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 "$@" -c $R/multitask_hydranet_amd/csrc/$f -o $T/${f%.hip}.o &
  objs="$objs $T/${f%.hip}.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/multitask_hydranet_amd/libhydranet_hip_$NAME.so $objs
rm -rf $T
ls -la $R/multitask_hydranet_amd/libhydranet_hip_$NAME.so
