#!/bin/bash
# Build variant B = the library as of git revision $1 (default HEAD) into multitask_hydranet_amd/libhydranet_hip_B.so (same ABI assumed),
# so that one GPU visit can run the working tree (A) against it on the SAME box (HN_TUNING=ab HN_LIB_AB=<that file>).  The source list is
# that revision's own _lib.SOURCES, and every header of its csrc/ is copied next to the sources.
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
REV=${1:-HEAD}
C=multitask_hydranet_amd/csrc
T=$(mktemp -d)
SRCS=$(git -C $R show $REV:multitask_hydranet_amd/_lib.py | python3 $R/tools/lib_sources.py)
HDRS=$(git -C $R ls-tree --name-only $REV $C/ | grep '\.h$' | xargs -n1 basename)
for f in $SRCS $HDRS; do git -C $R show $REV:$C/$f > $T/$f; done
objs=""
for f in $SRCS; do
  while [ $(jobs -rp | wc -l) -ge 16 ]; do wait -n; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c $T/$f -o $T/${f%.hip}.o &
  objs="$objs $T/${f%.hip}.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $R/multitask_hydranet_amd/libhydranet_hip_B.so $objs
rm -rf $T
ls -la $R/multitask_hydranet_amd/libhydranet_hip_B.so
