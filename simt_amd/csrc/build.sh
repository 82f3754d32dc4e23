#!/bin/bash
# Build libsimt_hip.so for gfx950 (in-tree; the .so is git-ignored but travels with gpurun snapshots).
set -e
cd "$(dirname "$0")"
OUT=../libsimt_hip.so
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
# -packed-fp32-ops: v_pk_*_f32 cannot issue in the shadow of an MFMA (profiles/microbench/mixbench2.hip: one per MFMA costs +77 %), plain VALU can
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wno-unused-result -Xclang -target-feature -Xclang -packed-fp32-ops"
SRCS=(*.hip)
BUILD=${BUILD:-../_build}
mkdir -p $BUILD
objs=()
pids=()
for f in "${SRCS[@]}"; do
  b=$(basename "$f")
  o=$BUILD/${b%.hip}.o
  objs+=("$o")
  stale=0
  if [ ! -f "$o" ] || [ "$f" -nt "$o" ]; then stale=1; fi
  for h in *.h ../../include/simt_hip.h; do      # any header here, or the C ABI, newer than the object
    if [ "$h" -nt "$o" ]; then stale=1; fi
  done
  if [ $stale = 1 ]; then
    $HIPCC $FLAGS -c "$f" -o "$o" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC "${objs[@]}" -o $OUT
echo "built $OUT"
