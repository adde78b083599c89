#!/bin/bash
# Build libttt_hip.so for gfx950 (cross-compiles without a GPU).  Usage: csrc/build.sh [-j]
set -e
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result"
OUT=../lib
mkdir -p "$OUT" build
pids=()
for src in capi ttt_generic ttt_mfma ttt_mfma2 ttt_mfma16 ttt_mfma_bwd2 ttt_mfma_bwd4 ttt_mfma_rc4 ttt_prepost attn_fwd attn_bwd attn_pre attn_v2; do
  # rebuild when the source, any header here or the public header is newer than the object
  if [ ! -f build/$src.o ] || [ -n "$(find $src.hip *.h ../../include/ttt_hip.h ../../include/ttt_hip_parts.h ../../include/ttt_hip_bwd_parts.h ../../include/ttt_hip_pair16.h ../../include/ttt_hip_mlp_bwd_parts.h ../../include/ttt_hip_lin_bwd_front.h ../../include/ttt_hip_lin_split16.h ../../include/ttt_hip_lin64_bwd_front.h -newer build/$src.o)" ]; then
    $HIPCC $FLAGS -c $src.hip -o build/$src.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC build/capi.o build/ttt_generic.o build/ttt_mfma.o build/ttt_mfma2.o build/ttt_mfma16.o build/ttt_mfma_bwd2.o build/ttt_mfma_bwd4.o build/ttt_mfma_rc4.o build/ttt_prepost.o build/attn_fwd.o build/attn_bwd.o build/attn_pre.o build/attn_v2.o -o $OUT/libttt_hip.so
echo "built $OUT/libttt_hip.so"
