// Device helpers of the segment-attention kernels (gfx950, wave64, v_mfma_f32_32x32x16_bf16).
// Fragment / tile layout algebra: see ttt_mfma_dev.h (A: lane=i, regs=k; B: lane=j, regs=k; C/D: lane=col,
// regs=rows row_of(r,h); a C tile is re-usable in place as an operand contracting over its row index, with
// k-slot order pi_s(h,e) = 16s + 8(e>>2) + 4h + (e&3)).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ttt_mfma_dev.h"

namespace ttt {
namespace attn {
using namespace ttt::mf;

constexpr int AS = 72;                 // LDS row stride (elements) of a [rows][64] bf16 tile: 144 B, conflict-free b128 / tr_b64
constexpr int ATILE = 64 * AS;         // elements of one [64][64] tile

// plain operand fragment: lane c reads 8 contiguous elements of its row (outer index = row, contraction = column)
__device__ __forceinline__ bf16x8 row_frag(const __bf16* img, int stride, int row0, int col0, int l) {
    return *reinterpret_cast<const bf16x8*>(img + (row0 + (l & 31)) * stride + col0 + 8 * (l >> 5));
}
// fragment whose k-slots follow the pi order along the COLUMNS of a row-major image (outer index = row)
__device__ __forceinline__ bf16x8 row_frag_pi(const __bf16* img, int stride, int row0, int col0, int s, int l) {
    return pi_read(img + (row0 + (l & 31)) * stride, col0, s, l >> 5);
}

__device__ __forceinline__ float half_swap(float v) { return __shfl_xor(v, 32, 64); }

}  // namespace attn
}  // namespace ttt
