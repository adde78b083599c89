// DPP lane moves and the reductions over aligned lane groups built from them (gfx950, wave64), shared by every kernel file.
#pragma once
#include <hip/hip_runtime.h>

namespace ttt {

// v of the lane that DPP control CTRL selects (0 where it selects none: bound_ctrl)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float sum4(float v) {   // sum over the aligned group of 4 lanes
    v += dpp_f<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_f<0x4E>(v);      // quad_perm [2,3,0,1]
    return v;
}
__device__ __forceinline__ float sum8(float v) {   // sum over the aligned group of 8 lanes
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);     // row_half_mirror
    return v;
}
__device__ __forceinline__ float sum16(float v) {  // sum over the 16 lanes of a DPP row
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);     // row_mirror
    return v;
}

}  // namespace ttt
