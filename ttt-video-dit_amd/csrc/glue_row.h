// Row toolkit of the HBM-bound glue kernels (ttt_prepost.hip, attn_pre.hip): a lane holds 8 consecutive bf16 features (16 bytes)
// as 8 floats, a 64-feature head row is 8 such lanes.
#pragma once
#include <hip/hip_runtime.h>
#include "ttt_dpp.h"

namespace ttt {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8 ld8_raw(const __bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ bf16x8 zero8_raw() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (__bf16)0.0f;
    return z;
}
__device__ __forceinline__ void cvt8(const bf16x8& a, float (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (float)a[j];
}
__device__ __forceinline__ void ld8(const __bf16* p, float (&o)[8]) { cvt8(ld8_raw(p), o); }
__device__ __forceinline__ void st8(__bf16* p, const float (&v)[8]) {
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (__bf16)v[j];
    *reinterpret_cast<bf16x8*>(p) = a;
}
__device__ __forceinline__ void ldf8(const float* p, float (&o)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3]; o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3];
}
__device__ __forceinline__ float bf16_round(float x) { return (float)(__bf16)x; }

// Centre a 64-feature head row (8 lanes x 8 features) in place; returns the sum of squares of the centred row.  The caller applies
// its own variance convention: / 63 with eps on the std (reconstruction target), / 64 with eps under the root (LayerNorm).
__device__ __forceinline__ float centre_row(float (&d)[8]) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += d[j];
    const float mean = sum8(s) * (1.0f / 64.0f);
    float vs = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { d[j] -= mean; vs += d[j] * d[j]; }
    return sum8(vs);
}

}  // namespace ttt
