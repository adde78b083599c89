// Host-side entry points of the MFMA (bf16 matrix-core) kernels: CS=64, F=64, bf16 activations.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/ttt_hip.h"

namespace ttt {
namespace mfma {
bool   supports(const ttt_dims* d, bool mlp, bool backward);
size_t workspace_bytes(const ttt_dims* d, bool mlp, bool backward);
void set_debug_timing(void* device_buffer_16_u64);
void set_debug_groups_per_chunk(int groups);   // 0 = automatic
void set_debug_dump(float* device_buffer);     // revision-2 forward: intermediates of workgroup 0, step 0 (>= 120000 floats)
void mlp_forward(const ttt_dims* d, const ttt_mlp_fwd_args* a, void* ws, hipStream_t s);
void mlp_forward_chunk(const ttt_dims* d, const ttt_mlp_fwd_args* a, int step0, int nsteps, float* W1f, float* b1f, float* W2f, float* b2f,
                       void* ws, hipStream_t s);          // CS = 64 only; ws: the forward workspace or null (one workgroup per (b,h))
int  mlp_forward_chunk_pair16(const ttt_dims* d, const ttt_mlp_fwd_args* a, int step0, int nsteps, float* W1f, float* b1f, float* W2f, float* b2f,
                              void* ws, hipStream_t s);   // CS = 16 as a pair of workgroups per (b,h): 0 pairs, 1 one workgroup, < 0 nothing launched
int  mlp_backward(const ttt_dims* d, const ttt_mlp_bwd_args* a, void* ws, hipStream_t s);   // 0, or < 0: no kernel was launched
void linear_forward(const ttt_dims* d, const ttt_linear_fwd_args* a, void* ws, hipStream_t s);
void linear_forward_chunk(const ttt_dims* d, const ttt_linear_fwd_args* a, int step0, int nsteps, float* W1f, float* b1f,
                          hipStream_t s);                    // CS = 16 or 64; any [step0, step0 + nsteps) inside [0, NC)
void linear_forward_chunk_split16(const ttt_dims* d, const ttt_linear_fwd_args* a, int step0, int nsteps, float* W1f, float* b1f,
                                  hipStream_t s);            // CS = 16 only: the two-wave form (include/ttt_hip_lin_split16.h)
void linear_backward(const ttt_dims* d, const ttt_linear_bwd_args* a, void* ws, hipStream_t s);
// the TTT-Linear backward in parts (include/ttt_hip_bwd_parts.h): checkpoint groups [k0, k0 + nk) of the sequence `d` / `a` describe
size_t linear_backward_parts_slots(const ttt_dims* d, int nk);
size_t linear_backward_parts_carry(const ttt_dims* d);
void linear_recompute_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, void* slots, hipStream_t s);
void linear_sweep_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, float* ln_carry, hipStream_t s);
// ... and its third stage at mini-batches of 16 (include/ttt_hip_lin_bwd_front.h)
size_t linear_backward_front_records(const ttt_dims* d, int nk);
void linear_front_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, void* records, hipStream_t s);
void linear_chain_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, const void* records,
                         float* ln_carry, hipStream_t s);
// ... and at mini-batches of 64 (include/ttt_hip_lin64_bwd_front.h)
size_t linear_backward_front64_records(const ttt_dims* d, int nk);
void linear_front64_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, void* records, hipStream_t s);
void linear_chain64_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, const void* records,
                           float* ln_carry, hipStream_t s);
// the TTT-MLP backward at mini-batches of 16 in parts (include/ttt_hip_mlp_bwd_parts.h): checkpoint groups [k0, k0 + nk)
size_t mlp_backward_parts_slots(const ttt_dims* d, int nk);
size_t mlp_backward_parts_carry(const ttt_dims* d);
void mlp_recompute_groups(const ttt_dims* d, const ttt_mlp_bwd_args* a, int k0, int nk, void* slots, hipStream_t s);
void mlp_sweep_groups(const ttt_dims* d, const ttt_mlp_bwd_args* a, int k0, int nk, const void* slots, float* ln_carry, hipStream_t s);
}  // namespace mfma
}  // namespace ttt
