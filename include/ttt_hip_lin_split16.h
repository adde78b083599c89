/*
 * ttt_hip_lin_split16.h - the TTT-Linear forward scan at mini-batches of 16 with its output path on a second wave: an opt-in
 * extension of libttt_hip.so BESIDE ttt_hip.h and the other extension headers.  Same conventions as ttt_hip.h (caller-allocated
 * contiguous device buffers, kernels enqueued on `stream` without synchronising, 0 = enqueued, negative = error with
 * ttt_hip_last_error()).  Additive: TTT_HIP_ABI_VERSION stays what ttt_hip.h says, and every declaration of the other headers is
 * unchanged.
 *
 * ttt_hip_linear_forward / ttt_hip_linear_forward_chunk run one wave per (b, h).  Here one workgroup of two waves serves a (b, h):
 * the first carries the state from step to step (Z1, the fused LayerNorm / L2 gradient, the update) and hands the updated state, as
 * the packed bf16 operands of its own next step plus the fp32 bias, to the second through LDS - one workgroup barrier per step -,
 * which computes Z1b = Q W1' + b1', the output LayerNorm and the store.  Outputs, checkpoints and the final state are the bits of
 * ttt_hip_linear_forward_chunk.  No workspace, no flags, no residency requirement.
 */
#ifndef TTT_HIP_LIN_SPLIT16_H
#define TTT_HIP_LIN_SPLIT16_H

#include "ttt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Steps [step0, step0 + nsteps) of the TTT-Linear forward in the two-wave form; the contract of ttt_hip_linear_forward_chunk
 * (ttt_hip_parts.h) at mini-batches of 16: `d` / `a` describe the whole sequence, a->W1_init / a->b1_init hold the state entering
 * step0, the state after the last step goes to W1_final / b1_final (may alias the initial state; both NULL: not stored; exactly one
 * NULL: refused), a part is any [step0, step0 + nsteps) inside [0, NC); [0, NC) with both finals NULL is the one-call scan.
 * Served: bf16 activations, F = 64, mini-batches of 16, TTT_IMPL_AUTO or TTT_IMPL_MFMA.  Everything else (mini-batches of 64, fp32
 * activations, F != 64, TTT_IMPL_GENERIC) is refused with nothing enqueued.  `workspace` / `workspace_bytes` are accepted and
 * ignored; they keep the signature parallel to ttt_hip_linear_forward_chunk. */
int ttt_hip_linear_forward_chunk_split16(const ttt_dims* d, const ttt_linear_fwd_args* a, int step0, int nsteps,
                                         float* W1_final, float* b1_final, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTT_HIP_LIN_SPLIT16_H */
