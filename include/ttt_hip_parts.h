/*
 * ttt_hip_parts.h - extensions of libttt_hip.so BESIDE the reference's operator boundary (ttt_hip.h): scans over a part of the
 * sequence that have no counterpart among the reference's call sites.  Same conventions as ttt_hip.h (caller-allocated contiguous
 * device buffers, kernels enqueued on `stream` without synchronising, 0 = enqueued, negative = error with ttt_hip_last_error()).
 * Additive: TTT_HIP_ABI_VERSION stays what ttt_hip.h says, and every declaration of ttt_hip.h is unchanged.
 * (The TTT-MLP counterpart, ttt_hip_mlp_forward_chunk, predates this header and lives in ttt_hip.h.)
 */
#ifndef TTT_HIP_PARTS_H
#define TTT_HIP_PARTS_H

#include "ttt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The TTT-Linear forward over steps [step0, step0 + nsteps) of the sequence that `d` and `a` describe (d->NC = the whole
 * sequence; the tensors of `a` are the whole sequence's), started from the state in a->W1_init / a->b1_init and leaving the state
 * after its last step in W1_final / b1_final ([B,NH,F,F] / [B,NH,1,F] fp32 like the initial state; may alias it; both NULL: not
 * stored; exactly one NULL: refused).  Outputs and checkpoints land where ttt_hip_linear_forward puts them, with the same bits: the
 * kernels hold the whole state in fp32 registers and rebuild everything else a step takes from its predecessor from it, so a part
 * is ANY [step0, step0 + nsteps) inside [0, NC) at either mini-batch size - there is no checkpoint-group rule.
 * MFMA scan only: bf16 activations, F = 64, mini-batches of 16, or of 64 on an explicit TTT_IMPL_MFMA (TTT_IMPL_AUTO resolves
 * TTT-Linear at mini-batches of 64 to the generic kernels, which do not continue from a state: refused).
 * `workspace` / `workspace_bytes` are accepted and ignored (ttt_hip_linear_forward_workspace is 0 for these kernels); they keep
 * the signature parallel to ttt_hip_mlp_forward_chunk.  Lets a caller run the projections of the next part of the sequence beside
 * the scan of the current one (ttt_amd/models/ssm/pipeline.py). */
int ttt_hip_linear_forward_chunk(const ttt_dims* d, const ttt_linear_fwd_args* a, int step0, int nsteps,
                                 float* W1_final, float* b1_final, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTT_HIP_PARTS_H */
