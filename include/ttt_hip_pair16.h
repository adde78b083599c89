/*
 * ttt_hip_pair16.h - the TTT-MLP forward scan at mini-batches of 16 as a PAIR of workgroups per (b, h): an opt-in extension of
 * libttt_hip.so BESIDE ttt_hip.h and the two parts headers.  Same conventions as ttt_hip.h (caller-allocated contiguous device
 * buffers, kernels enqueued on `stream` without synchronising, negative = error with ttt_hip_last_error()).
 * Additive: TTT_HIP_ABI_VERSION stays what ttt_hip.h says, every declaration of the other headers is unchanged, and
 * ttt_hip_mlp_forward_workspace() still answers 0 at mini-batches of 16 - the pair form has a workspace query of its own.
 *
 * One workgroup (role A) carries the state from step to step and publishes, per step, the updated state as the operands of the
 * output path into a ring of TTT_HIP_PAIR16_RING records of 64 KiB + 1 KiB + 256 B; a second workgroup (role B) computes the outputs
 * from the records.  Outputs, checkpoints and the final state are the bits of ttt_hip_mlp_forward / ttt_hip_mlp_forward_chunk.
 * A hand-over whose partner never arrives gives up after 2 s, poisons the outputs with NaN and sets the process's sticky error word
 * (ttt_hip_debug_sweep_error / ttt_hip_sweep_error_clear in ttt_hip.h): every later TTT-MLP call is refused until acknowledged.
 */
#ifndef TTT_HIP_PAIR16_H
#define TTT_HIP_PAIR16_H

#include "ttt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* records in flight per (b, h) */
#define TTT_HIP_PAIR16_RING 4

/* Bytes of the workspace of ttt_hip_mlp_forward_chunk_pair16: a block of flag words (B * NH * 256 bytes) followed by
 * B * NH * TTT_HIP_PAIR16_RING records of 64 KiB + 1 KiB + 256 B.  0 where the pair form does not serve the geometry (anything but bf16
 * activations, F = 64, mini-batches of 16 on the MFMA scan). */
size_t ttt_hip_mlp_forward_pair16_workspace(const ttt_dims* d);

/* Steps [step0, step0 + nsteps) of the TTT-MLP forward as a pair of workgroups per (b, h); the contract of ttt_hip_mlp_forward_chunk
 * at mini-batches of 16: `d` / `a` describe the whole sequence, a->*_init hold the state entering step0, the state after the last
 * step goes to the four *_final buffers (may alias the initial state; all four NULL: not stored; one to three NULL: refused), a part
 * is any [step0, step0 + nsteps) inside [0, NC) (the whole scan: step0 = 0, nsteps = NC).  `workspace`: at least
 * ttt_hip_mlp_forward_pair16_workspace(d) bytes, 16-byte aligned; one workspace serves consecutive launches of a stream.
 * Returns 0 = enqueued as pairs, 1 = enqueued on the one-workgroup kernel (both workgroups of every pair must be resident: B * NH
 * rounded up to 8, plus B * NH, exceeds the device's compute units), negative = error, nothing enqueued. */
int ttt_hip_mlp_forward_chunk_pair16(const ttt_dims* d, const ttt_mlp_fwd_args* a, int step0, int nsteps,
                                     float* W1_final, float* b1_final, float* W2_final, float* b2_final,
                                     void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTT_HIP_PAIR16_H */
