/*
 * ttt_hip_mlp_bwd_parts.h - the TTT-MLP backward at mini-batches of 16 over RANGES of checkpoint groups: a fifth header of
 * libttt_hip.so, beside ttt_hip.h (the reference's operator boundary), ttt_hip_parts.h, ttt_hip_bwd_parts.h (the TTT-Linear backward
 * over ranges, whose contract this one follows) and ttt_hip_pair16.h.  Same conventions as ttt_hip.h (caller-allocated contiguous
 * device buffers, kernels enqueued on `stream` without synchronising, 0 = enqueued, negative = error with ttt_hip_last_error()).
 * Additive: TTT_HIP_ABI_VERSION stays what ttt_hip.h says, and every declaration of the other headers is unchanged.
 *
 * ttt_hip_mlp_backward on its MFMA body walks the K = ceil(NC / G) checkpoint groups of a sequence from the last to the first and
 * does two things per group: it re-runs the state-update half of the group forward from its checkpoint, keeping the fp32 state that
 * enters every step, and then walks the group in reverse.  The first half depends on the checkpoint alone, the second on the
 * gradient state the later groups leave.  Here the halves are calls of their own over a range [k0, k0 + nk) of groups:
 *
 *   ttt_hip_mlp_recompute_groups   group k of the range -> G "slots" of the caller's slot workspace: slot j = the fp32 state
 *                                  entering step j of the group, W1 [64,256], b1 [256], W2 [256,64], b2 [64] one after the other
 *                                  (132 352 bytes) - the bits ttt_hip_mlp_backward leaves in the four *_init_group buffers.
 *                                  Layout [B*NH][nk][G] slots; a ragged last group uses fewer.  B*NH*nk independent workgroups
 *                                  (more than the device has compute units is fine: none waits for another).
 *   ttt_hip_mlp_sweep_groups       the reverse walk over the groups k0 + nk - 1 .. k0 from those slots.  It CARRIES
 *                                  - dW1 / db1 / dW2 / db2: read from a->grad_L_{W1,b1,W2,b2}_last, written to
 *                                    a->grad_L_{W1,b1,W2,b2}_init at the end; the two may be the same buffers (carried in place);
 *                                  - the un-reduced shares of the LayerNorm gradients in `ln_carry`, [B*NH][2][16][64] fp32 (dln_w
 *                                    then dln_b, per token row of the mini-batch): not read by the range that ends the sequence
 *                                    (k0 + nk == K: the sums start from zero), read by every other, always written; the range that
 *                                    holds group 0 (k0 == 0) also reduces them, in token order, into a->grad_L_ttt_norm_weight /
 *                                    grad_L_ttt_norm_bias, which no other range touches.
 *                                  grad_L_last_eta / grad_L_XQ / grad_L_XK / grad_L_XV of the swept steps land where
 *                                  ttt_hip_mlp_backward puts them.
 *
 * Swept from the last range to the first with the carries handed on, any cutting of [0, K) into ranges gives the BITS of
 * ttt_hip_mlp_backward under TTT_IMPL_MFMA: the steps are its steps, rounded alike.  `d` and `a` describe the whole sequence.  The
 * ordering between a recompute and the sweep that reads its slots (and between a sweep and a recompute that reuses its workspace)
 * is the caller's: the same stream, or events.  The slot workspace and ln_carry are 16-byte aligned.
 *
 * Geometry: bf16 activations, F = 64, mini-batches of 16.  The parts exist on the MFMA body alone, so d->impl = TTT_IMPL_AUTO has
 * nothing to choose between and is taken like TTT_IMPL_MFMA (what ttt_hip_mlp_backward resolves TTT_IMPL_AUTO to at this geometry -
 * the generic kernels - is not changed by this header); TTT_IMPL_GENERIC, mini-batches of 64 and fp32 activations are errors.
 *
 *                         recompute_groups                                      sweep_groups
 *   needs                 XK XV last_eta ttt_norm_weight ttt_norm_bias          every field of ttt_hip_mlp_backward except the four
 *                         W1 / b1 / W2 / b2_checkpoints                         checkpoints and the sixteen *_init_group ... buffers
 *   may be NULL           everything else                                       the checkpoints, every *_init_group ... buffer
 */
#ifndef TTT_HIP_MLP_BWD_PARTS_H
#define TTT_HIP_MLP_BWD_PARTS_H

#include "ttt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the slot workspace for nk groups: B * NH * nk * G * 132352 ; 0 for bad dims or nk <= 0 */
size_t ttt_hip_mlp_backward_parts_slots(const ttt_dims* d, int nk);
/* bytes of ln_carry: B * NH * 8192 ; 0 for bad dims */
size_t ttt_hip_mlp_backward_parts_carry(const ttt_dims* d);

int ttt_hip_mlp_recompute_groups(const ttt_dims* d, const ttt_mlp_bwd_args* a, int k0, int nk,
                                 void* slots, size_t slots_bytes, void* stream);
int ttt_hip_mlp_sweep_groups(const ttt_dims* d, const ttt_mlp_bwd_args* a, int k0, int nk,
                             const void* slots, size_t slots_bytes, float* ln_carry, size_t carry_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTT_HIP_MLP_BWD_PARTS_H */
