/*
 * ttt_hip_bwd_parts.h - the TTT-Linear backward over RANGES of checkpoint groups: a third header of libttt_hip.so, beside
 * ttt_hip.h (the reference's operator boundary) and ttt_hip_parts.h (the forward over parts of the sequence).  Same conventions as
 * ttt_hip.h (caller-allocated contiguous device buffers, kernels enqueued on `stream` without synchronising, 0 = enqueued,
 * negative = error with ttt_hip_last_error()).  Additive: TTT_HIP_ABI_VERSION stays what ttt_hip.h says, and every declaration of
 * the other two headers is unchanged.
 *
 * ttt_hip_linear_backward walks the K = ceil(NC / G) checkpoint groups of a sequence from the last to the first and does two
 * things per group: it re-runs the group forward from its checkpoint, keeping the state that enters every step, and then walks the
 * group in reverse.  The first half depends on the checkpoint alone, the second on the gradient state the later groups leave.
 * Here the halves are calls of their own over a range [k0, k0 + nk) of groups:
 *
 *   ttt_hip_linear_recompute_groups   group k of the range -> G + 1 "slots" of the caller's slot workspace: slot j = the state
 *                                     entering step j of the group (both orientations as packed bf16 MFMA operands, 16 KiB, then
 *                                     the fp32 bias row, 256 bytes), the last used slot = the state that ends the group.  Layout
 *                                     [B*NH][nk][G + 1] slots; a ragged last group uses fewer.  B*NH*nk independent waves /
 *                                     workgroups: every group of a sequence can be recomputed at once.
 *   ttt_hip_linear_sweep_groups       the reverse walk over the groups k0 + nk - 1 .. k0 from those slots.  It CARRIES
 *                                     - dW1 / db1: read from a->grad_L_W1_last / grad_L_b1_last, written to a->grad_L_W1_init /
 *                                       grad_L_b1_init at the end; the two may be the same buffers (carried in place);
 *                                     - the un-reduced per-lane partial sums of the LayerNorm gradients in `ln_carry`: not read by
 *                                       the range that ends the sequence (k0 + nk == K: the sums start from zero), read by every
 *                                       other, always written; the range that holds group 0 (k0 == 0) also reduces them into
 *                                       a->grad_L_ttt_norm_weight / grad_L_ttt_norm_bias, which no other range touches.
 *                                     grad_L_last_eta / grad_L_XQ / grad_L_XK / grad_L_XV of the swept steps land where
 *                                     ttt_hip_linear_backward puts them.
 *
 * Swept from the last range to the first with the carries handed on, any cutting of [0, K) into ranges gives the BITS of
 * ttt_hip_linear_backward: the steps are its steps, rounded alike, and the slots hold the operands the one call keeps in its scratch.
 * `d` and `a` describe the whole sequence.  The ordering between a recompute and the sweep that reads its slots (and between a
 * sweep and a recompute that reuses its workspace) is the caller's: the same stream, or events.
 * MFMA sweep only: bf16 activations, F = 64, mini-batches of 16, or of 64 on an explicit TTT_IMPL_MFMA - the geometries
 * ttt_hip_linear_forward_chunk takes.
 *
 *                         recompute_groups                                      sweep_groups
 *   needs                 XK XV last_eta ttt_norm_weight ttt_norm_bias          every field of ttt_hip_linear_backward except the
 *                         W1_checkpoints b1_checkpoints                         checkpoints and W1_init_group / b1_init_group
 *   may be NULL           everything else                                       the checkpoints, W1_init_group, b1_init_group
 */
#ifndef TTT_HIP_BWD_PARTS_H
#define TTT_HIP_BWD_PARTS_H

#include "ttt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the slot workspace for nk groups: B * NH * nk * (G + 1) * (16384 + 256) ; 0 for bad dims or nk <= 0 */
size_t ttt_hip_linear_backward_parts_slots(const ttt_dims* d, int nk);
/* bytes of ln_carry: B * NH * 8 * lanes * 4, lanes = 64 at mini-batches of 16, 256 at mini-batches of 64 ; 0 for bad dims */
size_t ttt_hip_linear_backward_parts_carry(const ttt_dims* d);

int ttt_hip_linear_recompute_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk,
                                    void* slots, size_t slots_bytes, void* stream);
int ttt_hip_linear_sweep_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk,
                                const void* slots, size_t slots_bytes, float* ln_carry, size_t carry_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTT_HIP_BWD_PARTS_H */
