/*
 * ttt_hip_lin_bwd_front.h - a third stage of the TTT-Linear backward over ranges of checkpoint groups, at mini-batches of 16: a sixth
 * header of libttt_hip.so, beside ttt_hip.h and ttt_hip_bwd_parts.h (whose conventions, workspaces and carries these entries share).
 * Additive: TTT_HIP_ABI_VERSION stays what ttt_hip.h says, and every declaration of the other five headers is unchanged.
 *
 * A step of the reverse walk of ttt_hip_linear_sweep_groups does three things that do not depend on the gradient state it carries:
 * the backward of the outer LayerNorm (Z1b = Q W1' + b1', dZ1b and its sums), dXQ = dOut + dZ1b W1'^T, and the inner forward of the
 * step (Z1 = K W1 + b1, the fused LayerNorm / L2 gradient).  All of them read the step's tiles and the slots that
 * ttt_hip_linear_recompute_groups left, so they can run for every step of a range at once:
 *
 *   ttt_hip_linear_front_groups   every step of the groups [k0, k0 + nk), one wave each: writes grad_L_XQ of the step (final) and a
 *                                 19 456-byte RECORD of what the rest of the step takes from those blocks - per lane dZ1b as bf16
 *                                 (32 bytes), its fp32 column sums (16), the addends of the LayerNorm-gradient partial sums (32),
 *                                 x_hat / output gradient / dZ1 of the inner LayerNorm (192), 1/std and sum (go gamma) x_hat (32).
 *                                 Layout [B*NH][nk][G] records; a ragged last group uses fewer.
 *   ttt_hip_linear_chain_groups   the walk that remains, over the groups k0 + nk - 1 .. k0, from the slots AND the records of the same
 *                                 range.  It carries exactly what ttt_hip_linear_sweep_groups carries, the same way: dW1 / db1 from
 *                                 a->grad_L_W1_last / grad_L_b1_last to a->grad_L_W1_init / grad_L_b1_init (may be the same buffers),
 *                                 `ln_carry`, and the reduction into grad_L_ttt_norm_weight / _bias in the range with k0 == 0.  It
 *                                 writes grad_L_last_eta / grad_L_XK / grad_L_XV of its steps.
 *
 * recompute -> front -> chain per range, the ranges walked from the last to the first with the carries handed on, gives the BITS of
 * ttt_hip_linear_backward for any cutting of [0, K).  A range may also mix: sweep_groups and front + chain hand each other the same
 * carries.  Ordering between the three calls of a range, and against calls that reuse a workspace, is the caller's: one stream, or events.
 * MFMA sweep, bf16 activations, F = 64, mini-batches of 16 ONLY (mini-batches of 64 are refused, also on an explicit TTT_IMPL_MFMA).
 *
 *                         front_groups                                          chain_groups
 *   needs                 XQ XK XV grad_L_XQW ttt_norm_weight ttt_norm_bias     what ttt_hip_linear_sweep_groups needs, except
 *   writes                grad_L_XQ, records                                    XV, grad_L_XQW, grad_L_XQ
 *   may be NULL           everything else                                       those three, the checkpoints, W1/b1_init_group
 */
#ifndef TTT_HIP_LIN_BWD_FRONT_H
#define TTT_HIP_LIN_BWD_FRONT_H

#include "ttt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the record workspace for nk groups: B * NH * nk * G * 19456 ; 0 for bad dims, nk <= 0 or CS != 16 */
size_t ttt_hip_linear_backward_front_records(const ttt_dims* d, int nk);

int ttt_hip_linear_front_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk,
                                const void* slots, size_t slots_bytes, void* records, size_t records_bytes, void* stream);
int ttt_hip_linear_chain_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk,
                                const void* slots, size_t slots_bytes, const void* records, size_t records_bytes,
                                float* ln_carry, size_t carry_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTT_HIP_LIN_BWD_FRONT_H */
