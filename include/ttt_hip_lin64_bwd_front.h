/*
 * ttt_hip_lin64_bwd_front.h - the third stage of the TTT-Linear backward over ranges of checkpoint groups at mini-batches of 64: an
 * eighth header of libttt_hip.so, beside ttt_hip_bwd_parts.h and ttt_hip_lin_bwd_front.h (whose conventions, workspaces and carries
 * these entries share).  Additive: TTT_HIP_ABI_VERSION stays what ttt_hip.h says, and every declaration of the other seven headers is
 * unchanged - in particular the entries of ttt_hip_lin_bwd_front.h keep refusing mini-batches of 64.
 *
 * As at mini-batches of 16, a step of the reverse walk of ttt_hip_linear_sweep_groups does three things that do not depend on the
 * gradient state it carries: the backward of the outer LayerNorm, dXQ = dOut + dZ1b W1'^T and the inner forward of the step.  At
 * mini-batches of 64 each of the four waves of the walk does them for its own 16 token rows, without a word from the others:
 *
 *   ttt_hip_linear_front64_groups every step of the groups [k0, k0 + nk), one wave per 16-row token block (four per step, none waits
 *                                 for another): writes grad_L_XQ of the step (final) and a 77 824-byte RECORD per step - four block
 *                                 records [w] of 19 456 bytes in the field layout of ttt_hip_lin_bwd_front.h.
 *                                 Layout [B*NH][nk][G] records; a ragged last group uses fewer.
 *   ttt_hip_linear_chain64_groups the walk that remains, one workgroup of four waves per (batch, head) over the groups
 *                                 k0 + nk - 1 .. k0, from the slots AND the records of the same range.  It carries exactly what
 *                                 ttt_hip_linear_sweep_groups carries at mini-batches of 64, the same way: dW1 / db1 from
 *                                 a->grad_L_W1_last / grad_L_b1_last to a->grad_L_W1_init / grad_L_b1_init (may be the same buffers),
 *                                 `ln_carry`, and the reduction into grad_L_ttt_norm_weight / _bias in the range with k0 == 0.  It
 *                                 writes grad_L_last_eta / grad_L_XK / grad_L_XV of its steps.
 *
 * recompute -> front -> chain per range, the ranges walked from the last to the first with the carries handed on, gives the BITS of
 * ttt_hip_linear_backward (TTT_IMPL_MFMA, mini-batches of 64) for any cutting of [0, K).  A range may also mix: sweep_groups and
 * front + chain hand each other the same carries.  Ordering between the three calls of a range, and against calls that reuse a
 * workspace, is the caller's: one stream, or events.
 * MFMA sweep, bf16 activations, F = 64, mini-batches of 64 on an explicit TTT_IMPL_MFMA ONLY (mini-batches of 16, TTT_IMPL_AUTO and
 * fp32 activations are refused).
 *
 *                         front64_groups                                        chain64_groups
 *   needs                 XQ XK XV grad_L_XQW ttt_norm_weight ttt_norm_bias     what ttt_hip_linear_sweep_groups needs, except
 *   writes                grad_L_XQ, records                                    XV, grad_L_XQW, grad_L_XQ
 *   may be NULL           everything else                                       those three, the checkpoints, W1/b1_init_group
 */
#ifndef TTT_HIP_LIN64_BWD_FRONT_H
#define TTT_HIP_LIN64_BWD_FRONT_H

#include "ttt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the record workspace for nk groups: B * NH * nk * G * 77824 ; 0 for bad dims, nk <= 0, or anything but bf16 activations,
 * F = 64, CS = 64 on an explicit TTT_IMPL_MFMA */
size_t ttt_hip_linear_backward_front64_records(const ttt_dims* d, int nk);

int ttt_hip_linear_front64_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk,
                                  const void* slots, size_t slots_bytes, void* records, size_t records_bytes, void* stream);
int ttt_hip_linear_chain64_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk,
                                  const void* slots, size_t slots_bytes, const void* records, size_t records_bytes,
                                  float* ln_carry, size_t carry_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TTT_HIP_LIN64_BWD_FRONT_H */
