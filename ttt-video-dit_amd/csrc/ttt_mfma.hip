// Host-side entry points of the MFMA (bf16 matrix-core) TTT kernels for gfx950: geometry check and launch of
//   TTT-MLP forward   CS = 64: ttt_mfma2.hip (8-wave register-resident scan)   CS = 16: ttt_mfma16.hip
//   TTT-MLP backward  CS = 64: revision 4 - ttt_mfma_rc4.hip (group recompute), ttt_mfma_bwd4.hip (cluster sweep with deriver
//                     waves, tail), orchestrated by ttt_mfma_bwd2.hip
//                     CS = 16 (explicit TTT_IMPL_MFMA only): ttt_mlp16_bwd_body.h, one kernel in ttt_mfma16.hip
//   TTT-Linear forward / backward at CS = 16: ttt_mfma16.hip ; at CS = 64 (explicit TTT_IMPL_MFMA only): ttt_lin64_body.h, same file
// (Round 1's 4-wave scan / recompute kernel lived here; its last user, revision 3 of the backward, lost its round-3 A/B against
// revision 4 - 17.8 vs 13.4 ms per backward at NC = 804, profiles/r3h_* - and was removed with it.)
#include "ttt_mfma.h"
#include "ttt_mfma_dev.h"
#include "ttt_mfma_int.h"

namespace ttt {
namespace mfma {
using namespace ttt::mf;

static unsigned long long* g_dbg = nullptr;
void set_debug_timing(void* buf) { g_dbg = (unsigned long long*)buf; }
unsigned long long* get_debug_timing() { return g_dbg; }

bool supports(const ttt_dims* d, bool mlp, bool backward) {
    if (!(d->F == 64 && d->act_dtype == TTT_DTYPE_BF16)) return false;
    // mini-batches of 16 (ttt_mfma16.hip): MLP and Linear, forward and backward; capi.hip keeps AUTO on the generic MLP backward
    if (d->CS == 16) return true;
    if (!mlp) return d->CS == 64;                // TTT-Linear at 64 (ttt_lin64_body.h); capi.hip keeps AUTO on the generic kernels
    return d->CS == 64 && (!backward || bwd_available());
}

static int n_bh(const ttt_dims* d) { return d->B * d->NH; }
static int n_groups(const ttt_dims* d) { return (d->NC + d->G - 1) / d->G; }

// the fifteen tensors and the geometry of the whole sequence, NCs = 0 ("one call", no final-state store): a part sets NC, NCs, ck0, W1f .. b2f
static ScanParams scan_params(const ttt_dims* d, const ttt_mlp_fwd_args* a) {
    ScanParams p = {};
    p.XQ = (const __bf16*)a->XQ; p.XK = (const __bf16*)a->XK; p.XV = (const __bf16*)a->XV; p.eta = (const __bf16*)a->last_eta;
    p.ln_w = a->ttt_norm_weight; p.ln_b = a->ttt_norm_bias;
    p.W1 = a->W1_init; p.b1 = a->b1_init; p.W2 = a->W2_init; p.b2 = a->b2_init;
    p.W1c = a->W1_checkpoints; p.b1c = a->b1_checkpoints; p.W2c = a->W2_checkpoints; p.b2c = a->b2_checkpoints;
    p.out = (__bf16*)a->XQW;
    p.NH = d->NH; p.NC = d->NC; p.G = d->G; p.K = n_groups(d); p.eps = d->eps;
    return p;
}
void mlp_forward(const ttt_dims* d, const ttt_mlp_fwd_args* a, void* ws, hipStream_t s) {
    const ScanParams p = scan_params(d, a);
    if (d->CS == 16) launch_scan_forward_cs16(p, n_bh(d), g_dbg, s);
    else launch_scan_forward_v2(p, n_bh(d), ws, g_dbg, s);
}
// TTT-MLP backward at CS = 16: the per-step state lives in the caller's four *_init_group buffers, nothing in `ws`
static wv::Mlp16BwdParams mlp16_bwd_params(const ttt_dims* d, const ttt_mlp_bwd_args* a) {
    wv::Mlp16BwdParams p = {};
    p.XQ = (const __bf16*)a->XQ; p.XK = (const __bf16*)a->XK; p.XV = (const __bf16*)a->XV; p.eta = (const __bf16*)a->last_eta;
    p.ln_w = a->ttt_norm_weight; p.ln_b = a->ttt_norm_bias;
    p.W1c = a->W1_checkpoints; p.b1c = a->b1_checkpoints; p.W2c = a->W2_checkpoints; p.b2c = a->b2_checkpoints;
    p.dOut = (const __bf16*)a->grad_L_XQW;
    p.dW1_last = a->grad_L_W1_last; p.db1_last = a->grad_L_b1_last; p.dW2_last = a->grad_L_W2_last; p.db2_last = a->grad_L_b2_last;
    p.W1s = a->W1_init_group; p.b1s = a->b1_init_group; p.W2s = a->W2_init_group; p.b2s = a->b2_init_group;
    p.dln_w = a->grad_L_ttt_norm_weight; p.dln_b = a->grad_L_ttt_norm_bias;
    p.dW1 = a->grad_L_W1_init; p.db1 = a->grad_L_b1_init; p.dW2 = a->grad_L_W2_init; p.db2 = a->grad_L_b2_init;
    p.deta = (__bf16*)a->grad_L_last_eta; p.dXQ = (__bf16*)a->grad_L_XQ; p.dXK = (__bf16*)a->grad_L_XK; p.dXV = (__bf16*)a->grad_L_XV;
    p.NH = d->NH; p.NC = d->NC; p.G = d->G; p.K = n_groups(d); p.eps = d->eps;
    return p;
}
void mlp_backward_cs16(const ttt_dims* d, const ttt_mlp_bwd_args* a, hipStream_t s) {
    launch_mlp_backward_cs16(mlp16_bwd_params(d, a), n_bh(d), s);
}
// The same backward in parts (ttt_wave_types.h: Mlp16BwdPartParams).  G slots per group: the fp32 state entering each step ; the
// carry: the 2 x 16 x 64 cells of the owners' dln shares per (b, h).
size_t mlp_backward_parts_slots(const ttt_dims* d, int nk) {
    return (size_t)d->B * d->NH * (size_t)nk * (size_t)d->G * wv::MLP16_PART_SLOT_BYTES;
}
size_t mlp_backward_parts_carry(const ttt_dims* d) { return (size_t)d->B * d->NH * wv::MLP16_PART_CARRY_FLOATS * sizeof(float); }
void mlp_recompute_groups(const ttt_dims* d, const ttt_mlp_bwd_args* a, int k0, int nk, void* slots, hipStream_t s) {
    const wv::Mlp16BwdPartParams q = {mlp16_bwd_params(d, a), k0, nk, (float*)slots, nullptr};
    launch_mlp_recompute_groups(q, n_bh(d), s);
}
void mlp_sweep_groups(const ttt_dims* d, const ttt_mlp_bwd_args* a, int k0, int nk, const void* slots, float* ln_carry, hipStream_t s) {
    const wv::Mlp16BwdPartParams q = {mlp16_bwd_params(d, a), k0, nk, (float*)const_cast<void*>(slots), ln_carry};
    launch_mlp_sweep_groups(q, n_bh(d), s);
}
// steps [step0, step0 + nsteps) of the scan: the same kernel over a part of the sequence, started from the state in
// a->*_init (what the previous part left in *_final), its checkpoints written at their places in the whole sequence's arrays.
// CS = 64: parts start at checkpoint-group boundaries, the tile pointers are offset to the part.  CS = 16: parts start at any
// step; the body (ttt_mlp16_body.h) takes the whole sequence's pointers and the first step.
void mlp_forward_chunk(const ttt_dims* d, const ttt_mlp_fwd_args* a, int step0, int nsteps, float* W1f, float* b1f, float* W2f, float* b2f,
                       void* ws, hipStream_t s) {
    ScanParams p = scan_params(d, a);
    p.NC = nsteps; p.NCs = d->NC;
    p.W1f = W1f; p.b1f = b1f; p.W2f = W2f; p.b2f = b2f;
    if (d->CS == 16) {
        p.ck0 = step0;
        launch_scan_forward_cs16(p, n_bh(d), g_dbg, s);
    } else {
        const size_t t0 = (size_t)step0 * 64 * 64, e0 = (size_t)step0 * 64;
        p.XQ += t0; p.XK += t0; p.XV += t0; p.eta += e0; p.out += t0;
        p.ck0 = step0 / d->G;
        launch_scan_forward_v2(p, n_bh(d), ws, g_dbg, s);
    }
}
// the same part at CS = 16 as a pair of workgroups per (b, h) (ttt_mlp16_pair_body.h); `ws`: scan_pair16_workspace_bytes
int mlp_forward_chunk_pair16(const ttt_dims* d, const ttt_mlp_fwd_args* a, int step0, int nsteps, float* W1f, float* b1f, float* W2f,
                             float* b2f, void* ws, hipStream_t s) {
    ScanParams p = scan_params(d, a);
    p.NC = nsteps; p.NCs = d->NC; p.ck0 = step0;
    p.W1f = W1f; p.b1f = b1f; p.W2f = W2f; p.b2f = b2f;
    return launch_scan_forward_pair16(p, n_bh(d), ws, s);
}
// steps [step0, step0 + nsteps) of the TTT-Linear scan: the same kernel over a part of the sequence, started from the state in
// a->W1_init / b1_init, its checkpoints written at their places in the whole sequence's arrays, the state after its last step
// left in W1f / b1f (both null: not stored).  Parts start at any step at both mini-batch sizes (ttt_wave_types.h).
static wv::Lin16Params lin16_fwd_params(const ttt_dims* d, const ttt_linear_fwd_args* a) {
    wv::Lin16Params p = {};
    p.XQ = (const __bf16*)a->XQ; p.XK = (const __bf16*)a->XK; p.XV = (const __bf16*)a->XV; p.eta = (const __bf16*)a->last_eta;
    p.ln_w = a->ttt_norm_weight; p.ln_b = a->ttt_norm_bias;
    p.W1 = a->W1_init; p.b1 = a->b1_init;
    p.W1c = a->W1_checkpoints; p.b1c = a->b1_checkpoints;
    p.out = (__bf16*)a->XQW;
    p.NH = d->NH; p.NC = d->NC; p.G = d->G; p.K = n_groups(d); p.eps = d->eps;
    return p;
}
void linear_forward_chunk(const ttt_dims* d, const ttt_linear_fwd_args* a, int step0, int nsteps, float* W1f, float* b1f, hipStream_t s) {
    wv::Lin16ChunkParams c = {lin16_fwd_params(d, a), step0, d->NC, W1f, b1f};
    c.p.NC = nsteps;
    if (d->CS == 16) launch_linear_forward_cs16(c, n_bh(d), s);
    else launch_linear_forward_cs64(c, n_bh(d), s);
}
void linear_forward_chunk_split16(const ttt_dims* d, const ttt_linear_fwd_args* a, int step0, int nsteps, float* W1f, float* b1f,
                                  hipStream_t s) {
    wv::Lin16ChunkParams c = {lin16_fwd_params(d, a), step0, d->NC, W1f, b1f};
    c.p.NC = nsteps;
    launch_linear_forward_split16(c, n_bh(d), s);
}
void linear_forward(const ttt_dims* d, const ttt_linear_fwd_args* a, void*, hipStream_t s) {
    linear_forward_chunk(d, a, 0, d->NC, nullptr, nullptr, s);
}
static wv::Lin16Params linear_bwd_params(const ttt_dims* d, const ttt_linear_bwd_args* a) {
    wv::Lin16Params p = {};
    p.XQ = (const __bf16*)a->XQ; p.XK = (const __bf16*)a->XK; p.XV = (const __bf16*)a->XV; p.eta = (const __bf16*)a->last_eta;
    p.ln_w = a->ttt_norm_weight; p.ln_b = a->ttt_norm_bias;
    p.W1c = const_cast<float*>(a->W1_checkpoints); p.b1c = const_cast<float*>(a->b1_checkpoints);      // read only here
    p.dOut = (const __bf16*)a->grad_L_XQW;
    p.dW1_last = a->grad_L_W1_last; p.db1_last = a->grad_L_b1_last;
    p.scratch_w = (char*)a->W1_init_group; p.scratch_b = a->b1_init_group;      // G x 16 KiB and G x 64 floats per (b,h)
    p.dln_w = a->grad_L_ttt_norm_weight; p.dln_b = a->grad_L_ttt_norm_bias;
    p.dW1 = a->grad_L_W1_init; p.db1 = a->grad_L_b1_init;
    p.deta = (__bf16*)a->grad_L_last_eta; p.dXQ = (__bf16*)a->grad_L_XQ; p.dXK = (__bf16*)a->grad_L_XK; p.dXV = (__bf16*)a->grad_L_XV;
    p.NH = d->NH; p.NC = d->NC; p.G = d->G; p.K = n_groups(d); p.eps = d->eps;
    return p;
}
void linear_backward(const ttt_dims* d, const ttt_linear_bwd_args* a, void*, hipStream_t s) {
    const wv::Lin16Params p = linear_bwd_params(d, a);
    if (d->CS == 16) launch_linear_backward_cs16(p, n_bh(d), s);
    else launch_linear_backward_cs64(p, n_bh(d), s);
}
// The backward in parts (ttt_wave_types.h: Lin16BwdPartParams).  G + 1 slots per group: the state entering each step and the state
// that ends the group ; the carry: 8 partial sums per lane of the scan's wave (CS = 16) or four waves (CS = 64).
size_t linear_backward_parts_slots(const ttt_dims* d, int nk) {
    return (size_t)d->B * d->NH * (size_t)nk * (size_t)(d->G + 1) * wv::LIN_PART_SLOT_BYTES;
}
size_t linear_backward_parts_carry(const ttt_dims* d) {
    return (size_t)d->B * d->NH * wv::LIN_PART_CARRY_FLOATS * (d->CS == 16 ? 64 : 256) * sizeof(float);
}
void linear_recompute_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, void* slots, hipStream_t s) {
    const wv::Lin16BwdPartParams q = {linear_bwd_params(d, a), k0, nk, (char*)slots, nullptr};
    launch_linear_recompute_groups(q, d->CS, n_bh(d), s);
}
void linear_sweep_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, float* ln_carry, hipStream_t s) {
    const wv::Lin16BwdPartParams q = {linear_bwd_params(d, a), k0, nk, (char*)const_cast<void*>(slots), ln_carry};
    launch_linear_sweep_groups(q, d->CS, n_bh(d), s);
}
// The third stage at mini-batches of 16 (ttt_wave_types.h: Lin16BwdFrontParams): one record per step of the range.
size_t linear_backward_front_records(const ttt_dims* d, int nk) {
    return (size_t)d->B * d->NH * (size_t)nk * (size_t)d->G * wv::LIN_FRONT_RECORD_BYTES;
}
void linear_front_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, void* records, hipStream_t s) {
    const wv::Lin16BwdFrontParams f = {{linear_bwd_params(d, a), k0, nk, (char*)const_cast<void*>(slots), nullptr}, (char*)records};
    const int s_hi = (k0 + nk) * d->G < d->NC ? (k0 + nk) * d->G : d->NC;
    launch_linear_front_groups(f, n_bh(d) * (s_hi - k0 * d->G), s);
}
void linear_chain_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, const void* records,
                         float* ln_carry, hipStream_t s) {
    const wv::Lin16BwdFrontParams f = {{linear_bwd_params(d, a), k0, nk, (char*)const_cast<void*>(slots), ln_carry},
                                       (char*)const_cast<void*>(records)};
    launch_linear_chain_groups(f, n_bh(d), s);
}
// The same stage at mini-batches of 64: a step's record is the records of its four 16-row token blocks, one front wave each.
size_t linear_backward_front64_records(const ttt_dims* d, int nk) {
    return (size_t)d->B * d->NH * (size_t)nk * (size_t)d->G * wv::LIN64_FRONT_RECORD_BYTES;
}
void linear_front64_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, void* records, hipStream_t s) {
    const wv::Lin16BwdFrontParams f = {{linear_bwd_params(d, a), k0, nk, (char*)const_cast<void*>(slots), nullptr}, (char*)records};
    const int s_hi = (k0 + nk) * d->G < d->NC ? (k0 + nk) * d->G : d->NC;
    launch_linear_front64_groups(f, n_bh(d) * (s_hi - k0 * d->G) * 4, s);
}
void linear_chain64_groups(const ttt_dims* d, const ttt_linear_bwd_args* a, int k0, int nk, const void* slots, const void* records,
                           float* ln_carry, hipStream_t s) {
    const wv::Lin16BwdFrontParams f = {{linear_bwd_params(d, a), k0, nk, (char*)const_cast<void*>(slots), ln_carry},
                                       (char*)const_cast<void*>(records)};
    launch_linear_chain64_groups(f, n_bh(d), s);
}

}  // namespace mfma
}  // namespace ttt
