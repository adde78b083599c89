// TTT-Linear scans at mini-batches of 64 tokens (F = 64) on the wave backend of ttt_lin16_body.h: one workgroup of FOUR waves owns
// one (batch, head) scan.  The step is the step of the mini-batch-16 body (same primal form, same rounding points: MFMA operands in
// bf16, state / checkpoints / bias sums as documented there); what changes is who holds what:
//   * wave w owns the token rows [16w, 16w + 16) of the mini-batch for everything that is row-wise - Z1 = K W1 + b1, the fused
//     LayerNorm / L2 gradient, Z1b = Q W1' + b1', the output LayerNorm + residual and, in the sweep, every per-token gradient; row
//     reductions stay inside the wave (lin16::rowsum64), exactly as at mini-batch 16;
//   * wave w owns the column slice W1[:, 16w .. 16w + 16) of the fp32 state (4 accumulator tiles, rows = f_in, lane = f_out), and of
//     dW1 in the sweep: the updates W1 += K^T Gs, dW1 += Q^T dZ1b, dW1 += K^T dZ1 contract over all 64 tokens, so the wave takes the
//     token-side operand of every token block from the K / Q tiles in LDS (transposed reads) and the gradient-side operand of every
//     token block from an exchange buffer the four waves fill;
//   * products that read the whole state (Z1, Z1b; in the sweep K dW1 and gZ1 dW1^T) take it from a bf16 image in LDS that the four
//     waves publish slice by slice: L_WI holds the 8 rho-order operand fragments [ks][fb] (what lin16 keeps as W1F), L_TR the
//     [f_out][f_in] image for the transposed fragments.
//   * bias: every wave keeps the whole b1 (db1 in the sweep); the per-wave column sums over its 16 tokens go through L_PS and are
//     added by every wave in the same order, so the four copies stay bit-identical.
// Workgroup barriers per step.  Forward: 2 (A: Gs + column sums published | update | B: new W1 image published | Z1b, output; the
// image of step i is also what Z1 of step i + 1 reads, kept in registers).  Sweep: 2 per recomputed step, 3 per reverse step (A: dZ1b
// published | dW1 update, dW1 images | B | per-token gradients of the inner step, dZ1 published | C | dW1 update).  Every shared
// buffer has its writer phase and its reader phase on opposite sides of a barrier; the hazards are written next to each buffer below
// and the CPU suite runs this body on the wave emulator with its LDS race detector (tests/test_emul_lin64_cpu.py).  One exchange the
// detector does not see: the state that ends a checkpoint group goes to L_WHI through lin16::st_pack / ld_pack on raw pointers
// (the same code path as a scratch slot in global memory), so that one rests on the barrier placement alone - each wave writes its
// four fragments after R1, the barrier before `break` follows, and only the first reverse step of the group reads them.
// K / V / Q / dOut tiles are double-buffered by a toggle (`cur`), each wave staging its own 16 rows; the tiles of the next step are
// requested at the top of a step and parked where no wave can still be reading the other buffer (forward: after B; recompute: at
// the end of the step; reverse: between A and B).
// The sweep parks the state entering every step of a checkpoint group as packed operands in both orientations in the caller's
// scratch, 16 KiB per step and (b, h) - the slot layout of lin16 (fragments 0..7 = [ks][fb], 8..15 transposed [ks][fa]); wave w
// writes the four fragments of its slice.  Global stores of one wave are read by the others only across a workgroup barrier.
// Math: reference ops/ttt_linear.py:8-54, kernels/linear_backward.py:73-197, SURVEY.md Appendix A, oracle/ttt_oracle.py.
#pragma once
#include "ttt_lin16_body.h"

namespace ttt {
namespace lin64 {
using namespace ttt::wv;
using lin16::cat;
using lin16::IMG_BYTES;
using lin16::InnerGrad;
using lin16::IS;
using lin16::pack4;
using lin16::SLOT_BYTES;
using lin16::stack;
using lin16::Stage;
using lin16::TRS;
using lin16::TS;
using lin16::zero4;

constexpr int WAVES = 4;
constexpr int TILE_B = lin16::TILE * 2;          // bytes of a padded [16][64] bf16 tile: one wave's rows
constexpr int T64_B = WAVES * TILE_B;            // a whole mini-batch
constexpr int FRAG_B = 64 * 16;                  // one operand fragment: 64 lanes x 16 bytes
// workgroup LDS map (bytes)
constexpr int L_K = 0, L_V = L_K + 2 * T64_B, L_Q = L_V + 2 * T64_B;      // 2 buffers each
constexpr int L_IMG = L_Q + 2 * T64_B;                                      // per wave: 2 private images [64][IS] bf16
constexpr int L_ETA = L_IMG + WAVES * 2 * IMG_BYTES;                        // per wave: [2][16] fp32
constexpr int L_WI = L_ETA + WAVES * 128;                                   // state image: 8 fragments [ks][fb]
constexpr int L_X = L_WI + 8 * FRAG_B;                                      // exchange [token block][fb][lane] x 8 bytes
constexpr int L_PS = L_X + 16 * 512;                                        // [wave][64] fp32 column sums
constexpr int GROUP_LDS = L_PS + WAVES * 256;                               // what forward() uses
// backward() only
constexpr int L_D = GROUP_LDS;                                              // dOut tiles, 2 buffers
constexpr int L_X2 = L_D + 2 * T64_B, L_PS2 = L_X2 + 16 * 512;              // second exchange (dZ1) and its column sums
constexpr int L_TR = L_PS2 + WAVES * 256;                                   // [64 f_out][TRS] bf16
constexpr int L_WHI = L_TR + 64 * TRS * 2;                                  // the state that ends a checkpoint group: one slot
constexpr int GROUP_LDS_BWD = L_WHI + SLOT_BYTES;
static_assert(GROUP_LDS_BWD <= 160 * 1024, "LDS budget");
static_assert(T64_B % 16 == 0 && L_WI % 16 == 0 && L_X % 16 == 0 && L_TR % 16 == 0 && L_WHI % 16 == 0, "alignment");

// tiles shared between waves are written with the tracked stores (the emulator's race detector sees them)
template <class BK>
TTT_WV_FN void park(BK& bk, const Stage& st, int tile_off) {
    const int l = bk.lane();
    const int o = tile_off + ((l >> 3) * TS + (l & 7) * 8) * 2;
    bk.template lds_store<u32x4>(o, st.lo);
    bk.template lds_store<u32x4>(o + 8 * TS * 2, st.hi);
}
template <class BK>
TTT_WV_FN void park_eta(BK& bk, unsigned short pe, int eta_off) {
    if (bk.lane() < 16) bk.template lds<float>(eta_off + bk.lane() * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
}

// this wave's slice of a 64 x 64 matrix (tiles T[fa]: rows = f_in, lane = f_out in block w) -> its two fragments of the L_WI image
template <class BK>
TTT_WV_FN void publish_slice(BK& bk, int w, const f32x4 (&T)[4], bf16x8 (&own)[2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        own[ks] = stack(T[2 * ks], T[2 * ks + 1]);
        bk.template lds_store<bf16x8>(L_WI + (ks * 4 + w) * FRAG_B + bk.lane() * 16, own[ks]);
    }
}
template <class BK>
TTT_WV_FN void load_image(BK& bk, bf16x8 (&Wp)[8]) {
#pragma unroll
    for (int f = 0; f < 8; ++f) Wp[f] = bk.template lds_load<bf16x8>(L_WI + f * FRAG_B + bk.lane() * 16);
}
// ... and its rows of the [f_out][f_in] image at L_TR
template <class BK>
TTT_WV_FN void publish_transposed(BK& bk, int w, const f32x4 (&T)[4]) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fa = 0; fa < 4; ++fa) bk.template lds_store<bf16x4>(L_TR + ((16 * w + i) * TRS + 16 * fa + 4 * g) * 2, pack4(T[fa]));
}
// transposed fragment [ks][fa] of the L_TR image: lane = f_in of block fa, k = f_out in [32 ks, 32 ks + 32) in rho order
template <class BK>
TTT_WV_FN bf16x8 transposed_frag(BK& bk, int ks, int fa16) {
    return cat(lin16::tr4(bk, L_TR, TRS, 32 * ks, fa16), lin16::tr4(bk, L_TR, TRS, 32 * ks + 16, fa16));
}
// a wave's (rows = t, lane = f) packs and fp32 column sums -> exchange buffer `x_off` / `ps_off`
template <class BK>
TTT_WV_FN void publish_rows(BK& bk, int w, int x_off, int ps_off, const bf16x4 (&xp)[4], const float (&cs)[4]) {
    const int l = bk.lane(), g = l >> 4, i = l & 15;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        bk.template lds_store<bf16x4>(x_off + ((w * 4 + fb) * 64 + l) * 8, xp[fb]);
        if (g == 0) bk.template lds_store<float>(ps_off + (w * 64 + 16 * fb + i) * 4, cs[fb]);
    }
}
// T[fa] += X^T Y over all 64 tokens: X = the tiles at `tiles_off` (K or Q of the step), Y = this wave's feature block of the exchange ;
// bias[fb] += column sums of all four waves (every wave, same order)
template <class BK>
TTT_WV_FN void update_slice(BK& bk, int w, int tiles_off, int x_off, int ps_off, f32x4 (&T)[4], float (&bias)[4]) {
    const int l = bk.lane(), i = l & 15;
#pragma unroll
    for (int tb = 0; tb < 4; ++tb) {
        const bf16x4 y = bk.template lds_load<bf16x4>(x_off + ((tb * 4 + w) * 64 + l) * 8);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) T[fa] = bk.mma16(lin16::tr4(bk, tiles_off + tb * TILE_B, TS, 0, 16 * fa), y, T[fa]);
    }
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const int o = ps_off + (16 * fb + i) * 4;
        bias[fb] += (bk.template lds_load<float>(o) + bk.template lds_load<float>(o + 256)) +
                    (bk.template lds_load<float>(o + 512) + bk.template lds_load<float>(o + 768));
    }
}

struct Consts {
    bf16x4 ONES, IDP, IDN;       // ones / +-identity as mma16 A operand (lane = t = i, k-slot e = token 4g + e)
    float gam[4], bet[4];
};
template <class BK>
TTT_WV_FN void make_consts(BK& bk, const Lin16Params& p, int head, Consts& c) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        c.ONES[e] = (__bf16)1.0f;
        c.IDP[e] = (__bf16)((4 * g + e) == i ? 1.0f : 0.0f);
        c.IDN[e] = (__bf16)((4 * g + e) == i ? -1.0f : 0.0f);
    }
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        c.gam[fb] = p.ln_w[(size_t)head * 64 + 16 * fb + i];
        c.bet[fb] = p.ln_b[(size_t)head * 64 + 16 * fb + i];
    }
}

// first half of the forward step for this wave's 16 tokens: Z1 = K W1 + b1, fused LayerNorm / L2 gradient, Gs = -eta gZ1 and its
// column sums (of the ROUNDED Gs, by a ones-MFMA, as at mini-batch 16) -> L_X / L_PS.  Kt, Vt: this wave's tiles.
template <class BK>
TTT_WV_FN void inner_publish(BK& bk, int w, int Kt, int Vt, int eta_off, const bf16x8 (&Wp)[8], const float (&b1v)[4], const Consts& c, float eps) {
    const int g = bk.lane() >> 4;
    const bf16x8 kA0 = lin16::rho_read(bk, Kt, 0), kA1 = lin16::rho_read(bk, Kt, 32);
    const f32x4 eta4 = bk.template lds<f32x4>(eta_off + 4 * g * 4);
    f32x4 z[4], tg[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const bf16x4 kT = lin16::tr4(bk, Kt, TS, 0, 16 * fb);
        f32x4 a = zero4();
        a = bk.mma32(kA0, Wp[fb], a);
        a = bk.mma32(kA1, Wp[4 + fb], a);
        z[fb] = a + b1v[fb];
        tg[fb] = bk.mma16(c.IDN, kT, bk.mma16(c.IDP, lin16::tr4(bk, Vt, TS, 0, 16 * fb), zero4()));       // exact V - K
    }
    InnerGrad ig;
    lin16::inner_grad(bk, z, tg, c.gam, c.bet, eps, ig);
    bf16x4 gzp[4];
    float cs[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        gzp[fb] = pack4(ig.gz[fb] * (-eta4));
        cs[fb] = bk.mma16(c.ONES, gzp[fb], zero4())[0];
    }
    publish_rows(bk, w, L_X, L_PS, gzp, cs);
}

// ===================================================================================================================
// forward scan of (b, h) = bh over the steps [c.step0, c.step0 + c.p.NC) of a scan of c.NCs steps (Lin16ChunkParams,
// ttt_wave_types.h) ; the four waves of the workgroup call it together.  The hand-over between parts is the fp32 state (every
// wave its slice W1t, all of them b1v): the L_WI image is published from it before the first step and after every update, so a
// part that starts at any step reproduces the bits of the one-call scan.
template <class BK>
TTT_WV_FN void forward_part(BK& bk, const Lin16ChunkParams& c, int bh) {
    const Lin16Params& p = c.p;
    const int l0 = bk.lane(), w = bk.wave();
    const int NC = p.NC, G = p.G, head = bh % p.NH, step0 = c.step0;
    const int IMG = L_IMG + w * 2 * IMG_BYTES, ETA = L_ETA + w * 128, own = w * TILE_B;

    f32x4 W1t[4];        // [fa]  W1[16fa + 4g + r][16w + i]
    float b1v[4];
    Consts k;
    make_consts(bk, p, head, k);
    {
        const int g = l0 >> 4, i = l0 & 15;
        const float* W1g = p.W1 + (size_t)bh * 64 * 64;
#pragma unroll
        for (int fa = 0; fa < 4; ++fa)
#pragma unroll
            for (int r = 0; r < 4; ++r) W1t[fa][r] = W1g[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * w + i];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) b1v[fb] = p.b1[(size_t)bh * 64 + 16 * fb + i];
    }
    const size_t tile0 = (size_t)bh * c.NCs + step0;
    Stage sk, sv, sq;
    unsigned short pe;
    lin16::stage_request(bk, sk, p.XK + tile0 * 4096 + w * 1024);
    lin16::stage_request(bk, sv, p.XV + tile0 * 4096 + w * 1024);
    lin16::stage_request(bk, sq, p.XQ + tile0 * 4096 + w * 1024);
    pe = *reinterpret_cast<const unsigned short*>(p.eta + tile0 * 64 + 16 * w + (l0 & 15));
    park(bk, sk, L_K + own); park(bk, sv, L_V + own); park(bk, sq, L_Q + own);
    park_eta(bk, pe, ETA);
    bf16x8 Wp[8], mine[2];
    publish_slice(bk, w, W1t, mine);
    bk.barrier();
    load_image(bk, Wp);

    for (int it = 0; it < NC; ++it) {
        const size_t tile = tile0 + it;
        const int buf = it & 1, nb = buf ^ 1;
        const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        {   // next step's inputs, parked at the end of this step
            const size_t tn = tile0 + (it + 1 < NC ? it + 1 : it);
            lin16::stage_request(bk, sk, p.XK + tn * 4096 + w * 1024);
            lin16::stage_request(bk, sv, p.XV + tn * 4096 + w * 1024);
            lin16::stage_request(bk, sq, p.XQ + tn * 4096 + w * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + tn * 64 + 16 * w + (l & 15));
        }
        if ((step0 + it) % G == 0) {      // checkpoint: state entering step `step0 + it` ; wave w its slice, wave 0 the bias
            const size_t ck = (size_t)bh * p.K + (step0 + it) / G;
            float* W1g = p.W1c + ck * 64 * 64;
#pragma unroll
            for (int fa = 0; fa < 4; ++fa)
#pragma unroll
                for (int r = 0; r < 4; ++r) W1g[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * w + i] = W1t[fa][r];
            if (w == 0 && g == 0)
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) p.b1c[ck * 64 + 16 * fb + i] = b1v[fb];
        }
        inner_publish(bk, w, L_K + buf * T64_B + own, L_V + buf * T64_B + own, ETA + buf * 64, Wp, b1v, k, p.eps);
        bk.barrier();                                                   // A: L_X, L_PS written | read
        update_slice(bk, w, L_K + buf * T64_B, L_X, L_PS, W1t, b1v);    // W1 += K^T Gs ; b1 += colsum Gs
        publish_slice(bk, w, W1t, mine);
        bk.barrier();                                                   // B: L_WI written | read (until A of the next step)
        load_image(bk, Wp);
        {   // Z1b = Q W1' + b1' ; LayerNorm ; + Q -> XQW
            const int Qt = L_Q + buf * T64_B + own;
            const bf16x8 qA0 = lin16::rho_read(bk, Qt, 0), qA1 = lin16::rho_read(bk, Qt, 32);
            f32x4 y[4], qc[4];
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                f32x4 a = zero4();
                a = bk.mma32(qA0, Wp[fb], a);
                a = bk.mma32(qA1, Wp[4 + fb], a);
                y[fb] = a + b1v[fb];
                qc[fb] = bk.mma16(k.IDP, lin16::tr4(bk, Qt, TS, 0, 16 * fb), zero4());
            }
            lin16::normalize_rows(bk, y, p.eps);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) y[fb] = qc[fb] + k.gam[fb] * y[fb] + k.bet[fb];
            lin16::store_rows(bk, IMG, y, p.out + tile * 4096 + w * 1024);
        }
        // the other buffer's K tiles were last read by other waves before B of the step before this one
        park(bk, sk, L_K + nb * T64_B + own); park(bk, sv, L_V + nb * T64_B + own); park(bk, sq, L_Q + nb * T64_B + own);
        park_eta(bk, pe, ETA + nb * 64);
        bk.lds_fence();
    }
    if (c.W1f) {      // hand the state on: wave w its column slice, wave 0 the bias, as the checkpoint store does.
        // W1f / b1f MAY ALIAS p.W1 / p.b1 (the pipeline carries the state in place).  Global memory, so the emulator's race detector
        // does not see this one; it rests on the barriers: all four waves read b1 and their own W1 slice before the first barrier
        // (in front of the step loop), and these stores come behind barriers A and B of the last step - no wave can still be
        // reading the initial state, and a wave overwrites only the slice that it alone read.  (Lane indices of its own, so that
        // the store keeps nothing alive across the step loop.)
        const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        float* W1g = c.W1f + (size_t)bh * 64 * 64;
#pragma unroll
        for (int fa = 0; fa < 4; ++fa)
#pragma unroll
            for (int r = 0; r < 4; ++r) W1g[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * w + i] = W1t[fa][r];
        if (w == 0 && g == 0)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) c.b1f[(size_t)bh * 64 + 16 * fb + i] = b1v[fb];
    }
}
// the whole sequence in one call: the part [0, NC) without a final-state store
template <class BK>
TTT_WV_FN void forward(BK& bk, const Lin16Params& p, int bh) {
    Lin16ChunkParams c;
    c.p = p;
    c.step0 = 0;
    c.NCs = p.NC;
    c.W1f = c.b1f = nullptr;
    forward_part(bk, c, bh);
}

// ---- the pieces of the backward in parts (recompute_groups / sweep_groups, behind backward() below): the steps of backward() as
// functions ; backward() keeps them inline and lin16::fma4 fixes the fused products its compiled code takes (see ttt_lin16_body.h) ------
// what a sweep carries from step to step
struct BwdCarry {
    f32x4 dWt[4];         // [fa]  dW1[16fa + 4g + r][16w + i]
    float db[4];          // db1[16fb + i], the same in every wave
    float dgam[4], dbet[4];     // per-lane partial sums over this lane's token rows
};
// this wave's column slice of a [64][64] fp32 matrix in global memory <-> tiles T[fa]
template <class BK>
TTT_WV_FN void load_slice(BK& bk, int w, const float* M, f32x4 (&T)[4]) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fa = 0; fa < 4; ++fa)
#pragma unroll
        for (int r = 0; r < 4; ++r) T[fa][r] = M[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * w + i];
}
template <class BK>
TTT_WV_FN void store_slice(BK& bk, int w, float* M, const f32x4 (&T)[4]) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fa = 0; fa < 4; ++fa)
#pragma unroll
        for (int r = 0; r < 4; ++r) M[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * w + i] = T[fa][r];
}
// parks the state (every wave its slice W1t) as packed operands in both orientations at `slot`: publishes the L_WI / L_TR images,
// barrier R1 (L_WI, L_TR written | read), then wave w stores the four fragments of its slice
template <class BK>
TTT_WV_FN void park_state(BK& bk, int w, const f32x4 (&W1t)[4], char* slot) {
    bf16x8 mine[2];
    publish_slice(bk, w, W1t, mine);
    publish_transposed(bk, w, W1t);
    bk.barrier();                                           // R1: L_WI, L_TR written | read
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        lin16::st_pack(bk, slot, ks * 4 + w, mine[ks]);
        lin16::st_pack(bk, slot, 8 + ks * 4 + w, transposed_frag(bk, ks, 16 * w));
    }
}
// one recomputed step from the L_WI image park_state published: this wave's tokens through the inner step, barrier R2, the update
// of its slice.  Kb / Vb: the K / V tiles of the mini-batch (all four waves' rows).
template <class BK>
TTT_WV_FN void recompute_step(BK& bk, int w, const Consts& c, float eps, int Kb, int Vb, int eta_off, f32x4 (&W1t)[4], float (&b1v)[4]) {
    {
        bf16x8 Wp[8];
        load_image(bk, Wp);
        inner_publish(bk, w, Kb + w * TILE_B, Vb + w * TILE_B, eta_off, Wp, b1v, c, eps);
    }
    bk.barrier();                                           // R2: L_X, L_PS written | read (until R1 of the next step)
    update_slice(bk, w, Kb, L_X, L_PS, W1t, b1v);
}
// one step of the reverse walk (step numbers (n): oracle/ttt_oracle.py:_lin_step_bwd in the order lin16 lists them).  Kb .. Db: the
// tiles of the mini-batch, eta_off: this wave's eta ; slot / b1v: the state entering the step, slot_n / b1n: the state after it ; y:
// the carried gradients ; `tile`: the step's tile of the whole sequence.  `mid()` runs between barriers A and B: where the caller parks
// the tiles it requested for the next step into the other buffer, which was last read (K in (10), Q in (3)) by the step before this
// one.  Ends with the carried update (10); the caller fences LDS behind it.
template <class BK, class Mid>
TTT_WV_FN void reverse_step(BK& bk, int l, int w, const Lin16Params& p, const Consts& c, BwdCarry& y, size_t tile, int Kb, int Vb, int Qb,
                            int Db, int eta_off, const char* slot, const char* slot_n, const float (&b1v)[4], const float (&b1n)[4],
                            Mid&& mid) {
    const int g = l >> 4, i = l & 15;
    const int IMG = L_IMG + w * 2 * IMG_BYTES, own = w * TILE_B;
    const int Kt = Kb + own, Vt = Vb + own, Qt = Qb + own, Dt = Db + own;
    const f32x4 eta4 = bk.template lds<f32x4>(eta_off + 4 * g * 4);
    // ---- (2) outer LayerNorm backward for this wave's tokens: Z1b = Q W1n + b1n ; dZ1b -> L_X, its column sums -> L_PS ------
    f32x4 dq[4];                     // starts as dOut (accumulator layout), becomes dQ
    {
        bf16x4 dZbp[4];
        float cs[4];
        const bf16x8 qA0 = lin16::rho_read(bk, Qt, 0), qA1 = lin16::rho_read(bk, Qt, 32);
        f32x4 yy[4], dxl[4], t2[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            f32x4 a = zero4();
            a = bk.mma32(qA0, lin16::ld_pack(bk, slot_n, fb), a);
            a = bk.mma32(qA1, lin16::ld_pack(bk, slot_n, 4 + fb), a);
            yy[fb] = a + b1n[fb];
            dq[fb] = bk.mma16(c.IDP, lin16::tr4(bk, Dt, TS, 0, 16 * fb), zero4());                // exact dOut
        }
        const f32x4 rstdl = lin16::normalize_rows(bk, yy, p.eps);                                 // yy <- x_hat of the output LN
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dx = dq[fb] * yy[fb];
            y.dgam[fb] += dx[0] + dx[1] + dx[2] + dx[3];
            y.dbet[fb] += dq[fb][0] + dq[fb][1] + dq[fb][2] + dq[fb][3];
            dxl[fb] = dq[fb] * c.gam[fb];
            t2[fb] = dxl[fb] * yy[fb];
        }
        const f32x4 u1 = lin16::rowsum64(bk, dxl), u2 = lin16::rowsum64(bk, t2);
        const f32x4 sc = rstdl * (1.0f / 64.0f);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dzb = (64.0f * dxl[fb] - u1 - yy[fb] * u2) * sc;
            dZbp[fb] = pack4(dzb);
            cs[fb] = lin16::colsum16(bk, dzb);                                                    // fp32 sums, as at mini-batch 16
        }
        publish_rows(bk, w, L_X, L_PS, dZbp, cs);
        // ---- (4) dQ = dOut + dZ1b W1n^T --------------------------------------------------------------------------------------
        bf16x8 aZ[2];
        lin16::image_of(bk, IMG, dZbp, aZ);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            dq[fa] = bk.mma32(aZ[0], lin16::ld_pack(bk, slot_n, 8 + fa), dq[fa]);
            dq[fa] = bk.mma32(aZ[1], lin16::ld_pack(bk, slot_n, 12 + fa), dq[fa]);
        }
        lin16::store_rows(bk, IMG + IMG_BYTES, dq, p.dXQ + tile * 4096 + w * 1024);
    }
    bk.lds_fence();
    // ---- (1) inner forward of the step for this wave's tokens: Z1 = K W + b, LN / L2 gradient ------------------------------
    const bf16x8 kA0 = lin16::rho_read(bk, Kt, 0), kA1 = lin16::rho_read(bk, Kt, 32);
    bf16x4 kT[4];
    InnerGrad ig;
    {
        f32x4 z[4], tg[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            kT[fb] = lin16::tr4(bk, Kt, TS, 0, 16 * fb);
            f32x4 a = zero4();
            a = bk.mma32(kA0, lin16::ld_pack(bk, slot, fb), a);
            a = bk.mma32(kA1, lin16::ld_pack(bk, slot, 4 + fb), a);
            z[fb] = a + b1v[fb];
            tg[fb] = bk.mma16(c.IDN, kT[fb], bk.mma16(c.IDP, lin16::tr4(bk, Vt, TS, 0, 16 * fb), zero4()));   // exact V - K
        }
        lin16::inner_grad(bk, z, tg, c.gam, c.bet, p.eps, ig);
    }
    bk.barrier();                                               // A: L_X, L_PS written | read ; every wave has left the step before
    // ---- (3) dW1n += Q^T dZ1b ; db1n += colsum dZ1b ; the images of dW1n -----------------------------------------------------
    update_slice(bk, w, Qb, L_X, L_PS, y.dWt, y.db);
    {
        bf16x8 mine[2];
        publish_slice(bk, w, y.dWt, mine);
        publish_transposed(bk, w, y.dWt);
    }
    mid();
    bk.barrier();                                               // B: L_WI, L_TR written | read (until A of the next step)
    // ---- (6) dgZ1 = -eta (K dW1n + db1n) ; (8) backward of the fused LN / L2 gradient -> dZ1, dt, dgamma, dbeta -----------------
    bf16x4 dZ1p[4];
    f32x4 dk[4];                     // starts as -dt (dt = gradient w.r.t. the target V - K = dV)
    {
        f32x4 dgz[4], mGr[4], t2[4];
        {
            bf16x8 DWp[8];
            load_image(bk, DWp);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                f32x4 a = zero4();
                a = bk.mma32(kA0, DWp[fb], a);
                a = bk.mma32(kA1, DWp[4 + fb], a);
                dgz[fb] = (a + y.db[fb]) * (-eta4);
                mGr[fb] = dgz[fb] * (-ig.rstd);
                t2[fb] = mGr[fb] * ig.xh[fb];
            }
        }
        const f32x4 s1 = lin16::rowsum64(bk, mGr) * (1.0f / 64.0f), s2 = lin16::rowsum64(bk, t2) * (1.0f / 64.0f);
        const f32x4 c2 = ig.s2g * (1.0f / 64.0f);
        f32x4 dxh[4], dstd[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dgxh = lin16::fma4(dgz[fb], ig.rstd, s1) + ig.xh[fb] * s2;
            const f32x4 dy = dgxh * c.gam[fb];
            const f32x4 dg = lin16::fma4(ig.go[fb], dgxh, dy * ig.xh[fb]);
            y.dgam[fb] += dg[0] + dg[1] + dg[2] + dg[3];
            y.dbet[fb] += dy[0] + dy[1] + dy[2] + dy[3];
            dk[fb] = dy;                                                                       // = -dt
            dxh[fb] = lin16::fma4(ig.go[fb] * c.gam[fb], s2, dy * c.gam[fb]) + mGr[fb] * c2;
            dstd[fb] = lin16::fma4(dgz[fb], ig.gz[fb], dxh[fb] * ig.xh[fb]) * (-ig.rstd);
        }
        const f32x4 v1 = lin16::rowsum64(bk, dxh) * (1.0f / 64.0f), v2 = lin16::rowsum64(bk, dstd) * (1.0f / 64.0f);
        float cs[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dz1 = lin16::fma4(dxh[fb] - v1, ig.rstd, ig.xh[fb] * v2);
            dZ1p[fb] = pack4(dz1);
            cs[fb] = lin16::colsum16(bk, dz1);
        }
        publish_rows(bk, w, L_X2, L_PS2, dZ1p, cs);                                               // for (10)
        f32x4 dv[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) dv[fb] = -dk[fb];
        lin16::store_rows(bk, IMG + IMG_BYTES, dv, p.dXV + tile * 4096 + w * 1024);              // dV = dt
    }
    bk.lds_fence();
    // ---- (5, 7, 9) A1 = gZ1 dW1n^T ; d eta ; dK = -eta A1 - dt + dZ1 W^T --------------------------------------------------------------
    {
        bf16x4 gzq[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) gzq[fb] = pack4(ig.gz[fb]);
        bf16x8 aG[2];
        lin16::image_of(bk, IMG, gzq, aG);
        f32x4 acc[4];
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            f32x4 a1 = zero4();
            a1 = bk.mma32(aG[0], transposed_frag(bk, 0, 16 * fa), a1);
            a1 = bk.mma32(aG[1], transposed_frag(bk, 1, 16 * fa), a1);
            dk[fa] -= a1 * eta4;
            const f32x4 kc = bk.mma16(c.IDP, kT[fa], zero4());                                // exact K, accumulator layout
            acc[fa] = lin16::fma4(ig.gz[fa], lin16::splat4(y.db[fa]), kc * a1);
        }
        const f32x4 de = lin16::rowsum64(bk, acc);
        if (i == 0) *reinterpret_cast<bf16x4*>(p.deta + tile * 64 + 16 * w + 4 * g) = pack4(-de);
    }
    bk.lds_fence();
    {
        bf16x8 aD[2];
        lin16::image_of(bk, IMG, dZ1p, aD);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            dk[fa] = bk.mma32(aD[0], lin16::ld_pack(bk, slot, 8 + fa), dk[fa]);
            dk[fa] = bk.mma32(aD[1], lin16::ld_pack(bk, slot, 12 + fa), dk[fa]);
        }
        lin16::store_rows(bk, IMG + IMG_BYTES, dk, p.dXK + tile * 4096 + w * 1024);
    }
    bk.barrier();                                               // C: L_X2, L_PS2 written | read (until B of the next step)
    // ---- (10) dW1 = dW1n + K^T dZ1 ; db1 = db1n + colsum dZ1 --------------------------------------------------------------------------
    update_slice(bk, w, Kb, L_X2, L_PS2, y.dWt, y.db);
}
// dgamma / dbeta of (b, h): the per-lane partial sums over the lane groups, then over the waves through L_X (last read in (3) of
// the last step, two barriers back)
template <class BK>
TTT_WV_FN void store_ln_grads(BK& bk, int w, const Lin16Params& p, int bh, const BwdCarry& y) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const float dg = bk.xor_add(bk.xor_add(y.dgam[fb], 16), 32), dbt = bk.xor_add(bk.xor_add(y.dbet[fb], 16), 32);
        if (g == 0) {
            bk.template lds_store<float>(L_X + (w * 64 + 16 * fb + i) * 4, dg);
            bk.template lds_store<float>(L_X + 1024 + (w * 64 + 16 * fb + i) * 4, dbt);
        }
    }
    bk.barrier();
    if (w == 0 && g == 0)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const int o = L_X + (16 * fb + i) * 4;
            p.dln_w[(size_t)bh * 64 + 16 * fb + i] = (bk.template lds_load<float>(o) + bk.template lds_load<float>(o + 256)) +
                                                     (bk.template lds_load<float>(o + 512) + bk.template lds_load<float>(o + 768));
            p.dln_b[(size_t)bh * 64 + 16 * fb + i] = (bk.template lds_load<float>(o + 1024) + bk.template lds_load<float>(o + 1280)) +
                                                     (bk.template lds_load<float>(o + 1536) + bk.template lds_load<float>(o + 1792));
        }
}

// ===================================================================================================================
// backward of the scan of (b, h) = bh: checkpoint groups from the last to the first, each re-run forward (parking the state that
// enters every step) and then walked in reverse, as in lin16::backward.
template <class BK>
TTT_WV_FN void backward(BK& bk, const Lin16Params& p, int bh) {
    const int l0 = bk.lane(), w = bk.wave();
    const int NC = p.NC, G = p.G, K = p.K, head = bh % p.NH;
    const size_t tile0 = (size_t)bh * NC;
    const int IMG = L_IMG + w * 2 * IMG_BYTES, ETA = L_ETA + w * 128, own = w * TILE_B;
    char* scr_w = p.scratch_w + (size_t)bh * G * SLOT_BYTES;
    float* scr_b = p.scratch_b + (size_t)bh * G * 64;

    Consts c;
    make_consts(bk, p, head, c);
    f32x4 dWt[4];         // [fa]  dW1[16fa + 4g + r][16w + i]
    float db[4];          // db1[16fb + i], the same in every wave
    float dgam[4] = {0.f, 0.f, 0.f, 0.f}, dbet[4] = {0.f, 0.f, 0.f, 0.f};     // per-lane partial sums over this lane's token rows
    {
        const int g = l0 >> 4, i = l0 & 15;
        const float* dWl = p.dW1_last + (size_t)bh * 64 * 64;
#pragma unroll
        for (int fa = 0; fa < 4; ++fa)
#pragma unroll
            for (int r = 0; r < 4; ++r) dWt[fa][r] = dWl[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * w + i];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) db[fb] = p.db1_last[(size_t)bh * 64 + 16 * fb + i];
    }
    int cur = 0;          // the tile / eta buffer of the step at hand
    Stage sk, sv, sq, sd;
    unsigned short pe = 0;
    {   // first tiles of the last group's recompute pass
        const size_t t = tile0 + (size_t)(K - 1) * G;
        lin16::stage_request(bk, sk, p.XK + t * 4096 + w * 1024);
        lin16::stage_request(bk, sv, p.XV + t * 4096 + w * 1024);
        pe = *reinterpret_cast<const unsigned short*>(p.eta + t * 64 + 16 * w + (l0 & 15));
        park(bk, sk, L_K + own); park(bk, sv, L_V + own);
        park_eta(bk, pe, ETA);
        bk.lds_fence();
    }

    for (int k = K - 1; k >= 0; --k) {
        const int lo = k * G, hi = (lo + G < NC) ? lo + G : NC;
        float b1hi[4];                       // bias that ends the group
        // ================= re-run the group forward, parking the state entering each step ================================
        {
            f32x4 W1t[4];
            float b1v[4];
            {
                const int g = l0 >> 4, i = l0 & 15;
                const float* W1g = p.W1c + ((size_t)bh * K + k) * 64 * 64;
#pragma unroll
                for (int fa = 0; fa < 4; ++fa)
#pragma unroll
                    for (int r = 0; r < 4; ++r) W1t[fa][r] = W1g[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * w + i];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) b1v[fb] = p.b1c[((size_t)bh * K + k) * 64 + 16 * fb + i];
            }
            for (int it = lo; it <= hi; ++it) {      // iteration hi only parks the state that ends the group
                const int l = bk.opaque(l0), i = l & 15;
                const bool fin = (it == hi), last = (it + 1 == hi);
                bf16x8 mine[2];
                publish_slice(bk, w, W1t, mine);
                publish_transposed(bk, w, W1t);
                bk.barrier();                                           // R1: L_WI, L_TR written | read
                {
                    char* slot = fin ? bk.lds_ptr(L_WHI) : scr_w + (size_t)(it - lo) * SLOT_BYTES;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        lin16::st_pack(bk, slot, ks * 4 + w, mine[ks]);
                        lin16::st_pack(bk, slot, 8 + ks * 4 + w, transposed_frag(bk, ks, 16 * w));
                    }
                }
                if (fin) {
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) b1hi[fb] = b1v[fb];
                    bk.barrier();                                       // the slots of the group and L_WHI are complete
                    break;
                }
                if (w == 0)
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) scr_b[(size_t)(it - lo) * 64 + 16 * fb + i] = b1v[fb];      // every lane group: same value
                if (!last) {        // K, V, eta of the next step
                    const size_t t = tile0 + it + 1;
                    lin16::stage_request(bk, sk, p.XK + t * 4096 + w * 1024);
                    lin16::stage_request(bk, sv, p.XV + t * 4096 + w * 1024);
                    pe = *reinterpret_cast<const unsigned short*>(p.eta + t * 64 + 16 * w + (l & 15));
                } else {            // Q, dOut of this step: the reverse pass starts here
                    const size_t t = tile0 + it;
                    lin16::stage_request(bk, sq, p.XQ + t * 4096 + w * 1024);
                    lin16::stage_request(bk, sd, p.dOut + t * 4096 + w * 1024);
                }
                {
                    bf16x8 Wp[8];
                    load_image(bk, Wp);
                    inner_publish(bk, w, L_K + cur * T64_B + own, L_V + cur * T64_B + own, ETA + cur * 64, Wp, b1v, c, p.eps);
                }
                bk.barrier();                                           // R2: L_X, L_PS written | read (until R1 of the next step)
                update_slice(bk, w, L_K + cur * T64_B, L_X, L_PS, W1t, b1v);
                // (the other buffer's K tiles were last read by other waves before R1 of this step)
                if (!last) {
                    const int nb = cur ^ 1;
                    park(bk, sk, L_K + nb * T64_B + own); park(bk, sv, L_V + nb * T64_B + own);
                    park_eta(bk, pe, ETA + nb * 64);
                    cur = nb;
                } else {
                    park(bk, sq, L_Q + cur * T64_B + own); park(bk, sd, L_D + cur * T64_B + own);
                }
                bk.lds_fence();
            }
        }

        // ================= reverse pass over the group ======================================================================
        for (int it = hi - 1; it >= lo; --it) {
            const size_t tile = tile0 + it;
            const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
            const int Kt = L_K + cur * T64_B + own, Vt = L_V + cur * T64_B + own, Qt = L_Q + cur * T64_B + own, Dt = L_D + cur * T64_B + own;
            const int nxt = (it > lo) ? it - 1 : lo - G;          // step whose tiles are requested now (< 0: nothing left)
            if (nxt >= 0) {
                const size_t t = tile0 + nxt;
                lin16::stage_request(bk, sk, p.XK + t * 4096 + w * 1024);
                lin16::stage_request(bk, sv, p.XV + t * 4096 + w * 1024);
                pe = *reinterpret_cast<const unsigned short*>(p.eta + t * 64 + 16 * w + (l & 15));
                if (it > lo) {
                    lin16::stage_request(bk, sq, p.XQ + t * 4096 + w * 1024);
                    lin16::stage_request(bk, sd, p.dOut + t * 4096 + w * 1024);
                }
            }
            const char* slot = scr_w + (size_t)(it - lo) * SLOT_BYTES;                                   // state entering / after the step
            const char* slot_n = (it + 1 < hi) ? slot + SLOT_BYTES : bk.lds_ptr(L_WHI);
            const f32x4 eta4 = bk.template lds<f32x4>(ETA + cur * 64 + 4 * g * 4);
            float b1v[4], b1n[4];
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                b1v[fb] = scr_b[(size_t)(it - lo) * 64 + 16 * fb + i];
                b1n[fb] = (it + 1 < hi) ? scr_b[(size_t)(it + 1 - lo) * 64 + 16 * fb + i] : b1hi[fb];
            }

            // ---- (2) outer LayerNorm backward for this wave's tokens: Z1b = Q W1n + b1n ; dZ1b -> L_X, its column sums -> L_PS ------
            f32x4 dq[4];                     // starts as dOut (accumulator layout), becomes dQ
            {
                bf16x4 dZbp[4];
                float cs[4];
                const bf16x8 qA0 = lin16::rho_read(bk, Qt, 0), qA1 = lin16::rho_read(bk, Qt, 32);
                f32x4 y[4], dxl[4], t2[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    f32x4 a = zero4();
                    a = bk.mma32(qA0, lin16::ld_pack(bk, slot_n, fb), a);
                    a = bk.mma32(qA1, lin16::ld_pack(bk, slot_n, 4 + fb), a);
                    y[fb] = a + b1n[fb];
                    dq[fb] = bk.mma16(c.IDP, lin16::tr4(bk, Dt, TS, 0, 16 * fb), zero4());                // exact dOut
                }
                const f32x4 rstdl = lin16::normalize_rows(bk, y, p.eps);                                  // y <- x_hat of the output LN
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 dx = dq[fb] * y[fb];
                    dgam[fb] += dx[0] + dx[1] + dx[2] + dx[3];
                    dbet[fb] += dq[fb][0] + dq[fb][1] + dq[fb][2] + dq[fb][3];
                    dxl[fb] = dq[fb] * c.gam[fb];
                    t2[fb] = dxl[fb] * y[fb];
                }
                const f32x4 u1 = lin16::rowsum64(bk, dxl), u2 = lin16::rowsum64(bk, t2);
                const f32x4 sc = rstdl * (1.0f / 64.0f);
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 dzb = (64.0f * dxl[fb] - u1 - y[fb] * u2) * sc;
                    dZbp[fb] = pack4(dzb);
                    cs[fb] = lin16::colsum16(bk, dzb);                                                    // fp32 sums, as at mini-batch 16
                }
                publish_rows(bk, w, L_X, L_PS, dZbp, cs);
                // ---- (4) dQ = dOut + dZ1b W1n^T --------------------------------------------------------------------------------------
                bf16x8 aZ[2];
                lin16::image_of(bk, IMG, dZbp, aZ);
#pragma unroll
                for (int fa = 0; fa < 4; ++fa) {
                    dq[fa] = bk.mma32(aZ[0], lin16::ld_pack(bk, slot_n, 8 + fa), dq[fa]);
                    dq[fa] = bk.mma32(aZ[1], lin16::ld_pack(bk, slot_n, 12 + fa), dq[fa]);
                }
                lin16::store_rows(bk, IMG + IMG_BYTES, dq, p.dXQ + tile * 4096 + w * 1024);
            }
            bk.lds_fence();
            // ---- (1) inner forward of the step for this wave's tokens: Z1 = K W + b, LN / L2 gradient ------------------------------
            const bf16x8 kA0 = lin16::rho_read(bk, Kt, 0), kA1 = lin16::rho_read(bk, Kt, 32);
            bf16x4 kT[4];
            InnerGrad ig;
            {
                f32x4 z[4], tg[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    kT[fb] = lin16::tr4(bk, Kt, TS, 0, 16 * fb);
                    f32x4 a = zero4();
                    a = bk.mma32(kA0, lin16::ld_pack(bk, slot, fb), a);
                    a = bk.mma32(kA1, lin16::ld_pack(bk, slot, 4 + fb), a);
                    z[fb] = a + b1v[fb];
                    tg[fb] = bk.mma16(c.IDN, kT[fb], bk.mma16(c.IDP, lin16::tr4(bk, Vt, TS, 0, 16 * fb), zero4()));   // exact V - K
                }
                lin16::inner_grad(bk, z, tg, c.gam, c.bet, p.eps, ig);
            }
            bk.barrier();                                               // A: L_X, L_PS written | read ; every wave has left the step before
            // ---- (3) dW1n += Q^T dZ1b ; db1n += colsum dZ1b ; the images of dW1n -----------------------------------------------------
            update_slice(bk, w, L_Q + cur * T64_B, L_X, L_PS, dWt, db);
            {
                bf16x8 mine[2];
                publish_slice(bk, w, dWt, mine);
                publish_transposed(bk, w, dWt);
            }
            if (nxt >= 0) {      // the other buffer was last read (K in (10), Q in (3)) by the step before this one
                const int nb = cur ^ 1;
                park(bk, sk, L_K + nb * T64_B + own); park(bk, sv, L_V + nb * T64_B + own);
                park_eta(bk, pe, ETA + nb * 64);
                if (it > lo) { park(bk, sq, L_Q + nb * T64_B + own); park(bk, sd, L_D + nb * T64_B + own); }
            }
            bk.barrier();                                               // B: L_WI, L_TR written | read (until A of the next step)
            // ---- (6) dgZ1 = -eta (K dW1n + db1n) ; (8) backward of the fused LN / L2 gradient -> dZ1, dt, dgamma, dbeta -----------------
            bf16x4 dZ1p[4];
            f32x4 dk[4];                     // starts as -dt (dt = gradient w.r.t. the target V - K = dV)
            {
                f32x4 dgz[4], mGr[4], t2[4];
                {
                    bf16x8 DWp[8];
                    load_image(bk, DWp);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) {
                        f32x4 a = zero4();
                        a = bk.mma32(kA0, DWp[fb], a);
                        a = bk.mma32(kA1, DWp[4 + fb], a);
                        dgz[fb] = (a + db[fb]) * (-eta4);
                        mGr[fb] = dgz[fb] * (-ig.rstd);
                        t2[fb] = mGr[fb] * ig.xh[fb];
                    }
                }
                const f32x4 s1 = lin16::rowsum64(bk, mGr) * (1.0f / 64.0f), s2 = lin16::rowsum64(bk, t2) * (1.0f / 64.0f);
                const f32x4 c2 = ig.s2g * (1.0f / 64.0f);
                f32x4 dxh[4], dstd[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 dgxh = dgz[fb] * ig.rstd + s1 + ig.xh[fb] * s2;
                    const f32x4 dy = dgxh * c.gam[fb];
                    const f32x4 dg = ig.go[fb] * dgxh + dy * ig.xh[fb];
                    dgam[fb] += dg[0] + dg[1] + dg[2] + dg[3];
                    dbet[fb] += dy[0] + dy[1] + dy[2] + dy[3];
                    dk[fb] = dy;                                                                       // = -dt
                    dxh[fb] = dy * c.gam[fb] + (ig.go[fb] * c.gam[fb]) * s2 + mGr[fb] * c2;
                    dstd[fb] = (dxh[fb] * ig.xh[fb] + dgz[fb] * ig.gz[fb]) * (-ig.rstd);
                }
                const f32x4 v1 = lin16::rowsum64(bk, dxh) * (1.0f / 64.0f), v2 = lin16::rowsum64(bk, dstd) * (1.0f / 64.0f);
                float cs[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 dz1 = (dxh[fb] - v1) * ig.rstd + ig.xh[fb] * v2;
                    dZ1p[fb] = pack4(dz1);
                    cs[fb] = lin16::colsum16(bk, dz1);
                }
                publish_rows(bk, w, L_X2, L_PS2, dZ1p, cs);                                               // for (10)
                f32x4 dv[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) dv[fb] = -dk[fb];
                lin16::store_rows(bk, IMG + IMG_BYTES, dv, p.dXV + tile * 4096 + w * 1024);              // dV = dt
            }
            bk.lds_fence();
            // ---- (5, 7, 9) A1 = gZ1 dW1n^T ; d eta ; dK = -eta A1 - dt + dZ1 W^T --------------------------------------------------------------
            {
                bf16x4 gzq[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) gzq[fb] = pack4(ig.gz[fb]);
                bf16x8 aG[2];
                lin16::image_of(bk, IMG, gzq, aG);
                f32x4 acc[4];
#pragma unroll
                for (int fa = 0; fa < 4; ++fa) {
                    f32x4 a1 = zero4();
                    a1 = bk.mma32(aG[0], transposed_frag(bk, 0, 16 * fa), a1);
                    a1 = bk.mma32(aG[1], transposed_frag(bk, 1, 16 * fa), a1);
                    dk[fa] -= a1 * eta4;
                    const f32x4 kc = bk.mma16(c.IDP, kT[fa], zero4());                                // exact K, accumulator layout
                    acc[fa] = kc * a1 + ig.gz[fa] * db[fa];
                }
                const f32x4 de = lin16::rowsum64(bk, acc);
                if (i == 0) *reinterpret_cast<bf16x4*>(p.deta + tile * 64 + 16 * w + 4 * g) = pack4(-de);
            }
            bk.lds_fence();
            {
                bf16x8 aD[2];
                lin16::image_of(bk, IMG, dZ1p, aD);
#pragma unroll
                for (int fa = 0; fa < 4; ++fa) {
                    dk[fa] = bk.mma32(aD[0], lin16::ld_pack(bk, slot, 8 + fa), dk[fa]);
                    dk[fa] = bk.mma32(aD[1], lin16::ld_pack(bk, slot, 12 + fa), dk[fa]);
                }
                lin16::store_rows(bk, IMG + IMG_BYTES, dk, p.dXK + tile * 4096 + w * 1024);
            }
            bk.barrier();                                               // C: L_X2, L_PS2 written | read (until B of the next step)
            // ---- (10) dW1 = dW1n + K^T dZ1 ; db1 = db1n + colsum dZ1 --------------------------------------------------------------------------
            update_slice(bk, w, L_K + cur * T64_B, L_X2, L_PS2, dWt, db);
            if (nxt >= 0) cur ^= 1;
            bk.lds_fence();
        }
    }
    // ---- results: wave w its slice of dW1 ; dgamma / dbeta summed over the lane groups, then over the waves through L_X -----------
    {
        const int g = l0 >> 4, i = l0 & 15;
        float* dWg = p.dW1 + (size_t)bh * 64 * 64;
#pragma unroll
        for (int fa = 0; fa < 4; ++fa)
#pragma unroll
            for (int r = 0; r < 4; ++r) dWg[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * w + i] = dWt[fa][r];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const float dg = bk.xor_add(bk.xor_add(dgam[fb], 16), 32), dbt = bk.xor_add(bk.xor_add(dbet[fb], 16), 32);
            if (g == 0) {
                bk.template lds_store<float>(L_X + (w * 64 + 16 * fb + i) * 4, dg);
                bk.template lds_store<float>(L_X + 1024 + (w * 64 + 16 * fb + i) * 4, dbt);
            }
        }
        bk.barrier();
        if (w == 0 && g == 0)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const int o = L_X + (16 * fb + i) * 4;
                p.db1[(size_t)bh * 64 + 16 * fb + i] = db[fb];
                p.dln_w[(size_t)bh * 64 + 16 * fb + i] = (bk.template lds_load<float>(o) + bk.template lds_load<float>(o + 256)) +
                                                         (bk.template lds_load<float>(o + 512) + bk.template lds_load<float>(o + 768));
                p.dln_b[(size_t)bh * 64 + 16 * fb + i] = (bk.template lds_load<float>(o + 1024) + bk.template lds_load<float>(o + 1280)) +
                                                         (bk.template lds_load<float>(o + 1536) + bk.template lds_load<float>(o + 1792));
            }
    }
}

// ===================================================================================================================
// The backward in parts (Lin16BwdPartParams, ttt_wave_types.h ; see lin16::recompute_groups / sweep_groups): the same two entries
// with a workgroup of four waves in place of the wave, running the steps of backward() above as functions.  The state that ends a group is a
// slot of the workspace like every other (no L_WHI), written and read in different kernels; within recompute_groups no wave reads a
// slot, within sweep_groups no wave writes one.
//
// workgroup `bhk` = bh * nk + j recomputes group k0 + j of (b, h) = bh
template <class BK>
TTT_WV_FN void recompute_groups(BK& bk, const Lin16BwdPartParams& q, int bhk) {
    const Lin16Params& p = q.p;
    const int l0 = bk.lane(), w = bk.wave();
    const int NC = p.NC, G = p.G, K = p.K;
    const int bh = bhk / q.nk, k = q.k0 + bhk % q.nk, head = bh % p.NH;
    const int lo = k * G, hi = (lo + G < NC) ? lo + G : NC;
    const size_t tile0 = (size_t)bh * NC;
    const int ETA = L_ETA + w * 128, own = w * TILE_B;
    char* slots = q.slots + (size_t)bhk * (G + 1) * LIN_PART_SLOT_BYTES;

    Consts c;
    make_consts(bk, p, head, c);
    f32x4 W1t[4];
    float b1v[4];
    load_slice(bk, w, p.W1c + ((size_t)bh * K + k) * 64 * 64, W1t);
    lin16::load_row(bk, p.b1c + ((size_t)bh * K + k) * 64, b1v);
    int cur = 0;
    Stage sk, sv;
    unsigned short pe;
    lin16::stage_request(bk, sk, p.XK + (tile0 + lo) * 4096 + w * 1024);
    lin16::stage_request(bk, sv, p.XV + (tile0 + lo) * 4096 + w * 1024);
    pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + lo) * 64 + 16 * w + (l0 & 15));
    park(bk, sk, L_K + own); park(bk, sv, L_V + own);       // (other waves read these K rows behind R1 and R2 of the first step)
    park_eta(bk, pe, ETA);
    bk.lds_fence();
    for (int it = lo; it <= hi; ++it) {          // iteration hi only parks the state that ends the group
        const int l = bk.opaque(l0), i = l & 15;
        char* slot = slots + (size_t)(it - lo) * LIN_PART_SLOT_BYTES;
        park_state(bk, w, W1t, slot);
        if (w == 0 && (l >> 4) == 0)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) reinterpret_cast<float*>(slot + SLOT_BYTES)[16 * fb + i] = b1v[fb];
        if (it == hi) break;
        const bool last = (it + 1 == hi);
        if (!last) {        // K, V, eta of the next step
            const size_t t = tile0 + it + 1;
            lin16::stage_request(bk, sk, p.XK + t * 4096 + w * 1024);
            lin16::stage_request(bk, sv, p.XV + t * 4096 + w * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + t * 64 + 16 * w + (l & 15));
        }
        recompute_step(bk, w, c, p.eps, L_K + cur * T64_B, L_V + cur * T64_B, ETA + cur * 64, W1t, b1v);
        if (!last) {        // (the other buffer's K tiles were last read by other waves before R1 of this step)
            const int nb = cur ^ 1;
            park(bk, sk, L_K + nb * T64_B + own); park(bk, sv, L_V + nb * T64_B + own);
            park_eta(bk, pe, ETA + nb * 64);
            cur = nb;
        }
        bk.lds_fence();
    }
}

// the reverse walk of (b, h) = bh over the groups k0 + nk - 1 .. k0 from the slots recompute_groups left ; carries as in
// lin16::sweep_groups (the partial sums of dgamma / dbeta per lane of each of the four waves)
template <class BK>
TTT_WV_FN void sweep_groups(BK& bk, const Lin16BwdPartParams& q, int bh) {
    const Lin16Params& p = q.p;
    const int l0 = bk.lane(), w = bk.wave();
    const int NC = p.NC, G = p.G, K = p.K, head = bh % p.NH;
    const int k0 = q.k0, nk = q.nk;
    const int s_lo = k0 * G, s_hi = ((k0 + nk) * G < NC) ? (k0 + nk) * G : NC;      // the steps [s_lo, s_hi)
    const size_t tile0 = (size_t)bh * NC;
    const int ETA = L_ETA + w * 128, own = w * TILE_B;
    const char* slots = q.slots + (size_t)bh * nk * (G + 1) * LIN_PART_SLOT_BYTES;
    float* carry = q.ln_carry + (size_t)bh * LIN_PART_CARRY_FLOATS * 64 * WAVES + w * 64 + l0;

    Consts c;
    make_consts(bk, p, head, c);
    BwdCarry y;
    load_slice(bk, w, p.dW1_last + (size_t)bh * 64 * 64, y.dWt);
    lin16::load_row(bk, p.db1_last + (size_t)bh * 64, y.db);
    if (k0 + nk == K) {      // the range that ends the sequence starts the sums
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) y.dgam[fb] = y.dbet[fb] = 0.f;
    } else {
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) { y.dgam[fb] = carry[fb * 64 * WAVES]; y.dbet[fb] = carry[(4 + fb) * 64 * WAVES]; }
    }
    int cur = 0;
    Stage sk, sv, sq, sd;
    unsigned short pe = 0;
    {   // tiles of the first step of the walk: the combined kernel gets these from its recompute loop.  Every wave its own rows; the
        // rows of other waves are read behind barrier A of the first step at the earliest (Q in (3), K in (10)).
        const size_t t = tile0 + s_hi - 1;
        lin16::stage_request(bk, sk, p.XK + t * 4096 + w * 1024);
        lin16::stage_request(bk, sv, p.XV + t * 4096 + w * 1024);
        lin16::stage_request(bk, sq, p.XQ + t * 4096 + w * 1024);
        lin16::stage_request(bk, sd, p.dOut + t * 4096 + w * 1024);
        pe = *reinterpret_cast<const unsigned short*>(p.eta + t * 64 + 16 * w + (l0 & 15));
        park(bk, sk, L_K + own); park(bk, sv, L_V + own); park(bk, sq, L_Q + own); park(bk, sd, L_D + own);
        park_eta(bk, pe, ETA);
        bk.lds_fence();
    }
    int k = k0 + nk - 1, lo = k * G;          // the group of step `it`
    for (int it = s_hi - 1; it >= s_lo; --it) {
        if (it < lo) { --k; lo -= G; }
        const int l = bk.opaque(l0), i = l & 15;
        const bool more = it > s_lo;
        if (more) {
            const size_t t = tile0 + it - 1;
            lin16::stage_request(bk, sk, p.XK + t * 4096 + w * 1024);
            lin16::stage_request(bk, sv, p.XV + t * 4096 + w * 1024);
            lin16::stage_request(bk, sq, p.XQ + t * 4096 + w * 1024);
            lin16::stage_request(bk, sd, p.dOut + t * 4096 + w * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + t * 64 + 16 * w + (l & 15));
        }
        const char* slot = slots + ((size_t)(k - k0) * (G + 1) + (it - lo)) * LIN_PART_SLOT_BYTES;       // state entering the step
        const char* slot_n = slot + LIN_PART_SLOT_BYTES;                                                 // ... and after it
        float b1v[4], b1n[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            b1v[fb] = reinterpret_cast<const float*>(slot + SLOT_BYTES)[16 * fb + i];
            b1n[fb] = reinterpret_cast<const float*>(slot_n + SLOT_BYTES)[16 * fb + i];
        }
        reverse_step(bk, l, w, p, c, y, tile0 + it, L_K + cur * T64_B, L_V + cur * T64_B, L_Q + cur * T64_B, L_D + cur * T64_B,
                     ETA + cur * 64, slot, slot_n, b1v, b1n, [&] {
                         if (more) {
                             const int nb = cur ^ 1;
                             park(bk, sk, L_K + nb * T64_B + own); park(bk, sv, L_V + nb * T64_B + own);
                             park(bk, sq, L_Q + nb * T64_B + own); park(bk, sd, L_D + nb * T64_B + own);
                             park_eta(bk, pe, ETA + nb * 64);
                         }
                     });
        if (more) cur ^= 1;
        bk.lds_fence();
    }
    // ---- hand-over.  q.p.dW1 / db1 MAY ALIAS dW1_last / db1_last (the caller carries the gradient state in place).  Global memory, so
    // the emulator's race detector does not see this one; it rests on the barriers: every wave reads db1_last and its own slice of
    // dW1_last in front of the step loop, and these stores come behind barriers A, B and C of the last step (a range has at least one
    // step) - no wave can still be reading, and a wave overwrites only the slice that it alone read.  ln_carry is read (above) and
    // written by the same lane only.
    store_slice(bk, w, p.dW1 + (size_t)bh * 64 * 64, y.dWt);
    if (w == 0 && (l0 >> 4) == 0)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) p.db1[(size_t)bh * 64 + 16 * fb + (l0 & 15)] = y.db[fb];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) { carry[fb * 64 * WAVES] = y.dgam[fb]; carry[(4 + fb) * 64 * WAVES] = y.dbet[fb]; }
    if (k0 == 0) store_ln_grads(bk, w, p, bh, y);
}

// ===================================================================================================================
// A third stage of the backward in parts (Lin16BwdFrontParams, ttt_wave_types.h ; see lin16::front_groups / chain_groups).  The blocks
// (2), (4) and (1) of reverse_step stand in front of barrier A: every wave runs them on its own 16 token rows from the step's tiles
// and the two slots, with no exchange between waves.  They are the statements of lin16::front_step on token block 4 * tile + w, so
// front_groups runs them as ONE WAVE per (b, h, step of the range, token block), on the LDS map of ttt_lin16_body.h - no workgroup,
// no barrier.  It stores the block's rows of dXQ and leaves the block's record in the field layout of lin16 (REC_*); a step's record
// is [w][field][lane] (LIN64_FRONT_RECORD_BYTES).  chain_groups is the walk that remains, a workgroup of four waves.
//
// inner_grad for front_step, as lin16::inner_grad_pinned - but the walk kernels of THIS body (linear_bwd_cs64_kernel,
// linear_sweep_cs64_groups_kernel) start the sum of the four products gxh[fb] = go[fb] gamma[fb] of a row the other way round:
// fma(go0, gamma0, gxh1), where the mini-batch-16 walk has fma(go1, gamma1, gxh0) ; read from their assembly.  The other sums are
// taken as at mini-batch 16.  (On the host a sum of rounded products either way: same bits.)
template <class BK>
TTT_WV_FN void inner_grad_pinned(BK& bk, const f32x4 (&z)[4], const f32x4 (&tg)[4], const float (&gam)[4], const float (&bet)[4], float eps,
                                 InnerGrad& o) {
    using lin16::fma4;
    using lin16::splat4;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) o.xh[fb] = z[fb];
    o.rstd = lin16::normalize_rows(bk, o.xh, eps);
    f32x4 gxh[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        o.go[fb] = fma4(splat4(gam[fb]), o.xh[fb], splat4(bet[fb])) - tg[fb];
        gxh[fb] = o.go[fb] * gam[fb];
    }
    f32x4 s1 = fma4(o.go[0], splat4(gam[0]), gxh[1]);                     // gxh[0] + gxh[1] + gxh[2] + gxh[3]
    s1 = fma4(o.go[2], splat4(gam[2]), s1);
    s1 = fma4(o.go[3], splat4(gam[3]), s1);
    f32x4 s2 = fma4(o.xh[0], gxh[0], gxh[1] * o.xh[1]);                   // the same sum of gxh[fb] xh[fb]
    s2 = fma4(o.xh[2], gxh[2], s2);
    s2 = fma4(o.xh[3], gxh[3], s2);
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[r] = bk.sum16(s1[r]); s2[r] = bk.sum16(s2[r]); }
    o.s2g = s2;
    const f32x4 sc = o.rstd * (1.0f / 64.0f);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) o.gz[fb] = fma4(-o.xh[fb], o.s2g, fma4(splat4(64.0f), gxh[fb], -s1)) * sc;
}

// blocks (2), (4), (1) of reverse_step for ONE 16-row token block, on the single-wave LDS map of ttt_lin16_body.h: the statements of
// lin16::front_step with the inner_grad above.  Tiles of the block at Kt, Vt, Qt, Dt ; slot / b1v: the state entering the step,
// slot_n / b1n: the state after it ; dXQ of the block goes to 16-row tile `blk`, everything the chain needs to `rec`.
template <class BK>
TTT_WV_FN void front_step(BK& bk, const Lin16Params& p, const lin16::BwdConsts& c, size_t blk, int Kt, int Vt, int Qt, int Dt,
                          const char* slot, const char* slot_n, const float (&b1v)[4], const float (&b1n)[4], char* rec) {
    using namespace lin16;      // (the REC_* fields, st_rec, vec4 and the wave helpers; L_IMG is spelled out: the single-wave map)
    // ---- (2) outer LayerNorm backward: Z1b = Q W1n + b1n ; dZ1b -----------------------------------------------------------
    bf16x4 dZbp[4];
    f32x4 dq[4];                     // starts as dOut (accumulator layout), becomes dQ
    {
        const bf16x8 qA0 = rho_read(bk, Qt, 0), qA1 = rho_read(bk, Qt, 32);
        f32x4 yy[4], dxl[4], t2[4];
        float addg[4], addb[4], csum[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            f32x4 a = lin16::zero4();
            a = bk.mma32(qA0, ld_pack(bk, slot_n, fb), a);
            a = bk.mma32(qA1, ld_pack(bk, slot_n, 4 + fb), a);
            yy[fb] = a + b1n[fb];
            dq[fb] = bk.mma16(c.IDP, tr4(bk, Dt, lin16::TS, 0, 16 * fb), lin16::zero4());         // exact dOut
        }
        const f32x4 rstdl = normalize_rows(bk, yy, c.eps);                                    // yy <- x_hat of the output LN
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dx = dq[fb] * yy[fb];
            addg[fb] = dx[0] + dx[1] + dx[2] + dx[3];
            addb[fb] = dq[fb][0] + dq[fb][1] + dq[fb][2] + dq[fb][3];
            dxl[fb] = dq[fb] * c.gam[fb];
            t2[fb] = dxl[fb] * yy[fb];
        }
        const f32x4 u1 = rowsum64(bk, dxl), u2 = rowsum64(bk, t2);
        const f32x4 sc = rstdl * (1.0f / 64.0f);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dzb = (64.0f * dxl[fb] - u1 - yy[fb] * u2) * sc;
            dZbp[fb] = lin16::pack4(dzb);
            csum[fb] = colsum16(bk, dzb);
        }
        st_rec(bk, rec, REC_DZB, lin16::cat(dZbp[0], dZbp[1]));
        st_rec(bk, rec, REC_DZB + 1, lin16::cat(dZbp[2], dZbp[3]));
        st_rec(bk, rec, REC_CSUM, vec4(csum));
        st_rec(bk, rec, REC_DGAM, vec4(addg));
        st_rec(bk, rec, REC_DBET, vec4(addb));
    }
    // ---- (4) dQ = dOut + dZ1b W1n^T ------------------------------------------------------------------------------------------------
    {
        bf16x8 aZ[2];
        image_of(bk, lin16::L_IMG, dZbp, aZ);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            dq[fa] = bk.mma32(aZ[0], ld_pack(bk, slot_n, 8 + fa), dq[fa]);
            dq[fa] = bk.mma32(aZ[1], ld_pack(bk, slot_n, 12 + fa), dq[fa]);
        }
        store_rows(bk, lin16::L_IMG + lin16::IMG_BYTES, dq, p.dXQ + blk * 1024);
    }
    bk.lds_fence();
    // ---- (1) inner forward of the step: Z1 = K W + b, LN / L2 gradient ------------------------------------------------
    const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
    lin16::InnerGrad ig;
    {
        f32x4 z[4], tg[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const bf16x4 kT = tr4(bk, Kt, lin16::TS, 0, 16 * fb);
            f32x4 a = lin16::zero4();
            a = bk.mma32(kA0, ld_pack(bk, slot, fb), a);
            a = bk.mma32(kA1, ld_pack(bk, slot, 4 + fb), a);
            z[fb] = a + b1v[fb];
            tg[fb] = bk.mma16(c.IDN, kT, bk.mma16(c.IDP, tr4(bk, Vt, lin16::TS, 0, 16 * fb), lin16::zero4()));   // exact V - K
        }
        lin64::inner_grad_pinned(bk, z, tg, c.gam, c.bet, c.eps, ig);
    }
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        st_rec(bk, rec, REC_XH + fb, ig.xh[fb]);
        st_rec(bk, rec, REC_GO + fb, ig.go[fb]);
        st_rec(bk, rec, REC_GZ + fb, ig.gz[fb]);
    }
    st_rec(bk, rec, REC_RSTD, ig.rstd);
    st_rec(bk, rec, REC_S2G, ig.s2g);
}

// wave `unit` = (bh * (steps of the range) + j) * 4 + w runs the front of token block w of step k0 * G + j of (b, h) = bh
template <class BK>
TTT_WV_FN void front_groups(BK& bk, const Lin16BwdFrontParams& f, int unit) {
    const Lin16BwdPartParams& q = f.q;
    const Lin16Params& p = q.p;
    const int NC = p.NC, G = p.G;
    const int s_lo = q.k0 * G, s_hi = ((q.k0 + q.nk) * G < NC) ? (q.k0 + q.nk) * G : NC, ns = s_hi - s_lo;
    const int w = unit % WAVES, su = unit / WAVES;
    const int bh = su / ns, it = s_lo + su % ns, k = it / G, lo = k * G, head = bh % p.NH;
    const int i = bk.lane() & 15;
    const size_t blk = ((size_t)bh * NC + it) * WAVES + w;                                          // the [16][64] tile of the block
    const size_t cell = (size_t)bh * q.nk + (k - q.k0);                                             // (b, h, group of the range)
    const char* slot = q.slots + (cell * (G + 1) + (it - lo)) * LIN_PART_SLOT_BYTES;                // state entering the step
    const char* slot_n = slot + LIN_PART_SLOT_BYTES;                                                // ... and after it
    char* rec = f.records + (cell * G + (it - lo)) * LIN64_FRONT_RECORD_BYTES + (size_t)w * LIN_FRONT_RECORD_BYTES;

    lin16::BwdConsts c;
    lin16::bwd_consts(bk, p, head, c);
    Stage sk, sv, sq, sd;
    lin16::stage_request(bk, sk, p.XK + blk * 1024);
    lin16::stage_request(bk, sv, p.XV + blk * 1024);
    lin16::stage_request(bk, sq, p.XQ + blk * 1024);
    lin16::stage_request(bk, sd, p.dOut + blk * 1024);
    float b1v[4], b1n[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        b1v[fb] = reinterpret_cast<const float*>(slot + SLOT_BYTES)[16 * fb + i];
        b1n[fb] = reinterpret_cast<const float*>(slot_n + SLOT_BYTES)[16 * fb + i];
    }
    lin16::stage_park(bk, sk, lin16::L_K); lin16::stage_park(bk, sv, lin16::L_V);
    lin16::stage_park(bk, sq, lin16::L_Q); lin16::stage_park(bk, sd, lin16::L_D);
    bk.lds_fence();
    lin64::front_step(bk, p, c, blk, lin16::L_K, lin16::L_V, lin16::L_Q, lin16::L_D, slot, slot_n, b1v, b1n, rec);
}

// The chain keeps the LDS map of the sweep (the V and dOut tiles and L_WHI unused).  A step's record does not fit the LDS that is
// left twice, and a wave has its SIMD - 512 registers - to itself: wave w holds its block's record of the step at hand in registers
// (what reverse_step holds as `ig`, plus dZ1b and the addends until they are published in front of barrier A) and fetches the record
// of the step in front into a second set while the step runs.
constexpr int GROUP_LDS_CHAIN = L_WHI;
static_assert(GROUP_LDS_CHAIN <= 160 * 1024, "LDS budget");
struct StepRecord {
    u32x4 f[lin16::REC_FIELDS];
};
template <class BK>
TTT_WV_FN void rec_request(BK& bk, int l, const char* rec, StepRecord& r) {
#pragma unroll
    for (int j = 0; j < lin16::REC_FIELDS; ++j) r.f[j] = *reinterpret_cast<const u32x4*>(rec + ((size_t)j * 64 + l) * 16);
}
TTT_WV_FN f32x4 rec_f32(const StepRecord& r, int j) { return __builtin_bit_cast(f32x4, r.f[j]); }

// reverse_step without its blocks (2), (4), (1): their results come from the block's record `r`.  Kb, Qb: the K / Q tiles of the
// mini-batch, eta_off: this wave's eta ; slot: the state entering the step (its transposed packs 8..15 only).  `mid()` runs between
// barriers A and B, as in reverse_step.  Ends with the carried update (10); the caller fences LDS behind it.
template <class BK, class Mid>
TTT_WV_FN void chain_step(BK& bk, int l, int w, const Lin16Params& p, const Consts& c, BwdCarry& y, size_t tile, int Kb, int Qb, int eta_off,
                          const char* slot, const StepRecord& r, Mid&& mid) {
    const int g = l >> 4, i = l & 15;
    const int IMG = L_IMG + w * 2 * IMG_BYTES, own = w * TILE_B;
    const int Kt = Kb + own;
    const f32x4 eta4 = bk.template lds<f32x4>(eta_off + 4 * g * 4);
    // ---- what (2) left: the addends of the carry ; dZ1b -> L_X, its column sums -> L_PS ------------------------------------------
    {
        const f32x4 addg = rec_f32(r, lin16::REC_DGAM), addb = rec_f32(r, lin16::REC_DBET), csum = rec_f32(r, lin16::REC_CSUM);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            y.dgam[fb] += addg[fb];
            y.dbet[fb] += addb[fb];
        }
        const bf16x8 d01 = __builtin_bit_cast(bf16x8, r.f[lin16::REC_DZB]), d23 = __builtin_bit_cast(bf16x8, r.f[lin16::REC_DZB + 1]);
        const bf16x4 dZbp[4] = {__builtin_shufflevector(d01, d01, 0, 1, 2, 3), __builtin_shufflevector(d01, d01, 4, 5, 6, 7),
                                __builtin_shufflevector(d23, d23, 0, 1, 2, 3), __builtin_shufflevector(d23, d23, 4, 5, 6, 7)};
        const float cs[4] = {csum[0], csum[1], csum[2], csum[3]};
        publish_rows(bk, w, L_X, L_PS, dZbp, cs);
    }
    // ---- what (1) left ------------------------------------------------------------------------------------------------------------
    InnerGrad ig;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        ig.xh[fb] = rec_f32(r, lin16::REC_XH + fb);
        ig.go[fb] = rec_f32(r, lin16::REC_GO + fb);
        ig.gz[fb] = rec_f32(r, lin16::REC_GZ + fb);
    }
    ig.rstd = rec_f32(r, lin16::REC_RSTD);
    ig.s2g = rec_f32(r, lin16::REC_S2G);
    const bf16x8 kA0 = lin16::rho_read(bk, Kt, 0), kA1 = lin16::rho_read(bk, Kt, 32);
    bf16x4 kT[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) kT[fb] = lin16::tr4(bk, Kt, TS, 0, 16 * fb);
    bk.barrier();                                               // A: L_X, L_PS written | read ; every wave has left the step before
    // ---- (3) dW1n += Q^T dZ1b ; db1n += colsum dZ1b ; the images of dW1n -----------------------------------------------------
    update_slice(bk, w, Qb, L_X, L_PS, y.dWt, y.db);
    {
        bf16x8 mine[2];
        publish_slice(bk, w, y.dWt, mine);
        publish_transposed(bk, w, y.dWt);
    }
    mid();
    bk.barrier();                                               // B: L_WI, L_TR written | read (until A of the next step)
    // ---- (6) dgZ1 = -eta (K dW1n + db1n) ; (8) backward of the fused LN / L2 gradient -> dZ1, dt, dgamma, dbeta -----------------
    bf16x4 dZ1p[4];
    f32x4 dk[4];                     // starts as -dt (dt = gradient w.r.t. the target V - K = dV)
    {
        f32x4 dgz[4], mGr[4], t2[4];
        {
            bf16x8 DWp[8];
            load_image(bk, DWp);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                f32x4 a = zero4();
                a = bk.mma32(kA0, DWp[fb], a);
                a = bk.mma32(kA1, DWp[4 + fb], a);
                dgz[fb] = (a + y.db[fb]) * (-eta4);
                mGr[fb] = dgz[fb] * (-ig.rstd);
                t2[fb] = mGr[fb] * ig.xh[fb];
            }
        }
        const f32x4 s1 = lin16::rowsum64(bk, mGr) * (1.0f / 64.0f), s2 = lin16::rowsum64(bk, t2) * (1.0f / 64.0f);
        const f32x4 c2 = ig.s2g * (1.0f / 64.0f);
        f32x4 dxh[4], dstd[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dgxh = lin16::fma4(dgz[fb], ig.rstd, s1) + ig.xh[fb] * s2;
            const f32x4 dy = dgxh * c.gam[fb];
            const f32x4 dg = lin16::fma4(ig.go[fb], dgxh, dy * ig.xh[fb]);
            y.dgam[fb] += dg[0] + dg[1] + dg[2] + dg[3];
            y.dbet[fb] += dy[0] + dy[1] + dy[2] + dy[3];
            dk[fb] = dy;                                                                       // = -dt
            dxh[fb] = lin16::fma4(ig.go[fb] * c.gam[fb], s2, dy * c.gam[fb]) + mGr[fb] * c2;
            dstd[fb] = lin16::fma4(dgz[fb], ig.gz[fb], dxh[fb] * ig.xh[fb]) * (-ig.rstd);
        }
        const f32x4 v1 = lin16::rowsum64(bk, dxh) * (1.0f / 64.0f), v2 = lin16::rowsum64(bk, dstd) * (1.0f / 64.0f);
        float cs[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dz1 = lin16::fma4(dxh[fb] - v1, ig.rstd, ig.xh[fb] * v2);
            dZ1p[fb] = pack4(dz1);
            cs[fb] = lin16::colsum16(bk, dz1);
        }
        publish_rows(bk, w, L_X2, L_PS2, dZ1p, cs);                                               // for (10)
        f32x4 dv[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) dv[fb] = -dk[fb];
        lin16::store_rows(bk, IMG + IMG_BYTES, dv, p.dXV + tile * 4096 + w * 1024);              // dV = dt
    }
    bk.lds_fence();
    // ---- (5, 7, 9) A1 = gZ1 dW1n^T ; d eta ; dK = -eta A1 - dt + dZ1 W^T --------------------------------------------------------------
    {
        bf16x4 gzq[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) gzq[fb] = pack4(ig.gz[fb]);
        bf16x8 aG[2];
        lin16::image_of(bk, IMG, gzq, aG);
        f32x4 acc[4];
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            f32x4 a1 = zero4();
            a1 = bk.mma32(aG[0], transposed_frag(bk, 0, 16 * fa), a1);
            a1 = bk.mma32(aG[1], transposed_frag(bk, 1, 16 * fa), a1);
            dk[fa] -= a1 * eta4;
            const f32x4 kc = bk.mma16(c.IDP, kT[fa], zero4());                                // exact K, accumulator layout
            acc[fa] = lin16::fma4(ig.gz[fa], lin16::splat4(y.db[fa]), kc * a1);
        }
        const f32x4 de = lin16::rowsum64(bk, acc);
        if (i == 0) *reinterpret_cast<bf16x4*>(p.deta + tile * 64 + 16 * w + 4 * g) = pack4(-de);
    }
    bk.lds_fence();
    {
        bf16x8 aD[2];
        lin16::image_of(bk, IMG, dZ1p, aD);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            dk[fa] = bk.mma32(aD[0], lin16::ld_pack(bk, slot, 8 + fa), dk[fa]);
            dk[fa] = bk.mma32(aD[1], lin16::ld_pack(bk, slot, 12 + fa), dk[fa]);
        }
        lin16::store_rows(bk, IMG + IMG_BYTES, dk, p.dXK + tile * 4096 + w * 1024);
    }
    bk.barrier();                                               // C: L_X2, L_PS2 written | read (until B of the next step)
    // ---- (10) dW1 = dW1n + K^T dZ1 ; db1 = db1n + colsum dZ1 --------------------------------------------------------------------------
    update_slice(bk, w, Kb, L_X2, L_PS2, y.dWt, y.db);
}

// the walk of (b, h) = bh over the groups k0 + nk - 1 .. k0 from the slots recompute_groups and the records front_groups left: the
// loop and the carry contract of sweep_groups (dW1_last / db1_last -> dW1 / db1, which may alias ; ln_carry ; dln_w / dln_b in the
// range with k0 == 0) around chain_step.  K, Q, eta and the record of the step in front are fetched while a step runs - none of their
// addresses depends on the carry.  No V, no dOut.
template <class BK>
TTT_WV_FN void chain_groups(BK& bk, const Lin16BwdFrontParams& f, int bh) {
    const Lin16BwdPartParams& q = f.q;
    const Lin16Params& p = q.p;
    const int l0 = bk.lane(), w = bk.wave();
    const int NC = p.NC, G = p.G, K = p.K, head = bh % p.NH;
    const int k0 = q.k0, nk = q.nk;
    const int s_lo = k0 * G, s_hi = ((k0 + nk) * G < NC) ? (k0 + nk) * G : NC;      // the steps [s_lo, s_hi)
    const size_t tile0 = (size_t)bh * NC;
    const int ETA = L_ETA + w * 128, own = w * TILE_B;
    const char* slots = q.slots + (size_t)bh * nk * (G + 1) * LIN_PART_SLOT_BYTES;
    const char* recs = f.records + (size_t)bh * nk * G * LIN64_FRONT_RECORD_BYTES + (size_t)w * LIN_FRONT_RECORD_BYTES;
    float* carry = q.ln_carry + (size_t)bh * LIN_PART_CARRY_FLOATS * 64 * WAVES + w * 64 + l0;

    Consts c;
    make_consts(bk, p, head, c);
    BwdCarry y;
    load_slice(bk, w, p.dW1_last + (size_t)bh * 64 * 64, y.dWt);
    lin16::load_row(bk, p.db1_last + (size_t)bh * 64, y.db);
    if (k0 + nk == K) {      // the range that ends the sequence starts the sums
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) y.dgam[fb] = y.dbet[fb] = 0.f;
    } else {
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) { y.dgam[fb] = carry[fb * 64 * WAVES]; y.dbet[fb] = carry[(4 + fb) * 64 * WAVES]; }
    }
    int k = k0 + nk - 1, lo = k * G;          // the group of step `it`
    int cur = 0;
    Stage sk, sq;
    unsigned short pe = 0;
    StepRecord r, rn;
    {   // the first step of the walk.  Every wave its own rows; the rows of other waves are read behind barrier A of the first step
        // at the earliest (Q in (3), K in (10)).
        const size_t t = tile0 + s_hi - 1;
        lin16::stage_request(bk, sk, p.XK + t * 4096 + w * 1024);
        lin16::stage_request(bk, sq, p.XQ + t * 4096 + w * 1024);
        pe = *reinterpret_cast<const unsigned short*>(p.eta + t * 64 + 16 * w + (l0 & 15));
        rec_request(bk, l0, recs + ((size_t)(k - k0) * G + (s_hi - 1 - lo)) * LIN64_FRONT_RECORD_BYTES, r);
        park(bk, sk, L_K + own); park(bk, sq, L_Q + own);
        park_eta(bk, pe, ETA);
        bk.lds_fence();
    }
    for (int it = s_hi - 1; it >= s_lo; --it) {
        if (it < lo) { --k; lo -= G; }
        const int l = bk.opaque(l0);
        const bool more = it > s_lo;
        if (more) {
            const size_t t = tile0 + it - 1;
            const int kn = (it - 1 < lo) ? k - 1 : k, lon = (it - 1 < lo) ? lo - G : lo;      // the group of the step in front
            lin16::stage_request(bk, sk, p.XK + t * 4096 + w * 1024);
            lin16::stage_request(bk, sq, p.XQ + t * 4096 + w * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + t * 64 + 16 * w + (l & 15));
            rec_request(bk, l, recs + ((size_t)(kn - k0) * G + (it - 1 - lon)) * LIN64_FRONT_RECORD_BYTES, rn);
        }
        const char* slot = slots + ((size_t)(k - k0) * (G + 1) + (it - lo)) * LIN_PART_SLOT_BYTES;       // state entering the step
        chain_step(bk, l, w, p, c, y, tile0 + it, L_K + cur * T64_B, L_Q + cur * T64_B, ETA + cur * 64, slot, r, [&] {
            if (more) {      // the other buffer was last read (K in (10), Q in (3)) by the step before this one
                const int nb = cur ^ 1;
                park(bk, sk, L_K + nb * T64_B + own); park(bk, sq, L_Q + nb * T64_B + own);
                park_eta(bk, pe, ETA + nb * 64);
            }
        });
        if (more) {
            cur ^= 1;
            r = rn;
        }
        bk.lds_fence();
    }
    // ---- hand-over, as in sweep_groups: q.p.dW1 / db1 may alias dW1_last / db1_last (every wave reads db1_last and its own slice of
    // dW1_last in front of the step loop, these stores come behind the barriers of the last step) ; ln_carry is read and written by
    // the same lane only
    store_slice(bk, w, p.dW1 + (size_t)bh * 64 * 64, y.dWt);
    if (w == 0 && (l0 >> 4) == 0)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) p.db1[(size_t)bh * 64 + 16 * fb + (l0 & 15)] = y.db[fb];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) { carry[fb * 64 * WAVES] = y.dgam[fb]; carry[(4 + fb) * 64 * WAVES] = y.dbet[fb]; }
    if (k0 == 0) store_ln_grads(bk, w, p, bh, y);
}

}  // namespace lin64
}  // namespace ttt
