// TTT-Linear forward scan at mini-batches of 16 tokens with the OUTPUT path on a second wave (opt-in; lin16::forward_part of
// ttt_lin16_body.h stays the default and the yardstick).  One workgroup of two waves serves one (batch, head):
//   wave 0, the chain role : Z1 = K W1 + b1 -> fused LayerNorm / L2 gradient -> Gs -> W1 += K^T Gs, b1 += colsum Gs -> repack.  This
//                            is the whole step-to-step dependency of the scan; it never touches Q, `out` or the output LayerNorm.
//   wave 1, the output role: Z1b = Q W1' + b1' -> LayerNorm -> + Q -> XQW, from the packed state W1F (the 8 bf16 operand fragments
//                            the chain role builds for its own next step) and the fp32 b1' - the same operands the one-wave step
//                            feeds its second half, so the same bits.
// Hand-over through LDS: two slots of SLOT_BYTES (fragment idx = ks * 4 + fb at (idx * 64 + lane) * 16, as lin16::st_pack lays
// fragments out, then the bias row as [lane & 15][fb] fp32).  The chain role writes slot (it & 1) in step `it` and reaches the
// workgroup barrier; the output role reads slot (it & 1) behind that barrier.  Two slots because, in the barrier interval in which
// the output role reads slot (it & 1), the chain role is already writing slot ((it + 1) & 1); slot (it & 1) is written again in step
// it + 2, i.e. behind barrier it + 1, which the output role reaches only when it is done with step `it`.
// INVARIANT: both roles execute exactly ONE bk.barrier() per step of the part, inside their `for (it ...)` loop, and neither returns
// before its loop ends - a role that skipped or added one would leave the other waiting at a barrier for good.
// LDS map (bytes): [0, WAVE_LDS) the chain role's private region (K, V, eta; map of ttt_lin16_body.h), [WAVE_LDS, 2 WAVE_LDS) the
// output role's (Q, image), then the two slots.  The helpers of ttt_lin16_body.h take their tile / image offsets from the caller.
#pragma once
#include "ttt_lin16_body.h"

namespace ttt {
namespace lin16 {
namespace split {

constexpr int WAVES = 2;
constexpr int R_CHAIN = 0, R_OUT = WAVE_LDS;                       // the two private regions
constexpr int SLOT_W_BYTES = 8 * 64 * 16, SLOT_B_BYTES = 16 * 16;   // 8 fragments x 64 lanes x 16 bytes ; [16 i][4 fb] fp32
constexpr int SLOT_BYTES = SLOT_W_BYTES + SLOT_B_BYTES;            // 8 448
constexpr int L_SLOT = 2 * WAVE_LDS;
constexpr int GROUP_LDS = L_SLOT + 2 * SLOT_BYTES;
static_assert(SLOT_BYTES == 8448, "hand-over slot: W1F[2][4] + b1'");
static_assert(R_OUT % 16 == 0 && L_SLOT % 16 == 0 && SLOT_BYTES % 16 == 0, "alignment");
static_assert(2 * GROUP_LDS <= 160 * 1024, "two workgroups per CU");

// ---- wave 0: the chain.  lin16::forward_part without its output half; what it would have kept in W1F / b1v for that half goes to
// the slot instead.
template <class BK>
TTT_WV_FN void chain_role(BK& bk, const Lin16ChunkParams& c, int bh) {
    const Lin16Params& p = c.p;
    const int l0 = bk.lane();
    const int NC = p.NC, G = p.G, head = bh % p.NH, step0 = c.step0;
    constexpr int LK = R_CHAIN + L_K, LV = R_CHAIN + L_V, LE = R_CHAIN + L_ETA;

    f32x4 W1t[4][4];     // [fa][fb]  W1[16fa + 4g + r][16fb + i]     (rows = f_in, lane = f_out)
    float b1v[4], gam[4], bet[4];
    {
        const int g = l0 >> 4, i = l0 & 15;
        const float* W1g = p.W1 + (size_t)bh * 64 * 64;
#pragma unroll
        for (int fa = 0; fa < 4; ++fa)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                for (int r = 0; r < 4; ++r) W1t[fa][fb][r] = W1g[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * fb + i];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            b1v[fb] = p.b1[(size_t)bh * 64 + 16 * fb + i];
            gam[fb] = p.ln_w[(size_t)head * 64 + 16 * fb + i];
            bet[fb] = p.ln_b[(size_t)head * 64 + 16 * fb + i];
        }
    }
    const bf16x4 ONES = {(__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f};
    bf16x4 IDP, IDN;     // +-identity as mma16 A operand: lane = t = i, k-slot e = token 4g + e
    {
        const int g = l0 >> 4, i = l0 & 15;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            IDP[e] = (__bf16)((4 * g + e) == i ? 1.0f : 0.0f);
            IDN[e] = (__bf16)((4 * g + e) == i ? -1.0f : 0.0f);
        }
    }
    bf16x8 W1F[2][4];    // [ks][fb] packed entering state, carried across steps
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) W1F[ks][fb] = stack(W1t[2 * ks][fb], W1t[2 * ks + 1][fb]);

    const size_t tile0 = (size_t)bh * c.NCs + step0;
    Stage sk, sv;
    unsigned short pe;
    stage_request(bk, sk, p.XK + tile0 * 1024);
    stage_request(bk, sv, p.XV + tile0 * 1024);
    pe = *reinterpret_cast<const unsigned short*>(p.eta + tile0 * 16 + (l0 & 15));
    stage_park(bk, sk, LK); stage_park(bk, sv, LV);
    if (l0 < 16) bk.template lds<float>(LE + l0 * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
    bk.lds_fence();

    for (int it = 0; it < NC; ++it) {       // exactly one bk.barrier() per iteration, no early exit (see the invariant above)
        const int buf = it & 1;
        const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        const int Kt = LK + buf * TILE * 2, Vt = LV + buf * TILE * 2;
        {   // next step's inputs, parked at the end of this step
            const size_t tn = tile0 + (it + 1 < NC ? it + 1 : it);
            stage_request(bk, sk, p.XK + tn * 1024);
            stage_request(bk, sv, p.XV + tn * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + tn * 16 + (l & 15));
        }
        if ((step0 + it) % G == 0) {      // checkpoint: state entering step `step0 + it`
            const size_t ck = (size_t)bh * p.K + (step0 + it) / G;
            float* W1g = p.W1c + ck * 64 * 64;
#pragma unroll
            for (int fa = 0; fa < 4; ++fa)
#pragma unroll
                for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) W1g[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * fb + i] = W1t[fa][fb][r];
            if (g == 0)
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) p.b1c[ck * 64 + 16 * fb + i] = b1v[fb];
        }
        // ---- Z1 = K W1 + b1 ; target = V - K, both (rows = t, lane = f) -----------------------------------------------
        const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
        const f32x4 eta4 = bk.template lds<f32x4>(LE + (buf * 16 + 4 * g) * 4);          // eta of token rows 4g .. 4g+3
        bf16x4 kT[4];
        f32x4 z[4], tg[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            kT[fb] = tr4(bk, Kt, TS, 0, 16 * fb);                                            // lane = f, k = t
            f32x4 a = zero4();
            a = bk.mma32(kA0, W1F[0][fb], a);
            a = bk.mma32(kA1, W1F[1][fb], a);
            z[fb] = a + b1v[fb];
            tg[fb] = bk.mma16(IDN, kT[fb], bk.mma16(IDP, tr4(bk, Vt, TS, 0, 16 * fb), zero4()));   // exact V - K
        }
        // ---- fused LayerNorm + L2 backward per token row ; Gs = -eta gZ1 ------------------------------------------------
        bf16x4 gzp[4];
        {
            InnerGrad ig;
            inner_grad(bk, z, tg, gam, bet, p.eps, ig);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) gzp[fb] = pack4(ig.gz[fb] * (-eta4));                       // lane = f, k = t
        }
        // ---- W1 += K^T Gs ; b1 += colsum Gs ; repack -----------------------------------------------------------------------
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            b1v[fb] += bk.mma16(ONES, gzp[fb], zero4())[0];
#pragma unroll
            for (int fa = 0; fa < 4; ++fa) W1t[fa][fb] = bk.mma16(kT[fa], gzp[fb], W1t[fa][fb]);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) W1F[ks][fb] = stack(W1t[2 * ks][fb], W1t[2 * ks + 1][fb]);
        // ---- publish W1', b1' for the output role and meet it ------------------------------------------------------------------
        {
            const int slot = L_SLOT + buf * SLOT_BYTES;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) bk.template lds_store<bf16x8>(slot + ((ks * 4 + fb) * 64 + l) * 16, W1F[ks][fb]);
            const f32x4 bv = {b1v[0], b1v[1], b1v[2], b1v[3]};
            bk.template lds_store<f32x4>(slot + SLOT_W_BYTES + i * 16, bv);     // every row group g: the same value to the same cell
        }
        bk.barrier();                       // slot (it & 1) written | read by the output role (until barrier it + 1)
        const int nb = buf ^ 1;
        stage_park(bk, sk, LK + nb * TILE * 2); stage_park(bk, sv, LV + nb * TILE * 2);
        if (l < 16) bk.template lds<float>(LE + (nb * 16 + l) * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
        bk.lds_fence();
    }
    if (c.W1f) {      // hand the state on.  May overwrite the initial state: this wave is the only reader of its (b, h)'s p.W1 /
                      // p.b1 and read all of it before the first step.
        const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        float* W1g = c.W1f + (size_t)bh * 64 * 64;
#pragma unroll
        for (int fa = 0; fa < 4; ++fa)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                for (int r = 0; r < 4; ++r) W1g[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * fb + i] = W1t[fa][fb][r];
        if (g == 0)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) c.b1f[(size_t)bh * 64 + 16 * fb + i] = b1v[fb];
    }
}

// ---- wave 1: the outputs.  WORK = false (the bench tool's chain-alone arm): only the barriers - nothing is read, computed or
// stored, so the part's time is the chain role's alone.
template <bool WORK, class BK>
TTT_WV_FN void output_role(BK& bk, const Lin16ChunkParams& c, int bh) {
    const Lin16Params& p = c.p;
    const int NC = p.NC;
    if (!WORK) {
        for (int it = 0; it < NC; ++it) bk.barrier();       // one per step, as the chain role
        return;
    }
    const int l0 = bk.lane();
    const int head = bh % p.NH;
    constexpr int LQ = R_OUT + L_Q, LI = R_OUT + L_IMG;
    float gam[4], bet[4];
    bf16x4 IDP;
    {
        const int g = l0 >> 4, i = l0 & 15;
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            gam[fb] = p.ln_w[(size_t)head * 64 + 16 * fb + i];
            bet[fb] = p.ln_b[(size_t)head * 64 + 16 * fb + i];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) IDP[e] = (__bf16)((4 * g + e) == i ? 1.0f : 0.0f);
    }
    const size_t tile0 = (size_t)bh * c.NCs + c.step0;
    Stage sq;
    stage_request(bk, sq, p.XQ + tile0 * 1024);
    stage_park(bk, sq, LQ);
    bk.lds_fence();

    for (int it = 0; it < NC; ++it) {       // exactly one bk.barrier() per iteration, no early exit (see the invariant above)
        const size_t tile = tile0 + it;
        const int buf = it & 1;
        const int l = bk.opaque(l0), i = l & 15;
        const int Qt = LQ + buf * TILE * 2;
        stage_request(bk, sq, p.XQ + (tile0 + (it + 1 < NC ? it + 1 : it)) * 1024);       // next step's Q, parked at the end of this one
        bk.barrier();                       // slot (it & 1) written by the chain role | read here
        const int slot = L_SLOT + buf * SLOT_BYTES;
        bf16x8 W1F[2][4];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) W1F[ks][fb] = bk.template lds_load<bf16x8>(slot + ((ks * 4 + fb) * 64 + l) * 16);
        const f32x4 b1v = bk.template lds_load<f32x4>(slot + SLOT_W_BYTES + i * 16);
        // ---- Z1b = Q W1' + b1' ; LayerNorm ; + Q -> XQW --------------------------------------------------------------------------
        {
            const bf16x8 qA0 = rho_read(bk, Qt, 0), qA1 = rho_read(bk, Qt, 32);
            f32x4 y[4], qc[4];
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                f32x4 a = zero4();
                a = bk.mma32(qA0, W1F[0][fb], a);
                a = bk.mma32(qA1, W1F[1][fb], a);
                y[fb] = a + b1v[fb];
                qc[fb] = bk.mma16(IDP, tr4(bk, Qt, TS, 0, 16 * fb), zero4());                // exact Q in the accumulator layout
            }
            normalize_rows(bk, y, p.eps);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) y[fb] = qc[fb] + gam[fb] * y[fb] + bet[fb];
            store_rows(bk, LI, y, p.out + tile * 1024);
        }
        stage_park(bk, sq, LQ + (buf ^ 1) * TILE * 2);
        bk.lds_fence();
    }
}

template <bool WORK, class BK>
TTT_WV_FN void forward_part_roles(BK& bk, const Lin16ChunkParams& c, int bh) {
    if (bk.wave() == 0) chain_role(bk, c, bh);
    else output_role<WORK>(bk, c, bh);
}
// steps [c.step0, c.step0 + c.p.NC) of (b, h) = bh: parameters and semantics of lin16::forward_part
template <class BK>
TTT_WV_FN void forward_part(BK& bk, const Lin16ChunkParams& c, int bh) { forward_part_roles<true>(bk, c, bh); }
// the same part with the output role's work removed (`out` is not written): what the chain role alone costs
template <class BK>
TTT_WV_FN void chain_alone_part(BK& bk, const Lin16ChunkParams& c, int bh) { forward_part_roles<false>(bk, c, bh); }

}  // namespace split
}  // namespace lin16
}  // namespace ttt
