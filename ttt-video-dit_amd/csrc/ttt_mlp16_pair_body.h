// TTT-MLP forward scan at mini-batches of 16 tokens as a PAIR of workgroups per (b, h) (opt-in; the one-workgroup body is
// mlp16::forward_part of ttt_mlp16_body.h, which this file does not touch).  The chain that carries the state from step to step is
//   A1 -> A2 -> B1 -> P3 -> B2 -> C (state updates)
// and the OUTPUT path of a step - Z1b = Q W1' + b1', its GELU, the E partials, P6 (LayerNorm, + Q) - hangs off the UPDATED state;
// nothing downstream waits for it.  In pair form
//   state_role  (role A) runs the chain only, with the arithmetic of forward_part, writes the checkpoints and the final state, and
//               after the updates of step `it` every wave publishes the operands the output path consumes exactly as it holds them:
//               W1F[2][2] and W2F[4] (bf16x8: 128 B per lane, 64 KiB per workgroup), b1' (256 fp32) and b2' (64 fp32) - record `it`,
//               slot it % RING of this (b, h)'s ring;
//   output_role (role B, another workgroup) waits for record `it`, loads its waves' fragments and bias rows and runs the output path
//               with the calls of forward_part in their order: `out` carries the bits of the one-workgroup scan.
// The hand-over is ONE-WAY (cdna_hip_programming.md Guideline 16, form R1, as the CS = 64 pair scan of ttt_mfma2.hip): A never waits
// for B unless it is RING steps ahead.  Both roles take wv::Mlp16ChunkParams: a part [step0, step0 + NC) like forward_part.
//
// The hand-over itself is a POLICY `HO` (second template parameter), so that the CPU suite runs both roles on the wave emulator with
// host memory and std::atomic (tests/emul/mlp16_pair_emul.cpp); the device policy is in ttt_mfma16.hip.  Per thread:
//   ho.store16(voff, soff, u32x4) / ho.store4(voff, soff, unsigned)   record payload to ring byte voff + soff (device: write-through,
//                                                                     soff wave-uniform)
//   ho.load16(voff, soff) -> u32x4                                    record payload (device: never served by the reading CU's L1)
//   ho.drain()                    every record store / load this wave has issued is complete
//   ho.post(word, v)              relaxed agent-scope store of a flag word - ONE lane of the workgroup calls it
//   ho.peek(word) -> unsigned     relaxed agent-scope load of a flag word, wave-uniform
//   ho.wait_ge(word, need) -> bool   poll until the flag word is >= need; bounded (device: 2 s of the 100 MHz wall clock);
//                                    false = gave up (wave-uniform)
//   ho.fail(bh)                   1 + bh into the process's error word (the next extension call raises "hand-over") - one lane
#pragma once
#include "ttt_mlp16_body.h"

namespace ttt {
namespace mlp16 {
namespace pair {

constexpr int RING = 4;                                       // records in flight per (b, h)
// record: the layout idea of v2::REC_* (ttt_mfma2.hip)
constexpr int REC_W1F = 0;                                    // 8 waves x 4 fragments x 1 KiB: W1F[ks][nb] of wave w at (4 w + 2 ks + nb) KiB + 16 lane
constexpr int REC_W2F = 32 * 1024;                            // the same of W2F[fb]
constexpr int REC_B1 = 64 * 1024;                             // b1' [256] fp32
constexpr int REC_B2 = REC_B1 + 1024;                         // b2' [64] fp32
constexpr int REC_BYTES = REC_B2 + 256;
static_assert(REC_BYTES % 256 == 0, "records are line aligned");
constexpr int FLAG_WORDS = 64;                                // per (b, h): two 128-byte lines
constexpr int FL_A = 0;                                       // [0] records published by A, [1] A gave up (poison)
constexpr int FL_B = 32;                                      // [32] steps finished by B
// workspace: the flag words of every (b, h) in a block of their own at the start (zeroed in front of every launch), then the rings
constexpr size_t flags_bytes(int n_bh) { return (size_t)n_bh * FLAG_WORDS * sizeof(unsigned); }
constexpr size_t workspace_bytes(int n_bh) { return flags_bytes(n_bh) + (size_t)n_bh * RING * REC_BYTES; }
static_assert(flags_bytes(1) % 16 == 0, "the memset block is a multiple of 16 bytes");

// role A: K, V (2 buffers each), Gs, the X2 image, the redA partials, eta[2][16] b2[64] gamma[64] beta[64] - no Q, no redB
constexpr int A_K = 0, A_V = A_K + 2 * TILE * 2, A_G = A_V + 2 * TILE * 2, A_IMG = A_G + TILE * 2;
constexpr int A_REDA = A_IMG + 8 * IMG_BYTES, A_ETA = A_REDA + RED_BYTES, A_B2 = A_ETA + 32 * 4, A_GAM = A_B2 + 64 * 4, A_BET = A_GAM + 64 * 4;
constexpr int STATE_LDS = A_BET + 64 * 4;
// role B: Q (3 buffers), the X2b image, the redB partials twice (by step parity: one barrier per step), gamma, beta, the poison word
constexpr int B_Q = 0, B_IMG = B_Q + 3 * TILE * 2, B_RED = B_IMG + 8 * IMG_BYTES, B_GAM = B_RED + 2 * RED_BYTES, B_BET = B_GAM + 64 * 4;
constexpr int B_POISON = B_BET + 64 * 4;
constexpr int OUTPUT_LDS = B_POISON + 16;
constexpr int PAIR_LDS = STATE_LDS > OUTPUT_LDS ? STATE_LDS : OUTPUT_LDS;
static_assert(PAIR_LDS <= 160 * 1024 && A_IMG % 16 == 0 && A_REDA % 16 == 0 && A_ETA % 16 == 0 && B_IMG % 16 == 0 && B_RED % 16 == 0 &&
              B_GAM % 16 == 0, "LDS map");

// gather8 (ttt_mlp16_body.h) with the bias handed in: bias + the 8 waves' partials in wave order
template <class BK>
TTT_WV_FN f32x4 gather8_from(BK& bk, f32x4 z, int red_off, int ot, int of0) {
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) z += bk.template lds_load<f32x4>(red_off + ((ww * CS + ot) * PS + of0) * 4);
    return z;
}

// gelu_fwd_grad (ttt_mlp16_body.h) of A1 for element r of hidden block nb, with the ROUNDINGS of the one-workgroup kernel.  The host
// build rounds every product (what it does for forward_part too).  On the device the compiler contracts a*b + c wherever it sees
// fit, and in the kernel of forward_part it does so unevenly: for nb = 1, r = 2, 3 the products x2 (2 * 3ac) and y s are packed with
// other multiplies (v_pk_mul_f32) and rounded before the add, every other element gets the fused forms.  gelu' feeds the state through
// a bf16 rounding, so a last-bit difference there flips a state bit once in ~10^6 elements: invisible in short scans, a different
// scan after a few hundred steps of 96 heads.  So role A spells out that kernel's choice, fused or not, operation by operation
// (tests/test_mlp16_pair_gpu.py compares the final state after 600 steps; the long A/B of tools/mlp16_pair_bench.py compares bits).
template <class BK>
TTT_WV_FN void gelu_fwd_grad_a1(BK& bk, float x, int nb, int r, float& y, float& dy) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
    const float x2 = x * x;
    const float s = bk.rcp(1.0f + bk.exp2(x * __builtin_fmaf(x2, GELU_K1, GELU_K0)));
    y = x * s;
    float t, u;
    if (nb == 1 && r >= 2) {
        const float ys = y * s, xc = x2 * (2.0f * GELU_3AC);
        t = y - ys;
        u = xc + 2.0f * GELU_A;
    } else {
        t = __builtin_fmaf(-y, s, y);
        u = __builtin_fmaf(x2, 2.0f * GELU_3AC, 2.0f * GELU_A);
    }
    dy = __builtin_fmaf(t, u, s);
#else
    (void)nb; (void)r;
    gelu_fwd_grad(bk, x, y, dy);
#endif
}

// ---- role A: the chain of forward_part, the record of the updated state in place of the output path -------------------------------
template <class BK, class HO>
TTT_WV_FN void state_role(BK& bk, HO& ho, const Mlp16ChunkParams& c, int bh) {
    const Mlp16Params& p = c.p;
    const int tid0 = bk.thread(), wv = bk.wave(), l0 = bk.lane();
    const int n0 = 32 * wv, img = A_IMG + wv * IMG_BYTES;
    const int NC = p.NC, G = p.G, head = bh % p.NH, step0 = c.step0;

    f32x4 W1t[4][2], W2t[2][4], W2Tt[4][2];      // (rows = f, lane = n) ; (rows = n, lane = f) ; (rows = f, lane = n)
    float b1v[2], b2v[4];
    {
        const int g = l0 >> 4, i = l0 & 15;
        const float* W1g = p.W1 + (size_t)bh * 64 * 256;
        const float* W2g = p.W2 + (size_t)bh * 256 * 64;
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    W1t[fb][nb][r] = W1g[(size_t)(16 * fb + 4 * g + r) * 256 + n0 + 16 * nb + i];
                    W2t[nb][fb][r] = W2g[(size_t)(n0 + 16 * nb + 4 * g + r) * 64 + 16 * fb + i];
                }
                W2Tt[fb][nb] = *reinterpret_cast<const f32x4*>(W2g + (size_t)(n0 + 16 * nb + i) * 64 + 16 * fb + 4 * g);
            }
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) b1v[nb] = p.b1[(size_t)bh * 256 + n0 + 16 * nb + i];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) b2v[fb] = p.b2[(size_t)bh * 64 + 16 * fb + i];
        if (tid0 < 64) {
            bk.template lds_store<float>(A_B2 + tid0 * 4, p.b2[(size_t)bh * 64 + tid0]);
            bk.template lds_store<float>(A_GAM + tid0 * 4, p.ln_w[(size_t)head * 64 + tid0]);
            bk.template lds_store<float>(A_BET + tid0 * 4, p.ln_b[(size_t)head * 64 + tid0]);
        }
    }
    const bf16x4 ONES = {(__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f};
    bf16x8 W1F[2][2], W2F[4];                    // packed operands of the current state, carried across steps
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) W1F[ks][nb] = stack(W1t[2 * ks][nb], W1t[2 * ks + 1][nb]);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) W2F[fb] = stack(W2t[0][fb], W2t[1][fb]);

    // input staging: waves 0, 1 move K, waves 2, 3 move V (one 16-byte chunk per thread); waves 4 - 7 load nothing (no Q here)
    const size_t tile0 = (size_t)bh * c.NCs + step0;
    const int which = wv >> 1;
    const bool stager = which < 2;
    const __bf16* src = which == 0 ? p.XK : p.XV;
    const int dstb = which == 0 ? A_K : A_V;
    const int lt0 = tid0 & 127, lofs = ((lt0 >> 3) * TS + (lt0 & 7) * 8) * 2;
    const size_t gofs = (size_t)(lt0 >> 3) * 64 + (lt0 & 7) * 8;
    u32x4 pfO = {0u, 0u, 0u, 0u};
    unsigned short pfEO;
    {
        if (stager) bk.template lds_store<u32x4>(dstb + lofs, *reinterpret_cast<const u32x4*>(src + tile0 * 1024 + gofs));
        if (tid0 < 16) bk.template lds_store<float>(A_ETA + tid0 * 4, (float)p.eta[tile0 * 16 + tid0]);
        const size_t t1 = tile0 + (NC > 1 ? 1 : 0);
        if (stager) pfO = *reinterpret_cast<const u32x4*>(src + t1 * 1024 + gofs);
        pfEO = *reinterpret_cast<const unsigned short*>(p.eta + t1 * 16 + (tid0 & 15));
    }
    bool gave_up = false;                         // this wave stopped waiting for role B (error word stored)
    bk.barrier();

    for (int it = 0; it < NC; ++it) {
        const int buf = it & 1;
        const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        const int tid = bk.opaque(tid0);
        const int ot = (tid & 255) >> 4, of0 = 4 * (tid & 15);
        const int Kt = A_K + buf * TILE * 2, Vt = A_V + buf * TILE * 2;

        const size_t tn = tile0 + (it + 2 < NC ? it + 2 : NC - 1);
        u32x4 pfN = pfO;
        if (stager) pfN = *reinterpret_cast<const u32x4*>(src + tn * 1024 + gofs);
        const unsigned short pfEN = *reinterpret_cast<const unsigned short*>(p.eta + tn * 16 + (tid & 15));
        // role B's progress, asked for a whole step before it may matter (slot it % RING held record it - RING)
        unsigned b_done = 0u;
        if (it >= RING && !gave_up) b_done = ho.peek(FL_B);

        f32x4 D1[2];
        bf16x4 X2p[2];
        if ((step0 + it) % G == 0) {
            const size_t ck = (size_t)bh * p.K + (step0 + it) / G;
            store_state(p.W1c + ck * 64 * 256, p.b1c + ck * 256, p.W2c + ck * 256 * 64, p.b2c + ck * 64, W1t, W2Tt, b1v, b2v, wv, g, i);
        }
        // A1: Z1 = K W1 + b1 ; X2, D1 (rows = t, lane = n) ; X2 image [n][t]
        const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f32x4 Z = zero4();
            Z = bk.mma32(kA0, W1F[0][nb], Z);
            Z = bk.mma32(kA1, W1F[1][nb], Z);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float y, dy;
                gelu_fwd_grad_a1(bk, Z[r] + b1v[nb], nb, r, y, dy);
                Z[r] = y;
                D1[nb][r] = dy;
            }
            X2p[nb] = pack4(Z);
            bk.template lds_store<bf16x4>(img + ((16 * nb + i) * IS + 4 * g) * 2, X2p[nb]);
        }
        bk.lds_fence();
        // A2: partial Z2^T[f, t] over this wave's hidden slice
        const bf16x8 xB = cat(tr4(bk, img, IS, 0, 0), tr4(bk, img, IS, 16, 0));           // lane = t, k = n (rho)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
            bk.template lds_store<f32x4>(A_REDA + ((wv * CS + i) * PS + 4 * g + 16 * fb) * 4, bk.mma32(W2F[fb], xB, zero4()));
        ho.drain();                   // record it - 1: this wave's stores are complete (a whole A1 / A2 after they were issued)
        bk.barrier();                 // B1
        if (tid == 0 && it > 0) ho.post(FL_A, (unsigned)it);      // records 0 .. it - 1 are published

        if (wv < 4) {                 // P3: owners - reduce, fused LN / L2 backward -> Gs = -eta gZ2
            f32x4 z = gather8_from(bk, bk.template lds_load<f32x4>(A_B2 + of0 * 4), A_REDA, ot, of0);
            float mu, rstd;
            row_stats(bk, z, p.eps, mu, rstd);
            const bf16x4 kk = bk.template lds_load<bf16x4>(Kt + (ot * TS + of0) * 2);
            const bf16x4 vv = bk.template lds_load<bf16x4>(Vt + (ot * TS + of0) * 2);
            const f32x4 gm = bk.template lds_load<f32x4>(A_GAM + of0 * 4), bt = bk.template lds_load<f32x4>(A_BET + of0 * 4);
            float s1 = 0.f, s2 = 0.f, gx[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xh = (z[j] - mu) * rstd;
                gx[j] = (gm[j] * xh + bt[j] - ((float)vv[j] - (float)kk[j])) * gm[j];
                z[j] = xh;
                s1 += gx[j]; s2 += gx[j] * xh;
            }
            s1 = bk.sum16(s1);
            s2 = bk.sum16(s2);
            const float sc = -bk.template lds_load<float>(A_ETA + (buf * 16 + ot) * 4) * rstd * (1.0f / 64.0f);
            bf16x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (__bf16)((64.0f * gx[j] - s1 - z[j] * s2) * sc);
            bk.template lds_store<bf16x4>(A_G + (ot * TS + of0) * 2, o);
        }
        // park tile it+1 (requested one step ago)
        if (stager) bk.template lds_store<u32x4>(dstb + ((it + 1) & 1) * TILE * 2 + lofs, pfO);
        if (tid < 16) bk.template lds_store<float>(A_ETA + ((buf ^ 1) * 16 + tid) * 4, (float)*reinterpret_cast<const __bf16*>(&pfEO));
        pfO = pfN;
        pfEO = pfEN;
        bk.barrier();                 // B2

        // C: state updates ; gX2 ; W1 update
        {
            bf16x8 W2TF[2][2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) W2TF[ks][nb] = stack(W2Tt[2 * ks][nb], W2Tt[2 * ks + 1][nb]);
            const bf16x8 gA0 = rho_read(bk, A_G, 0), gA1 = rho_read(bk, A_G, 32);
            bf16x4 gzp[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                f32x4 gx = zero4();
                gx = bk.mma32(gA0, W2TF[0][nb], gx);
                gx = bk.mma32(gA1, W2TF[1][nb], gx);
                gx *= D1[nb];
                gzp[nb] = pack4(gx);
                b1v[nb] += bk.mma16(ONES, gzp[nb], zero4())[0];
            }
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const bf16x4 kT = tr4(bk, Kt, TS, 0, 16 * fb);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) W1t[fb][nb] = bk.mma16(kT, gzp[nb], W1t[fb][nb]);
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) W1F[ks][nb] = stack(W1t[2 * ks][nb], W1t[2 * ks + 1][nb]);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const bf16x4 gT = tr4(bk, A_G, TS, 0, 16 * fb);
                b2v[fb] += bk.mma16(ONES, gT, zero4())[0];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    W2t[nb][fb] = bk.mma16(X2p[nb], gT, W2t[nb][fb]);
                    W2Tt[fb][nb] = bk.mma16(gT, X2p[nb], W2Tt[fb][nb]);
                }
                W2F[fb] = stack(W2t[0][fb], W2t[1][fb]);
            }
        }
        if (wv == 0 && g == 0) {      // b2' -> LDS (P3 of the next step)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) bk.template lds_store<float>(A_B2 + (16 * fb + i) * 4, b2v[fb]);
        }
        // record `it` goes to slot it % RING, which held record it - RING: role B must have finished that step
        if (it >= RING && !gave_up && b_done + RING <= (unsigned)it) {
            if (!ho.wait_ge(FL_B, (unsigned)(it - RING + 1))) {
                gave_up = true;       // role B is not running: loud, not silent - the error word, a poison word for B, and go on
                if (l == 0) {
                    ho.fail(bh);
                    ho.post(FL_A + 1, 1u);
                }
            }
        }
        {
            const int soff = (it % RING) * REC_BYTES, vo = (wv * 4) * 1024 + l * 16;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) ho.store16(vo + (2 * ks + nb) * 1024, soff + REC_W1F, __builtin_bit_cast(u32x4, W1F[ks][nb]));
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) ho.store16(vo + fb * 1024, soff + REC_W2F, __builtin_bit_cast(u32x4, W2F[fb]));
            if (g == 0) {
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) ho.store4((n0 + 16 * nb + i) * 4, soff + REC_B1, __builtin_bit_cast(unsigned, b1v[nb]));
                if (wv == 0) {
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) ho.store4((16 * fb + i) * 4, soff + REC_B2, __builtin_bit_cast(unsigned, b2v[fb]));
                }
            }
        }
    }
    ho.drain();                       // the last record
    bk.barrier();
    if (tid0 == 0) ho.post(FL_A, (unsigned)NC);
    if (c.W1f) {      // hand the state on (may overwrite the initial state: every wave read its slice before the first barrier)
        const int l = bk.opaque(l0);
        store_state(c.W1f + (size_t)bh * 64 * 256, c.b1f + (size_t)bh * 256, c.W2f + (size_t)bh * 256 * 64, c.b2f + (size_t)bh * 64,
                    W1t, W2Tt, b1v, b2v, wv, l >> 4, l & 15);
    }
}

// ---- role B: the output path of every step of the part, from the records role A publishes -----------------------------------------
// Wave w does what wave w of forward_part does behind its W1 / W2 updates with the operands that wave packed; P6 stays on waves 4 - 7
// with the (ot, of0) mapping of forward_part.  One barrier per step: the partials alternate between two buffers, Q between three.
template <class BK, class HO>
TTT_WV_FN void output_role(BK& bk, HO& ho, const Mlp16ChunkParams& c, int bh) {
    const Mlp16Params& p = c.p;
    const int tid0 = bk.thread(), wv = bk.wave(), l0 = bk.lane();
    const int n0 = 32 * wv, img = B_IMG + wv * IMG_BYTES;
    const int NC = p.NC, head = bh % p.NH;
    const size_t tile0 = (size_t)bh * c.NCs + c.step0;
    const bool stager = wv < 2;       // waves 0, 1 move Q: one 16-byte chunk per thread
    const int lt0 = tid0 & 127, lofs = ((lt0 >> 3) * TS + (lt0 & 7) * 8) * 2;
    const size_t gofs = (size_t)(lt0 >> 3) * 64 + (lt0 & 7) * 8;
    if (tid0 < 64) {
        bk.template lds_store<float>(B_GAM + tid0 * 4, p.ln_w[(size_t)head * 64 + tid0]);
        bk.template lds_store<float>(B_BET + tid0 * 4, p.ln_b[(size_t)head * 64 + tid0]);
    }
    if (tid0 == 0) bk.template lds<unsigned>(B_POISON) = 0u;      // set when a poll of this workgroup gave up, or role A did
    u32x4 pfO = {0u, 0u, 0u, 0u};
    if (stager) {
        bk.template lds_store<u32x4>(B_Q + lofs, *reinterpret_cast<const u32x4*>(p.XQ + tile0 * 1024 + gofs));
        pfO = *reinterpret_cast<const u32x4*>(p.XQ + (tile0 + (NC > 1 ? 1 : 0)) * 1024 + gofs);
    }
    bool gave_up = false;
    bk.barrier();

    for (int it = 0; it < NC; ++it) {
        const size_t tile = tile0 + it;
        const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        const int tid = bk.opaque(tid0);
        const int ot = (tid & 255) >> 4, of0 = 4 * (tid & 15);
        const int Qt = B_Q + (it % 3) * TILE * 2, red = B_RED + (it & 1) * RED_BYTES;
        const size_t tn = tile0 + (it + 2 < NC ? it + 2 : NC - 1);
        u32x4 pfN = pfO;
        if (stager) pfN = *reinterpret_cast<const u32x4*>(p.XQ + tn * 1024 + gofs);

        // ---- wait for record it (every wave for itself, bounded)
        if (!gave_up) {
            if (!ho.wait_ge(FL_A, (unsigned)(it + 1))) {
                gave_up = true;
                if (l == 0) {
                    ho.fail(bh);
                    bk.template lds<unsigned>(B_POISON) = 1u;
                }
            }
            if (ho.peek(FL_A + 1) != 0u) {        // role A gave up on this workgroup (its ring was overwritten): poison from here on
                gave_up = true;
                if (l == 0) bk.template lds<unsigned>(B_POISON) = 1u;
            }
        }
        // ---- record it: this wave's fragments, its rows of b1', the owner's chunk of b2'
        const int soff = (it % RING) * REC_BYTES, vo = (wv * 4) * 1024 + l * 16;
        bf16x8 W1F[2][2], W2F[4];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) W1F[ks][nb] = __builtin_bit_cast(bf16x8, ho.load16(vo + (2 * ks + nb) * 1024, soff + REC_W1F));
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) W2F[fb] = __builtin_bit_cast(bf16x8, ho.load16(vo + fb * 1024, soff + REC_W2F));
        float b1v[2];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const f32x4 v = __builtin_bit_cast(f32x4, ho.load16((n0 + 16 * nb + (i & ~3)) * 4, soff + REC_B1));
            const int e = i & 3;
            b1v[nb] = e == 0 ? v[0] : e == 1 ? v[1] : e == 2 ? v[2] : v[3];
        }
        f32x4 b2o = zero4();
        if (wv >= 4) b2o = __builtin_bit_cast(f32x4, ho.load16(of0 * 4, soff + REC_B2));

        // Z1b = Q W1' + b1' ; X2b = gelu ; X2b image
        const bf16x8 qA0 = rho_read(bk, Qt, 0), qA1 = rho_read(bk, Qt, 32);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f32x4 Z = zero4();
            Z = bk.mma32(qA0, W1F[0][nb], Z);
            Z = bk.mma32(qA1, W1F[1][nb], Z);
#pragma unroll
            for (int r = 0; r < 4; ++r) Z[r] = gelu_fwd(bk, Z[r] + b1v[nb]);
            bk.template lds_store<bf16x4>(img + ((16 * nb + i) * IS + 4 * g) * 2, pack4(Z));
        }
        bk.lds_fence();
        // E: partial Z2b^T -> this step's partials buffer
        {
            const bf16x8 xB = cat(tr4(bk, img, IS, 0, 0), tr4(bk, img, IS, 16, 0));
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
                bk.template lds_store<f32x4>(red + ((wv * CS + i) * PS + 4 * g + 16 * fb) * 4, bk.mma32(W2F[fb], xB, zero4()));
        }
        // park Q of step it + 1 (its buffer was last read by P6 of step it - 2, in front of the barrier of step it - 1)
        if (stager) bk.template lds_store<u32x4>(B_Q + ((it + 1) % 3) * TILE * 2 + lofs, pfO);
        pfO = pfN;
        ho.drain();                   // every load of record it has landed before its slot is released
        bk.barrier();
        if (tid == 0) ho.post(FL_B, (unsigned)(it + 1));

        if (wv >= 4) {                // P6: owners - reduce, LayerNorm, residual -> XQW
            const f32x4 z = gather8_from(bk, b2o, red, ot, of0);
            float mu, rstd;
            row_stats(bk, z, p.eps, mu, rstd);
            const bf16x4 q = bk.template lds_load<bf16x4>(Qt + (ot * TS + of0) * 2);
            const f32x4 gm = bk.template lds_load<f32x4>(B_GAM + of0 * 4), bt = bk.template lds_load<f32x4>(B_BET + of0 * 4);
            const bool poisoned = bk.template lds<unsigned>(B_POISON) != 0u;
            bf16x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float y = (float)q[j] + gm[j] * ((z[j] - mu) * rstd) + bt[j];
                o[j] = (__bf16)(poisoned ? __builtin_nanf("") : y);
            }
            *reinterpret_cast<bf16x4*>(p.out + tile * 1024 + (size_t)ot * 64 + of0) = o;
        }
    }
}

}  // namespace pair
}  // namespace mlp16
}  // namespace ttt
