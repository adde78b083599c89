// TTT-Linear scans at mini-batches of 16 tokens (F = 64), written against a "wave backend" BK: one wavefront owns one
// (batch, head) scan - the whole state (W1 64x64 fp32 = 16 accumulator tiles, b1) fits its registers - so a step has no
// workgroup barrier at all.  The backend supplies the gfx950 primitives (ttt_mfma16.hip: DeviceWave) or, in the CPU tests,
// their lane-by-lane emulation (tests/emul/wave_emul.h), so the SAME body is what runs on the GPU and what the CPU suite
// checks against the oracle:
//   bk.lane()                       0..63
//   bk.mma32(a, b, c) / mma16       v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x16_bf16
//   bk.tr_read(byte_addr)           ds_read_b64_tr_b16
//   bk.lds<T>(byte_off)             reference into the wave's private LDS region ; bk.lds_ptr(byte_off) generic pointer to it
//   bk.lds_fence()                  ordering point between this wave's LDS writes and reads (free on the device)
//   bk.sum16(x)                     sum over the 16 lanes of a DPP row ; bk.xor_add(x, m) = x + x[lane ^ m]
//   bk.rsq(x), bk.opaque(i)
// Layout algebra (lane (g, i) = (l >> 4, l & 15)): a 16x16 fp32 tile holds D[4g + r][i], r = 0..3.  A tile X (rows = R,
// lane = C) is in place an mma16 operand contracting over R (k-slot e = row 4g + e) and, stacked with a second tile along
// R, an mma32 operand (k-slot (g, e) = row 4g + e of the first (e < 4) / second tile: "rho" order; the partner operand
// presents the same order from a row-major LDS tile with two 8-byte reads at columns c0 + 4g and c0 + 16 + 4g).  A
// contraction over the LANE index goes through an LDS image [lane index][row index] and transposed reads.
// Math: reference ops/ttt_linear.py:8-54 (forward, primal form), kernels/linear_backward.py:73-197 (backward structure),
// SURVEY.md Appendix A.
#pragma once
#include "ttt_wave_types.h"

#ifndef TTT_WV_FN
#define TTT_WV_FN inline
#endif

namespace ttt {
namespace lin16 {
using namespace ttt::wv;

constexpr int TS = 72;                       // row stride (elements) of a padded [16][64] bf16 tile
constexpr int TILE = 16 * TS;                // elements
constexpr int IS = 24;                       // row stride of an image [64 f][16 t] bf16
// wave-private LDS map (bytes)
constexpr int L_K = 0, L_V = L_K + 2 * TILE * 2, L_Q = L_V + 2 * TILE * 2, L_D = L_Q + 2 * TILE * 2;   // K, V, Q, dOut x 2 buffers
constexpr int L_IMG = L_D + 2 * TILE * 2;    // 2 images [64][IS] bf16
constexpr int IMG_BYTES = 64 * IS * 2;
constexpr int L_ETA = L_IMG + 2 * IMG_BYTES; // [2][16] fp32
constexpr int WAVE_LDS = L_ETA + 2 * 16 * 4;   // what forward() uses
// backward() only: a [64][TRS] bf16 image for transposing a 64 x 64 matrix of operand values, and the packed state that
// ends a checkpoint group (16 operand fragments x 64 lanes x 16 bytes)
constexpr int TRS = 72;
constexpr int L_TR = WAVE_LDS, L_WHI = L_TR + 64 * TRS * 2;
// (Keeping a group's per-step state slots in LDS instead of the caller's L2-resident scratch was measured in round 2 -
// 14.7 vs 13.9 ms per backward at the 3 s geometry - and removed.)
constexpr int WAVE_LDS_BWD = L_WHI + 16 * 1024;
static_assert(WAVE_LDS_BWD <= 160 * 1024, "LDS budget");
static_assert(WAVE_LDS % 16 == 0 && L_WHI % 16 == 0, "alignment");

TTT_WV_FN f32x4 zero4() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }
TTT_WV_FN bf16x4 pack4(f32x4 v) {
    bf16x4 r = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    return r;
}
TTT_WV_FN bf16x8 stack(f32x4 a, f32x4 b) {
    bf16x8 r = {(__bf16)a[0], (__bf16)a[1], (__bf16)a[2], (__bf16)a[3], (__bf16)b[0], (__bf16)b[1], (__bf16)b[2], (__bf16)b[3]};
    return r;
}
// a * b + c as ONE fused multiply-add, fixed in the source.  For the sums of two products in the reverse step of the backward in
// parts: left to the compiler, which of the two products is fused into the add depends on the code around the expression, and the
// part kernels have to round as the one-call kernels do (tests/test_linear_bwd_parts_gpu.py compares the bits).  The other product is
// passed as `c`, rounded.  (The emulator's host arithmetic fuses nothing, in backward() as here.)
TTT_WV_FN f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
#ifdef __HIP_DEVICE_COMPILE__
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(a[e], b[e], c[e]);
    return r;
#else
    return a * b + c;
#endif
}
TTT_WV_FN f32x4 splat4(float v) { f32x4 r = {v, v, v, v}; return r; }
TTT_WV_FN bf16x8 cat(bf16x4 lo, bf16x4 hi) { return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7); }

// rho-order operand (lane = this lane's row i of the tile, k = columns c0 .. c0 + 31) of a row-major [16][TS] LDS tile
template <class BK>
TTT_WV_FN bf16x8 rho_read(BK& bk, int tile_off, int c0) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
    const int o = tile_off + (i * TS + c0 + 4 * g) * 2;
    return cat(bk.template lds<bf16x4>(o), bk.template lds<bf16x4>(o + 32));
}
// transposed read: lane (g, i) gets img[row0 + 4g + e][col0 + i], e = 0..3   (operand with outer = column, k = row)
template <class BK>
TTT_WV_FN bf16x4 tr4(BK& bk, int img_off, int stride, int row0, int col0) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
    return bk.tr_read(img_off + ((row0 + 4 * g + (i >> 2)) * stride + col0 + 4 * (i & 3)) * 2);
}
// per-token-row reduction over the 64 features of tiles (rows = t, lane = f): in-lane over the 4 feature tiles, then the
// 16 lanes of the row
template <class BK>
TTT_WV_FN f32x4 rowsum64(BK& bk, const f32x4 (&v)[4]) {
    f32x4 s = v[0] + v[1] + v[2] + v[3];
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = bk.sum16(s[r]);
    return s;
}
// column sums over the 16 tokens of a (rows = t, lane = f) tile, in fp32: the lane's four rows, then the four row groups (lanes
// l ^ 16, l ^ 32) - replicated over the row groups like the first row of a ones-MFMA product.  Round 4: the bias gradients
// db1 are summed from the fp32 tiles instead of by a ones-MFMA over their bf16 packs (the same finding as in the TTT-MLP sweep,
// tests/test_rounding_budget_cpu.py: db enters d(eta) of every token of every earlier step).
template <class BK>
TTT_WV_FN float colsum16(BK& bk, const f32x4& v) {
    return bk.xor_add(bk.xor_add((v[0] + v[1]) + (v[2] + v[3]), 16), 32);
}
// (rows = t, lane = f) tiles -> [16 t][64 f] bf16 in global memory, 8 bytes per lane and feature block, through the [f][t]
// image `img_off`
template <class BK>
TTT_WV_FN void store_rows(BK& bk, int img_off, const f32x4 (&v)[4], __bf16* dst) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) bk.template lds<bf16x4>(img_off + ((16 * fb + i) * IS + 4 * g) * 2) = pack4(v[fb]);
    bk.lds_fence();
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
        *reinterpret_cast<bf16x4*>(dst + (size_t)i * 64 + 16 * fb + 4 * g) = tr4(bk, img_off, IS, 16 * fb, 0);
}
// one 2-KiB tile: 2 x 16 bytes per lane (rows l >> 3 and 8 + (l >> 3))
struct Stage {
    u32x4 lo, hi;
};
template <class BK>
TTT_WV_FN void stage_request(BK& bk, Stage& st, const __bf16* src_tile) {
    const int l = bk.lane();
    const __bf16* s = src_tile + (size_t)(l >> 3) * 64 + (l & 7) * 8;
    st.lo = *reinterpret_cast<const u32x4*>(s);
    st.hi = *reinterpret_cast<const u32x4*>(s + 512);
}
template <class BK>
TTT_WV_FN void stage_park(BK& bk, const Stage& st, int tile_off) {
    const int l = bk.lane();
    const int o = tile_off + ((l >> 3) * TS + (l & 7) * 8) * 2;
    bk.template lds<u32x4>(o) = st.lo;
    bk.template lds<u32x4>(o + 8 * TS * 2) = st.hi;
}

// LayerNorm statistics of z (rows = t, lane = f): z <- x_hat, returns 1/std per token row
template <class BK>
TTT_WV_FN f32x4 normalize_rows(BK& bk, f32x4 (&z)[4], float eps) {
    const f32x4 mu = rowsum64(bk, z) * (1.0f / 64.0f);
    f32x4 d2[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) { z[fb] -= mu; d2[fb] = z[fb] * z[fb]; }
    const f32x4 var = rowsum64(bk, d2) * (1.0f / 64.0f);
    f32x4 rstd;
#pragma unroll
    for (int r = 0; r < 4; ++r) rstd[r] = bk.rsq(var[r] + eps);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) z[fb] *= rstd;
    return rstd;
}


// Fused LayerNorm + L2-loss gradient of one mini-batch (ops/utils.py:17-45), tiles (rows = t, lane = f).
// in: z = Z1 (bias included), tg = V - K.  out: xh, go = gamma xh + beta - tg, gz = dl/dZ1, rstd, s2g = sum_f (go gamma) xh
struct InnerGrad {
    f32x4 xh[4], go[4], gz[4];
    f32x4 rstd, s2g;
};
template <class BK>
TTT_WV_FN void inner_grad(BK& bk, const f32x4 (&z)[4], const f32x4 (&tg)[4], const float (&gam)[4], const float (&bet)[4], float eps,
                          InnerGrad& o) {
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) o.xh[fb] = z[fb];
    o.rstd = normalize_rows(bk, o.xh, eps);
    f32x4 gxh[4], gxx[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        o.go[fb] = gam[fb] * o.xh[fb] + bet[fb] - tg[fb];
        gxh[fb] = o.go[fb] * gam[fb];
        gxx[fb] = gxh[fb] * o.xh[fb];
    }
    const f32x4 s1 = rowsum64(bk, gxh);
    o.s2g = rowsum64(bk, gxx);
    const f32x4 sc = o.rstd * (1.0f / 64.0f);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) o.gz[fb] = (64.0f * gxh[fb] - s1 - o.xh[fb] * o.s2g) * sc;
}

// ===================================================================================================================
// forward scan of (b, h) = bh over the steps [c.step0, c.step0 + c.p.NC) of a scan of c.NCs steps (Lin16ChunkParams,
// ttt_wave_types.h).  `it` counts the steps of the part; tiles and checkpoints are addressed in the whole sequence.  The
// hand-over between parts is the fp32 state the wave holds (W1t, b1v): the packed W1F is rebuilt from it every step, so a part
// that starts at any step reproduces the bits of the one-call scan.
template <class BK>
TTT_WV_FN void forward_part(BK& bk, const Lin16ChunkParams& c, int bh) {
    const Lin16Params& p = c.p;
    const int l0 = bk.lane();
    const int NC = p.NC, G = p.G, head = bh % p.NH, step0 = c.step0;

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
    Stage sk, sv, sq;
    unsigned short pe;
    stage_request(bk, sk, p.XK + tile0 * 1024);
    stage_request(bk, sv, p.XV + tile0 * 1024);
    stage_request(bk, sq, p.XQ + tile0 * 1024);
    pe = *reinterpret_cast<const unsigned short*>(p.eta + tile0 * 16 + (l0 & 15));
    stage_park(bk, sk, L_K); stage_park(bk, sv, L_V); stage_park(bk, sq, L_Q);
    if (l0 < 16) bk.template lds<float>(L_ETA + l0 * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
    bk.lds_fence();

    for (int it = 0; it < NC; ++it) {
        const size_t tile = tile0 + it;
        const int buf = it & 1;
        const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        const int Kt = L_K + buf * TILE * 2, Vt = L_V + buf * TILE * 2, Qt = L_Q + buf * TILE * 2;
        {   // next step's inputs, parked at the end of this step
            const size_t tn = tile0 + (it + 1 < NC ? it + 1 : it);
            stage_request(bk, sk, p.XK + tn * 1024);
            stage_request(bk, sv, p.XV + tn * 1024);
            stage_request(bk, sq, p.XQ + tn * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + tn * 16 + (l & 15));
        }
        if ((step0 + it) % G == 0) {      // checkpoint: state entering step `step0 + it` (linear_triton.py:84-97)
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
        const f32x4 eta4 = bk.template lds<f32x4>(L_ETA + (buf * 16 + 4 * g) * 4);          // eta of token rows 4g .. 4g+3
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
            store_rows(bk, L_IMG, y, p.out + tile * 1024);
        }
        const int nb = buf ^ 1;
        stage_park(bk, sk, L_K + nb * TILE * 2); stage_park(bk, sv, L_V + nb * TILE * 2); stage_park(bk, sq, L_Q + nb * TILE * 2);
        if (l < 16) bk.template lds<float>(L_ETA + (nb * 16 + l) * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
        bk.lds_fence();
    }
    if (c.W1f) {      // hand the state on.  May overwrite the initial state: this wave is the only reader of its (b, h)'s p.W1 /
                      // p.b1 and read all of it before the first step.  (Lane indices of its own: the loop's are not kept alive.)
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

// ===================================================================================================================
// backward of the scan of (b, h) = bh.  Checkpoint groups are walked from the last to the first; a group is first
// re-run forward, parking the state entering every step as packed MFMA operands in BOTH orientations in the caller's
// scratch (16 KiB per step = the W1_init_group storage; the state that ends the group goes to LDS), then walked in reverse
// carrying dW1, db1, dgamma, dbeta.  Products that contract over the feature a tile keeps in its LANES (dZ W^T, gZ1 dW^T)
// take their token-side operand from an LDS image + transposed reads and their weight-side operand from a transposed
// pack made the same way (one fp32 accumulator copy per matrix; a second, transposed accumulator copy was 128 registers
// too many for one wave).  Math: oracle/ttt_oracle.py:_lin_step_bwd.
constexpr int SLOT_BYTES = 16 * 1024;           // [16 operand fragments][64 lanes][16 bytes]: 0..7 (rows = f_in), 8..15 transposed

template <class BK>
TTT_WV_FN void st_pack(BK& bk, char* slot, int idx, bf16x8 v) { *reinterpret_cast<bf16x8*>(slot + ((size_t)idx * 64 + bk.lane()) * 16) = v; }
template <class BK>
TTT_WV_FN bf16x8 ld_pack(BK& bk, const char* slot, int idx) { return *reinterpret_cast<const bf16x8*>(slot + ((size_t)idx * 64 + bk.lane()) * 16); }

// token-side operand of a contraction over the features of X (rows = t, lane = f): lane = t, k = features 32ks .. 32ks+31
// in rho order, through the [f][t] image at img_off.  The packed X goes in (it is what the update MFMAs use as well).
template <class BK>
TTT_WV_FN void image_of(BK& bk, int img_off, const bf16x4 (&xp)[4], bf16x8 (&a)[2]) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) bk.template lds<bf16x4>(img_off + ((16 * fb + i) * IS + 4 * g) * 2) = xp[fb];
    bk.lds_fence();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) a[ks] = cat(tr4(bk, img_off, IS, 32 * ks, 0), tr4(bk, img_off, IS, 32 * ks + 16, 0));
}
// weight-side operands of a contraction over the f_out index of M (tiles T[fa][fb]: rows = f_in, lane = f_out):
// out[ks][fa]: lane = f_in of block fa, k = f_out in [32ks, 32ks + 32) in rho order.  Image [f_out][f_in] at L_TR.
template <class BK>
TTT_WV_FN void transposed_packs(BK& bk, const f32x4 (&T)[4][4], bf16x8 (&out)[2][4]) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fa = 0; fa < 4; ++fa)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) bk.template lds<bf16x4>(L_TR + ((16 * fb + i) * TRS + 16 * fa + 4 * g) * 2) = pack4(T[fa][fb]);
    bk.lds_fence();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) out[ks][fa] = cat(tr4(bk, L_TR, TRS, 32 * ks, 16 * fa), tr4(bk, L_TR, TRS, 32 * ks + 16, 16 * fa));
}

// ---- the pieces of the backward in parts (recompute_groups / sweep_groups, behind backward() below): the state loads, the recompute
// step and the reverse step of backward() as functions.  backward() itself keeps its steps inline: moving them into these functions
// was tried and changed which products its compiled code fuses into multiply-adds, i.e. the bits of an existing kernel.  The
// arithmetic here is backward()'s, statement by statement; where the source leaves the compiler a choice of fused product (sums of
// two products), fma4 fixes the one backward()'s compiled code takes, so that the parts round as the one call does. --------------
static_assert(LIN_PART_SLOT_BYTES == SLOT_BYTES + 64 * sizeof(float), "a slot of the backward in parts: packed state + bias row");

struct BwdConsts {
    float gam[4], bet[4];
    bf16x4 ONES, IDP, IDN;    // ones / +-identity as mma16 A operand (lane = t = i, k-slot e = token 4g + e)
    float eps;
};
// what a sweep carries from step to step
struct BwdCarry {
    f32x4 dWt[4][4];      // [fa][fb]  dW1[16fa + 4g + r][16fb + i]    (rows = f_in, lane = f_out)
    float db[4];          // db1[16fb + i]
    float dgam[4], dbet[4];     // per-lane partial sums over this lane's token rows
};
template <class BK>
TTT_WV_FN void bwd_consts(BK& bk, const Lin16Params& p, int head, BwdConsts& c) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        c.gam[fb] = p.ln_w[(size_t)head * 64 + 16 * fb + i];
        c.bet[fb] = p.ln_b[(size_t)head * 64 + 16 * fb + i];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        c.ONES[e] = (__bf16)1.0f;
        c.IDP[e] = (__bf16)((4 * g + e) == i ? 1.0f : 0.0f);
        c.IDN[e] = (__bf16)((4 * g + e) == i ? -1.0f : 0.0f);
    }
    c.eps = p.eps;
}
// a [64][64] fp32 matrix in global memory <-> tiles T[fa][fb] (rows = f_in, lane = f_out) ; a [64] row <-> v[fb] (lane = f)
template <class BK>
TTT_WV_FN void load_matrix(BK& bk, const float* M, f32x4 (&T)[4][4]) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fa = 0; fa < 4; ++fa)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 4; ++r) T[fa][fb][r] = M[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * fb + i];
}
template <class BK>
TTT_WV_FN void store_matrix(BK& bk, float* M, const f32x4 (&T)[4][4]) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fa = 0; fa < 4; ++fa)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int r = 0; r < 4; ++r) M[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * fb + i] = T[fa][fb][r];
}
template <class BK>
TTT_WV_FN void load_row(BK& bk, const float* v, float (&o)[4]) {
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) o[fb] = v[16 * fb + (bk.lane() & 15)];
}
// parks the state W1t as packed operands in both orientations at `slot` ; WF: the packs the forward step takes
template <class BK>
TTT_WV_FN void park_state(BK& bk, const f32x4 (&W1t)[4][4], char* slot, bf16x8 (&WF)[2][4]) {
    bf16x8 WT[2][4];
    transposed_packs(bk, W1t, WT);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            WF[ks][f] = stack(W1t[2 * ks][f], W1t[2 * ks + 1][f]);
            st_pack(bk, slot, ks * 4 + f, WF[ks][f]);
            st_pack(bk, slot, 8 + ks * 4 + f, WT[ks][f]);
        }
}
// one recomputed step (same arithmetic as forward_part): K, V tiles at Kt, Vt, eta at eta_off, WF the packed entering state ;
// W1t, b1v: the state entering the step -> the state after it.  `l`: the lane index the step loop made opaque.
template <class BK>
TTT_WV_FN void recompute_step(BK& bk, int l, const BwdConsts& c, int Kt, int Vt, int eta_off, const bf16x8 (&WF)[2][4],
                              f32x4 (&W1t)[4][4], float (&b1v)[4]) {
    const int g = l >> 4;
    const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
    const f32x4 eta4 = bk.template lds<f32x4>(eta_off + 4 * g * 4);
    bf16x4 kT[4];
    f32x4 z[4], tg[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        kT[fb] = tr4(bk, Kt, TS, 0, 16 * fb);
        f32x4 a = zero4();
        a = bk.mma32(kA0, WF[0][fb], a);
        a = bk.mma32(kA1, WF[1][fb], a);
        z[fb] = a + b1v[fb];
        tg[fb] = bk.mma16(c.IDN, kT[fb], bk.mma16(c.IDP, tr4(bk, Vt, TS, 0, 16 * fb), zero4()));
    }
    bf16x4 gzp[4];
    {
        InnerGrad ig;
        inner_grad(bk, z, tg, c.gam, c.bet, c.eps, ig);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) gzp[fb] = pack4(ig.gz[fb] * (-eta4));
    }
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        b1v[fb] += bk.mma16(c.ONES, gzp[fb], zero4())[0];
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) W1t[fa][fb] = bk.mma16(kT[fa], gzp[fb], W1t[fa][fb]);
    }
}
// one step of the reverse walk.  Tiles of the step at Kt, Vt, Qt, Dt, eta at eta_off ; slot / b1v: the state entering the step,
// slot_n / b1n: the state after it ; y: the carried gradients, entering as those of the state after the step, leaving as those of
// the state entering it ; deta, dXQ, dXK, dXV of the step go to tile `tile` of the whole sequence.  `mid()` runs between the outer
// LayerNorm backward and the inner step: where the caller parks the tiles it requested for the next step into the buffers this
// step does not use.  Ends with the carried update (10); the caller fences LDS behind it.
template <class BK, class Mid>
TTT_WV_FN void reverse_step(BK& bk, int l, const Lin16Params& p, const BwdConsts& c, BwdCarry& y, size_t tile, int Kt, int Vt, int Qt,
                            int Dt, int eta_off, const char* slot, const char* slot_n, const float (&b1v)[4], const float (&b1n)[4],
                            Mid&& mid) {
    const int g = l >> 4, i = l & 15;
    const f32x4 eta4 = bk.template lds<f32x4>(eta_off + 4 * g * 4);
    // ---- (2) outer LayerNorm backward: Z1b = Q W1n + b1n ; dZ1b -----------------------------------------------------------
    bf16x4 qT[4], dZbp[4];
    f32x4 dq[4];                     // starts as dOut (accumulator layout), becomes dQ
    {
        const bf16x8 qA0 = rho_read(bk, Qt, 0), qA1 = rho_read(bk, Qt, 32);
        f32x4 yy[4], dxl[4], t2[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            qT[fb] = tr4(bk, Qt, TS, 0, 16 * fb);
            f32x4 a = zero4();
            a = bk.mma32(qA0, ld_pack(bk, slot_n, fb), a);
            a = bk.mma32(qA1, ld_pack(bk, slot_n, 4 + fb), a);
            yy[fb] = a + b1n[fb];
            dq[fb] = bk.mma16(c.IDP, tr4(bk, Dt, TS, 0, 16 * fb), zero4());                     // exact dOut
        }
        const f32x4 rstdl = normalize_rows(bk, yy, c.eps);                                    // yy <- x_hat of the output LN
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dx = dq[fb] * yy[fb];
            y.dgam[fb] += dx[0] + dx[1] + dx[2] + dx[3];
            y.dbet[fb] += dq[fb][0] + dq[fb][1] + dq[fb][2] + dq[fb][3];
            dxl[fb] = dq[fb] * c.gam[fb];
            t2[fb] = dxl[fb] * yy[fb];
        }
        const f32x4 u1 = rowsum64(bk, dxl), u2 = rowsum64(bk, t2);
        const f32x4 sc = rstdl * (1.0f / 64.0f);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dzb = (64.0f * dxl[fb] - u1 - yy[fb] * u2) * sc;
            dZbp[fb] = pack4(dzb);
            y.db[fb] += colsum16(bk, dzb);                                                      // db1n += colsum dZ1b (fp32)
        }
    }
    // ---- (3) dW1n += Q^T dZ1b ; db1n += colsum dZ1b ------------------------------------------------------------------------------
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) y.dWt[fa][fb] = bk.mma16(qT[fa], dZbp[fb], y.dWt[fa][fb]);
    }
    // ---- (4) dQ = dOut + dZ1b W1n^T ------------------------------------------------------------------------------------------------
    {
        bf16x8 aZ[2];
        image_of(bk, L_IMG, dZbp, aZ);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            dq[fa] = bk.mma32(aZ[0], ld_pack(bk, slot_n, 8 + fa), dq[fa]);
            dq[fa] = bk.mma32(aZ[1], ld_pack(bk, slot_n, 12 + fa), dq[fa]);
        }
        store_rows(bk, L_IMG + IMG_BYTES, dq, p.dXQ + tile * 1024);
    }
    mid();
    bk.lds_fence();
    // ---- (1) inner forward of the step: Z1 = K W + b, LN / L2 gradient ------------------------------------------------
    const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
    bf16x4 kT[4];
    InnerGrad ig;
    {
        f32x4 z[4], tg[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            kT[fb] = tr4(bk, Kt, TS, 0, 16 * fb);
            f32x4 a = zero4();
            a = bk.mma32(kA0, ld_pack(bk, slot, fb), a);
            a = bk.mma32(kA1, ld_pack(bk, slot, 4 + fb), a);
            z[fb] = a + b1v[fb];
            tg[fb] = bk.mma16(c.IDN, kT[fb], bk.mma16(c.IDP, tr4(bk, Vt, TS, 0, 16 * fb), zero4()));   // exact V - K
        }
        inner_grad(bk, z, tg, c.gam, c.bet, c.eps, ig);
    }
    bk.lds_fence();
    // ---- (6) dgZ1 = -eta (K dW1n + db1n) ; (8) backward of the fused LN / L2 gradient -> dZ1, dt, dgamma, dbeta -----------------
    bf16x4 dZ1p[4];
    float dbz[4];                        // colsum dZ1 (fp32), added to db1 in (10) - d(eta) in (7) needs db1n
    f32x4 dk[4];                     // starts as -dt (dt = gradient w.r.t. the target V - K = dV)
    {
        f32x4 dgz[4], mGr[4], t2[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            f32x4 a = zero4();
            a = bk.mma32(kA0, stack(y.dWt[0][fb], y.dWt[1][fb]), a);
            a = bk.mma32(kA1, stack(y.dWt[2][fb], y.dWt[3][fb]), a);
            dgz[fb] = (a + y.db[fb]) * (-eta4);
            mGr[fb] = dgz[fb] * (-ig.rstd);
            t2[fb] = mGr[fb] * ig.xh[fb];
        }
        const f32x4 s1 = rowsum64(bk, mGr) * (1.0f / 64.0f), s2 = rowsum64(bk, t2) * (1.0f / 64.0f);
        const f32x4 c2 = ig.s2g * (1.0f / 64.0f);
        f32x4 dxh[4], dstd[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dgxh = fma4(dgz[fb], ig.rstd, s1) + ig.xh[fb] * s2;
            const f32x4 dy = dgxh * c.gam[fb];
            const f32x4 dg = fma4(ig.go[fb], dgxh, dy * ig.xh[fb]);
            y.dgam[fb] += dg[0] + dg[1] + dg[2] + dg[3];
            y.dbet[fb] += dy[0] + dy[1] + dy[2] + dy[3];
            dk[fb] = dy;                                                                       // = -dt
            dxh[fb] = fma4(ig.go[fb] * c.gam[fb], s2, dy * c.gam[fb]) + mGr[fb] * c2;
            dstd[fb] = fma4(dgz[fb], ig.gz[fb], dxh[fb] * ig.xh[fb]) * (-ig.rstd);
        }
        const f32x4 v1 = rowsum64(bk, dxh) * (1.0f / 64.0f), v2 = rowsum64(bk, dstd) * (1.0f / 64.0f);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dz1 = fma4(dxh[fb] - v1, ig.rstd, ig.xh[fb] * v2);
            dZ1p[fb] = pack4(dz1);
            dbz[fb] = colsum16(bk, dz1);
        }
        f32x4 dv[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) dv[fb] = -dk[fb];
        store_rows(bk, L_IMG + IMG_BYTES, dv, p.dXV + tile * 1024);                              // dV = dt
    }
    bk.lds_fence();
    // ---- (5, 7, 9) A1 = gZ1 dW1n^T ; d eta ; dK = -eta A1 - dt + dZ1 W^T --------------------------------------------------------------
    {
        bf16x8 dWT[2][4];
        transposed_packs(bk, y.dWt, dWT);
        bf16x4 gzq[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) gzq[fb] = pack4(ig.gz[fb]);
        bf16x8 aG[2];
        image_of(bk, L_IMG, gzq, aG);
        f32x4 acc[4];
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            f32x4 a1 = zero4();
            a1 = bk.mma32(aG[0], dWT[0][fa], a1);
            a1 = bk.mma32(aG[1], dWT[1][fa], a1);
            dk[fa] -= a1 * eta4;
            const f32x4 kc = bk.mma16(c.IDP, kT[fa], zero4());                                  // exact K, accumulator layout
            acc[fa] = fma4(ig.gz[fa], splat4(y.db[fa]), kc * a1);
        }
        const f32x4 de = rowsum64(bk, acc);
        if (i == 0) *reinterpret_cast<bf16x4*>(p.deta + tile * 16 + 4 * g) = pack4(-de);
    }
    bk.lds_fence();
    {
        bf16x8 aD[2];
        image_of(bk, L_IMG, dZ1p, aD);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            dk[fa] = bk.mma32(aD[0], ld_pack(bk, slot, 8 + fa), dk[fa]);
            dk[fa] = bk.mma32(aD[1], ld_pack(bk, slot, 12 + fa), dk[fa]);
        }
        store_rows(bk, L_IMG + IMG_BYTES, dk, p.dXK + tile * 1024);
    }
    // ---- (10) dW1 = dW1n + K^T dZ1 ; db1 = db1n + colsum dZ1 --------------------------------------------------------------------------------
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        y.db[fb] += dbz[fb];
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) y.dWt[fa][fb] = bk.mma16(kT[fa], dZ1p[fb], y.dWt[fa][fb]);
    }
}
// dgamma / dbeta of (b, h): the per-lane partial sums over the four row groups
template <class BK>
TTT_WV_FN void store_ln_grads(BK& bk, const Lin16Params& p, int bh, const BwdCarry& y) {
    const int g = bk.lane() >> 4, i = bk.lane() & 15;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const float dg = bk.xor_add(bk.xor_add(y.dgam[fb], 16), 32), dbt = bk.xor_add(bk.xor_add(y.dbet[fb], 16), 32);
        if (g == 0) {
            p.dln_w[(size_t)bh * 64 + 16 * fb + i] = dg;
            p.dln_b[(size_t)bh * 64 + 16 * fb + i] = dbt;
        }
    }
}
// the eta row of a step: 16 bf16 in global memory -> fp32 in LDS
template <class BK>
TTT_WV_FN void park_eta(BK& bk, int l, unsigned short pe, int eta_off) {
    if (l < 16) bk.template lds<float>(eta_off + l * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
}

template <class BK>
TTT_WV_FN void backward(BK& bk, const Lin16Params& p, int bh) {
    const int l0 = bk.lane();
    const int NC = p.NC, G = p.G, K = p.K, head = bh % p.NH;
    const size_t tile0 = (size_t)bh * NC;
    char* scr_w = p.scratch_w + (size_t)bh * G * SLOT_BYTES;
    float* scr_b = p.scratch_b + (size_t)bh * G * 64;

    float gam[4], bet[4];
    f32x4 dWt[4][4];      // [fa][fb]  dW1[16fa + 4g + r][16fb + i]    (rows = f_in, lane = f_out)
    float db[4];          // db1[16fb + i]
    float dgam[4] = {0.f, 0.f, 0.f, 0.f}, dbet[4] = {0.f, 0.f, 0.f, 0.f};     // per-lane partial sums over this lane's token rows
    {
        const int g = l0 >> 4, i = l0 & 15;
        const float* dWl = p.dW1_last + (size_t)bh * 64 * 64;
#pragma unroll
        for (int fa = 0; fa < 4; ++fa)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                for (int r = 0; r < 4; ++r) dWt[fa][fb][r] = dWl[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * fb + i];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            db[fb] = p.db1_last[(size_t)bh * 64 + 16 * fb + i];
            gam[fb] = p.ln_w[(size_t)head * 64 + 16 * fb + i];
            bet[fb] = p.ln_b[(size_t)head * 64 + 16 * fb + i];
        }
    }
    const bf16x4 ONES = {(__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f};
    bf16x4 IDP, IDN;
    {
        const int g = l0 >> 4, i = l0 & 15;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            IDP[e] = (__bf16)((4 * g + e) == i ? 1.0f : 0.0f);
            IDN[e] = (__bf16)((4 * g + e) == i ? -1.0f : 0.0f);
        }
    }
    // tiles of step s live in buffer (s & 1) of their kind; eta likewise
    Stage sk, sv, sq, sd;
    unsigned short pe = 0;
    {   // first tiles of the last group's recompute pass
        const int s0 = (K - 1) * G;
        stage_request(bk, sk, p.XK + (tile0 + s0) * 1024);
        stage_request(bk, sv, p.XV + (tile0 + s0) * 1024);
        pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + s0) * 16 + (l0 & 15));
        stage_park(bk, sk, L_K + (s0 & 1) * TILE * 2);
        stage_park(bk, sv, L_V + (s0 & 1) * TILE * 2);
        if (l0 < 16) bk.template lds<float>(L_ETA + ((s0 & 1) * 16 + l0) * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
        bk.lds_fence();
    }

    for (int k = K - 1; k >= 0; --k) {
        const int lo = k * G, hi = (lo + G < NC) ? lo + G : NC;
        float b1hi[4];                       // bias that ends the group
        // ================= re-run the group forward, parking the state entering each step ================================
        {
            f32x4 W1t[4][4];                 // [fa][fb] (rows = f_in, lane = f_out)
            float b1v[4];
            {
                const int g = l0 >> 4, i = l0 & 15;
                const float* W1g = p.W1c + ((size_t)bh * K + k) * 64 * 64;
#pragma unroll
                for (int fa = 0; fa < 4; ++fa)
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) W1t[fa][fb][r] = W1g[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * fb + i];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) b1v[fb] = p.b1c[((size_t)bh * K + k) * 64 + 16 * fb + i];
            }
            for (int it = lo; it <= hi; ++it) {      // iteration hi only parks the state that ends the group
                const int buf = it & 1;
                const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
                const bool fin = (it == hi), last = (it + 1 == hi);
                bf16x8 WF[2][4];
                {
                    char* slot = fin ? bk.lds_ptr(L_WHI) : scr_w + (size_t)(it - lo) * SLOT_BYTES;
                    bf16x8 WT[2][4];
                    transposed_packs(bk, W1t, WT);
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                        for (int f = 0; f < 4; ++f) {
                            WF[ks][f] = stack(W1t[2 * ks][f], W1t[2 * ks + 1][f]);
                            st_pack(bk, slot, ks * 4 + f, WF[ks][f]);
                            st_pack(bk, slot, 8 + ks * 4 + f, WT[ks][f]);
                        }
                }
                if (fin) {
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) b1hi[fb] = b1v[fb];
                    bk.lds_fence();
                    break;
                }
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) scr_b[(size_t)(it - lo) * 64 + 16 * fb + i] = b1v[fb];       // every lane group: same value
                const int Kt = L_K + buf * TILE * 2, Vt = L_V + buf * TILE * 2;
                if (!last) {        // K, V, eta of the next step
                    stage_request(bk, sk, p.XK + (tile0 + it + 1) * 1024);
                    stage_request(bk, sv, p.XV + (tile0 + it + 1) * 1024);
                    pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + it + 1) * 16 + (l & 15));
                } else {            // Q, dOut of this step: the reverse pass starts here
                    stage_request(bk, sq, p.XQ + (tile0 + it) * 1024);
                    stage_request(bk, sd, p.dOut + (tile0 + it) * 1024);
                }
                // forward step (same arithmetic as forward())
                const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
                const f32x4 eta4 = bk.template lds<f32x4>(L_ETA + (buf * 16 + 4 * g) * 4);
                bf16x4 kT[4];
                f32x4 z[4], tg[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    kT[fb] = tr4(bk, Kt, TS, 0, 16 * fb);
                    f32x4 a = zero4();
                    a = bk.mma32(kA0, WF[0][fb], a);
                    a = bk.mma32(kA1, WF[1][fb], a);
                    z[fb] = a + b1v[fb];
                    tg[fb] = bk.mma16(IDN, kT[fb], bk.mma16(IDP, tr4(bk, Vt, TS, 0, 16 * fb), zero4()));
                }
                bf16x4 gzp[4];
                {
                    InnerGrad ig;
                    inner_grad(bk, z, tg, gam, bet, p.eps, ig);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) gzp[fb] = pack4(ig.gz[fb] * (-eta4));
                }
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    b1v[fb] += bk.mma16(ONES, gzp[fb], zero4())[0];
#pragma unroll
                    for (int fa = 0; fa < 4; ++fa) W1t[fa][fb] = bk.mma16(kT[fa], gzp[fb], W1t[fa][fb]);
                }
                if (!last) {
                    const int nb = (it + 1) & 1;
                    stage_park(bk, sk, L_K + nb * TILE * 2);
                    stage_park(bk, sv, L_V + nb * TILE * 2);
                    if (l < 16) bk.template lds<float>(L_ETA + (nb * 16 + l) * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
                } else {
                    stage_park(bk, sq, L_Q + buf * TILE * 2);
                    stage_park(bk, sd, L_D + buf * TILE * 2);
                }
                bk.lds_fence();
            }
        }

        // ================= reverse pass over the group ======================================================================
        for (int it = hi - 1; it >= lo; --it) {
            const size_t tile = tile0 + it;
            const int buf = it & 1;
            const int l = bk.opaque(l0), g = l >> 4, i = l & 15;
            const int Kt = L_K + buf * TILE * 2, Vt = L_V + buf * TILE * 2, Qt = L_Q + buf * TILE * 2, Dt = L_D + buf * TILE * 2;
            const int nxt = (it > lo) ? it - 1 : lo - G;          // step whose tiles are requested now (< 0: nothing left)
            if (nxt >= 0) {
                stage_request(bk, sk, p.XK + (tile0 + nxt) * 1024);
                stage_request(bk, sv, p.XV + (tile0 + nxt) * 1024);
                pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + nxt) * 16 + (l & 15));
                if (it > lo) {
                    stage_request(bk, sq, p.XQ + (tile0 + nxt) * 1024);
                    stage_request(bk, sd, p.dOut + (tile0 + nxt) * 1024);
                }
            }
            const char* slot = scr_w + (size_t)(it - lo) * SLOT_BYTES;                                   // state entering / after the step
            const char* slot_n = (it + 1 < hi) ? slot + SLOT_BYTES : bk.lds_ptr(L_WHI);
            const f32x4 eta4 = bk.template lds<f32x4>(L_ETA + (buf * 16 + 4 * g) * 4);
            float b1v[4], b1n[4];
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                b1v[fb] = scr_b[(size_t)(it - lo) * 64 + 16 * fb + i];
                b1n[fb] = (it + 1 < hi) ? scr_b[(size_t)(it + 1 - lo) * 64 + 16 * fb + i] : b1hi[fb];
            }

            // ---- (2) outer LayerNorm backward: Z1b = Q W1n + b1n ; dZ1b -----------------------------------------------------------
            bf16x4 qT[4], dZbp[4];
            f32x4 dq[4];                     // starts as dOut (accumulator layout), becomes dQ
            {
                const bf16x8 qA0 = rho_read(bk, Qt, 0), qA1 = rho_read(bk, Qt, 32);
                f32x4 y[4], dxl[4], t2[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    qT[fb] = tr4(bk, Qt, TS, 0, 16 * fb);
                    f32x4 a = zero4();
                    a = bk.mma32(qA0, ld_pack(bk, slot_n, fb), a);
                    a = bk.mma32(qA1, ld_pack(bk, slot_n, 4 + fb), a);
                    y[fb] = a + b1n[fb];
                    dq[fb] = bk.mma16(IDP, tr4(bk, Dt, TS, 0, 16 * fb), zero4());                     // exact dOut
                }
                const f32x4 rstdl = normalize_rows(bk, y, p.eps);                                     // y <- x_hat of the output LN
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 dx = dq[fb] * y[fb];
                    dgam[fb] += dx[0] + dx[1] + dx[2] + dx[3];
                    dbet[fb] += dq[fb][0] + dq[fb][1] + dq[fb][2] + dq[fb][3];
                    dxl[fb] = dq[fb] * gam[fb];
                    t2[fb] = dxl[fb] * y[fb];
                }
                const f32x4 u1 = rowsum64(bk, dxl), u2 = rowsum64(bk, t2);
                const f32x4 sc = rstdl * (1.0f / 64.0f);
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 dzb = (64.0f * dxl[fb] - u1 - y[fb] * u2) * sc;
                    dZbp[fb] = pack4(dzb);
                    db[fb] += colsum16(bk, dzb);                                                        // db1n += colsum dZ1b (fp32)
                }
            }
            // ---- (3) dW1n += Q^T dZ1b ; db1n += colsum dZ1b ------------------------------------------------------------------------------
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
#pragma unroll
                for (int fa = 0; fa < 4; ++fa) dWt[fa][fb] = bk.mma16(qT[fa], dZbp[fb], dWt[fa][fb]);
            }
            // ---- (4) dQ = dOut + dZ1b W1n^T ------------------------------------------------------------------------------------------------
            {
                bf16x8 aZ[2];
                image_of(bk, L_IMG, dZbp, aZ);
#pragma unroll
                for (int fa = 0; fa < 4; ++fa) {
                    dq[fa] = bk.mma32(aZ[0], ld_pack(bk, slot_n, 8 + fa), dq[fa]);
                    dq[fa] = bk.mma32(aZ[1], ld_pack(bk, slot_n, 12 + fa), dq[fa]);
                }
                store_rows(bk, L_IMG + IMG_BYTES, dq, p.dXQ + tile * 1024);
            }
            // The tiles requested at the top of the step are parked as early as their buffers allow: right here when they
            // belong to the other parity (idle during this step: the usual case), at the end of the step when the next group's
            // first step shares this step's parity (even group sizes).
            const bool park_early = nxt >= 0 && (nxt & 1) != buf;
            const bool park_late = nxt >= 0 && !park_early;
            if (park_early) {
                const int nb = nxt & 1;
                stage_park(bk, sk, L_K + nb * TILE * 2);
                stage_park(bk, sv, L_V + nb * TILE * 2);
                if (l < 16) bk.template lds<float>(L_ETA + (nb * 16 + l) * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
                if (it > lo) {
                    stage_park(bk, sq, L_Q + nb * TILE * 2);
                    stage_park(bk, sd, L_D + nb * TILE * 2);
                }
            }
            bk.lds_fence();
            // ---- (1) inner forward of the step: Z1 = K W + b, LN / L2 gradient ------------------------------------------------
            const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
            bf16x4 kT[4];
            InnerGrad ig;
            {
                f32x4 z[4], tg[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    kT[fb] = tr4(bk, Kt, TS, 0, 16 * fb);
                    f32x4 a = zero4();
                    a = bk.mma32(kA0, ld_pack(bk, slot, fb), a);
                    a = bk.mma32(kA1, ld_pack(bk, slot, 4 + fb), a);
                    z[fb] = a + b1v[fb];
                    tg[fb] = bk.mma16(IDN, kT[fb], bk.mma16(IDP, tr4(bk, Vt, TS, 0, 16 * fb), zero4()));   // exact V - K
                }
                inner_grad(bk, z, tg, gam, bet, p.eps, ig);
            }
            bk.lds_fence();
            // ---- (6) dgZ1 = -eta (K dW1n + db1n) ; (8) backward of the fused LN / L2 gradient -> dZ1, dt, dgamma, dbeta -----------------
            bf16x4 dZ1p[4];
            float dbz[4];                        // colsum dZ1 (fp32), added to db1 in (10) - d(eta) in (7) needs db1n
            f32x4 dk[4];                     // starts as -dt (dt = gradient w.r.t. the target V - K = dV)
            {
                f32x4 dgz[4], mGr[4], t2[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    f32x4 a = zero4();
                    a = bk.mma32(kA0, stack(dWt[0][fb], dWt[1][fb]), a);
                    a = bk.mma32(kA1, stack(dWt[2][fb], dWt[3][fb]), a);
                    dgz[fb] = (a + db[fb]) * (-eta4);
                    mGr[fb] = dgz[fb] * (-ig.rstd);
                    t2[fb] = mGr[fb] * ig.xh[fb];
                }
                const f32x4 s1 = rowsum64(bk, mGr) * (1.0f / 64.0f), s2 = rowsum64(bk, t2) * (1.0f / 64.0f);
                const f32x4 c2 = ig.s2g * (1.0f / 64.0f);
                f32x4 dxh[4], dstd[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 dgxh = dgz[fb] * ig.rstd + s1 + ig.xh[fb] * s2;
                    const f32x4 dy = dgxh * gam[fb];
                    const f32x4 dg = ig.go[fb] * dgxh + dy * ig.xh[fb];
                    dgam[fb] += dg[0] + dg[1] + dg[2] + dg[3];
                    dbet[fb] += dy[0] + dy[1] + dy[2] + dy[3];
                    dk[fb] = dy;                                                                       // = -dt
                    dxh[fb] = dy * gam[fb] + (ig.go[fb] * gam[fb]) * s2 + mGr[fb] * c2;
                    dstd[fb] = (dxh[fb] * ig.xh[fb] + dgz[fb] * ig.gz[fb]) * (-ig.rstd);
                }
                const f32x4 v1 = rowsum64(bk, dxh) * (1.0f / 64.0f), v2 = rowsum64(bk, dstd) * (1.0f / 64.0f);
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const f32x4 dz1 = (dxh[fb] - v1) * ig.rstd + ig.xh[fb] * v2;
                    dZ1p[fb] = pack4(dz1);
                    dbz[fb] = colsum16(bk, dz1);
                }
                f32x4 dv[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) dv[fb] = -dk[fb];
                store_rows(bk, L_IMG + IMG_BYTES, dv, p.dXV + tile * 1024);                              // dV = dt
            }
            bk.lds_fence();
            // ---- (5, 7, 9) A1 = gZ1 dW1n^T ; d eta ; dK = -eta A1 - dt + dZ1 W^T --------------------------------------------------------------
            {
                bf16x8 dWT[2][4];
                transposed_packs(bk, dWt, dWT);
                bf16x4 gzq[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) gzq[fb] = pack4(ig.gz[fb]);
                bf16x8 aG[2];
                image_of(bk, L_IMG, gzq, aG);
                f32x4 acc[4];
#pragma unroll
                for (int fa = 0; fa < 4; ++fa) {
                    f32x4 a1 = zero4();
                    a1 = bk.mma32(aG[0], dWT[0][fa], a1);
                    a1 = bk.mma32(aG[1], dWT[1][fa], a1);
                    dk[fa] -= a1 * eta4;
                    const f32x4 kc = bk.mma16(IDP, kT[fa], zero4());                                  // exact K, accumulator layout
                    acc[fa] = kc * a1 + ig.gz[fa] * db[fa];
                }
                const f32x4 de = rowsum64(bk, acc);
                if (i == 0) *reinterpret_cast<bf16x4*>(p.deta + tile * 16 + 4 * g) = pack4(-de);
            }
            bk.lds_fence();
            {
                bf16x8 aD[2];
                image_of(bk, L_IMG, dZ1p, aD);
#pragma unroll
                for (int fa = 0; fa < 4; ++fa) {
                    dk[fa] = bk.mma32(aD[0], ld_pack(bk, slot, 8 + fa), dk[fa]);
                    dk[fa] = bk.mma32(aD[1], ld_pack(bk, slot, 12 + fa), dk[fa]);
                }
                store_rows(bk, L_IMG + IMG_BYTES, dk, p.dXK + tile * 1024);
            }
            // ---- (10) dW1 = dW1n + K^T dZ1 ; db1 = db1n + colsum dZ1 --------------------------------------------------------------------------------
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                db[fb] += dbz[fb];
#pragma unroll
                for (int fa = 0; fa < 4; ++fa) dWt[fa][fb] = bk.mma16(kT[fa], dZ1p[fb], dWt[fa][fb]);
            }
            if (park_late) {                 // only K, V, eta of the next group's first step (it == lo)
                const int nb = nxt & 1;
                stage_park(bk, sk, L_K + nb * TILE * 2);
                stage_park(bk, sv, L_V + nb * TILE * 2);
                if (l < 16) bk.template lds<float>(L_ETA + (nb * 16 + l) * 4) = (float)*reinterpret_cast<const __bf16*>(&pe);
            }
            bk.lds_fence();
        }
    }
    // ---- results ---------------------------------------------------------------------------------------------------------
    {
        const int g = l0 >> 4, i = l0 & 15;
        float* dWg = p.dW1 + (size_t)bh * 64 * 64;
#pragma unroll
        for (int fa = 0; fa < 4; ++fa)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                for (int r = 0; r < 4; ++r) dWg[(size_t)(16 * fa + 4 * g + r) * 64 + 16 * fb + i] = dWt[fa][fb][r];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const float dg = bk.xor_add(bk.xor_add(dgam[fb], 16), 32), dbt = bk.xor_add(bk.xor_add(dbet[fb], 16), 32);
            if (g == 0) {
                p.db1[(size_t)bh * 64 + 16 * fb + i] = db[fb];
                p.dln_w[(size_t)bh * 64 + 16 * fb + i] = dg;
                p.dln_b[(size_t)bh * 64 + 16 * fb + i] = dbt;
            }
        }
    }
}

// ===================================================================================================================
// The backward in parts (Lin16BwdPartParams, ttt_wave_types.h).  The two halves of a checkpoint group's backward depend on
// different things: the recompute on the group's checkpoint alone - every group of a sequence can be recomputed at once -, the
// reverse walk on the gradient state the later groups leave.  recompute_groups is the first half, one wave per (b, h, group) of the
// range, sweep_groups the second, one wave per (b, h) over the range; both run the steps of backward() above (as the functions
// park_state / recompute_step / reverse_step), and the state a step reads is the same packed operands (a slot of the workspace
// instead of the scratch / L_WHI), so the gradients are the bits of the one call however the K groups are cut into ranges.
//
// wave `bhk` = bh * nk + j recomputes group k0 + j of (b, h) = bh: slots 0 .. steps of the group, each with its bias row
template <class BK>
TTT_WV_FN void recompute_groups(BK& bk, const Lin16BwdPartParams& q, int bhk) {
    const Lin16Params& p = q.p;
    const int l0 = bk.lane();
    const int NC = p.NC, G = p.G, K = p.K;
    const int bh = bhk / q.nk, k = q.k0 + bhk % q.nk, head = bh % p.NH;
    const int lo = k * G, hi = (lo + G < NC) ? lo + G : NC;
    const size_t tile0 = (size_t)bh * NC;
    char* slots = q.slots + (size_t)bhk * (G + 1) * LIN_PART_SLOT_BYTES;

    BwdConsts c;
    bwd_consts(bk, p, head, c);
    f32x4 W1t[4][4];
    float b1v[4];
    load_matrix(bk, p.W1c + ((size_t)bh * K + k) * 64 * 64, W1t);
    load_row(bk, p.b1c + ((size_t)bh * K + k) * 64, b1v);
    Stage sk, sv;
    unsigned short pe;
    stage_request(bk, sk, p.XK + (tile0 + lo) * 1024);
    stage_request(bk, sv, p.XV + (tile0 + lo) * 1024);
    pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + lo) * 16 + (l0 & 15));
    stage_park(bk, sk, L_K + (lo & 1) * TILE * 2);
    stage_park(bk, sv, L_V + (lo & 1) * TILE * 2);
    park_eta(bk, l0, pe, L_ETA + (lo & 1) * 64);
    bk.lds_fence();
    for (int it = lo; it <= hi; ++it) {          // iteration hi only parks the state that ends the group
        const int buf = it & 1;
        const int l = bk.opaque(l0), i = l & 15;
        char* slot = slots + (size_t)(it - lo) * LIN_PART_SLOT_BYTES;
        bf16x8 WF[2][4];
        park_state(bk, W1t, slot, WF);
        if ((l >> 4) == 0)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) reinterpret_cast<float*>(slot + SLOT_BYTES)[16 * fb + i] = b1v[fb];
        if (it == hi) break;
        const bool last = (it + 1 == hi);
        if (!last) {        // K, V, eta of the next step
            stage_request(bk, sk, p.XK + (tile0 + it + 1) * 1024);
            stage_request(bk, sv, p.XV + (tile0 + it + 1) * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + it + 1) * 16 + (l & 15));
        }
        recompute_step(bk, l, c, L_K + buf * TILE * 2, L_V + buf * TILE * 2, L_ETA + buf * 64, WF, W1t, b1v);
        if (!last) {
            const int nb = buf ^ 1;
            stage_park(bk, sk, L_K + nb * TILE * 2);
            stage_park(bk, sv, L_V + nb * TILE * 2);
            park_eta(bk, l, pe, L_ETA + nb * 64);
        }
        bk.lds_fence();
    }
}

// the reverse walk of (b, h) = bh over the groups k0 + nk - 1 .. k0, from the slots recompute_groups left.  Carries dW1 / db1
// (q.p.dW1_last / db1_last -> q.p.dW1 / db1) and the un-reduced dgamma / dbeta partial sums (q.ln_carry) from the range behind it to
// the range in front of it; the range that holds group 0 also reduces the partial sums into dln_w / dln_b.  Consecutive steps
// alternate tile buffers, so the tiles of the step in front are always parked in the middle of a step (the park-late case of
// backward() - a next group whose first recomputed step shares the parity - does not arise: there is no recompute in between).
template <class BK>
TTT_WV_FN void sweep_groups(BK& bk, const Lin16BwdPartParams& q, int bh) {
    const Lin16Params& p = q.p;
    const int l0 = bk.lane();
    const int NC = p.NC, G = p.G, K = p.K, head = bh % p.NH;
    const int k0 = q.k0, nk = q.nk;
    const int s_lo = k0 * G, s_hi = ((k0 + nk) * G < NC) ? (k0 + nk) * G : NC;      // the steps [s_lo, s_hi)
    const size_t tile0 = (size_t)bh * NC;
    const char* slots = q.slots + (size_t)bh * nk * (G + 1) * LIN_PART_SLOT_BYTES;
    float* carry = q.ln_carry + (size_t)bh * LIN_PART_CARRY_FLOATS * 64 + l0;

    BwdConsts c;
    BwdCarry y;
    load_matrix(bk, p.dW1_last + (size_t)bh * 64 * 64, y.dWt);
    load_row(bk, p.db1_last + (size_t)bh * 64, y.db);
    bwd_consts(bk, p, head, c);
    if (k0 + nk == K) {      // the range that ends the sequence starts the sums
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) y.dgam[fb] = y.dbet[fb] = 0.f;
    } else {
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) { y.dgam[fb] = carry[fb * 64]; y.dbet[fb] = carry[(4 + fb) * 64]; }
    }
    Stage sk, sv, sq, sd;
    unsigned short pe = 0;
    {   // tiles of the first step of the walk: the combined kernel gets these from its recompute loop
        const int s0 = s_hi - 1, o = (s0 & 1) * TILE * 2;
        stage_request(bk, sk, p.XK + (tile0 + s0) * 1024);
        stage_request(bk, sv, p.XV + (tile0 + s0) * 1024);
        stage_request(bk, sq, p.XQ + (tile0 + s0) * 1024);
        stage_request(bk, sd, p.dOut + (tile0 + s0) * 1024);
        pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + s0) * 16 + (l0 & 15));
        stage_park(bk, sk, L_K + o); stage_park(bk, sv, L_V + o); stage_park(bk, sq, L_Q + o); stage_park(bk, sd, L_D + o);
        park_eta(bk, l0, pe, L_ETA + (s0 & 1) * 64);
        bk.lds_fence();
    }
    int k = k0 + nk - 1, lo = k * G;          // the group of step `it`
    for (int it = s_hi - 1; it >= s_lo; --it) {
        if (it < lo) { --k; lo -= G; }
        const int buf = it & 1, nb = buf ^ 1;
        const int l = bk.opaque(l0), i = l & 15;
        const bool more = it > s_lo;
        if (more) {
            stage_request(bk, sk, p.XK + (tile0 + it - 1) * 1024);
            stage_request(bk, sv, p.XV + (tile0 + it - 1) * 1024);
            stage_request(bk, sq, p.XQ + (tile0 + it - 1) * 1024);
            stage_request(bk, sd, p.dOut + (tile0 + it - 1) * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + it - 1) * 16 + (l & 15));
        }
        const char* slot = slots + ((size_t)(k - k0) * (G + 1) + (it - lo)) * LIN_PART_SLOT_BYTES;       // state entering the step
        const char* slot_n = slot + LIN_PART_SLOT_BYTES;                                                 // ... and after it
        float b1v[4], b1n[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            b1v[fb] = reinterpret_cast<const float*>(slot + SLOT_BYTES)[16 * fb + i];
            b1n[fb] = reinterpret_cast<const float*>(slot_n + SLOT_BYTES)[16 * fb + i];
        }
        reverse_step(bk, l, p, c, y, tile0 + it, L_K + buf * TILE * 2, L_V + buf * TILE * 2, L_Q + buf * TILE * 2, L_D + buf * TILE * 2,
                     L_ETA + buf * 64, slot, slot_n, b1v, b1n, [&] {
                         if (more) {
                             stage_park(bk, sk, L_K + nb * TILE * 2); stage_park(bk, sv, L_V + nb * TILE * 2);
                             stage_park(bk, sq, L_Q + nb * TILE * 2); stage_park(bk, sd, L_D + nb * TILE * 2);
                             park_eta(bk, l, pe, L_ETA + nb * 64);
                         }
                     });
        bk.lds_fence();
    }
    // ---- hand-over.  q.p.dW1 / db1 MAY ALIAS dW1_last / db1_last (the caller carries the gradient state in place): this wave is the
    // only reader of its (b, h)'s dW1_last / db1_last and read all of it before the first step.  ln_carry is read (above) and written
    // by the same lane only.
    store_matrix(bk, p.dW1 + (size_t)bh * 64 * 64, y.dWt);
    if ((l0 >> 4) == 0)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) p.db1[(size_t)bh * 64 + 16 * fb + (l0 & 15)] = y.db[fb];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) { carry[fb * 64] = y.dgam[fb]; carry[(4 + fb) * 64] = y.dbet[fb]; }
    if (k0 == 0) store_ln_grads(bk, p, bh, y);
}

// ===================================================================================================================
// A third stage of the backward in parts (Lin16BwdFrontParams, ttt_wave_types.h).  Of a reverse step, the blocks (2), (4) and (1)
// depend on the step's tiles and on the slots alone, not on the carried gradients: like the recompute they can run for every step of
// a range at once.  front_groups does that, one wave per (b, h, step): it stores the step's dXQ and leaves a RECORD of what the rest
// of the step takes from those blocks; chain_groups is the walk that remains - (3), (6), (8), (5/7/9), (10) - reading the records.
// front_step + chain_step are the statements of reverse_step, in its order per carried variable, so the bits are the one call's.
// A record: REC_FIELDS 16-byte fields per lane, field-major ([field][lane][16 bytes]: a wave's access to a field is contiguous).
constexpr int REC_DZB = 0;       // 2 fields: dZbp[0..3] (bf16x4 each)
constexpr int REC_CSUM = 2;      // colsum16(dzb)[fb]: the addends of db1
constexpr int REC_DGAM = 3, REC_DBET = 4;     // the addends of block (2) to the dgamma / dbeta partial sums, [fb]
constexpr int REC_XH = 5, REC_GO = 9, REC_GZ = 13;       // InnerGrad: 4 fields each
constexpr int REC_RSTD = 17, REC_S2G = 18;
constexpr int REC_FIELDS = 19;
static_assert(LIN_FRONT_RECORD_BYTES == (size_t)REC_FIELDS * 64 * 16, "a step record of the backward's front");

template <class BK, class T>
TTT_WV_FN void st_rec(BK& bk, char* rec, int idx, T v) {
    static_assert(sizeof(T) == 16, "a record field");
    *reinterpret_cast<T*>(rec + ((size_t)idx * 64 + bk.lane()) * 16) = v;
}
TTT_WV_FN f32x4 vec4(const float (&v)[4]) { f32x4 r = {v[0], v[1], v[2], v[3]}; return r; }

// inner_grad for front_step.  In the walk kernels the compiled inner_grad sums the four products gxh[fb] = go[fb] gamma[fb] of a row as
// fma(go1, gamma1, gxh0) and fuses on from there; on its own in the front kernel the compiler rounds gxh1 and fuses gxh0 instead.  So
// the sums of products - and, with them, the remaining expressions where a product meets an add - are written out with fma4 the way
// the walk kernels' code takes them.  (On the host a sum of rounded products either way: same bits.)
template <class BK>
TTT_WV_FN void inner_grad_pinned(BK& bk, const f32x4 (&z)[4], const f32x4 (&tg)[4], const float (&gam)[4], const float (&bet)[4], float eps,
                                 InnerGrad& o) {
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) o.xh[fb] = z[fb];
    o.rstd = normalize_rows(bk, o.xh, eps);
    f32x4 gxh[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        o.go[fb] = fma4(splat4(gam[fb]), o.xh[fb], splat4(bet[fb])) - tg[fb];
        gxh[fb] = o.go[fb] * gam[fb];
    }
    f32x4 s1 = fma4(o.go[1], splat4(gam[1]), gxh[0]);                     // gxh[0] + gxh[1] + gxh[2] + gxh[3]
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

// blocks (2), (4), (1) of reverse_step.  Tiles of the step at Kt, Vt, Qt, Dt ; slot / b1v: the state entering the step, slot_n / b1n:
// the state after it ; dXQ of the step goes to tile `tile`, everything the chain needs to `rec`.
template <class BK>
TTT_WV_FN void front_step(BK& bk, const Lin16Params& p, const BwdConsts& c, size_t tile, int Kt, int Vt, int Qt, int Dt, const char* slot,
                          const char* slot_n, const float (&b1v)[4], const float (&b1n)[4], char* rec) {
    // ---- (2) outer LayerNorm backward: Z1b = Q W1n + b1n ; dZ1b -----------------------------------------------------------
    bf16x4 dZbp[4];
    f32x4 dq[4];                     // starts as dOut (accumulator layout), becomes dQ
    {
        const bf16x8 qA0 = rho_read(bk, Qt, 0), qA1 = rho_read(bk, Qt, 32);
        f32x4 yy[4], dxl[4], t2[4];
        float addg[4], addb[4], csum[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            f32x4 a = zero4();
            a = bk.mma32(qA0, ld_pack(bk, slot_n, fb), a);
            a = bk.mma32(qA1, ld_pack(bk, slot_n, 4 + fb), a);
            yy[fb] = a + b1n[fb];
            dq[fb] = bk.mma16(c.IDP, tr4(bk, Dt, TS, 0, 16 * fb), zero4());                     // exact dOut
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
            dZbp[fb] = pack4(dzb);
            csum[fb] = colsum16(bk, dzb);
        }
        st_rec(bk, rec, REC_DZB, cat(dZbp[0], dZbp[1]));
        st_rec(bk, rec, REC_DZB + 1, cat(dZbp[2], dZbp[3]));
        st_rec(bk, rec, REC_CSUM, vec4(csum));
        st_rec(bk, rec, REC_DGAM, vec4(addg));
        st_rec(bk, rec, REC_DBET, vec4(addb));
    }
    // ---- (4) dQ = dOut + dZ1b W1n^T ------------------------------------------------------------------------------------------------
    {
        bf16x8 aZ[2];
        image_of(bk, L_IMG, dZbp, aZ);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            dq[fa] = bk.mma32(aZ[0], ld_pack(bk, slot_n, 8 + fa), dq[fa]);
            dq[fa] = bk.mma32(aZ[1], ld_pack(bk, slot_n, 12 + fa), dq[fa]);
        }
        store_rows(bk, L_IMG + IMG_BYTES, dq, p.dXQ + tile * 1024);
    }
    bk.lds_fence();
    // ---- (1) inner forward of the step: Z1 = K W + b, LN / L2 gradient ------------------------------------------------
    const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
    InnerGrad ig;
    {
        f32x4 z[4], tg[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const bf16x4 kT = tr4(bk, Kt, TS, 0, 16 * fb);
            f32x4 a = zero4();
            a = bk.mma32(kA0, ld_pack(bk, slot, fb), a);
            a = bk.mma32(kA1, ld_pack(bk, slot, 4 + fb), a);
            z[fb] = a + b1v[fb];
            tg[fb] = bk.mma16(c.IDN, kT, bk.mma16(c.IDP, tr4(bk, Vt, TS, 0, 16 * fb), zero4()));   // exact V - K
        }
        inner_grad_pinned(bk, z, tg, c.gam, c.bet, c.eps, ig);
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

// wave `unit` = bh * (steps of the range) + j runs the front of step k0 * G + j of (b, h) = bh, from the slots recompute_groups left
// for the same range: dXQ of the step and its record.  The tiles are parked once, in buffer 0 of their kind.
template <class BK>
TTT_WV_FN void front_groups(BK& bk, const Lin16BwdFrontParams& f, int unit) {
    const Lin16BwdPartParams& q = f.q;
    const Lin16Params& p = q.p;
    const int NC = p.NC, G = p.G;
    const int s_lo = q.k0 * G, s_hi = ((q.k0 + q.nk) * G < NC) ? (q.k0 + q.nk) * G : NC, ns = s_hi - s_lo;
    const int bh = unit / ns, it = s_lo + unit % ns, k = it / G, lo = k * G, head = bh % p.NH;
    const int i = bk.lane() & 15;
    const size_t tile = (size_t)bh * NC + it;
    const size_t cell = (size_t)bh * q.nk + (k - q.k0);                                             // (b, h, group of the range)
    const char* slot = q.slots + (cell * (G + 1) + (it - lo)) * LIN_PART_SLOT_BYTES;                // state entering the step
    const char* slot_n = slot + LIN_PART_SLOT_BYTES;                                                // ... and after it
    char* rec = f.records + (cell * G + (it - lo)) * LIN_FRONT_RECORD_BYTES;

    BwdConsts c;
    bwd_consts(bk, p, head, c);
    Stage sk, sv, sq, sd;
    stage_request(bk, sk, p.XK + tile * 1024);
    stage_request(bk, sv, p.XV + tile * 1024);
    stage_request(bk, sq, p.XQ + tile * 1024);
    stage_request(bk, sd, p.dOut + tile * 1024);
    float b1v[4], b1n[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        b1v[fb] = reinterpret_cast<const float*>(slot + SLOT_BYTES)[16 * fb + i];
        b1n[fb] = reinterpret_cast<const float*>(slot_n + SLOT_BYTES)[16 * fb + i];
    }
    stage_park(bk, sk, L_K); stage_park(bk, sv, L_V); stage_park(bk, sq, L_Q); stage_park(bk, sd, L_D);
    bk.lds_fence();
    front_step(bk, p, c, tile, L_K, L_V, L_Q, L_D, slot, slot_n, b1v, b1n, rec);
}

// The chain keeps two step records in the wave's LDS behind the transposing image (where backward() keeps the state that ends a group):
// the record of the step in front is fetched in three batches of fields while a step runs, each held in registers from one hook of
// chain_step to the next only.
constexpr int L_REC = L_WHI;
constexpr int WAVE_LDS_CHAIN = L_REC + 2 * (int)LIN_FRONT_RECORD_BYTES;
static_assert(WAVE_LDS_CHAIN <= 160 * 1024 && L_REC % 16 == 0, "LDS budget");
constexpr int REC_B0 = 0, REC_N0 = 7, REC_B1 = 7, REC_N1 = 6, REC_B2 = 13, REC_N2 = 6;       // the batches: first field, fields
static_assert(REC_B0 + REC_N0 == REC_B1 && REC_B1 + REC_N1 == REC_B2 && REC_B2 + REC_N2 == REC_FIELDS, "the batches cover a record");

template <int F0, int N, class BK>
TTT_WV_FN void rec_request(BK& bk, int l, const char* rec, u32x4 (&r)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = *reinterpret_cast<const u32x4*>(rec + ((size_t)(F0 + j) * 64 + l) * 16);
}
template <int F0, int N, class BK>
TTT_WV_FN void rec_park(BK& bk, int l, int rec_off, const u32x4 (&r)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) bk.template lds<u32x4>(rec_off + ((F0 + j) * 64 + l) * 16) = r[j];
}

// reverse_step without its blocks (2), (4), (1): their results come from the step's record, in LDS at rec_off.  Tiles of the step at
// Kt, Qt, eta at eta_off ; slot: the state entering the step (its transposed packs 8..15 only).  h0 / h1 / h2 run after (3), after (8)
// and after (10): where the caller moves what it fetches for the step in front.  The caller fences LDS behind the step.
template <class BK, class H0, class H1, class H2>
TTT_WV_FN void chain_step(BK& bk, int l, const Lin16Params& p, const BwdConsts& c, BwdCarry& y, size_t tile, int Kt, int Qt, int eta_off,
                          const char* slot, int rec_off, H0&& h0, H1&& h1, H2&& h2) {
    const int g = l >> 4, i = l & 15;
    const f32x4 eta4 = bk.template lds<f32x4>(eta_off + 4 * g * 4);
    const int ro = rec_off + l * 16;                  // this lane's cell of field 0
    // ---- what (2) adds to the carry ----------------------------------------------------------------------------------------------
    {
        const f32x4 addg = bk.template lds<f32x4>(ro + REC_DGAM * 1024), addb = bk.template lds<f32x4>(ro + REC_DBET * 1024);
        const f32x4 csum = bk.template lds<f32x4>(ro + REC_CSUM * 1024);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            y.dgam[fb] += addg[fb];
            y.dbet[fb] += addb[fb];
        }
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) y.db[fb] += csum[fb];                                   // db1n += colsum dZ1b (fp32)
    }
    // ---- (3) dW1n += Q^T dZ1b ; db1n += colsum dZ1b ------------------------------------------------------------------------------
    {
        const bf16x8 d01 = bk.template lds<bf16x8>(ro + REC_DZB * 1024), d23 = bk.template lds<bf16x8>(ro + (REC_DZB + 1) * 1024);
        const bf16x4 dZbp[4] = {__builtin_shufflevector(d01, d01, 0, 1, 2, 3), __builtin_shufflevector(d01, d01, 4, 5, 6, 7),
                                __builtin_shufflevector(d23, d23, 0, 1, 2, 3), __builtin_shufflevector(d23, d23, 4, 5, 6, 7)};
        bf16x4 qT[4];
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) qT[fa] = tr4(bk, Qt, TS, 0, 16 * fa);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
#pragma unroll
            for (int fa = 0; fa < 4; ++fa) y.dWt[fa][fb] = bk.mma16(qT[fa], dZbp[fb], y.dWt[fa][fb]);
        }
    }
    h0();
    const bf16x8 kA0 = rho_read(bk, Kt, 0), kA1 = rho_read(bk, Kt, 32);
    bf16x4 kT[4];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) kT[fb] = tr4(bk, Kt, TS, 0, 16 * fb);
    const f32x4 ig_rstd = bk.template lds<f32x4>(ro + REC_RSTD * 1024);
    // ---- (6) dgZ1 = -eta (K dW1n + db1n) ; (8) backward of the fused LN / L2 gradient -> dZ1, dt, dgamma, dbeta -----------------
    bf16x4 dZ1p[4];
    float dbz[4];                        // colsum dZ1 (fp32), added to db1 in (10) - d(eta) in (7) needs db1n
    f32x4 dk[4];                     // starts as -dt (dt = gradient w.r.t. the target V - K = dV)
    {
        f32x4 dgz[4], mGr[4], t2[4], xh[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            xh[fb] = bk.template lds<f32x4>(ro + (REC_XH + fb) * 1024);
            f32x4 a = zero4();
            a = bk.mma32(kA0, stack(y.dWt[0][fb], y.dWt[1][fb]), a);
            a = bk.mma32(kA1, stack(y.dWt[2][fb], y.dWt[3][fb]), a);
            dgz[fb] = (a + y.db[fb]) * (-eta4);
            mGr[fb] = dgz[fb] * (-ig_rstd);
            t2[fb] = mGr[fb] * xh[fb];
        }
        const f32x4 s1 = rowsum64(bk, mGr) * (1.0f / 64.0f), s2 = rowsum64(bk, t2) * (1.0f / 64.0f);
        const f32x4 c2 = bk.template lds<f32x4>(ro + REC_S2G * 1024) * (1.0f / 64.0f);
        f32x4 dxh[4], dstd[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 go = bk.template lds<f32x4>(ro + (REC_GO + fb) * 1024), gz = bk.template lds<f32x4>(ro + (REC_GZ + fb) * 1024);
            const f32x4 dgxh = fma4(dgz[fb], ig_rstd, s1) + xh[fb] * s2;
            const f32x4 dy = dgxh * c.gam[fb];
            const f32x4 dg = fma4(go, dgxh, dy * xh[fb]);
            y.dgam[fb] += dg[0] + dg[1] + dg[2] + dg[3];
            y.dbet[fb] += dy[0] + dy[1] + dy[2] + dy[3];
            dk[fb] = dy;                                                                       // = -dt
            dxh[fb] = fma4(go * c.gam[fb], s2, dy * c.gam[fb]) + mGr[fb] * c2;
            dstd[fb] = fma4(dgz[fb], gz, dxh[fb] * xh[fb]) * (-ig_rstd);
        }
        const f32x4 v1 = rowsum64(bk, dxh) * (1.0f / 64.0f), v2 = rowsum64(bk, dstd) * (1.0f / 64.0f);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            const f32x4 dz1 = fma4(dxh[fb] - v1, ig_rstd, xh[fb] * v2);
            dZ1p[fb] = pack4(dz1);
            dbz[fb] = colsum16(bk, dz1);
        }
        f32x4 dv[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) dv[fb] = -dk[fb];
        store_rows(bk, L_IMG + IMG_BYTES, dv, p.dXV + tile * 1024);                              // dV = dt
    }
    h1();
    bk.lds_fence();
    // ---- (5, 7, 9) A1 = gZ1 dW1n^T ; d eta ; dK = -eta A1 - dt + dZ1 W^T --------------------------------------------------------------
    {
        bf16x8 dWT[2][4];
        transposed_packs(bk, y.dWt, dWT);
        f32x4 gz[4];
        bf16x4 gzq[4];
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
            gz[fb] = bk.template lds<f32x4>(ro + (REC_GZ + fb) * 1024);
            gzq[fb] = pack4(gz[fb]);
        }
        bf16x8 aG[2];
        image_of(bk, L_IMG, gzq, aG);
        f32x4 acc[4];
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            f32x4 a1 = zero4();
            a1 = bk.mma32(aG[0], dWT[0][fa], a1);
            a1 = bk.mma32(aG[1], dWT[1][fa], a1);
            dk[fa] -= a1 * eta4;
            const f32x4 kc = bk.mma16(c.IDP, kT[fa], zero4());                                  // exact K, accumulator layout
            acc[fa] = fma4(gz[fa], splat4(y.db[fa]), kc * a1);
        }
        const f32x4 de = rowsum64(bk, acc);
        if (i == 0) *reinterpret_cast<bf16x4*>(p.deta + tile * 16 + 4 * g) = pack4(-de);
    }
    bk.lds_fence();
    {
        bf16x8 aD[2];
        image_of(bk, L_IMG, dZ1p, aD);
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) {
            dk[fa] = bk.mma32(aD[0], ld_pack(bk, slot, 8 + fa), dk[fa]);
            dk[fa] = bk.mma32(aD[1], ld_pack(bk, slot, 12 + fa), dk[fa]);
        }
        store_rows(bk, L_IMG + IMG_BYTES, dk, p.dXK + tile * 1024);
    }
    // ---- (10) dW1 = dW1n + K^T dZ1 ; db1 = db1n + colsum dZ1 --------------------------------------------------------------------------------
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        y.db[fb] += dbz[fb];
#pragma unroll
        for (int fa = 0; fa < 4; ++fa) y.dWt[fa][fb] = bk.mma16(kT[fa], dZ1p[fb], y.dWt[fa][fb]);
    }
    h2();
}

// the walk of (b, h) = bh over the groups k0 + nk - 1 .. k0 from the slots recompute_groups and the records front_groups left: the
// loop and the carry contract of sweep_groups (dW1_last / db1_last -> dW1 / db1, which may alias ; ln_carry ; dln_w / dln_b in the
// range with k0 == 0) around chain_step.  K, Q, eta and the record of the step in front are fetched while a step runs - none of their
// addresses depends on the carry - into the LDS buffers of the other parity.
template <class BK>
TTT_WV_FN void chain_groups(BK& bk, const Lin16BwdFrontParams& f, int bh) {
    const Lin16BwdPartParams& q = f.q;
    const Lin16Params& p = q.p;
    const int l0 = bk.lane();
    const int NC = p.NC, G = p.G, K = p.K, head = bh % p.NH;
    const int k0 = q.k0, nk = q.nk;
    const int s_lo = k0 * G, s_hi = ((k0 + nk) * G < NC) ? (k0 + nk) * G : NC;      // the steps [s_lo, s_hi)
    const size_t tile0 = (size_t)bh * NC;
    const char* slots = q.slots + (size_t)bh * nk * (G + 1) * LIN_PART_SLOT_BYTES;
    const char* recs = f.records + (size_t)bh * nk * G * LIN_FRONT_RECORD_BYTES;
    float* carry = q.ln_carry + (size_t)bh * LIN_PART_CARRY_FLOATS * 64 + l0;

    BwdConsts c;
    BwdCarry y;
    load_matrix(bk, p.dW1_last + (size_t)bh * 64 * 64, y.dWt);
    load_row(bk, p.db1_last + (size_t)bh * 64, y.db);
    bwd_consts(bk, p, head, c);
    if (k0 + nk == K) {      // the range that ends the sequence starts the sums
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) y.dgam[fb] = y.dbet[fb] = 0.f;
    } else {
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) { y.dgam[fb] = carry[fb * 64]; y.dbet[fb] = carry[(4 + fb) * 64]; }
    }
    int k = k0 + nk - 1, lo = k * G;          // the group of step `it`
    Stage sk, sq;
    unsigned short pe = 0;
    u32x4 r0[REC_N0], r1[REC_N1], r2[REC_N2];
    {   // the first step of the walk
        const int s0 = s_hi - 1, o = (s0 & 1) * TILE * 2, ro = L_REC + (s0 & 1) * (int)LIN_FRONT_RECORD_BYTES;
        const char* rec = recs + ((size_t)(k - k0) * G + (s0 - lo)) * LIN_FRONT_RECORD_BYTES;
        stage_request(bk, sk, p.XK + (tile0 + s0) * 1024);
        stage_request(bk, sq, p.XQ + (tile0 + s0) * 1024);
        pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + s0) * 16 + (l0 & 15));
        stage_park(bk, sk, L_K + o); stage_park(bk, sq, L_Q + o);
        park_eta(bk, l0, pe, L_ETA + (s0 & 1) * 64);
        rec_request<REC_B0, REC_N0>(bk, l0, rec, r0); rec_park<REC_B0, REC_N0>(bk, l0, ro, r0);
        rec_request<REC_B1, REC_N1>(bk, l0, rec, r1); rec_park<REC_B1, REC_N1>(bk, l0, ro, r1);
        rec_request<REC_B2, REC_N2>(bk, l0, rec, r2); rec_park<REC_B2, REC_N2>(bk, l0, ro, r2);
        bk.lds_fence();
    }
    for (int it = s_hi - 1; it >= s_lo; --it) {
        if (it < lo) { --k; lo -= G; }
        const int buf = it & 1, nb = buf ^ 1;
        const int l = bk.opaque(l0);
        const bool more = it > s_lo;
        const char* rec_n = recs;
        const int ro_n = L_REC + nb * (int)LIN_FRONT_RECORD_BYTES;
        if (more) {
            const int kn = (it - 1 < lo) ? k - 1 : k, lon = (it - 1 < lo) ? lo - G : lo;      // the group of the step in front
            rec_n = recs + ((size_t)(kn - k0) * G + (it - 1 - lon)) * LIN_FRONT_RECORD_BYTES;
            stage_request(bk, sk, p.XK + (tile0 + it - 1) * 1024);
            stage_request(bk, sq, p.XQ + (tile0 + it - 1) * 1024);
            pe = *reinterpret_cast<const unsigned short*>(p.eta + (tile0 + it - 1) * 16 + (l & 15));
            rec_request<REC_B0, REC_N0>(bk, l, rec_n, r0);
        }
        const char* slot = slots + ((size_t)(k - k0) * (G + 1) + (it - lo)) * LIN_PART_SLOT_BYTES;       // state entering the step
        chain_step(bk, l, p, c, y, tile0 + it, L_K + buf * TILE * 2, L_Q + buf * TILE * 2, L_ETA + buf * 64, slot,
                   L_REC + buf * (int)LIN_FRONT_RECORD_BYTES,
                   [&] {
                       if (more) {
                           stage_park(bk, sk, L_K + nb * TILE * 2); stage_park(bk, sq, L_Q + nb * TILE * 2);
                           park_eta(bk, l, pe, L_ETA + nb * 64);
                           rec_park<REC_B0, REC_N0>(bk, l, ro_n, r0);
                           rec_request<REC_B1, REC_N1>(bk, l, rec_n, r1);
                       }
                   },
                   [&] {
                       if (more) {
                           rec_park<REC_B1, REC_N1>(bk, l, ro_n, r1);
                           rec_request<REC_B2, REC_N2>(bk, l, rec_n, r2);
                       }
                   },
                   [&] {
                       if (more) rec_park<REC_B2, REC_N2>(bk, l, ro_n, r2);
                   });
        bk.lds_fence();
    }
    // ---- hand-over, as in sweep_groups: q.p.dW1 / db1 may alias dW1_last / db1_last ; ln_carry is read and written by the same lane
    store_matrix(bk, p.dW1 + (size_t)bh * 64 * 64, y.dWt);
    if ((l0 >> 4) == 0)
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) p.db1[(size_t)bh * 64 + 16 * fb + (l0 & 15)] = y.db[fb];
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) { carry[fb * 64] = y.dgam[fb]; carry[(4 + fb) * 64] = y.dbet[fb]; }
    if (k0 == 0) store_ln_grads(bk, p, bh, y);
}

}  // namespace lin16
}  // namespace ttt
