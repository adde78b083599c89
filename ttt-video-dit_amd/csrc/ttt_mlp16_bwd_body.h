// TTT-MLP BACKWARD at mini-batches of 16 tokens as a WORKGROUP body over the wave backend (ttt_mlp16_body.h: the forward scan and
// the layout algebra): WAVES waves per (b, h), each owning NS of the forward's eight 32-unit slices of the hidden units (slice
// v = NS w + s covers Hv = [32 v, 32 v + 32); shipped: eight waves of one slice, as the forward); the only synchronisation is the
// workgroup barrier.  The math is oracle/ttt_oracle.py::_mlp_step_bwd with the forward's eta folding (Gs = -eta gZ2).
//
// The checkpoint groups are walked from the last to the first; per group
//   recompute_group  the STATE-UPDATE HALF of the forward step (phases A1, A2, P3, C of ttt_mlp16_body.h without the output path;
//                    the same MFMA sequence and the same bf16 roundings) from the group's checkpoint; the fp32 state entering
//                    step j goes to slot j of the caller's four *_init_group buffers (mlp16::store_state: [B,NH,G,F,H],
//                    [B,NH,G,1,H], [B,NH,G,H,F], [B,NH,G,1,F]), so a slot holds the bits the forward scan held there.
//   sweep_group      the reverse walk over the group's steps from those slots, carrying dW1, db1, dW2, db2.
// Register plan of the reverse walk: the fp32 state AND its gradient in both tile orientations would be the whole register file of
// the CU, so only the gradient is carried, in ONE orientation - tiles (rows = f, lane = n) of dW1[:, Hv] and dW2[Hv, :]^T, 64
// registers per slice - and it is parked in the call's own dW1 .. db2 outputs between groups (the recompute needs the registers for
// the state; a call over K groups therefore does at every group boundary exactly what K chained calls do).  The state of a step is
// needed as bf16 MFMA operands only: B-form (k = f, column = n) is a stack of two (rows = f, lane = n) tiles, A-form (row = f,
// k = n) comes from the slice's private [32 n][TS] image of the packed tiles read back transposed.  The fp32 tiles are re-read from
// the slot (and W1n / W2n re-made by the forward's update) where a later phase needs them again; between phases a slice keeps
// bf16 tiles only.  The slices are the forward's, so the recompute leaves the forward's eight partial sums, summed in its order.
//
// Everything with a hidden dimension is wave-local.  Every [16, 64] row quantity goes through LDS in a fixed order: per-wave
// partials [f][t] -> red buffer [slice][t][PS], summed slice 0 .. 7 by the OWNER thread of (token ot, features of0 .. of0 + 3)
// (threads 0 - 255, 16 lanes per token), which computes the row-wise LayerNorm algebra and broadcasts its rows as bf16 tiles.
// Per reverse step (S* = workgroup barriers):
//   stage  K, V, Q, dOut, eta, b2                                                                                     S0
//   P1  Z1 = K W1 + b1 -> X2, D1 = gelu', DD1 = gelu'' ; partial Z2^T -> redA                                          S1
//   P2  owners: Z2, LayerNorm / L2 backward -> gZ2, Gs = -eta gZ2 (bf16 tiles)                                         S2
//   P3  gX2 = gZ2 W2^T, gZ1 = gX2 D1 ; W2n, b2n, W1n, b1n (the forward's update) ; Z1b = Q W1n + b1n -> X2b, D1b ;
//       partial Z2b^T -> redB                                                                                         S3
//   P4  owners: Z2b, output LayerNorm statistics ; dln += ; dZ2b (bf16 tile)                                           S4
//   P5  dX2b = dZ2b W2n^T, dZ1b = dX2b D1b ; dW2n, db2n, dW1n, db1n += ; partial (dQ - dOut)^T -> redA ;
//       A2 = gZ2 dW2n^T, dgZ1 = -eta (K dW1n + db1n), u = dgZ1 D1, dZ1 = dgZ1 gX2 DD1 - eta A2 D1 ;
//       partial dgZ2^T = dW2n^T (-eta X2)^T + W2^T u^T -> redB ; dW2 += u^T gZ2 ; per-slice share of d eta                S5
//   P6  owners: dgZ2 = sum - eta db2n ; second-order LayerNorm backward -> dZ2 (bf16 tile), dt ; dln += ; dV, dQ out     S6
//   P7  dZ1 += (dZ2 W2^T) D1 (the -eta A2 D1 share went in at P5) ; partial A1^T = dW1n (gZ1)^T -> redB ; partial (dZ1 W1^T)^T -> redA ;
//       dW1 += K^T dZ1, db1 +=, dW2 += X2^T dZ2, db2 +=                                                                 S7
//   P8  owners: dK = sum redA - eta A1 - dt ; d eta                                                                    S8
#pragma once
#include "ttt_mlp16_body.h"

// Between the blocks of a phase nothing may be moved by the compiler's scheduler: left alone it overlaps the blocks (and the slices
// of a wave) until every transient tile of a phase is live at once.
// The lane indices g, i are taken afresh (through bk.opaque) for every block as well: LDS addresses formed from them are then
// re-made where they are used instead of being kept - dozens of them - across the whole step, or across the whole kernel.
#if defined(__HIP_DEVICE_COMPILE__)
#define TTT_MLP16_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define TTT_MLP16_SCHED_FENCE() ((void)0)
#endif
#define TTT_MLP16_BLOCK_END() \
    do { TTT_MLP16_SCHED_FENCE(); l = bk.opaque(l0); g = l >> 4; i = l & 15; tid = bk.opaque(tid0); ot = (tid & 255) >> 4; of0 = 4 * (tid & 15); } while (0)

namespace ttt {
namespace mlp16 {
namespace bwd {

constexpr int WAVES = 8, NS = 1;             // waves per workgroup, 32-unit slices of the hidden units per wave (WAVES * NS = 8)
constexpr int TB = TILE * 2;                 // bytes of a padded [16][64] bf16 tile
constexpr int B_K = 0, B_V = B_K + 2 * TB, B_Q = B_V + 2 * TB, B_D = B_Q + TB, B_G = B_D + TB, B_GZ = B_G + TB, B_DZB = B_GZ + TB,
              B_DZ2 = B_DZB + TB;
constexpr int XIMG_BYTES = 32 * IS * 2, WIMG_BYTES = 32 * TS * 2;
constexpr int B_XIMG = B_DZ2 + TB, B_WIMG = B_XIMG + 8 * XIMG_BYTES;
constexpr int B_REDA = B_WIMG + 8 * WIMG_BYTES, B_REDB = B_REDA + RED_BYTES;
constexpr int B_ETA = B_REDB + RED_BYTES, B_B2 = B_ETA + 32 * 4, B_B2N = B_B2 + 64 * 4, B_DB2 = B_B2N + 64 * 4, B_GAM = B_DB2 + 64 * 4,
              B_BET = B_GAM + 64 * 4, B_DETA = B_BET + 64 * 4;
constexpr int B_DLNW = B_DETA + 8 * CS * 4, B_DLNB = B_DLNW + CS * 64 * 4;      // [16 t][64 f] fp32: the owners' running shares of dln_w / dln_b
constexpr int B_OGZ = B_DLNB + CS * 64 * 4;                                     // [16 t][64 f] fp32: gZ2 from P2 for the owner's P6
constexpr int GROUP_LDS_BWD = B_OGZ + CS * 64 * 4;
static_assert(GROUP_LDS_BWD <= 160 * 1024 && B_XIMG % 16 == 0 && B_WIMG % 16 == 0 && B_REDA % 16 == 0 && B_ETA % 16 == 0, "LDS map");

// tanh-GELU with its first and second derivative, sigmoid form as gelu_fwd_grad: v = 2 a (x + c x^3), s = sigmoid(v), q = s (1 - s):
// gelu = x s ; gelu' = s + x q v' ; gelu'' = q (2 v' + x (v'^2 (1 - 2 s) + v''))
template <class BK>
TTT_WV_FN void gelu_fwd_grad2(BK& bk, float x, float& y, float& dy, float& ddy) {
    const float x2 = x * x;
    const float s = bk.rcp(1.0f + bk.exp2(x * (x2 * GELU_K1 + GELU_K0)));
    const float vp = x2 * (2.0f * GELU_3AC) + 2.0f * GELU_A;
    const float q = s - s * s;
    y = x * s;
    dy = x * q * vp + s;
    ddy = q * (2.0f * vp + x * (vp * vp * (1.0f - 2.0f * s) + 4.0f * GELU_3AC * x));
}

// tr4 / rho_read of ttt_lin16_body.h / ttt_mlp16_body.h with the lane indices given (see TTT_MLP16_BLOCK_END)
template <class BK>
TTT_WV_FN bf16x4 tr4x(BK& bk, int g, int i, int img_off, int stride, int row0, int col0) {
    return bk.tr_read(img_off + ((row0 + 4 * g + (i >> 2)) * stride + col0 + 4 * (i & 3)) * 2);
}
template <class BK>
TTT_WV_FN bf16x8 rho_readx(BK& bk, int g, int i, int tile_off, int c0) {
    const int o = tile_off + (i * TS + c0 + 4 * g) * 2;
    return cat(bk.template lds_load<bf16x4>(o), bk.template lds_load<bf16x4>(o + 32));
}
// a pair of packed tiles (rows = t, lane = n) -> operand (lane = t, k = n in rho order) through the slice's [32 n][IS] image
template <class BK>
TTT_WV_FN bf16x8 to_kn(BK& bk, int img, const bf16x4 (&p)[2], int g, int i) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) bk.template lds_store<bf16x4>(img + ((16 * nb + i) * IS + 4 * g) * 2, p[nb]);
    bk.lds_fence();
    return cat(tr4x(bk, g, i, img, IS, 0, 0), tr4x(bk, g, i, img, IS, 16, 0));
}
// fp32 tiles (rows = f, lane = n) of a [64 f][32 n] slice -> A-form operands (row = f, k = n in rho order) per 16 features,
// through the slice's [32 n][TS] image
template <class BK>
TTT_WV_FN void to_fn_A(BK& bk, int wimg, const f32x4 (&T)[4][2], bf16x8 (&A)[4], int g, int i) {
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) bk.template lds_store<bf16x4>(wimg + ((16 * nb + i) * TS + 16 * fb + 4 * g) * 2, pack4(T[fb][nb]));
    bk.lds_fence();
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) A[fb] = cat(tr4x(bk, g, i, wimg, TS, 0, 16 * fb), tr4x(bk, g, i, wimg, TS, 16, 16 * fb));
}
// B-form operands (k = f in rho order, column = n)
TTT_WV_FN void to_fn_B(const f32x4 (&T)[4][2], bf16x8 (&B)[2][2]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) B[ks][nb] = stack(T[2 * ks][nb], T[2 * ks + 1][nb]);
}
// the slice [n0, n0 + 32) of a [64][256] array / of a [256][64] array as tiles (rows = f, lane = n).  The address is the (uniform)
// base plus ONE 32-bit lane offset plus a compile-time constant - a scalar base, one offset register and immediates - and not a
// 64-bit address pair per load: 40 such pairs, shared by the phases of a step, were what overflowed the register file.
TTT_WV_FN void load_fn(const float* W1g, f32x4 (&T)[4][2], int n0, int g, int i) {
    const unsigned lane = (unsigned)(((4 * g) * 256 + n0 + i) * 4);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
        const char* rows = reinterpret_cast<const char*>(W1g) + (unsigned)(lane + 16u * fb * 256 * 4);      // uniform base + one 32-bit offset
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) T[fb][nb][r] = *reinterpret_cast<const float*>(rows + (r * 256 + 16 * nb) * 4);
    }
}
TTT_WV_FN void load_fn_T(const float* W2g, f32x4 (&T)[4][2], int n0, int g, int i) {
    const unsigned lane = (unsigned)(((n0 + i) * 64 + 4 * g) * 4);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const char* rows = reinterpret_cast<const char*>(W2g) + (unsigned)(lane + 16u * nb * 64 * 4);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) T[fb][nb] = *reinterpret_cast<const f32x4*>(rows + 16 * fb * 4);
    }
}
// a slice's partial [f][t] of a [16 t][64 f] row quantity -> red[slice][t][PS] ; the owner's ordered sum over the slices
template <class BK>
TTT_WV_FN void put_partial(BK& bk, int red_off, int vw, int fb, int g, int i, f32x4 v) {
    bk.template lds_store<f32x4>(red_off + ((vw * CS + i) * PS + 4 * g + 16 * fb) * 4, v);
}
template <class BK>
TTT_WV_FN f32x4 gather(BK& bk, int red_off, int ot, int of0, f32x4 z) {
#pragma unroll
    for (int ww = 0; ww < 8; ++ww) z += bk.template lds_load<f32x4>(red_off + ((ww * CS + ot) * PS + of0) * 4);
    return z;
}

// Where the per-step state of a group lives: slot j of the group is element first + j of four arrays.  One call: the caller's four
// *_init_group buffers, G slots per (b, h), each array dense (PACKED = false).  In parts: the slot workspace [B*NH][nk][G] of
// MLP16_PART_SLOT_FLOATS, the four arrays interleaved slot by slot (PACKED = true).  The strides are compile-time either way.
struct SlotView {
    float *W1, *b1, *W2, *b2;
    size_t first;
};
template <bool PACKED>
struct SlotStride {
    static constexpr size_t W1 = PACKED ? MLP16_PART_SLOT_FLOATS : 64 * 256, b1 = PACKED ? MLP16_PART_SLOT_FLOATS : 256,
                            W2 = PACKED ? MLP16_PART_SLOT_FLOATS : 256 * 64, b2 = PACKED ? MLP16_PART_SLOT_FLOATS : 64;
};

// the state entering steps lo .. lo + n - 1 of group k -> slots 0 .. n - 1 of the group (sv)
template <bool PACKED, class BK>
TTT_WV_FN void recompute_group(BK& bk, const Mlp16BwdParams& p, const SlotView& sv, int bh, int k, int n) {
    typedef SlotStride<PACKED> SS;
    const int tid0 = bk.thread(), wv = bk.wave(), l0 = bk.lane();
    const size_t ck = (size_t)bh * p.K + k;

    f32x4 W1t[NS][4][2], W2t[NS][2][4], W2Tt[NS][4][2];
    float b1v[NS][2], b2v[4];
    {
        const int lp = bk.opaque(l0), g = lp >> 4, i = lp & 15;      // (opaque: nothing here is carried across the groups)
        const float* W1g = p.W1c + ck * 64 * 256;
        const float* W2g = p.W2c + ck * 256 * 64;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int n0 = 32 * (NS * wv + s);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        W1t[s][fb][nb][r] = W1g[(size_t)(16 * fb + 4 * g + r) * 256 + n0 + 16 * nb + i];
                        W2t[s][nb][fb][r] = W2g[(size_t)(n0 + 16 * nb + 4 * g + r) * 64 + 16 * fb + i];
                    }
                    W2Tt[s][fb][nb] = *reinterpret_cast<const f32x4*>(W2g + (size_t)(n0 + 16 * nb + i) * 64 + 16 * fb + 4 * g);
                }
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) b1v[s][nb] = p.b1c[ck * 256 + n0 + 16 * nb + i];
        }
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) b2v[fb] = p.b2c[ck * 64 + 16 * fb + i];
        const int tp = bk.opaque(tid0);
        if (tp < 64) bk.template lds_store<float>(B_B2 + tp * 4, p.b2c[ck * 64 + tp]);
    }
    const bf16x4 ONES = {(__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f};
    bf16x8 W1F[NS][2][2], W2F[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) W1F[s][ks][nb] = stack(W1t[s][2 * ks][nb], W1t[s][2 * ks + 1][nb]);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) W2F[s][fb] = stack(W2t[s][0][fb], W2t[s][1][fb]);
    }

    const size_t tile0 = (size_t)bh * p.NC + (size_t)k * p.G, slot0 = sv.first;

    for (int j = 0; j < n; ++j) {
        int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        int tid = bk.opaque(tid0), ot = (tid & 255) >> 4, of0 = 4 * (tid & 15);
        const int lt0 = tid & 127, lofs = ((lt0 >> 3) * TS + (lt0 & 7) * 8) * 2;      // staging: this thread's 16-byte chunk of a tile
        const size_t gofs = (size_t)(lt0 >> 3) * 64 + (lt0 & 7) * 8;
        const int buf = j & 1;
        const int Kt = B_K + buf * TB, Vt = B_V + buf * TB;
        const size_t sl = slot0 + j;
#pragma unroll
        for (int s = 0; s < NS; ++s)
            store_state(sv.W1 + sl * SS::W1, sv.b1 + sl * SS::b1, sv.W2 + sl * SS::W2, sv.b2 + sl * SS::b2, W1t[s], W2Tt[s], b1v[s], b2v,
                        NS * wv + s, g, i);
        if (j == n - 1) break;
        const size_t tile = tile0 + j;
        if (tid < 256)      // threads 0 - 127 stage K, 128 - 255 V
            bk.template lds_store<u32x4>((tid < 128 ? Kt : Vt) + lofs, *reinterpret_cast<const u32x4*>((tid < 128 ? p.XK : p.XV) + tile * 1024 + gofs));
        if (tid < 16) bk.template lds_store<float>(B_ETA + (buf * 16 + tid) * 4, (float)p.eta[tile * 16 + tid]);
        bk.barrier();

        // A1, A2 of the forward step
        f32x4 D1[NS][2];
        bf16x4 X2p[NS][2];
        const bf16x8 kA0 = rho_readx(bk, g, i, Kt, 0), kA1 = rho_readx(bk, g, i, Kt, 32);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int vw = NS * wv + s, img = B_XIMG + vw * XIMG_BYTES;
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                f32x4 Z = zero4();
                Z = bk.mma32(kA0, W1F[s][0][nb], Z);
                Z = bk.mma32(kA1, W1F[s][1][nb], Z);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float y, dy;
                    gelu_fwd_grad(bk, Z[r] + b1v[s][nb], y, dy);
                    Z[r] = y;
                    D1[s][nb][r] = dy;
                }
                X2p[s][nb] = pack4(Z);
                bk.template lds_store<bf16x4>(img + ((16 * nb + i) * IS + 4 * g) * 2, X2p[s][nb]);
            }
            bk.lds_fence();
            const bf16x8 xB = cat(tr4x(bk, g, i, img, IS, 0, 0), tr4x(bk, g, i, img, IS, 16, 0));
#pragma unroll
            for (int fb = 0; fb < 4; ++fb)
                bk.template lds_store<f32x4>(B_REDA + ((vw * CS + i) * PS + 4 * g + 16 * fb) * 4, bk.mma32(W2F[s][fb], xB, zero4()));
            TTT_MLP16_BLOCK_END();
        }
        bk.barrier();

        if (tid < 256) {      // P3 of the forward step (owners)
            f32x4 z = bk.template lds_load<f32x4>(B_B2 + of0 * 4);
#pragma unroll
            for (int ww = 0; ww < 8; ++ww) z += bk.template lds_load<f32x4>(B_REDA + ((ww * CS + ot) * PS + of0) * 4);
            float mu, rstd;
            row_stats(bk, z, p.eps, mu, rstd);
            const bf16x4 kk = bk.template lds_load<bf16x4>(Kt + (ot * TS + of0) * 2);
            const bf16x4 vv = bk.template lds_load<bf16x4>(Vt + (ot * TS + of0) * 2);
            const f32x4 gm = bk.template lds_load<f32x4>(B_GAM + of0 * 4), bt = bk.template lds_load<f32x4>(B_BET + of0 * 4);
            float s1 = 0.f, s2 = 0.f, gx[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float xh = (z[jj] - mu) * rstd;
                gx[jj] = (gm[jj] * xh + bt[jj] - ((float)vv[jj] - (float)kk[jj])) * gm[jj];
                z[jj] = xh;
                s1 += gx[jj]; s2 += gx[jj] * xh;
            }
            s1 = bk.sum16(s1);
            s2 = bk.sum16(s2);
            const float sc = -bk.template lds_load<float>(B_ETA + (buf * 16 + ot) * 4) * rstd * (1.0f / 64.0f);
            bf16x4 o;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) o[jj] = (__bf16)((64.0f * gx[jj] - s1 - z[jj] * s2) * sc);
            bk.template lds_store<bf16x4>(B_G + (ot * TS + of0) * 2, o);
        }
        bk.barrier();

        // C of the forward step without its output path
        const bf16x8 gA0 = rho_readx(bk, g, i, B_G, 0), gA1 = rho_readx(bk, g, i, B_G, 32);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) b2v[fb] += bk.mma16(ONES, tr4x(bk, g, i, B_G, TS, 0, 16 * fb), zero4())[0];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            bf16x8 W2TF[2][2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) W2TF[ks][nb] = stack(W2Tt[s][2 * ks][nb], W2Tt[s][2 * ks + 1][nb]);
            bf16x4 gzp[2];
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                f32x4 gx = zero4();
                gx = bk.mma32(gA0, W2TF[0][nb], gx);
                gx = bk.mma32(gA1, W2TF[1][nb], gx);
                gx *= D1[s][nb];
                gzp[nb] = pack4(gx);
                b1v[s][nb] += bk.mma16(ONES, gzp[nb], zero4())[0];
            }
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const bf16x4 kT = tr4x(bk, g, i, Kt, TS, 0, 16 * fb);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) W1t[s][fb][nb] = bk.mma16(kT, gzp[nb], W1t[s][fb][nb]);
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) W1F[s][ks][nb] = stack(W1t[s][2 * ks][nb], W1t[s][2 * ks + 1][nb]);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                const bf16x4 gT = tr4x(bk, g, i, B_G, TS, 0, 16 * fb);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    W2t[s][nb][fb] = bk.mma16(X2p[s][nb], gT, W2t[s][nb][fb]);
                    W2Tt[s][fb][nb] = bk.mma16(gT, X2p[s][nb], W2Tt[s][fb][nb]);
                }
                W2F[s][fb] = stack(W2t[s][0][fb], W2t[s][1][fb]);
            }
            TTT_MLP16_BLOCK_END();
        }
        if (wv == 0 && g == 0) {
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) bk.template lds_store<float>(B_B2 + (16 * fb + i) * 4, b2v[fb]);
        }
    }
    bk.barrier();      // the slots are complete (each wave re-reads its own slices) and the LDS is free for the reverse walk
}

// the reverse walk over the n steps of group k from the slots (sv); an owner thread's share of dln_w / dln_b accumulates in its cell of
// B_DLNW / B_DLNB (eight registers less across the whole walk).  `last`: the state gradient comes from the upstream p.d*_last (the
// first group a call walks) and not from where the previous group parked it (p.dW1 .. p.db2, where this group parks it in turn).
template <bool PACKED, class BK>
TTT_WV_FN void sweep_group(BK& bk, const Mlp16BwdParams& p, const SlotView& sv, int bh, int k, int n, bool last) {
    typedef SlotStride<PACKED> SS;
    const int tid0 = bk.thread(), wv = bk.wave(), l0 = bk.lane();
    const bf16x4 ONES = {(__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f, (__bf16)1.0f};

    f32x4 dW1t[NS][4][2], dW2Tt[NS][4][2];          // (rows = f, lane = n)
    float db1v[NS][2], db2v[4];
    {
        const int lp = bk.opaque(l0), g = lp >> 4, i = lp & 15;      // (opaque: nothing here is carried across the groups)
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int n0 = 32 * (NS * wv + s);
            load_fn((last ? p.dW1_last : p.dW1) + (size_t)bh * 64 * 256, dW1t[s], n0, g, i);
            load_fn_T((last ? p.dW2_last : p.dW2) + (size_t)bh * 256 * 64, dW2Tt[s], n0, g, i);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) db1v[s][nb] = (last ? p.db1_last : p.db1)[(size_t)bh * 256 + n0 + 16 * nb + i];
        }
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) db2v[fb] = (last ? p.db2_last : p.db2)[(size_t)bh * 64 + 16 * fb + i];
    }

    // staging: chunks of 16 bytes, 128 per tile, in the order K, V, Q, dOut
    const size_t tile0 = (size_t)bh * p.NC + (size_t)k * p.G, slot0 = sv.first;

    for (int j = n - 1; j >= 0; --j) {
        int l = bk.opaque(l0), g = l >> 4, i = l & 15;
        int tid = bk.opaque(tid0), ot = (tid & 255) >> 4, of0 = 4 * (tid & 15);
        const int lt0 = tid & 127, lofs = ((lt0 >> 3) * TS + (lt0 & 7) * 8) * 2;      // staging: this thread's 16-byte chunk of a tile
        const size_t gofs = (size_t)(lt0 >> 3) * 64 + (lt0 & 7) * 8;
        const size_t tile = tile0 + j, sl = slot0 + j;
        const float* W1s = sv.W1 + sl * SS::W1;
        const float* W2s = sv.W2 + sl * SS::W2;

#pragma unroll
        for (int c = 0; c < 512; c += 64 * WAVES) {
            const int w = (c + tid) >> 7;
            const __bf16* src = w == 0 ? p.XK : w == 1 ? p.XV : w == 2 ? p.XQ : p.dOut;
            bk.template lds_store<u32x4>((w == 0 ? B_K : w == 1 ? B_V : w == 2 ? B_Q : B_D) + lofs, *reinterpret_cast<const u32x4*>(src + tile * 1024 + gofs));
        }
        if (tid < 16) bk.template lds_store<float>(B_ETA + tid * 4, (float)p.eta[tile * 16 + tid]);
        if (tid < 64) bk.template lds_store<float>(B_B2 + tid * 4, sv.b2[sl * SS::b2 + tid]);
        bk.barrier();                                                                                   // S0
        TTT_MLP16_BLOCK_END();

        // ---- P1
        float b1n[NS][2], b2n[4];
        f32x4 D1[NS][2], DD1[NS][2];             // gelu'(Z1), gelu''(Z1) in fp32 until P3 has used them
        bf16x4 X2p[NS][2];
        {
            const bf16x8 kA0 = rho_readx(bk, g, i, B_K, 0), kA1 = rho_readx(bk, g, i, B_K, 32);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int vw = NS * wv + s, n0 = 32 * vw, img = B_XIMG + vw * XIMG_BYTES, wimg = B_WIMG + vw * WIMG_BYTES;
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) b1n[s][nb] = sv.b1[sl * SS::b1 + n0 + 16 * nb + i];
                bf16x8 W1B[2][2];
                {
                    f32x4 W1t[4][2];
                    load_fn(W1s, W1t, n0, g, i);
                    to_fn_B(W1t, W1B);
                }
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    f32x4 Z = zero4();
                    Z = bk.mma32(kA0, W1B[0][nb], Z);
                    Z = bk.mma32(kA1, W1B[1][nb], Z);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float y, dy, ddy;
                        gelu_fwd_grad2(bk, Z[r] + b1n[s][nb], y, dy, ddy);
                        Z[r] = y;
                        D1[s][nb][r] = dy;
                        DD1[s][nb][r] = ddy;
                    }
                    X2p[s][nb] = pack4(Z);
                }
                TTT_MLP16_BLOCK_END();
                const bf16x8 xB = to_kn(bk, img, X2p[s], g, i);
                bf16x8 W2A[4];
                {
                    f32x4 W2Tt[4][2];
                    load_fn_T(W2s, W2Tt, n0, g, i);
                    to_fn_A(bk, wimg, W2Tt, W2A, g, i);
                }
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) put_partial(bk, B_REDA, vw, fb, g, i, bk.mma32(W2A[fb], xB, zero4()));
                TTT_MLP16_BLOCK_END();
            }
        }
        bk.barrier();                                                                                   // S1
        TTT_MLP16_BLOCK_END();

        // ---- P2 (owners): Z2 -> LayerNorm / L2 backward
        f32x4 o_xh = zero4(), o_go = zero4(), o_dt = zero4();
        float o_rstd = 0.f, o_eta = 0.f, o_sgx = 0.f, o_deta = 0.f;
        if (tid < 256) {
            const f32x4 z = gather(bk, B_REDA, ot, of0, bk.template lds_load<f32x4>(B_B2 + of0 * 4));
            float mu;
            row_stats(bk, z, p.eps, mu, o_rstd);
            const bf16x4 kk = bk.template lds_load<bf16x4>(B_K + (ot * TS + of0) * 2);
            const bf16x4 vv = bk.template lds_load<bf16x4>(B_V + (ot * TS + of0) * 2);
            const f32x4 gm = bk.template lds_load<f32x4>(B_GAM + of0 * 4), bt = bk.template lds_load<f32x4>(B_BET + of0 * 4);
            float s1 = 0.f, s2 = 0.f, gx[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                o_xh[jj] = (z[jj] - mu) * o_rstd;
                o_go[jj] = gm[jj] * o_xh[jj] + bt[jj] - ((float)vv[jj] - (float)kk[jj]);
                gx[jj] = o_go[jj] * gm[jj];
                s1 += gx[jj]; s2 += gx[jj] * o_xh[jj];
            }
            s1 = bk.sum16(s1);
            o_sgx = bk.sum16(s2);
            o_eta = bk.template lds_load<float>(B_ETA + ot * 4);
            const float sc = -o_eta * o_rstd * (1.0f / 64.0f);
            bf16x4 gs, gz;
            f32x4 o_gz;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float base = 64.0f * gx[jj] - s1 - o_xh[jj] * o_sgx;
                o_gz[jj] = base * (o_rstd * (1.0f / 64.0f));
                gs[jj] = (__bf16)(base * sc);
                gz[jj] = (__bf16)o_gz[jj];
            }
            bk.template lds_store<bf16x4>(B_G + (ot * TS + of0) * 2, gs);
            bk.template lds_store<bf16x4>(B_GZ + (ot * TS + of0) * 2, gz);
            bk.template lds_store<f32x4>(B_OGZ + (ot * 64 + of0) * 4, o_gz);
        }
        bk.barrier();                                                                                   // S2
        TTT_MLP16_BLOCK_END();

        // ---- P3: gX2, gZ1 ; the forward's update -> W2n, b2n, W1n, b1n ; Z1b -> X2b, D1b ; partial Z2b
        // kept for the later phases as bf16 tiles: gzp = gZ1s (what the forward's W1 update takes), D1, gX2 gelu''(Z1), gZ1, X2b, D1b
        bf16x4 gzp[NS][2], D1p[NS][2], gXDp[NS][2], gZ1p[NS][2], X2bp[NS][2], D1bp[NS][2];
        {
            const bf16x8 gA0 = rho_readx(bk, g, i, B_G, 0), gA1 = rho_readx(bk, g, i, B_G, 32);
            const bf16x8 zA0 = rho_readx(bk, g, i, B_GZ, 0), zA1 = rho_readx(bk, g, i, B_GZ, 32);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) b2n[fb] = sv.b2[sl * SS::b2 + 16 * fb + i] + bk.mma16(ONES, tr4x(bk, g, i, B_G, TS, 0, 16 * fb), zero4())[0];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int vw = NS * wv + s, n0 = 32 * vw, img = B_XIMG + vw * XIMG_BYTES, wimg = B_WIMG + vw * WIMG_BYTES;
                bf16x8 W2nA[4];
                {
                    f32x4 W2Tt[4][2];
                    load_fn_T(W2s, W2Tt, n0, g, i);
                    {
                        bf16x8 W2B[2][2];
                        to_fn_B(W2Tt, W2B);
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) {
                            f32x4 gx = zero4();
                            gx = bk.mma32(gA0, W2B[0][nb], gx);
                            gx = bk.mma32(gA1, W2B[1][nb], gx);
                            gx *= D1[s][nb];
                            gzp[s][nb] = pack4(gx);
                            b1n[s][nb] += bk.mma16(ONES, gzp[s][nb], zero4())[0];
                            f32x4 x = zero4();
                            x = bk.mma32(zA0, W2B[0][nb], x);
                            x = bk.mma32(zA1, W2B[1][nb], x);
                            gZ1p[s][nb] = pack4(x * D1[s][nb]);
                            gXDp[s][nb] = pack4(x * DD1[s][nb]);
                            D1p[s][nb] = pack4(D1[s][nb]);
                        }
                    }
                    TTT_MLP16_BLOCK_END();
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) {
                        const bf16x4 gT = tr4x(bk, g, i, B_G, TS, 0, 16 * fb);
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) W2Tt[fb][nb] = bk.mma16(gT, X2p[s][nb], W2Tt[fb][nb]);
                    }
                    to_fn_A(bk, wimg, W2Tt, W2nA, g, i);
                }
                TTT_MLP16_BLOCK_END();
                bf16x8 W1nB[2][2];
                {
                    f32x4 W1t[4][2];
                    load_fn(W1s, W1t, n0, g, i);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) {
                        const bf16x4 kT = tr4x(bk, g, i, B_K, TS, 0, 16 * fb);
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) W1t[fb][nb] = bk.mma16(kT, gzp[s][nb], W1t[fb][nb]);
                    }
                    to_fn_B(W1t, W1nB);
                }
                TTT_MLP16_BLOCK_END();
                const bf16x8 qA0 = rho_readx(bk, g, i, B_Q, 0), qA1 = rho_readx(bk, g, i, B_Q, 32);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    f32x4 Z = zero4(), Db;
                    Z = bk.mma32(qA0, W1nB[0][nb], Z);
                    Z = bk.mma32(qA1, W1nB[1][nb], Z);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float y, dy;
                        gelu_fwd_grad(bk, Z[r] + b1n[s][nb], y, dy);
                        Z[r] = y;
                        Db[r] = dy;
                    }
                    X2bp[s][nb] = pack4(Z);
                    D1bp[s][nb] = pack4(Db);
                }
                const bf16x8 xB = to_kn(bk, img, X2bp[s], g, i);
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) put_partial(bk, B_REDB, vw, fb, g, i, bk.mma32(W2nA[fb], xB, zero4()));
                TTT_MLP16_BLOCK_END();
            }
            if (wv == 0 && g == 0) {
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) bk.template lds_store<float>(B_B2N + (16 * fb + i) * 4, b2n[fb]);
            }
        }
        bk.barrier();                                                                                   // S3
        TTT_MLP16_BLOCK_END();

        // ---- P4 (owners): Z2b -> output LayerNorm ; dZ2b
        if (tid < 256) {
            const f32x4 z = gather(bk, B_REDB, ot, of0, bk.template lds_load<f32x4>(B_B2N + of0 * 4));
            float mu, rstd;
            row_stats(bk, z, p.eps, mu, rstd);
            const bf16x4 dd = bk.template lds_load<bf16x4>(B_D + (ot * TS + of0) * 2);
            const f32x4 gm = bk.template lds_load<f32x4>(B_GAM + of0 * 4);
            f32x4 dgam = bk.template lds_load<f32x4>(B_DLNW + (ot * 64 + of0) * 4), dbet = bk.template lds_load<f32x4>(B_DLNB + (ot * 64 + of0) * 4);
            float t1 = 0.f, t2 = 0.f, dxh[4], xh[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                xh[jj] = (z[jj] - mu) * rstd;
                const float d = (float)dd[jj];
                dgam[jj] += d * xh[jj];
                dbet[jj] += d;
                dxh[jj] = d * gm[jj];
                t1 += dxh[jj]; t2 += dxh[jj] * xh[jj];
            }
            bk.template lds_store<f32x4>(B_DLNW + (ot * 64 + of0) * 4, dgam);
            bk.template lds_store<f32x4>(B_DLNB + (ot * 64 + of0) * 4, dbet);
            t1 = bk.sum16(t1);
            t2 = bk.sum16(t2);
            bf16x4 o;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) o[jj] = (__bf16)((64.0f * dxh[jj] - t1 - xh[jj] * t2) * (rstd * (1.0f / 64.0f)));
            bk.template lds_store<bf16x4>(B_DZB + (ot * TS + of0) * 2, o);
        }
        bk.barrier();                                                                                   // S4
        TTT_MLP16_BLOCK_END();

        // ---- P5
        f32x4 dZ1[NS][2];                   // dgZ1 gX2 gelu''(Z1) - eta A2 D1 ; P7 adds (dZ2 W2^T) D1
        {
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) db2v[fb] += bk.mma16(ONES, tr4x(bk, g, i, B_DZB, TS, 0, 16 * fb), zero4())[0];
            if (wv == 0 && g == 0) {
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) bk.template lds_store<float>(B_DB2 + (16 * fb + i) * 4, db2v[fb]);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int vw = NS * wv + s, n0 = 32 * vw, img = B_XIMG + vw * XIMG_BYTES, wimg = B_WIMG + vw * WIMG_BYTES;
                bf16x4 dz1bp[2];
                {      // W2n again (the slot's W2 and the forward's update), B-form: dX2b = dZ2b W2n^T, dZ1b = dX2b D1b
                    f32x4 W2Tt[4][2];
                    load_fn_T(W2s, W2Tt, n0, g, i);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) {
                        const bf16x4 gT = tr4x(bk, g, i, B_G, TS, 0, 16 * fb);
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) W2Tt[fb][nb] = bk.mma16(gT, X2p[s][nb], W2Tt[fb][nb]);
                    }
                    bf16x8 W2nB[2][2];
                    to_fn_B(W2Tt, W2nB);
                    const bf16x8 dA0 = rho_readx(bk, g, i, B_DZB, 0), dA1 = rho_readx(bk, g, i, B_DZB, 32);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        f32x4 x = zero4();
                        x = bk.mma32(dA0, W2nB[0][nb], x);
                        x = bk.mma32(dA1, W2nB[1][nb], x);
#pragma unroll
                        for (int r = 0; r < 4; ++r) x[r] *= (float)D1bp[s][nb][r];
                        dz1bp[nb] = pack4(x);
                        db1v[s][nb] += bk.mma16(ONES, dz1bp[nb], zero4())[0];
                    }
                }
                TTT_MLP16_BLOCK_END();
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const bf16x4 qT = tr4x(bk, g, i, B_Q, TS, 0, 16 * fb);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) dW1t[s][fb][nb] = bk.mma16(qT, dz1bp[nb], dW1t[s][fb][nb]);
                }
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const bf16x4 dT = tr4x(bk, g, i, B_DZB, TS, 0, 16 * fb);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) dW2Tt[s][fb][nb] = bk.mma16(dT, X2bp[s][nb], dW2Tt[s][fb][nb]);
                }
                TTT_MLP16_BLOCK_END();
                {      // W1n again, A-form: partial (dQ - dOut)^T = W1n dZ1b^T
                    f32x4 W1t[4][2];
                    load_fn(W1s, W1t, n0, g, i);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) {
                        const bf16x4 kT = tr4x(bk, g, i, B_K, TS, 0, 16 * fb);
#pragma unroll
                        for (int nb = 0; nb < 2; ++nb) W1t[fb][nb] = bk.mma16(kT, gzp[s][nb], W1t[fb][nb]);
                    }
                    bf16x8 W1nA[4];
                    to_fn_A(bk, wimg, W1t, W1nA, g, i);
                    const bf16x8 xB = to_kn(bk, img, dz1bp, g, i);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) put_partial(bk, B_REDA, vw, fb, g, i, bk.mma32(W1nA[fb], xB, zero4()));
                }
                TTT_MLP16_BLOCK_END();
                // dW1n, db1n, dW2n, db2n are complete: what the state updates hand back
                f32x4 dep = zero4();
                bf16x4 up[2], ex2p[2];
                {
                    bf16x8 dW2B[2][2], dW1B[2][2];
                    to_fn_B(dW2Tt[s], dW2B);
                    to_fn_B(dW1t[s], dW1B);
                    const bf16x8 zA0 = rho_readx(bk, g, i, B_GZ, 0), zA1 = rho_readx(bk, g, i, B_GZ, 32);
                    const bf16x8 kA0 = rho_readx(bk, g, i, B_K, 0), kA1 = rho_readx(bk, g, i, B_K, 32);
                    const f32x4 eta = bk.template lds_load<f32x4>(B_ETA + 16 * g);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        f32x4 A2 = zero4(), dg = zero4(), u, ex;
                        A2 = bk.mma32(zA0, dW2B[0][nb], A2);
                        A2 = bk.mma32(zA1, dW2B[1][nb], A2);
                        dg = bk.mma32(kA0, dW1B[0][nb], dg);
                        dg = bk.mma32(kA1, dW1B[1][nb], dg);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float x2 = (float)X2p[s][nb][r];
                            dg[r] = -eta[r] * (dg[r] + db1v[s][nb]);
                            dep[r] += x2 * A2[r] + (float)gZ1p[s][nb][r] * db1v[s][nb];
                            ex[r] = -eta[r] * x2;
                            u[r] = dg[r] * (float)D1p[s][nb][r];
                            dZ1[s][nb][r] = dg[r] * (float)gXDp[s][nb][r] - eta[r] * A2[r] * (float)D1p[s][nb][r];
                        }
                        up[nb] = pack4(u);
                        ex2p[nb] = pack4(ex);
                    }
                }
                TTT_MLP16_BLOCK_END();
                f32x4 acc[4];
                {
                    bf16x8 dW2nA[4];
                    to_fn_A(bk, wimg, dW2Tt[s], dW2nA, g, i);
                    const bf16x8 xB = to_kn(bk, img, ex2p, g, i);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) acc[fb] = bk.mma32(dW2nA[fb], xB, zero4());
                }
                TTT_MLP16_BLOCK_END();
                {
                    f32x4 W2e[4][2];
                    load_fn_T(W2s, W2e, n0, g, i);
                    bf16x8 W2A[4];
                    to_fn_A(bk, wimg, W2e, W2A, g, i);
                    const bf16x8 xB = to_kn(bk, img, up, g, i);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) put_partial(bk, B_REDB, vw, fb, g, i, bk.mma32(W2A[fb], xB, acc[fb]));
                }
                TTT_MLP16_BLOCK_END();
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const bf16x4 zT = tr4x(bk, g, i, B_GZ, TS, 0, 16 * fb);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) dW2Tt[s][fb][nb] = bk.mma16(zT, up[nb], dW2Tt[s][fb][nb]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sm = bk.sum16(dep[r]);
                    if (i == 0) bk.template lds_store<float>(B_DETA + (vw * CS + 4 * g + r) * 4, -sm);
                }
                TTT_MLP16_BLOCK_END();
            }
        }
        bk.barrier();                                                                                   // S5
        TTT_MLP16_BLOCK_END();

        // ---- P6 (owners): dgZ2 -> second-order LayerNorm backward -> dZ2, dt ; dV, dQ
        if (tid < 256) {
            const f32x4 db2 = bk.template lds_load<f32x4>(B_DB2 + of0 * 4), o_gz = bk.template lds_load<f32x4>(B_OGZ + (ot * 64 + of0) * 4);
            f32x4 G_ = gather(bk, B_REDB, ot, of0, zero4());
            const f32x4 gm = bk.template lds_load<f32x4>(B_GAM + of0 * 4);
            const float r = o_rstd;
            float s1 = 0.f, s2 = 0.f, sd = 0.f, mGr[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                G_[jj] -= o_eta * db2[jj];
                mGr[jj] = -G_[jj] * r;
                s1 += mGr[jj]; s2 += mGr[jj] * o_xh[jj];
                sd += o_gz[jj] * db2[jj];
            }
            s1 = bk.sum16(s1) * (1.0f / 64.0f);
            s2 = bk.sum16(s2) * (1.0f / 64.0f);
            o_deta = -bk.sum16(sd);
            f32x4 dgam = bk.template lds_load<f32x4>(B_DLNW + (ot * 64 + of0) * 4), dbet = bk.template lds_load<f32x4>(B_DLNB + (ot * 64 + of0) * 4);
            float dxh[4], t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float dgxh = r * G_[jj] + s1 + o_xh[jj] * s2;
                const float dy = gm[jj] * dgxh;
                dgam[jj] += o_go[jj] * dgxh + dy * o_xh[jj];
                dbet[jj] += dy;
                o_dt[jj] = -dy;
                dxh[jj] = dy * gm[jj] + o_go[jj] * gm[jj] * s2 + o_sgx * mGr[jj] * (1.0f / 64.0f);
                t1 += dxh[jj];
                t2 += -dxh[jj] * o_xh[jj] * r - G_[jj] * o_gz[jj] * r;
            }
            bk.template lds_store<f32x4>(B_DLNW + (ot * 64 + of0) * 4, dgam);
            bk.template lds_store<f32x4>(B_DLNB + (ot * 64 + of0) * 4, dbet);
            t1 = bk.sum16(t1) * (1.0f / 64.0f);
            t2 = bk.sum16(t2) * (1.0f / 64.0f);
            bf16x4 dz, dv, dq;
            const f32x4 qp = gather(bk, B_REDA, ot, of0, zero4());
            const bf16x4 dd = bk.template lds_load<bf16x4>(B_D + (ot * TS + of0) * 2);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                dz[jj] = (__bf16)(dxh[jj] * r - t1 * r + t2 * o_xh[jj]);
                dv[jj] = (__bf16)o_dt[jj];
                dq[jj] = (__bf16)((float)dd[jj] + qp[jj]);
            }
            bk.template lds_store<bf16x4>(B_DZ2 + (ot * TS + of0) * 2, dz);
            *reinterpret_cast<bf16x4*>(p.dXV + tile * 1024 + (size_t)ot * 64 + of0) = dv;
            *reinterpret_cast<bf16x4*>(p.dXQ + tile * 1024 + (size_t)ot * 64 + of0) = dq;
        }
        bk.barrier();                                                                                   // S6
        TTT_MLP16_BLOCK_END();

        // ---- P7
        {
            const bf16x8 zA0 = rho_readx(bk, g, i, B_DZ2, 0), zA1 = rho_readx(bk, g, i, B_DZ2, 32);
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) db2v[fb] += bk.mma16(ONES, tr4x(bk, g, i, B_DZ2, TS, 0, 16 * fb), zero4())[0];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int vw = NS * wv + s, n0 = 32 * vw, img = B_XIMG + vw * XIMG_BYTES, wimg = B_WIMG + vw * WIMG_BYTES;
                bf16x4 dz1p[2];
                {      // dZ1 += (dZ2 W2^T) D1 with the entering W2
                    f32x4 W2e[4][2];
                    load_fn_T(W2s, W2e, n0, g, i);
                    bf16x8 W2B[2][2];
                    to_fn_B(W2e, W2B);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        f32x4 x = zero4();
                        x = bk.mma32(zA0, W2B[0][nb], x);
                        x = bk.mma32(zA1, W2B[1][nb], x);
#pragma unroll
                        for (int r = 0; r < 4; ++r) dZ1[s][nb][r] += x[r] * (float)D1p[s][nb][r];
                        dz1p[nb] = pack4(dZ1[s][nb]);
                    }
                }
                TTT_MLP16_BLOCK_END();
                {      // A1 = gZ1 dW1n^T, before dW1n becomes dW1
                    bf16x8 dW1nA[4];
                    to_fn_A(bk, wimg, dW1t[s], dW1nA, g, i);
                    const bf16x8 xB = to_kn(bk, img, gZ1p[s], g, i);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) put_partial(bk, B_REDB, vw, fb, g, i, bk.mma32(dW1nA[fb], xB, zero4()));
                }
                TTT_MLP16_BLOCK_END();
                {      // dZ1 W1^T with the entering W1
                    f32x4 W1e[4][2];
                    load_fn(W1s, W1e, n0, g, i);
                    bf16x8 W1A[4];
                    to_fn_A(bk, wimg, W1e, W1A, g, i);
                    const bf16x8 xB = to_kn(bk, img, dz1p, g, i);
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) put_partial(bk, B_REDA, vw, fb, g, i, bk.mma32(W1A[fb], xB, zero4()));
                }
                TTT_MLP16_BLOCK_END();
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) db1v[s][nb] += bk.mma16(ONES, dz1p[nb], zero4())[0];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const bf16x4 kT = tr4x(bk, g, i, B_K, TS, 0, 16 * fb);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) dW1t[s][fb][nb] = bk.mma16(kT, dz1p[nb], dW1t[s][fb][nb]);
                }
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) {
                    const bf16x4 zT = tr4x(bk, g, i, B_DZ2, TS, 0, 16 * fb);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) dW2Tt[s][fb][nb] = bk.mma16(zT, X2p[s][nb], dW2Tt[s][fb][nb]);
                }
                TTT_MLP16_BLOCK_END();
            }
        }
        bk.barrier();                                                                                   // S7
        TTT_MLP16_BLOCK_END();

        // ---- P8 (owners): dK, d eta
        if (tid < 256) {
            const f32x4 A1 = gather(bk, B_REDB, ot, of0, zero4());
            const f32x4 kp = gather(bk, B_REDA, ot, of0, zero4());
            const bf16x4 kk = bk.template lds_load<bf16x4>(B_K + (ot * TS + of0) * 2);
            bf16x4 dk;
            float ka = 0.f;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                dk[jj] = (__bf16)(kp[jj] - o_eta * A1[jj] - o_dt[jj]);
                ka += (float)kk[jj] * A1[jj];
            }
            *reinterpret_cast<bf16x4*>(p.dXK + tile * 1024 + (size_t)ot * 64 + of0) = dk;
            float de = o_deta - bk.sum16(ka);
#pragma unroll
            for (int ww = 0; ww < 8; ++ww) de += bk.template lds_load<float>(B_DETA + (ww * CS + ot) * 4);
            if ((tid & 15) == 0) p.deta[tile * 16 + ot] = (__bf16)de;
        }
        bk.barrier();                                                                                   // S8
        TTT_MLP16_BLOCK_END();
    }
    // park the state gradient in the outputs: the upstream of the next group, the result after the first
    {
        const int l = bk.opaque(l0);
#pragma unroll
        for (int s = 0; s < NS; ++s)
            store_state(p.dW1 + (size_t)bh * 64 * 256, p.db1 + (size_t)bh * 256, p.dW2 + (size_t)bh * 256 * 64, p.db2 + (size_t)bh * 64,
                        dW1t[s], dW2Tt[s], db1v[s], db2v, NS * wv + s, l >> 4, l & 15);
    }
    bk.barrier();
}

template <class BK>
TTT_WV_FN void backward(BK& bk, const Mlp16BwdParams& p, int bh) {
    const int tid = bk.thread(), head = bh % p.NH;
    if (tid < 64) {
        bk.template lds_store<float>(B_GAM + tid * 4, p.ln_w[(size_t)head * 64 + tid]);
        bk.template lds_store<float>(B_BET + tid * 4, p.ln_b[(size_t)head * 64 + tid]);
    }
    if (tid < 256) {
        const int ot = tid >> 4, of0 = 4 * (tid & 15);
        bk.template lds_store<f32x4>(B_DLNW + (ot * 64 + of0) * 4, zero4());
        bk.template lds_store<f32x4>(B_DLNB + (ot * 64 + of0) * 4, zero4());
    }
    for (int k = p.K - 1; k >= 0; --k) {
        const int n = (k + 1) * p.G <= p.NC ? p.G : p.NC - k * p.G;
        const SlotView sv = {p.W1s, p.b1s, p.W2s, p.b2s, (size_t)bh * p.G};      // the caller's four *_init_group buffers
        recompute_group<false>(bk, p, sv, bh, k, n);
        sweep_group<false>(bk, p, sv, bh, k, n, k == p.K - 1);
    }
    // dln_w, dln_b: the owners' shares summed over the 16 tokens in token order (the last walk ended with a barrier)
    if (tid < 128) {
        const int f = tid & 63, red = tid < 64 ? B_DLNW : B_DLNB;
        float sm = 0.f;
        for (int ot = 0; ot < 16; ++ot) sm += bk.template lds_load<float>(red + (ot * 64 + f) * 4);
        (tid < 64 ? p.dln_w : p.dln_b)[(size_t)bh * 64 + f] = sm;
    }
}

// ---- The backward in parts (Mlp16BwdPartParams, ttt_wave_types.h): the two halves of backward() above as kernels of their own over
// the checkpoint groups [k0, k0 + nk).  The recompute of a group depends on its checkpoint alone, the walk on the state gradient the
// later groups leave; both run recompute_group / sweep_group above, so every step is a step of backward(), rounded alike, and a slot
// holds the bits backward() leaves in the *_init_group buffers.  Within recompute_groups no workgroup reads a slot another wrote,
// within sweep_groups no wave writes one.
TTT_WV_FN SlotView part_slots(const Mlp16BwdPartParams& q, int bh, int k) {
    float* s = q.slots;
    return {s + MLP16_PART_W1_OFS, s + MLP16_PART_B1_OFS, s + MLP16_PART_W2_OFS, s + MLP16_PART_B2_OFS,
            ((size_t)bh * q.nk + (size_t)(k - q.k0)) * q.p.G};
}
// unit of work bhk = bh * nk + (k - k0): group k of (b, h) = bh
template <class BK>
TTT_WV_FN void recompute_groups(BK& bk, const Mlp16BwdPartParams& q, int bhk) {
    const Mlp16BwdParams& p = q.p;
    const int tid = bk.thread(), bh = bhk / q.nk, k = q.k0 + bhk % q.nk, head = bh % p.NH;
    if (tid < 64) {
        bk.template lds_store<float>(B_GAM + tid * 4, p.ln_w[(size_t)head * 64 + tid]);
        bk.template lds_store<float>(B_BET + tid * 4, p.ln_b[(size_t)head * 64 + tid]);
    }
    const int n = (k + 1) * p.G <= p.NC ? p.G : p.NC - k * p.G;
    recompute_group<true>(bk, p, part_slots(q, bh, k), bh, k, n);
}
// the reverse walk of (b, h) = bh over the groups k0 + nk - 1 .. k0 from the slots recompute_groups left.  Carries dW1 .. db2 (from
// p.d*_last into p.dW1 .. p.db2, which may be the same buffers: every thread has read its cells before any thread writes, S0 .. S8
// lie between) and the owners' dln shares: the B_DLNW / B_DLNB cells start from zero where the range ends the sequence and from
// q.ln_carry otherwise, go back there at the end, and the range that holds group 0 reduces them as backward() does.
template <class BK>
TTT_WV_FN void sweep_groups(BK& bk, const Mlp16BwdPartParams& q, int bh) {
    const Mlp16BwdParams& p = q.p;
    const int tid = bk.thread(), head = bh % p.NH;
    float* carry = q.ln_carry + (size_t)bh * MLP16_PART_CARRY_FLOATS;
    if (tid < 64) {
        bk.template lds_store<float>(B_GAM + tid * 4, p.ln_w[(size_t)head * 64 + tid]);
        bk.template lds_store<float>(B_BET + tid * 4, p.ln_b[(size_t)head * 64 + tid]);
    }
    if (tid < 256) {
        const int ot = tid >> 4, of0 = 4 * (tid & 15);
        const bool fresh = q.k0 + q.nk == p.K;
        bk.template lds_store<f32x4>(B_DLNW + (ot * 64 + of0) * 4, fresh ? zero4() : *reinterpret_cast<const f32x4*>(carry + ot * 64 + of0));
        bk.template lds_store<f32x4>(B_DLNB + (ot * 64 + of0) * 4, fresh ? zero4() : *reinterpret_cast<const f32x4*>(carry + 1024 + ot * 64 + of0));
    }
    // (no barrier: a cell of B_DLNW / B_DLNB is its owner's alone during the walk, and S0 lies in front of the first read of B_GAM / B_BET)
    for (int k = q.k0 + q.nk - 1; k >= q.k0; --k) {
        const int n = (k + 1) * p.G <= p.NC ? p.G : p.NC - k * p.G;
        sweep_group<true>(bk, p, part_slots(q, bh, k), bh, k, n, k == q.k0 + q.nk - 1);
    }
    if (tid < 256) {      // an owner's own cells (the last walk ended with a barrier)
        const int ot = tid >> 4, of0 = 4 * (tid & 15);
        *reinterpret_cast<f32x4*>(carry + ot * 64 + of0) = bk.template lds_load<f32x4>(B_DLNW + (ot * 64 + of0) * 4);
        *reinterpret_cast<f32x4*>(carry + 1024 + ot * 64 + of0) = bk.template lds_load<f32x4>(B_DLNB + (ot * 64 + of0) * 4);
    }
    if (q.k0 == 0 && tid < 128) {
        const int f = tid & 63, red = tid < 64 ? B_DLNW : B_DLNB;
        float sm = 0.f;
        for (int ot = 0; ot < 16; ++ot) sm += bk.template lds_load<float>(red + (ot * 64 + f) * 4);
        (tid < 64 ? p.dln_w : p.dln_b)[(size_t)bh * 64 + f] = sm;
    }
}

}  // namespace bwd
}  // namespace mlp16
}  // namespace ttt
