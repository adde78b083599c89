// MFMA TTT-MLP forward scan for mini-batches of 16 tokens (gfx950): the evaluation / sampling geometry of the reference
// (configs/eval/ttt-mlp/*.toml: mini_batch_size = 16, no scan checkpoints; ttt_layer.py:429-473 -> mlp_tk.py forward).
//
// Same primal-form step as the CS = 64 kernel (ttt_mfma2.hip) but a different machine mapping: with
// 16 tokens the products that carry a token dimension are 16 wide, so everything runs on the 16x16 MFMA shapes
//   mma32 = v_mfma_f32_16x16x32_bf16  (contractions over the 64 features / the hidden units),
//   mma16 = v_mfma_f32_16x16x16_bf16  (contractions over the 16 tokens: the state updates),
// and the state lives in 16x16 fp32 accumulator tiles (lane (g, i) = (l >> 4, l & 15) holds D[4g + r][i], r = 0..3).
// Layout algebra: a 16x16 tile X (rows = R, lane = C) is, in place,
//   * an mma16 operand contracting over R: lane's k-slot e carries row 4g + e            (identity order),
//   * half of an mma32 operand contracting over R: two tiles stacked along R give k-slot (g, e) = row 4g + e of the first
//     (e < 4) or of the second (e >= 4) tile ("rho" order); the partner operand presents the same order from a row-major
//     LDS tile with two 8-byte reads at columns c0 + 4g and c0 + 16 + 4g.
// Contraction over the LANE index goes through LDS: the wave writes its tile as an image [lane index][row index] (one
// 8-byte store per lane) and reads it back with ds_read_b64_tr_b16 (private region, no barrier).
//
// Work split: 8 waves; wave w owns hidden units Hw = [32w, 32w + 32): W1[:, Hw] (tiles rows = f, lane = n), W2[Hw, :]
// (rows = n, lane = f) and a second accumulator copy W2^T[:, Hw] (rows = f, lane = n) for the contraction over f in
// gX2 = gZ2 W2^T.  Layer 1 is local to the wave; the two contractions over the hidden units leave 8 fp32 partials per
// element in LDS, which "owner" threads (16 lanes x 4 features per token) reduce.  Per step i, B* = workgroup barriers:
//   A1  Z1 = K W1 + b1 -> X2 = gelu, D1 = gelu'   (rows = t, lane = n) ; X2 image
//   A2  partial Z2^T[f, t] = W2[Hw, :]^T X2[:, Hw]^T -> redA
//   B1
//   P3  waves 0-3: sum partials + b2, fused LayerNorm / L2 backward, Gs = -eta gZ2 -> LDS [t][f] bf16
//   P6  waves 4-7, for step i-1 (off the critical path): sum the redB partials + b2, LayerNorm, + Q -> XQW
//       all: park the inputs of step i+1 (loaded one step earlier)
//   B2
//   C   b2 += colsum Gs (ones MFMA) ; W2 += X2^T Gs ; W2^T += Gs^T X2 ; gX2s = Gs W2^T (entering W2) ; gZ1s = gX2s * D1 ;
//       W1 += K^T gZ1s ; b1 += colsum gZ1s ; Z1b = Q W1' + b1' ; X2b = gelu ; X2b image
//   E   partial Z2b^T = W2'[Hw, :]^T X2b^T -> redB
// Two barriers per step are enough because every shared buffer has one writer phase and one reader phase on opposite sides
// of a barrier: redA (A2 | P3), Gs (P3 | C), redB (E | P6 of the next step), b2 in LDS (C | P3, P6), K / V double-buffered
// and Q triple-buffered (parked between B1 and B2 of the step before they are used; Q of step i-1 is still being read by
// P6 at that time, hence the third buffer).
#include "ttt_mfma.h"
#include "ttt_mfma_dev.h"
#include "ttt_dpp.h"
#include "ttt_mfma_int.h"
#define TTT_WV_FN __device__ __forceinline__
#include "ttt_lin16_body.h"
#include "ttt_lin16_split_body.h"
#include "ttt_lin64_body.h"
#include "ttt_mlp16_body.h"
#include "ttt_mlp16_bwd_body.h"
#include "ttt_mlp16_pair_body.h"
#include "once_per_device.h"

namespace ttt {
namespace mfma {
using namespace ttt::mf;

namespace v16 {

constexpr int NT16 = 512;
constexpr int CS16 = 16;
constexpr int TILE16 = CS16 * TS;                     // elements of a padded [16][64] bf16 tile
constexpr int IS = 24;                                // row stride of a wave's [32 n][16 t] image (4 rows on disjoint banks)
constexpr int L_K = 0;                                // K, V: 2 buffers each, Q: 3
constexpr int L_V = L_K + 2 * TILE16 * 2;
constexpr int L_Q = L_V + 2 * TILE16 * 2;
constexpr int L_G = L_Q + 3 * TILE16 * 2;
constexpr int L_IMG = L_G + TILE16 * 2;
constexpr int IMG_BYTES = 32 * IS * 2;
constexpr int L_REDA = L_IMG + 8 * IMG_BYTES;
constexpr int RED16_BYTES = 8 * CS16 * PS * 4;        // [8 waves][16 t][PS] fp32
constexpr int L_REDB = L_REDA + RED16_BYTES;
constexpr int L_SMALL = L_REDB + RED16_BYTES;         // eta[2][16], b2[64], gamma[64], beta[64]
constexpr int LDS_V16 = L_SMALL + (32 + 64 + 64 + 64) * 4;
static_assert(LDS_V16 <= 160 * 1024, "LDS budget");
static_assert(L_IMG % 16 == 0 && L_REDA % 16 == 0 && L_SMALL % 16 == 0, "alignment");

typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mma32(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x4 mma16(bf16x4 a, bf16x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 zero4() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }
__device__ __forceinline__ bf16x4 pack4(f32x4 v) {
    bf16x4 r = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
    return r;
}
// two tiles stacked along their row index -> one K = 32 operand in rho order
__device__ __forceinline__ bf16x8 stack(f32x4 a, f32x4 b) {
    bf16x8 r = {(__bf16)a[0], (__bf16)a[1], (__bf16)a[2], (__bf16)a[3], (__bf16)b[0], (__bf16)b[1], (__bf16)b[2], (__bf16)b[3]};
    return r;
}
// rho-order operand from this lane's row of a row-major tile: columns c0 + 4g .. +3 and c0 + 16 + 4g .. +3
__device__ __forceinline__ bf16x8 rho_read(const __bf16* rowp, int c0, int g) {
    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(rowp + c0 + 4 * g);
    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(rowp + c0 + 16 + 4 * g);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// transposed read: lane (g, i) gets img[row0 + 4g + e][col0 + i], e = 0..3  (operand with outer = column, k = row)
__device__ __forceinline__ bf16x4 tr4(const __bf16* img, int stride, int row0, int col0, int l) {
    const int g = l >> 4, i = l & 15;
    typedef __attribute__((address_space(3))) bf16x4 lds_b4;
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)(img + (row0 + 4 * g + (i >> 2)) * stride + col0 + 4 * (i & 3)));
}

// (The hand-placed 8-wave kernel of round 1, mlp_scan16_kernel, lost its round-2 A/B against the backend-templated body of
// ttt_mlp16_body.h - 3.006 vs 2.924 ms per scan at NH = 48, NC = 1128, batch 2 - and was removed; the body is also what the CPU
// suite runs on the wave emulator.)

// ---------------------------------------------------------------------------------------------------------------------------
// TTT-Linear at mini-batches of 16 tokens (the reference trains and evaluates TTT-Linear at mini_batch_size 16:
// configs/train/ttt-linear/*.toml; replaces the Triton launches linear_triton.py:98-129, :203-246).  The kernel bodies live
// in ttt_lin16_body.h, written against a wave backend so that the CPU test-suite can execute the same code on a lane-level
// emulator (tests/emul); here is the device backend: the gfx950 instructions behind those primitives.  One wave per (b, h),
// 4 waves (4 heads) per workgroup only to fill the CU's four SIMDs; no workgroup barriers.
struct DeviceWave {
    char* base;                                                       // this wave's private LDS region
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int wave() const { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
    __device__ __forceinline__ int thread() const { return threadIdx.x; }
    __device__ __forceinline__ void barrier() const { __syncthreads(); }
    __device__ __forceinline__ float exp2(float x) const { return __builtin_amdgcn_exp2f(x); }
    __device__ __forceinline__ float rcp(float x) const { return __builtin_amdgcn_rcpf(x); }
    __device__ __forceinline__ int opaque(int v) const { asm volatile("" : "+v"(v)); return v; }
    __device__ __forceinline__ void lds_fence() const { asm volatile("" ::: "memory"); }    // LDS is in order within a wave
    template <class T> __device__ __forceinline__ T& lds(int byte_off) const { return *reinterpret_cast<T*>(base + byte_off); }
    __device__ __forceinline__ char* lds_ptr(int byte_off) const { return base + byte_off; }
    template <class T> __device__ __forceinline__ T lds_load(int byte_off) const { return *reinterpret_cast<const T*>(base + byte_off); }
    template <class T> __device__ __forceinline__ void lds_store(int byte_off, T v) const { *reinterpret_cast<T*>(base + byte_off) = v; }
    __device__ __forceinline__ float rsq(float x) const { return __builtin_amdgcn_rsqf(x); }
    __device__ __forceinline__ f32x4 mma32(bf16x8 a, bf16x8 b, f32x4 c) const { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
    __device__ __forceinline__ f32x4 mma16(bf16x4 a, bf16x4 b, f32x4 c) const {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
    }
    __device__ __forceinline__ bf16x4 tr_read(int byte_addr) const {
        typedef __attribute__((address_space(3))) bf16x4 lds_b4;
        return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)(base + byte_addr));
    }
    __device__ __forceinline__ float sum16(float v) const { return ttt::sum16(v); }
    __device__ __forceinline__ float xor_add(float v, int mask) const { return v + __shfl_xor(v, mask, 64); }
};

constexpr int LIN_WAVES = 4;
constexpr int LDS_LIN = LIN_WAVES * lin16::WAVE_LDS;

// (the whole sequence or a part of it - one kernel for both: the one-call scan is the part [0, NC) without a final-state store)
__global__ __launch_bounds__(64 * LIN_WAVES) void linear_scan16_kernel(wv::Lin16ChunkParams c, int n_bh) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bh = blockIdx.x * LIN_WAVES + w;
    if (bh >= n_bh) return;                                          // whole wave; no barriers in this kernel
    DeviceWave bk{smem + w * lin16::WAVE_LDS};
    lin16::forward_part(bk, c, bh);
}

// Every kernel below but the pair scan's has one form: NAME runs BODY(bk, p, blockIdx.x) with THREADS threads, on a DeviceWave over
// the workgroup's whole dynamic LDS
#define WAVE_KERNEL(NAME, THREADS, PARAMS, BODY)                                    \
    __global__ __launch_bounds__(THREADS) void NAME(PARAMS p) {                      \
        extern __shared__ __attribute__((aligned(16))) char smem[];                  \
        DeviceWave bk{smem};                                                         \
        BODY(bk, p, blockIdx.x);                                                     \
    }

// TTT-MLP forward scan at mini-batches of 16: the backend-templated workgroup body of ttt_mlp16_body.h, over the whole sequence
// or a part of it (one kernel for both: the one-call scan is the part [0, NC) without a final-state store)
WAVE_KERNEL(mlp_scan16_body_kernel, NT16, wv::Mlp16ChunkParams, mlp16::forward_part)

// TTT-MLP forward scan at mini-batches of 16 as a PAIR of workgroups per (b, h) (ttt_mlp16_pair_body.h; opt-in): the device side of
// the hand-over policy - cdna_hip_programming.md Guideline 16 form R1, as the CS = 64 pair scan (ttt_mfma2.hip).  Record payloads are
// write-through (sc1) buffer stores, drained by every storing wave in front of the workgroup barrier that precedes the flag; ONE lane
// stores the flag word (relaxed, agent scope); the consumer polls that word (bounded by the 100 MHz wall clock: 2 s) and reads the
// payload with sc1 buffer loads only.
struct Pair16Params {
    char* ring;                       // [B NH][RING][REC_BYTES]
    unsigned* flags;                  // [B NH][FLAG_WORDS], zeroed in front of every launch
    unsigned* err;                    // host-mapped error word of the process
    int nbh, nbh8;                    // workgroup b < nbh: role A of (b, h) = b ; b >= nbh8: role B of b - nbh8 (nbh8 % 8 == 0: same XCD)
};
struct DeviceHandover {
    __amdgpu_buffer_rsrc_t rR;        // this (b, h)'s ring
    unsigned* fl;                     // this (b, h)'s flag words
    unsigned* err;
    __device__ __forceinline__ DeviceHandover(const Pair16Params& q, int bh)
        : rR(__builtin_amdgcn_make_buffer_rsrc(q.ring + (size_t)bh * mlp16::pair::RING * mlp16::pair::REC_BYTES, 0,
                                               mlp16::pair::RING * mlp16::pair::REC_BYTES, 0x00020000)),
          fl(q.flags + (size_t)bh * mlp16::pair::FLAG_WORDS), err(q.err) {}
    __device__ __forceinline__ void store16(int voff, int soff, wv::u32x4 v) const { __builtin_amdgcn_raw_buffer_store_b128(v, rR, voff, soff, 16); }
    __device__ __forceinline__ void store4(int voff, int soff, unsigned v) const { __builtin_amdgcn_raw_buffer_store_b32(v, rR, voff, soff, 16); }
    __device__ __forceinline__ wv::u32x4 load16(int voff, int soff) const { return __builtin_amdgcn_raw_buffer_load_b128(rR, voff, soff, 16); }
    __device__ __forceinline__ void drain() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
    __device__ __forceinline__ void post(int word, unsigned v) const { __hip_atomic_store(fl + word, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ unsigned peek(int word) const {
        return (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(fl + word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    __device__ __forceinline__ bool wait_ge(int word, unsigned need) const {
        bool ok = true;
        if (peek(word) < need) {
            const unsigned long long t_poll = wall_clock64();
            const unsigned long long t_lim = 200000000ull;                      // 2 s of the constant 100 MHz counter
            unsigned spins = 0u;
            do {
                __builtin_amdgcn_s_sleep(1);
                if ((++spins & 255u) == 0u && wall_clock64() - t_poll > t_lim) ok = false;
            } while (ok && peek(word) < need);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                  // no instruction: keeps the record accesses behind the poll
        return ok;
    }
    __device__ __forceinline__ void fail(int bh) const { __hip_atomic_store(err, 1u + (unsigned)bh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
};
__global__ __launch_bounds__(NT16) void mlp_pair16_kernel(wv::Mlp16ChunkParams c, Pair16Params q) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    DeviceWave bk{smem};
    const int b = (int)blockIdx.x;
    if (b < q.nbh) {
        DeviceHandover ho(q, b);
        mlp16::pair::state_role(bk, ho, c, b);
    } else if (b >= q.nbh8) {
        DeviceHandover ho(q, b - q.nbh8);
        mlp16::pair::output_role(bk, ho, c, b - q.nbh8);
    }
}

// TTT-MLP backward at mini-batches of 16 (ttt_mlp16_bwd_body.h): one workgroup of eight waves per (b, h), each owning a slice of 32 hidden
// units as in the forward, walks the checkpoint groups from the last to the first: recompute into the caller's *_init_group slots, then
// the reverse walk.  Explicit TTT_IMPL_MFMA only (capi.hip).
WAVE_KERNEL(mlp_bwd16_kernel, 64 * mlp16::bwd::WAVES, wv::Mlp16BwdParams, mlp16::bwd::backward)

// The same backward in parts (mlp16::bwd::recompute_groups / sweep_groups): the recompute of a range of checkpoint groups, one workgroup
// per (b, h, group) - any number of them, none waits for another - into the caller's slot workspace, and the reverse walk over the range
// from those slots, one workgroup per (b, h).  Same LDS map as the one-call kernel.
WAVE_KERNEL(mlp_recompute16_groups_kernel, 64 * mlp16::bwd::WAVES, wv::Mlp16BwdPartParams, mlp16::bwd::recompute_groups)
WAVE_KERNEL(mlp_sweep16_groups_kernel, 64 * mlp16::bwd::WAVES, wv::Mlp16BwdPartParams, mlp16::bwd::sweep_groups)

// backward: one wave per workgroup (48 .. 96 scans on 256 CUs: a CU of its own per scan; up to 512 registers per lane)
WAVE_KERNEL(linear_bwd16_kernel, 64, wv::Lin16Params, lin16::backward)

// TTT-Linear at mini-batches of 64 tokens (ttt_lin64_body.h): one workgroup of four waves per (b, h), one wave per SIMD - up to 512
// registers per lane.  Runs on an explicit TTT_IMPL_MFMA only (capi.hip: resolve()).  The forward kernel serves the one-call scan
// and the scan in parts alike, as at mini-batches of 16.
WAVE_KERNEL(linear_fwd_cs64_kernel, 64 * lin64::WAVES, wv::Lin16ChunkParams, lin64::forward_part)
WAVE_KERNEL(linear_bwd_cs64_kernel, 64 * lin64::WAVES, wv::Lin16Params, lin64::backward)

// The TTT-Linear backward in parts (lin16:: / lin64::recompute_groups, sweep_groups): the recompute of a range of checkpoint groups,
// one wave (mini-batches of 16) or one four-wave workgroup (of 64) per (b, h, group), and the reverse walk over the range from the
// slots it left, one per (b, h).  Neither keeps the state that ends a group in LDS: their LDS ends where L_WHI begins.
WAVE_KERNEL(linear_recompute16_groups_kernel, 64, wv::Lin16BwdPartParams, lin16::recompute_groups)
WAVE_KERNEL(linear_sweep16_groups_kernel, 64, wv::Lin16BwdPartParams, lin16::sweep_groups)
WAVE_KERNEL(linear_recompute_cs64_groups_kernel, 64 * lin64::WAVES, wv::Lin16BwdPartParams, lin64::recompute_groups)
WAVE_KERNEL(linear_sweep_cs64_groups_kernel, 64 * lin64::WAVES, wv::Lin16BwdPartParams, lin64::sweep_groups)

// A third stage of the backward in parts at mini-batches of 16 (lin16::front_groups, chain_groups): the half of every reverse step
// that does not depend on the carried gradients, one wave per (b, h, step of the range), and the walk that consumes its records,
// one wave per (b, h).
WAVE_KERNEL(linear_front16_groups_kernel, 64, wv::Lin16BwdFrontParams, lin16::front_groups)
WAVE_KERNEL(linear_chain16_groups_kernel, 64, wv::Lin16BwdFrontParams, lin16::chain_groups)

// The same stage at mini-batches of 64 (lin64::front_groups, chain_groups): the front as one wave per (b, h, step of the range,
// 16-row token block) on the LDS map of the mini-batch-16 body, the chain as one four-wave workgroup per (b, h).
WAVE_KERNEL(linear_front_cs64_groups_kernel, 64, wv::Lin16BwdFrontParams, lin64::front_groups)
WAVE_KERNEL(linear_chain_cs64_groups_kernel, 64 * lin64::WAVES, wv::Lin16BwdFrontParams, lin64::chain_groups)

// The CS = 16 forward scan with its output path on a second wave (ttt_lin16_split_body.h; opt-in): one workgroup of two waves per
// (b, h) - the chain role and the output role, on two SIMDs of the compute unit, one workgroup barrier per step.  The second kernel
// is the bench tool's chain-alone arm: the output role keeps only its barriers.
WAVE_KERNEL(linear_split16_kernel, 64 * lin16::split::WAVES, wv::Lin16ChunkParams, lin16::split::forward_part)
WAVE_KERNEL(linear_split16_chain_alone_kernel, 64 * lin16::split::WAVES, wv::Lin16ChunkParams, lin16::split::chain_alone_part)
#undef WAVE_KERNEL

}  // namespace v16

// Host side: one ttt::launch_lds per kernel (once_per_device.h) - grid, threads and the dynamic LDS, which is also the limit the
// kernel's attribute is raised to at its first launch on a device.
constexpr int T_LIN64 = 64 * lin64::WAVES, T_MLP_BWD = 64 * mlp16::bwd::WAVES;

void launch_linear_forward_cs16(const wv::Lin16ChunkParams& c, int n_bh, hipStream_t s) {
    const int blocks = (n_bh + v16::LIN_WAVES - 1) / v16::LIN_WAVES;
    launch_lds<v16::linear_scan16_kernel>(blocks, 64 * v16::LIN_WAVES, v16::LDS_LIN, s, c, n_bh);
}
static int g_split16_chain_alone = 0;      // DEBUG (tools/lin16_split_bench.py): 1 = the split scan without its output role's work
void set_debug_lin_split16_chain_alone(int v) { g_split16_chain_alone = v; }
void launch_linear_forward_split16(const wv::Lin16ChunkParams& c, int n_bh, hipStream_t s) {
    constexpr int T = 64 * lin16::split::WAVES;
    if (g_split16_chain_alone) launch_lds<v16::linear_split16_chain_alone_kernel>(n_bh, T, lin16::split::GROUP_LDS, s, c);
    else launch_lds<v16::linear_split16_kernel>(n_bh, T, lin16::split::GROUP_LDS, s, c);
}
void launch_linear_backward_cs16(const wv::Lin16Params& p, int n_bh, hipStream_t s) {
    launch_lds<v16::linear_bwd16_kernel>(n_bh, 64, lin16::WAVE_LDS_BWD, s, p);
}
void launch_linear_forward_cs64(const wv::Lin16ChunkParams& c, int n_bh, hipStream_t s) {
    launch_lds<v16::linear_fwd_cs64_kernel>(n_bh, T_LIN64, lin64::GROUP_LDS, s, c);
}
void launch_linear_backward_cs64(const wv::Lin16Params& p, int n_bh, hipStream_t s) {
    launch_lds<v16::linear_bwd_cs64_kernel>(n_bh, T_LIN64, lin64::GROUP_LDS_BWD, s, p);
}
void launch_linear_recompute_groups(const wv::Lin16BwdPartParams& q, int cs, int n_bh, hipStream_t s) {
    if (cs == 16) launch_lds<v16::linear_recompute16_groups_kernel>(n_bh * q.nk, 64, lin16::L_WHI, s, q);
    else launch_lds<v16::linear_recompute_cs64_groups_kernel>(n_bh * q.nk, T_LIN64, lin64::L_WHI, s, q);
}
void launch_linear_sweep_groups(const wv::Lin16BwdPartParams& q, int cs, int n_bh, hipStream_t s) {
    if (cs == 16) launch_lds<v16::linear_sweep16_groups_kernel>(n_bh, 64, lin16::L_WHI, s, q);
    else launch_lds<v16::linear_sweep_cs64_groups_kernel>(n_bh, T_LIN64, lin64::L_WHI, s, q);
}
void launch_linear_front_groups(const wv::Lin16BwdFrontParams& f, int n_units, hipStream_t s) {
    launch_lds<v16::linear_front16_groups_kernel>(n_units, 64, lin16::WAVE_LDS, s, f);
}
void launch_linear_chain_groups(const wv::Lin16BwdFrontParams& f, int n_bh, hipStream_t s) {
    launch_lds<v16::linear_chain16_groups_kernel>(n_bh, 64, lin16::WAVE_LDS_CHAIN, s, f);
}
void launch_linear_front64_groups(const wv::Lin16BwdFrontParams& f, int n_units, hipStream_t s) {
    launch_lds<v16::linear_front_cs64_groups_kernel>(n_units, 64, lin16::WAVE_LDS, s, f);
}
void launch_linear_chain64_groups(const wv::Lin16BwdFrontParams& f, int n_bh, hipStream_t s) {
    launch_lds<v16::linear_chain_cs64_groups_kernel>(n_bh, T_LIN64, lin64::GROUP_LDS_CHAIN, s, f);
}

// a part of the sequence (mlp_forward_chunk): p.NC steps from step p.ck0 of p.NCs, the pointers those of the whole sequence
// (at CS = 16 a part may start at any step, so ck0 carries the first STEP, not a checkpoint index).  p.NCs == 0: one call.
static wv::Mlp16ChunkParams mlp16_chunk_params(const ScanParams& p) {
    const int NCs = p.NCs ? p.NCs : p.NC, step0 = p.NCs ? p.ck0 : 0;
    return {mlp16_params(p), step0, NCs, p.W1f, p.b1f, p.W2f, p.b2f};
}
void launch_scan_forward_cs16(const ScanParams& p, int n_bh, unsigned long long*, hipStream_t s) {
    launch_lds<v16::mlp_scan16_body_kernel>(n_bh, v16::NT16, mlp16::GROUP_LDS, s, mlp16_chunk_params(p));
}

// The pair form of the scan above (opt-in: ttt_hip_mlp_forward_chunk_pair16).  `ws`: scan_pair16_workspace_bytes(n_bh) bytes - the flag
// words of every (b, h) first, in a block of their own that is zeroed in front of EVERY launch, then the rings.  Both workgroups of
// every pair must be resident (role B polls): where n_bh8 + n_bh workgroups do not fit the device the one-workgroup kernel runs.
// 0 = enqueued as pairs, 1 = enqueued on the one-workgroup kernel, -1 = no host-mapped error word (nothing enqueued).
size_t scan_pair16_workspace_bytes(int n_bh) { return mlp16::pair::workspace_bytes(n_bh); }
int launch_scan_forward_pair16(const ScanParams& p, int n_bh, void* ws, hipStream_t s) {
    const int n_bh8 = (n_bh + 7) & ~7;
    if (n_bh8 + n_bh > device_cu_count()) {
        launch_scan_forward_cs16(p, n_bh, nullptr, s);
        return 1;
    }
    unsigned* err = sweep_error_word();
    if (!err) return -1;
    v16::Pair16Params q = {};
    q.flags = (unsigned*)ws;
    q.ring = (char*)ws + mlp16::pair::flags_bytes(n_bh);
    q.err = err;
    q.nbh = n_bh; q.nbh8 = n_bh8;
    (void)hipMemsetAsync(q.flags, 0, mlp16::pair::flags_bytes(n_bh), s);       // the flags restart at 0 for every launch
    launch_lds<v16::mlp_pair16_kernel>(n_bh8 + n_bh, v16::NT16, mlp16::pair::PAIR_LDS, s, mlp16_chunk_params(p), q);
    return 0;
}

void launch_mlp_backward_cs16(const wv::Mlp16BwdParams& p, int n_bh, hipStream_t s) {
    launch_lds<v16::mlp_bwd16_kernel>(n_bh, T_MLP_BWD, mlp16::bwd::GROUP_LDS_BWD, s, p);
}
void launch_mlp_recompute_groups(const wv::Mlp16BwdPartParams& q, int n_bh, hipStream_t s) {
    launch_lds<v16::mlp_recompute16_groups_kernel>(n_bh * q.nk, T_MLP_BWD, mlp16::bwd::GROUP_LDS_BWD, s, q);
}
void launch_mlp_sweep_groups(const wv::Mlp16BwdPartParams& q, int n_bh, hipStream_t s) {
    launch_lds<v16::mlp_sweep16_groups_kernel>(n_bh, T_MLP_BWD, mlp16::bwd::GROUP_LDS_BWD, s, q);
}

}  // namespace mfma
}  // namespace ttt
