// Plain vector / parameter types shared by the wave-level kernel bodies (ttt_lin16_body.h), the device backend
// (ttt_mfma16.hip) and the host-side wave emulator used by the CPU tests (tests/emul).  No HIP dependency.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ttt {
namespace wv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// arguments of the TTT-Linear scans at mini-batches of 16 tokens (F = 64)
struct Lin16Params {
    const __bf16 *XQ, *XK, *XV, *eta;      // [B,NH,NC,16,64] x3, [B,NH,NC,16,1]
    const float *ln_w, *ln_b;               // [NH,64]
    const float *W1, *b1;                   // forward: initial state [B,NH,64,64], [B,NH,1,64]
    float *W1c, *b1c;                       // checkpoints [B,NH,K,64,64], [B,NH,K,1,64] (forward: written; backward: read)
    __bf16* out;                            // forward: XQW
    // backward
    const __bf16* dOut;                     // [B,NH,NC,16,64]
    const float *dW1_last, *db1_last;       // upstream gradient of the final state
    char* scratch_w;                        // [B,NH,G] x 16 KiB: per-step state as packed operands (W1_init_group storage)
    float* scratch_b;                       // [B,NH,G,64]
    float *dln_w, *dln_b;                   // [B,NH,1,64]
    float *dW1, *db1;                       // [B,NH,64,64], [B,NH,1,64]
    __bf16 *deta, *dXQ, *dXK, *dXV;
    int NH, NC, G, K;
    float eps;
};

// the TTT-Linear forward scan (mini-batches of 16: ttt_lin16_body.h, of 64: ttt_lin64_body.h) over a PART of the sequence: steps
// [step0, step0 + p.NC) of a sequence of NCs steps.  The pointers of `p` are those of the whole sequence (consecutive heads NCs
// tiles apart, p.K = ceil(NCs / G) checkpoints per head); p.W1, p.b1 hold the state entering step0; the state after the last
// step of the part goes to W1f, b1f (layout of the initial state, may alias it; both null: not stored).  A part starts at any
// step: the kernels hold the whole state in fp32 and rebuild everything else a step takes from its predecessor from it.
// step0 = 0, NCs = p.NC, no final state: the one-call scan.
struct Lin16ChunkParams {
    Lin16Params p;
    int step0, NCs;
    float *W1f, *b1f;
};

// the TTT-Linear backward in parts (ttt_lin16_body.h / ttt_lin64_body.h: recompute_groups, sweep_groups): the checkpoint groups
// [k0, k0 + nk) of the K = p.K groups of the sequence that `p` describes (whole-sequence pointers; p.scratch_w / p.scratch_b unused).
// `slots`: [B*NH][nk][G + 1] slots of LIN_PART_SLOT_BYTES - slot j of a group is the state ENTERING its step j as packed operands in
// both orientations (the 16 KiB of lin16::SLOT_BYTES) followed by the bias row (64 fp32); slot `steps of the group` is the state that
// ends it (a ragged last group uses fewer than G + 1).  recompute_groups writes them from the checkpoints, sweep_groups reads them.
// `ln_carry`: [B*NH][8][lanes of the scan] fp32, the un-reduced per-lane partial sums of dgamma (rows 0..3) and dbeta (4..7) - 64 lanes
// at mini-batches of 16, 256 at mini-batches of 64 (LIN_PART_CARRY_FLOATS per lane) - handed from one sweep_groups call to the next.
constexpr size_t LIN_PART_SLOT_BYTES = 16 * 1024 + 64 * sizeof(float);
constexpr int LIN_PART_CARRY_FLOATS = 8;
struct Lin16BwdPartParams {
    Lin16Params p;
    int k0, nk;
    char* slots;
    float* ln_carry;
};

// a third stage of the TTT-Linear backward in parts, mini-batches of 16 only (ttt_lin16_body.h: front_groups, chain_groups): the half
// of every reverse step that does not depend on the carried gradients runs for all steps of the range `q` at once and leaves, per
// step, a record of LIN_FRONT_RECORD_BYTES for the walk: per lane dZ1b as bf16 (32 bytes), its column sums (16), the addends of the
// dgamma / dbeta partial sums (32), the inner LayerNorm's x_hat, output gradient and dZ1 (192), 1/std and sum_f (go gamma) x_hat (32).
// `records`: [B*NH][nk][G] records (a ragged last group uses fewer) ; q.slots: what recompute_groups left for the same range ;
// front_groups does not touch q.ln_carry.
constexpr size_t LIN_FRONT_RECORD_BYTES = 64 * (32 + 16 + 32 + 192 + 32);      // 19 456
struct Lin16BwdFrontParams {
    Lin16BwdPartParams q;
    char* records;
};
// the same stage at mini-batches of 64 (ttt_lin64_body.h: front_groups, chain_groups), with the same parameter block: a step's
// record is the four records of its 16-row token blocks, [w][field][lane] - each in the layout above, written by the wave that runs
// the front of block w and read by wave w of the chain.
constexpr size_t LIN64_FRONT_RECORD_BYTES = 4 * LIN_FRONT_RECORD_BYTES;        // 77 824

// arguments of the TTT-MLP forward scan at mini-batches of 16 tokens (F = 64, hidden 256)
struct Mlp16Params {
    const __bf16 *XQ, *XK, *XV, *eta;
    const float *ln_w, *ln_b;               // [NH,64] (also addressed as [1,NH,1,64])
    const float *W1, *b1, *W2, *b2;         // initial state [B,NH,64,256], [B,NH,1,256], [B,NH,256,64], [B,NH,1,64]
    float *W1c, *b1c, *W2c, *b2c;           // checkpoints [B,NH,K,...]
    __bf16* out;
    int NH, NC, G, K;
    float eps;
};

// the same scan over a PART of the sequence: steps [step0, step0 + p.NC) of a sequence of NCs steps.  The pointers of `p` are
// those of the whole sequence (consecutive heads NCs tiles apart, K = ceil(NCs / G) checkpoints per head); p.W1 .. p.b2 hold the
// state entering step0; the state after the last step of the part goes to W1f .. b2f (layout of the initial state, may alias
// it; all null: not stored).  step0 = 0, NCs = p.NC, no final state: the one-call scan.
struct Mlp16ChunkParams {
    Mlp16Params p;
    int step0, NCs;
    float *W1f, *b1f, *W2f, *b2f;
};

// arguments of the TTT-MLP backward at mini-batches of 16 tokens (ttt_mlp16_bwd_body.h)
struct Mlp16BwdParams {
    const __bf16 *XQ, *XK, *XV, *eta;       // [B,NH,NC,16,64] x3, [B,NH,NC,16,1]
    const float *ln_w, *ln_b;               // [NH,64]
    const float *W1c, *b1c, *W2c, *b2c;     // checkpoints [B,NH,K,...] (read only)
    const __bf16* dOut;                     // [B,NH,NC,16,64]
    const float *dW1_last, *db1_last, *dW2_last, *db2_last;      // upstream gradient of the final state
    float *W1s, *b1s, *W2s, *b2s;           // the four *_init_group buffers [B,NH,G,64,256], [B,NH,G,1,256], [B,NH,G,256,64], [B,NH,G,1,64]
    float *dln_w, *dln_b;                   // [B,NH,1,64]
    float *dW1, *db1, *dW2, *db2;           // gradient of the initial state (carried here between the groups of the call)
    __bf16 *deta, *dXQ, *dXK, *dXV;
    int NH, NC, G, K;
    float eps;
};

// the TTT-MLP backward at mini-batches of 16 in parts (ttt_mlp16_bwd_body.h: recompute_groups, sweep_groups): the checkpoint groups
// [k0, k0 + nk) of the K = p.K groups of the sequence that `p` describes (whole-sequence pointers; p.W1s .. p.b2s unused).
// `slots`: [B*NH][nk][G] slots of MLP16_PART_SLOT_FLOATS fp32 - slot j of a group is the state ENTERING its step j: W1 [64,256],
// b1 [256], W2 [256,64], b2 [64], one after the other (a ragged last group uses fewer than G).  recompute_groups writes them from the
// checkpoints, sweep_groups reads them.  `ln_carry`: [B*NH][2][16][64] fp32, the owner threads' un-reduced shares of dln_w and dln_b
// (the B_DLNW / B_DLNB cells of the one-call kernel's LDS), handed from one sweep_groups call to the next.
constexpr size_t MLP16_PART_W1_OFS = 0, MLP16_PART_B1_OFS = 64 * 256, MLP16_PART_W2_OFS = MLP16_PART_B1_OFS + 256,
                 MLP16_PART_B2_OFS = MLP16_PART_W2_OFS + 256 * 64, MLP16_PART_SLOT_FLOATS = MLP16_PART_B2_OFS + 64;
constexpr size_t MLP16_PART_SLOT_BYTES = MLP16_PART_SLOT_FLOATS * sizeof(float);      // 132 352
constexpr size_t MLP16_PART_CARRY_FLOATS = 2 * 16 * 64;
struct Mlp16BwdPartParams {
    Mlp16BwdParams p;
    int k0, nk;
    float* slots;
    float* ln_carry;
};

}  // namespace wv
}  // namespace ttt
