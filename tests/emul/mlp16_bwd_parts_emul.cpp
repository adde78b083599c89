// Host build of the TTT-MLP (mini-batch 16) backward in parts (mlp16::bwd::recompute_groups / sweep_groups of
// csrc/ttt_mlp16_bwd_body.h) on the wave emulator: TEST INFRASTRUCTURE, compiled on the fly by tests/mlp16_bwd_parts_cases.py with the
// host clang of the ROCm toolchain.  One emulated workgroup of eight waves per unit of work; `n` is the size of the grid the device
// launch would have (B*NH*nk for the recompute, B*NH for the sweep).  The one-call backward() and the forward of the same bodies are in
// mlp16_bwd_emul.cpp.  Every entry returns the number of LDS races the detector saw (0 expected); the first one is described in `msg`.
#include <cstdio>

#include "wave_emul.h"

#include "ttt_lin16_body.h"
#include "ttt_mlp16_body.h"
#include "ttt_mlp16_bwd_body.h"

using namespace ttt;

template <class F>
static int run_grid(int n, char* msg, int msg_len, F body) {
    int races = 0;
    for (int u = 0; u < n; ++u) {
        const emul::RaceReport r = emul::run_group(mlp16::bwd::WAVES, [&](emul::EmulWave& w) { body(w, u); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

extern "C" {

int emul_mlp16_recompute_groups(const wv::Mlp16BwdPartParams* q, int n, char* msg, int msg_len) {
    return run_grid(n, msg, msg_len, [&](emul::EmulWave& w, int u) { mlp16::bwd::recompute_groups(w, *q, u); });
}
int emul_mlp16_sweep_groups(const wv::Mlp16BwdPartParams* q, int n, char* msg, int msg_len) {
    return run_grid(n, msg, msg_len, [&](emul::EmulWave& w, int u) { mlp16::bwd::sweep_groups(w, *q, u); });
}

int emul_mlp16_bwd_part_params_size() { return (int)sizeof(wv::Mlp16BwdPartParams); }
int emul_mlp16_part_slot_bytes() { return (int)wv::MLP16_PART_SLOT_BYTES; }
int emul_mlp16_part_carry_floats() { return (int)wv::MLP16_PART_CARRY_FLOATS; }
}
