// Host build of the TTT-MLP (mini-batch 16) backward body (mlp16::bwd::backward of csrc/ttt_mlp16_bwd_body.h) and of the forward scan
// it re-runs (mlp16::forward) on the wave emulator: TEST INFRASTRUCTURE, compiled on the fly by tests/test_emul_mlp16_bwd_cpu.py
// with the host clang of the ROCm toolchain.  One emulated workgroup of eight waves per (b, h).
#include <cstdio>

#include "wave_emul.h"

#include "ttt_lin16_body.h"
#include "ttt_mlp16_body.h"
#include "ttt_mlp16_bwd_body.h"

using namespace ttt;

extern "C" {

// returns the number of LDS races the detector saw (0 expected); the first one is described in `msg`
int emul_mlp16_backward(const wv::Mlp16BwdParams* p, int n_bh, char* msg, int msg_len) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const emul::RaceReport r = emul::run_group(mlp16::bwd::WAVES, [&](emul::EmulWave& w) { mlp16::bwd::backward(w, *p, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

int emul_mlp16_forward(const wv::Mlp16Params* p, int n_bh, char* msg, int msg_len) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const emul::RaceReport r = emul::run_group(8, [&](emul::EmulWave& w) { mlp16::forward(w, *p, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

int emul_mlp16_bwd_params_size() { return (int)sizeof(wv::Mlp16BwdParams); }
int emul_mlp16_params_size() { return (int)sizeof(wv::Mlp16Params); }
int emul_mlp16_bwd_lds_bytes() { return mlp16::bwd::GROUP_LDS_BWD; }
}
