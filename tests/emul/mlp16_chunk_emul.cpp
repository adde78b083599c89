// Host build of the TTT-MLP (mini-batch 16) forward scan body over a PART of the sequence (mlp16::forward_part of
// csrc/ttt_mlp16_body.h) on the wave emulator: TEST INFRASTRUCTURE, compiled on the fly by tests/test_mlp16_chunk_emul_cpu.py
// with the host clang of the ROCm toolchain.  One emulated 8-wave workgroup per (b, h).
#include <cstdio>

#include "wave_emul.h"

#include "ttt_lin16_body.h"
#include "ttt_mlp16_body.h"

using namespace ttt;

extern "C" {

// returns the number of LDS races the detector saw (0 expected); the first one is described in `msg`
int emul_mlp16_forward_part(const wv::Mlp16ChunkParams* c, int n_bh, char* msg, int msg_len) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const emul::RaceReport r = emul::run_group(8, [&](emul::EmulWave& w) { mlp16::forward_part(w, *c, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

// the whole-sequence entry (what the one-call kernel and tests/emul/lin16_emul.cpp run): must be the part [0, NC) of the same body
int emul_mlp16_forward_whole(const wv::Mlp16Params* p, int n_bh, char* msg, int msg_len) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const emul::RaceReport r = emul::run_group(8, [&](emul::EmulWave& w) { mlp16::forward(w, *p, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

int emul_mlp16_chunk_params_size() { return (int)sizeof(wv::Mlp16ChunkParams); }
}
