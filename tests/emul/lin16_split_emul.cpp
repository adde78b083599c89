// Host build of the two-wave TTT-Linear forward scan at mini-batches of 16 (lin16::split::forward_part of
// csrc/ttt_lin16_split_body.h: chain role on wave 0, output role on wave 1, hand-over through two LDS slots) on the wave emulator:
// TEST INFRASTRUCTURE, compiled on the fly by tests/test_emul_lin16_split_cpu.py with the host clang of the ROCm toolchain.  One
// emulated two-wave workgroup per (b, h); the entry returns the number of LDS races the detector saw (0 expected; the first one is
// described in `msg`).  The one-wave lin16::forward_part is exposed beside it for the comparison.
#include <cstdio>

#include "wave_emul.h"

#include "ttt_lin16_split_body.h"

using namespace ttt;

extern "C" {

int emul_lin16_split_forward_part(const wv::Lin16ChunkParams* c, int n_bh, char* msg, int msg_len) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const emul::RaceReport r = emul::run_group(lin16::split::WAVES, [&](emul::EmulWave& w) { lin16::split::forward_part(w, *c, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

// the chain role with an output role that only keeps the barrier count (the bench tool's --chain-alone arm): `out` stays untouched
int emul_lin16_split_chain_alone_part(const wv::Lin16ChunkParams* c, int n_bh, char* msg, int msg_len) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const emul::RaceReport r = emul::run_group(lin16::split::WAVES, [&](emul::EmulWave& w) { lin16::split::chain_alone_part(w, *c, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

// the one-wave body, for the comparison
int emul_lin16_forward_part(const wv::Lin16ChunkParams* c, int n_bh) {
    for (int bh = 0; bh < n_bh; ++bh) emul::run_wave([&](emul::EmulWave& w) { lin16::forward_part(w, *c, bh); });
    return 0;
}

int emul_lin16_split_lds_bytes() { return lin16::split::GROUP_LDS; }
int emul_lin16_split_slot_bytes() { return lin16::split::SLOT_BYTES; }
int emul_lin16_wave_lds_bytes() { return lin16::WAVE_LDS; }
int emul_lin_chunk_params_size() { return (int)sizeof(wv::Lin16ChunkParams); }
}
