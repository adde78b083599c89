// Host build of the TTT-Linear forward scan bodies over a PART of the sequence (lin16::forward_part of csrc/ttt_lin16_body.h: one
// wave per (b, h); lin64::forward_part of csrc/ttt_lin64_body.h: one workgroup of four waves per (b, h)) on the wave emulator: TEST
// INFRASTRUCTURE, compiled on the fly by tests/test_emul_lin_parts_cpu.py with the host clang of the ROCm toolchain.  `cs` selects the
// geometry (16 or 64).  Every entry returns the number of LDS races the detector saw (0 expected; a single wave has none); the first
// one is described in `msg`.
#include <cstdio>

#include "wave_emul.h"

#include "ttt_lin64_body.h"

using namespace ttt;

template <class F16, class F64>
static int run_scans(int cs, int n_bh, char* msg, int msg_len, F16 body16, F64 body64) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        if (cs == 16) {
            emul::run_wave([&](emul::EmulWave& w) { body16(w, bh); });
            continue;
        }
        const emul::RaceReport r = emul::run_group(lin64::WAVES, [&](emul::EmulWave& w) { body64(w, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

extern "C" {

int emul_lin_forward_part(int cs, const wv::Lin16ChunkParams* c, int n_bh, char* msg, int msg_len) {
    if (cs != 16 && cs != 64) return -1;
    return run_scans(cs, n_bh, msg, msg_len, [&](emul::EmulWave& w, int bh) { lin16::forward_part(w, *c, bh); },
                     [&](emul::EmulWave& w, int bh) { lin64::forward_part(w, *c, bh); });
}

// the whole-sequence entries (what tests/emul/lin16_emul.cpp and lin64_emul.cpp run): must be the part [0, NC) of the same bodies
int emul_lin_forward_whole(int cs, const wv::Lin16Params* p, int n_bh, char* msg, int msg_len) {
    if (cs != 16 && cs != 64) return -1;
    return run_scans(cs, n_bh, msg, msg_len, [&](emul::EmulWave& w, int bh) { lin16::forward(w, *p, bh); },
                     [&](emul::EmulWave& w, int bh) { lin64::forward(w, *p, bh); });
}

int emul_lin_params_size() { return (int)sizeof(wv::Lin16Params); }
int emul_lin_chunk_params_size() { return (int)sizeof(wv::Lin16ChunkParams); }
}
