// Host build of the TTT-Linear (mini-batch 64) workgroup-level kernel bodies on the wave emulator: TEST INFRASTRUCTURE, compiled on
// the fly by tests/test_emul_lin64_cpu.py with the host clang of the ROCm toolchain.  Every (b, h) scan is one emulated workgroup
// of four waves (256 host threads).  Both entry points return the number of LDS races the detector saw (0 expected); the first one
// is described in `msg`.
#include <cstdio>

#include "wave_emul.h"

#include "ttt_lin64_body.h"

using namespace ttt;

template <class F>
static int run_scans(int n_bh, char* msg, int msg_len, F body) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const emul::RaceReport r = emul::run_group(lin64::WAVES, [&](emul::EmulWave& w) { body(w, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

extern "C" {

int emul_lin64_forward(const wv::Lin16Params* p, int n_bh, char* msg, int msg_len) {
    return run_scans(n_bh, msg, msg_len, [&](emul::EmulWave& w, int bh) { lin64::forward(w, *p, bh); });
}

int emul_lin64_backward(const wv::Lin16Params* p, int n_bh, char* msg, int msg_len) {
    return run_scans(n_bh, msg, msg_len, [&](emul::EmulWave& w, int bh) { lin64::backward(w, *p, bh); });
}

int emul_lin64_params_size() { return (int)sizeof(wv::Lin16Params); }
int emul_lin64_lds_bytes(int backward) { return backward ? lin64::GROUP_LDS_BWD : lin64::GROUP_LDS; }
}
