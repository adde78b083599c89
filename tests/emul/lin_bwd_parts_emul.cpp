// Host build of the TTT-Linear backward in parts (recompute_groups / sweep_groups of csrc/ttt_lin16_body.h: one wave per unit of work;
// of csrc/ttt_lin64_body.h: one workgroup of four waves) and of the one-call backward() of the same bodies on the wave emulator: TEST
// INFRASTRUCTURE, compiled on the fly by tests/test_emul_lin_bwd_parts_cpu.py with the host clang of the ROCm toolchain.  `cs` selects
// the geometry (16 or 64); `n` is the size of the grid the device launch would have (B*NH*nk for the recompute, B*NH otherwise).
// Every entry returns the number of LDS races the detector saw (0 expected; a single wave has none); the first one is described in `msg`.
#include <cstdio>

#include "wave_emul.h"

#include "ttt_lin64_body.h"

using namespace ttt;

template <class F16, class F64>
static int run_grid(int cs, int n, char* msg, int msg_len, F16 body16, F64 body64) {
    if (cs != 16 && cs != 64) return -1;
    int races = 0;
    for (int u = 0; u < n; ++u) {
        if (cs == 16) {
            emul::run_wave([&](emul::EmulWave& w) { body16(w, u); });
            continue;
        }
        const emul::RaceReport r = emul::run_group(lin64::WAVES, [&](emul::EmulWave& w) { body64(w, u); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

extern "C" {

int emul_lin_backward(int cs, const wv::Lin16Params* p, int n, char* msg, int msg_len) {
    return run_grid(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin16::backward(w, *p, u); },
                    [&](emul::EmulWave& w, int u) { lin64::backward(w, *p, u); });
}
int emul_lin_recompute_groups(int cs, const wv::Lin16BwdPartParams* q, int n, char* msg, int msg_len) {
    return run_grid(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin16::recompute_groups(w, *q, u); },
                    [&](emul::EmulWave& w, int u) { lin64::recompute_groups(w, *q, u); });
}
int emul_lin_sweep_groups(int cs, const wv::Lin16BwdPartParams* q, int n, char* msg, int msg_len) {
    return run_grid(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin16::sweep_groups(w, *q, u); },
                    [&](emul::EmulWave& w, int u) { lin64::sweep_groups(w, *q, u); });
}
// the forward that leaves the checkpoints
int emul_lin_forward(int cs, const wv::Lin16Params* p, int n, char* msg, int msg_len) {
    return run_grid(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin16::forward(w, *p, u); },
                    [&](emul::EmulWave& w, int u) { lin64::forward(w, *p, u); });
}

int emul_lin_params_size() { return (int)sizeof(wv::Lin16Params); }
int emul_lin_bwd_part_params_size() { return (int)sizeof(wv::Lin16BwdPartParams); }
int emul_lin_part_slot_bytes() { return (int)wv::LIN_PART_SLOT_BYTES; }
int emul_lin_part_carry_floats(int cs) { return wv::LIN_PART_CARRY_FLOATS * (cs == 16 ? 64 : 64 * lin64::WAVES); }
}
