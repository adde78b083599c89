// Host build of the third stage of the TTT-Linear backward in parts at mini-batches of 64 (front_groups / chain_groups of
// csrc/ttt_lin64_body.h) beside recompute_groups, sweep_groups and the one-call backward() of the same body on the wave emulator: TEST
// INFRASTRUCTURE, compiled on the fly by tests/test_emul_lin64_bwd_front_cpu.py with the host clang of the ROCm toolchain.  The front
// runs as SINGLE waves (one per 16-row token block: it has no workgroup), everything else as workgroups of four waves under the LDS
// race detector.  `n` is the size of the grid the device launch would have (B*NH*nk for the recompute, B*NH*steps of the range*4 for
// the front, B*NH otherwise).  Every entry returns the number of LDS races the detector saw; the first one is described in `msg`.
#include <cstdio>

#include "wave_emul.h"

#include "ttt_lin64_body.h"

using namespace ttt;

template <class F>
static int run_groups(int cs, int n, char* msg, int msg_len, F body) {
    if (cs != 64) return -1;                     // (the entries take the arguments of tests/emul/lin_bwd_parts_emul.cpp)
    int races = 0;
    for (int u = 0; u < n; ++u) {
        const emul::RaceReport r = emul::run_group(lin64::WAVES, [&](emul::EmulWave& w) { body(w, u); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

extern "C" {

int emul_lin_forward(int cs, const wv::Lin16Params* p, int n, char* msg, int msg_len) {
    return run_groups(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin64::forward(w, *p, u); });
}
int emul_lin_backward(int cs, const wv::Lin16Params* p, int n, char* msg, int msg_len) {
    return run_groups(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin64::backward(w, *p, u); });
}
int emul_lin_recompute_groups(int cs, const wv::Lin16BwdPartParams* q, int n, char* msg, int msg_len) {
    return run_groups(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin64::recompute_groups(w, *q, u); });
}
int emul_lin_sweep_groups(int cs, const wv::Lin16BwdPartParams* q, int n, char* msg, int msg_len) {
    return run_groups(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin64::sweep_groups(w, *q, u); });
}
int emul_lin_front_groups(int cs, const wv::Lin16BwdFrontParams* f, int n, char*, int) {
    if (cs != 64) return -1;
    for (int u = 0; u < n; ++u) emul::run_wave([&](emul::EmulWave& w) { lin64::front_groups(w, *f, u); });
    return 0;
}
int emul_lin_chain_groups(int cs, const wv::Lin16BwdFrontParams* f, int n, char* msg, int msg_len) {
    return run_groups(cs, n, msg, msg_len, [&](emul::EmulWave& w, int u) { lin64::chain_groups(w, *f, u); });
}

int emul_lin_params_size() { return (int)sizeof(wv::Lin16Params); }
int emul_lin_bwd_part_params_size() { return (int)sizeof(wv::Lin16BwdPartParams); }
int emul_lin_bwd_front_params_size() { return (int)sizeof(wv::Lin16BwdFrontParams); }
int emul_lin_part_slot_bytes() { return (int)wv::LIN_PART_SLOT_BYTES; }
int emul_lin_part_carry_floats(int) { return wv::LIN_PART_CARRY_FLOATS * 64 * lin64::WAVES; }
int emul_lin_front_record_bytes() { return (int)wv::LIN64_FRONT_RECORD_BYTES; }
int emul_lin_front_block_record_bytes() { return (int)wv::LIN_FRONT_RECORD_BYTES; }
int emul_lin_chain_lds_bytes() { return lin64::GROUP_LDS_CHAIN; }
}
