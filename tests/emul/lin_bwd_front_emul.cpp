// Host build of the third stage of the TTT-Linear backward in parts at mini-batches of 16 (front_groups / chain_groups of
// csrc/ttt_lin16_body.h, one wave per unit of work) beside recompute_groups, sweep_groups and the one-call backward() of the same body
// on the wave emulator: TEST INFRASTRUCTURE, compiled on the fly by tests/test_emul_lin_bwd_front_cpu.py with the host clang of the ROCm
// toolchain.  `n` is the size of the grid the device launch would have (B*NH*nk for the recompute, B*NH*steps of the range for the
// front, B*NH otherwise).
#include "wave_emul.h"

#include "ttt_lin16_body.h"

using namespace ttt;

template <class F>
static int run_grid(int cs, int n, F body) {
    if (cs != 16) return -1;                     // (the entries take the arguments of tests/emul/lin_bwd_parts_emul.cpp; one wave has no LDS race to report)
    for (int u = 0; u < n; ++u) emul::run_wave([&](emul::EmulWave& w) { body(w, u); });
    return 0;
}

extern "C" {

int emul_lin_forward(int cs, const wv::Lin16Params* p, int n, char*, int) {
    return run_grid(cs, n, [&](emul::EmulWave& w, int u) { lin16::forward(w, *p, u); });
}
int emul_lin_backward(int cs, const wv::Lin16Params* p, int n, char*, int) {
    return run_grid(cs, n, [&](emul::EmulWave& w, int u) { lin16::backward(w, *p, u); });
}
int emul_lin_recompute_groups(int cs, const wv::Lin16BwdPartParams* q, int n, char*, int) {
    return run_grid(cs, n, [&](emul::EmulWave& w, int u) { lin16::recompute_groups(w, *q, u); });
}
int emul_lin_sweep_groups(int cs, const wv::Lin16BwdPartParams* q, int n, char*, int) {
    return run_grid(cs, n, [&](emul::EmulWave& w, int u) { lin16::sweep_groups(w, *q, u); });
}
int emul_lin_front_groups(int cs, const wv::Lin16BwdFrontParams* f, int n, char*, int) {
    return run_grid(cs, n, [&](emul::EmulWave& w, int u) { lin16::front_groups(w, *f, u); });
}
int emul_lin_chain_groups(int cs, const wv::Lin16BwdFrontParams* f, int n, char*, int) {
    return run_grid(cs, n, [&](emul::EmulWave& w, int u) { lin16::chain_groups(w, *f, u); });
}

int emul_lin_params_size() { return (int)sizeof(wv::Lin16Params); }
int emul_lin_bwd_part_params_size() { return (int)sizeof(wv::Lin16BwdPartParams); }
int emul_lin_bwd_front_params_size() { return (int)sizeof(wv::Lin16BwdFrontParams); }
int emul_lin_part_slot_bytes() { return (int)wv::LIN_PART_SLOT_BYTES; }
int emul_lin_part_carry_floats(int) { return wv::LIN_PART_CARRY_FLOATS * 64; }
int emul_lin_front_record_bytes() { return (int)wv::LIN_FRONT_RECORD_BYTES; }
int emul_lin_chain_lds_bytes() { return lin16::WAVE_LDS_CHAIN; }
}
