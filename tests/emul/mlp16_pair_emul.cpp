// Host build of the TTT-MLP (mini-batch 16) forward scan in PAIR form (mlp16::pair::state_role / output_role of
// csrc/ttt_mlp16_pair_body.h) on the wave emulator: TEST INFRASTRUCTURE, compiled on the fly by tests/test_emul_mlp16_pair_cpu.py
// with the host clang of the ROCm toolchain.  Per (b, h) one emulated 8-wave workgroup per role, in two host threads, CONCURRENTLY;
// the hand-over policy is host memory plus std::atomic, the ring has the real RING depth.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <thread>

#include "wave_emul.h"

#include "ttt_lin16_body.h"
#include "ttt_mlp16_body.h"
#include "ttt_mlp16_pair_body.h"

using namespace ttt;
namespace pr = ttt::mlp16::pair;

namespace {
// the hand-over policy of the host: the ring is plain memory (the flag's release / acquire orders it), the flag words are atomics
struct HostHandover {
    char* ring;                                    // this (b, h)'s RING records
    std::atomic<unsigned>* fl;                     // this (b, h)'s FLAG_WORDS
    std::atomic<unsigned>* err;
    void store16(int voff, int soff, wv::u32x4 v) const { memcpy(ring + soff + voff, &v, 16); }
    void store4(int voff, int soff, unsigned v) const { memcpy(ring + soff + voff, &v, 4); }
    wv::u32x4 load16(int voff, int soff) const {
        wv::u32x4 v;
        memcpy(&v, ring + soff + voff, 16);
        return v;
    }
    void drain() const {}
    void post(int word, unsigned v) const { fl[word].store(v, std::memory_order_release); }
    unsigned peek(int word) const { return fl[word].load(std::memory_order_acquire); }
    bool wait_ge(int word, unsigned need) const {  // bounded like the device's (a generous bound: 1 024 host threads share the CPUs)
        const auto t0 = std::chrono::steady_clock::now();
        while (peek(word) < need) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) return false;
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
        return true;
    }
    void fail(int bh) const { err->store(1u + (unsigned)bh); }
};
}  // namespace

extern "C" {

int emul_mlp16_pair_ring() { return pr::RING; }
int emul_mlp16_pair_rec_bytes() { return pr::REC_BYTES; }
int emul_mlp16_pair_flag_words() { return pr::FLAG_WORDS; }
long emul_mlp16_pair_workspace_bytes(int n_bh) { return (long)pr::workspace_bytes(n_bh); }
int emul_mlp16_pair_lds_bytes(int role) { return role == 0 ? pr::STATE_LDS : role == 1 ? pr::OUTPUT_LDS : pr::PAIR_LDS; }
int emul_mlp16_one_workgroup_lds_bytes() { return mlp16::GROUP_LDS; }

// The part `c` as pairs.  `ws`: workspace_bytes(n_bh) bytes in the device layout (flag words first, then the rings) - the caller
// prefills the rings; the flag words are zeroed here, as the launch function does in front of every launch.  races[0] / races[1]:
// LDS races of role A / role B; returns the error word (0, or 1 + bh of a hand-over that gave up); the first race goes to `msg`.
unsigned emul_mlp16_forward_part_pair(const wv::Mlp16ChunkParams* c, int n_bh, char* ws, int* races, char* msg, int msg_len) {
    std::atomic<unsigned> err{0u};
    std::atomic<unsigned>* flags = reinterpret_cast<std::atomic<unsigned>*>(ws);
    for (int k = 0; k < n_bh * pr::FLAG_WORDS; ++k) flags[k].store(0u);
    char* rings = ws + pr::flags_bytes(n_bh);
    races[0] = races[1] = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const HostHandover ho0{rings + (size_t)bh * pr::RING * pr::REC_BYTES, flags + (size_t)bh * pr::FLAG_WORDS, &err};
        emul::RaceReport ra, rb;
        std::thread ta([&] { ra = emul::run_group(8, [&](emul::EmulWave& w) { HostHandover ho = ho0; pr::state_role(w, ho, *c, bh); }); });
        std::thread tb([&] { rb = emul::run_group(8, [&](emul::EmulWave& w) { HostHandover ho = ho0; pr::output_role(w, ho, *c, bh); }); });
        ta.join();
        tb.join();
        if ((ra.races || rb.races) && !(races[0] + races[1]) && msg)
            snprintf(msg, msg_len, "role %s: %s", ra.races ? "A" : "B", (ra.races ? ra.first : rb.first).c_str());
        races[0] += ra.races;
        races[1] += rb.races;
    }
    return err.load();
}

// the one-workgroup body, for the comparison
int emul_mlp16_forward_part(const wv::Mlp16ChunkParams* c, int n_bh, char* msg, int msg_len) {
    int races = 0;
    for (int bh = 0; bh < n_bh; ++bh) {
        const emul::RaceReport r = emul::run_group(8, [&](emul::EmulWave& w) { mlp16::forward_part(w, *c, bh); });
        if (r.races && !races && msg) snprintf(msg, msg_len, "%s", r.first.c_str());
        races += r.races;
    }
    return races;
}

int emul_mlp16_chunk_params_size() { return (int)sizeof(wv::Mlp16ChunkParams); }
}
