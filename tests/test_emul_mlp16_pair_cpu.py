"""The TTT-MLP forward scan at mini-batches of 16 as a PAIR of workgroups per (b, h) (csrc/ttt_mlp16_pair_body.h) on the multi-wave
emulator of tests/emul: role A (the state chain) and role B (the output path) of every (b, h) run as two emulated 8-wave workgroups in
two host threads at the same time, handing records over through a ring of the real depth in host memory with std::atomic flag words.
Outputs, checkpoints and the final state must be the bits of the one-workgroup body (``mlp16::forward_part``)."""
import ctypes
import os
import subprocess

import pytest
import torch

from helpers import rel_l2, tile_states
from oracle import ttt_oracle as O
from test_mlp16_chunk_emul_cpu import CLANG, HERE, ROOT, ChunkParams, _case

NAN = float("nan")


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    build = os.path.join(HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libmlp16_pair_emul.so")
    srcs = [os.path.join(HERE, "emul", f) for f in ("mlp16_pair_emul.cpp", "wave_emul.h")] + \
           [os.path.join(ROOT, "ttt-video-dit_amd", "csrc", f)
            for f in ("ttt_lin16_body.h", "ttt_mlp16_body.h", "ttt_mlp16_pair_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", os.path.join(ROOT, "ttt-video-dit_amd", "csrc"), "-I", os.path.join(HERE, "emul"),
                               srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.emul_mlp16_chunk_params_size() == ctypes.sizeof(ChunkParams)
    lib.emul_mlp16_pair_workspace_bytes.restype = ctypes.c_long
    lib.emul_mlp16_forward_part_pair.restype = ctypes.c_uint
    return lib


def _run(lib, t, B, NH, NC, G, cuts, paired):
    """the scan as consecutive parts of the given lengths, the state carried IN PLACE; ring (one workspace for all the parts),
    checkpoints, ``out`` and the state that a part leaves are NaN before anything writes them -> out, checkpoints, final state"""
    K = -(-NC // G)
    nan = lambda *s: torch.full(s, NAN)
    cks = (nan(B, NH, K, 64, 256), nan(B, NH, K, 1, 256), nan(B, NH, K, 256, 64), nan(B, NH, K, 1, 64))
    out = torch.full((B, NH, NC, 16, 64), NAN, dtype=torch.bfloat16)
    state = [t[k].clone() for k in ("W1", "b1", "W2", "b2")]
    ws = torch.full((lib.emul_mlp16_pair_workspace_bytes(B * NH) // 4,), NAN)           # (the flag block is zeroed per launch)
    msg = ctypes.create_string_buffer(256)
    s0 = 0
    for ns in cuts:
        c = ChunkParams()
        for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=state[0], b1=state[1],
                         W2=state[2], b2=state[3], W1c=cks[0], b1c=cks[1], W2c=cks[2], b2c=cks[3], out=out).items():
            setattr(c.p, n, v.data_ptr())
        c.p.NH, c.p.NC, c.p.G, c.p.K, c.p.eps = NH, ns, G, K, 1e-8
        c.step0, c.NCs = s0, NC
        c.W1f, c.b1f, c.W2f, c.b2f = (s.data_ptr() for s in state)
        if paired:
            races = (ctypes.c_int * 2)()
            err = lib.emul_mlp16_forward_part_pair(ctypes.byref(c), B * NH, ctypes.c_void_p(ws.data_ptr()), races, msg, 256)
            assert err == 0, f"a hand-over gave up: (b, h) {err - 1}"
            assert races[0] == 0, f"LDS race in role A, part [{s0}, {s0 + ns}): {msg.value.decode()}"
            assert races[1] == 0, f"LDS race in role B, part [{s0}, {s0 + ns}): {msg.value.decode()}"
        else:
            assert lib.emul_mlp16_forward_part(ctypes.byref(c), B * NH, msg, 256) == 0, msg.value.decode()
        s0 += ns
    assert s0 == NC
    return out, cks, state


def _same(a, b, what):
    out, cks, st = a
    out0, cks0, st0 = b
    assert not torch.isnan(out.float()).any() and not any(torch.isnan(x).any() for x in (*cks, *st)), what
    assert torch.equal(out, out0), what
    for name, c, c0 in zip(("W1c", "b1c", "W2c", "b2c"), cks, cks0):
        assert torch.equal(c, c0), (what, name)
    for name, s, s0 in zip(("W1", "b1", "W2", "b2"), st, st0):
        assert torch.equal(s, s0), (what, name)


def test_record_layout_constants(emul):
    """the header's ring depth is what the emulator (and the kernel) is built with; records of 64 KiB + 1 KiB + 256 B; the flag words of
    a (b, h) are two 128-byte lines, in a block of their own in front of the rings"""
    import re
    ring = int(re.search(r"#define TTT_HIP_PAIR16_RING (\d+)", open(os.path.join(ROOT, "include", "ttt_hip_pair16.h")).read()).group(1))
    assert emul.emul_mlp16_pair_ring() == ring
    assert emul.emul_mlp16_pair_rec_bytes() == 64 * 1024 + 1024 + 256 and emul.emul_mlp16_pair_flag_words() == 64
    assert emul.emul_mlp16_pair_workspace_bytes(3) == 3 * 256 + 3 * ring * (64 * 1024 + 1024 + 256)


def test_lds_maps_fit(emul):
    """role A allocates neither Q nor redB; role B holds the partials twice; the kernel's allocation is the larger map, <= 160 KiB"""
    a, b, k = (emul.emul_mlp16_pair_lds_bytes(r) for r in (0, 1, 2))
    assert 0 < a <= k <= 160 * 1024 and 0 < b <= k and k == max(a, b)
    assert a < emul.emul_mlp16_one_workgroup_lds_bytes() - 8 * 16 * 68 * 4


# (1, 2, 11, 4): more than two wraps of the ring, a ragged last group ; (1, 1, 1, 1) ; (1, 1, 3, 16): NC < RING and NC < G
@pytest.mark.parametrize("B,NH,NC,G", [(1, 2, 11, 4), (1, 1, 1, 1), (1, 1, 3, 16)])
def test_emulated_pair_is_the_one_workgroup_scan(emul, B, NH, NC, G):
    d, t = _case(B, NH, NC, seed=31 + NC)
    one = _run(emul, t, B, NH, NC, G, (NC,), paired=False)
    two = _run(emul, t, B, NH, NC, G, (NC,), paired=True)
    _same(two, one, (B, NH, NC, G))
    if NC == 11:
        # as parts, the state carried in place and one workspace reused: the uncut run
        _same(_run(emul, t, B, NH, NC, G, (5, 1, 5), paired=True), two, "parts (5, 1, 5)")
        # and the uncut run holds the suite's 1e-2 against the fp64 oracle
        d64 = {k: v.double() for k, v in d.items()}
        s64 = tile_states(d64, B)
        ro, rc, rf = O.mlp_forward(d64["XQ"], d64["XK"], d64["XV"], d64["eta"][:, :, :, -1, :, None], d64["ln_w"], d64["ln_b"],
                                   s64["W1"], s64["b1"], s64["W2"], s64["b2"], G)
        assert rel_l2(two[0], ro) < 1e-2
        for c, r in zip(two[1], rc):
            assert rel_l2(c, r) < 1e-2
