"""The TTT-Linear forward scan over PARTS of the sequence at both MFMA geometries (mini-batches of 16: csrc/ttt_lin16_body.h, one wave
per scan; of 64: csrc/ttt_lin64_body.h, four waves per scan) on the wave emulator of tests/emul: ``forward_part`` walks
[step0, step0 + nsteps) of the whole sequence's tensors from the fp32 state it is given and hands the state on.  Cut anywhere, the
parts reproduce the bits of the uncut scan - outputs, checkpoints, final state - because the kernels hold the whole state in fp32 and
rebuild everything else a step takes from its predecessor from it.  The same bodies are instantiated with the device backend in
csrc/ttt_mfma16.hip (linear_scan16_kernel / linear_fwd_cs64_kernel)."""
import ctypes
import os
import subprocess

import pytest
import torch

from helpers import rel_l2, tile_states
from oracle import ttt_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ttt-video-dit_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/amdclang++"


class LinParams(ctypes.Structure):            # wv::Lin16Params (csrc/ttt_wave_types.h)
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("XQ", "XK", "XV", "eta", "ln_w", "ln_b", "W1", "b1", "W1c", "b1c", "out", "dOut", "dW1_last", "db1_last",
                 "scratch_w", "scratch_b", "dln_w", "dln_b", "dW1", "db1", "deta", "dXQ", "dXK", "dXV")] + \
               [(n, ctypes.c_int) for n in ("NH", "NC", "G", "K")] + [("eps", ctypes.c_float)]


class ChunkParams(ctypes.Structure):          # wv::Lin16ChunkParams
    _fields_ = [("p", LinParams), ("step0", ctypes.c_int), ("NCs", ctypes.c_int), ("W1f", ctypes.c_void_p), ("b1f", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    build = os.path.join(HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "liblin_parts_emul.so")
    srcs = [os.path.join(HERE, "emul", f) for f in ("lin_parts_emul.cpp", "wave_emul.h")] + \
           [os.path.join(CSRC, f) for f in ("ttt_lin64_body.h", "ttt_lin16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", CSRC, "-I", os.path.join(HERE, "emul"), srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.emul_lin_params_size() == ctypes.sizeof(LinParams)
    assert lib.emul_lin_chunk_params_size() == ctypes.sizeof(ChunkParams)
    return lib


B, NH, NC = 1, 2, 7
_CASE = {}


def _case(CS):
    """bf16-valued inputs of the 7-step scan at this mini-batch size, as the tensors the body reads; made once"""
    if CS not in _CASE:
        d = O.make_inputs("linear", B, NH, NC, CS, 64, seed=41 + CS)
        for k in ("XQ", "XK", "XV", "eta"):
            d[k] = d[k].to(torch.bfloat16).to(torch.float32)
        bf = lambda x: x.to(torch.bfloat16).contiguous()
        st = tile_states(d, B)
        t = dict(XQ=bf(d["XQ"]), XK=bf(d["XK"]), XV=bf(d["XV"]), eta=bf(d["eta"][:, :, :, -1, :, None]),
                 ln_w=d["ln_w"].float().contiguous(), ln_b=d["ln_b"].float().contiguous(),
                 W1=st["W1"].float().contiguous(), b1=st["b1"].float().contiguous())
        _CASE[CS] = (d, t)
    return _CASE[CS]


def _buffers(CS, G):
    K = -(-NC // G)
    nan = lambda *s: torch.full(s, float("nan"))
    return (nan(B, NH, K, 64, 64), nan(B, NH, K, 1, 64)), torch.full((B, NH, NC, CS, 64), float("nan"), dtype=torch.bfloat16), K


def _fill(p, t, state, cks, out, n_steps, G, K):
    for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=state[0], b1=state[1],
                     W1c=cks[0], b1c=cks[1], out=out).items():
        setattr(p, n, v.data_ptr())
    p.NH, p.NC, p.G, p.K, p.eps = NH, n_steps, G, K, 1e-8


def _run(lib, CS, G, cuts, final=True):
    """the scan as consecutive parts of the given lengths, the state carried IN PLACE (the final state aliases the initial state, as
    pipeline.prepass carries it) -> out, checkpoints, final state.  Every buffer starts as NaN."""
    _, t = _case(CS)
    cks, out, K = _buffers(CS, G)
    state = [t["W1"].clone(), t["b1"].clone()]
    msg = ctypes.create_string_buffer(256)
    s0 = 0
    for ns in cuts:
        c = ChunkParams()
        _fill(c.p, t, state, cks, out, ns, G, K)
        c.step0, c.NCs = s0, NC
        c.W1f, c.b1f = (state[0].data_ptr(), state[1].data_ptr()) if final else (None, None)
        races = lib.emul_lin_forward_part(CS, ctypes.byref(c), B * NH, msg, 256)
        assert races == 0, f"LDS race between waves in the part [{s0}, {s0 + ns}): {msg.value.decode()}"
        s0 += ns
    return out, cks, state


_UNCUT = {}


def _uncut(lib, CS, G):
    if (CS, G) not in _UNCUT:
        _UNCUT[CS, G] = _run(lib, CS, G, (NC,))
    return _UNCUT[CS, G]


@pytest.mark.parametrize("G", [7, 2, 3])
@pytest.mark.parametrize("CS", [16, 64])
def test_emulated_linear_scan_in_parts_is_the_uncut_scan(emul, CS, G):
    """A scan of 7 steps cut as (7), (3, 4), (1, 1, 5), (6, 1) - cuts on and off the checkpoint-group boundaries, parts of one step, a
    part behind the last checkpoint -, the state carried in place: outputs, checkpoints and the final state of every cutting are the
    BITS of the uncut run, every buffer (pre-filled with NaN) is fully written, no LDS race in any part at CS = 64, and the uncut run
    holds the 1e-2 of the one-call emulator tests against the fp64 oracle."""
    d, t = _case(CS)
    out0, cks0, st0 = _uncut(emul, CS, G)
    assert not any(torch.isnan(c).any() for c in cks0) and not torch.isnan(out0.float()).any()
    assert not torch.equal(st0[0], t["W1"]) and not torch.equal(st0[1], t["b1"]), "the state did not move"
    for cuts in ((3, 4), (1, 1, 5), (6, 1)):
        out, cks, st = _run(emul, CS, G, cuts)
        assert torch.equal(out, out0), cuts
        for name, c, c0 in zip(("W1c", "b1c"), cks, cks0):
            assert torch.equal(c, c0), (cuts, name)
        for name, s, s0 in zip(("W1", "b1"), st, st0):
            assert torch.equal(s, s0), (cuts, name)
    d64 = {k: v.double() for k, v in d.items()}
    s64 = tile_states(d64, B)
    ro, rc, _ = O.linear_forward(d64["XQ"], d64["XK"], d64["XV"], d64["eta"][:, :, :, -1, :, None], d64["ln_w"], d64["ln_b"],
                                 s64["W1"], s64["b1"], G)
    assert rel_l2(out0, ro) < 1e-2
    for c, r in zip(cks0, rc):
        assert rel_l2(c, r) < 1e-2


@pytest.mark.parametrize("CS", [16, 64])
def test_final_state_of_a_part_is_the_next_checkpoint(emul, CS):
    """An exact check of the final-state store: the state that leaves the part [0, 6) at G = 3 is checkpoint 2 of the uncut run (the state
    entering step 6), bit for bit; without final-state buffers the part stores none (the state arrays keep the initial state)."""
    _, t = _case(CS)
    _, cks0, _ = _uncut(emul, CS, 3)
    _, _, st = _run(emul, CS, 3, (6,))
    assert torch.equal(st[0], cks0[0][:, :, 2]) and torch.equal(st[1], cks0[1][:, :, 2])
    _, _, kept = _run(emul, CS, 3, (6,), final=False)
    assert torch.equal(kept[0], t["W1"]) and torch.equal(kept[1], t["b1"])


@pytest.mark.parametrize("CS", [16, 64])
def test_whole_sequence_entry_is_the_part_from_step_zero(emul, CS):
    """``lin16::forward`` / ``lin64::forward`` (the entries the one-call emulator tests use) are the part [0, NC) of the same bodies."""
    G = 3
    _, t = _case(CS)
    out0, cks0, _ = _uncut(emul, CS, G)
    cks, out, K = _buffers(CS, G)
    p = LinParams()
    _fill(p, t, (t["W1"], t["b1"]), cks, out, NC, G, K)
    assert emul.emul_lin_forward_whole(CS, ctypes.byref(p), B * NH, None, 0) == 0
    assert torch.equal(out, out0) and all(torch.equal(a, b) for a, b in zip(cks, cks0))
