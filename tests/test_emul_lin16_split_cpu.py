"""The two-wave TTT-Linear forward scan at mini-batches of 16 (csrc/ttt_lin16_split_body.h: the chain role on wave 0, the output role
on wave 1, the packed state handed over through two LDS slots with one workgroup barrier per step) on the multi-wave emulator of
tests/emul.  Outputs, checkpoints and the final state of every cutting must be the BITS of the one-wave body (``lin16::forward_part``)
run the same way, with no LDS race between the two waves.  The emulator library is built and exercised in a child process with a time
limit first: a barrier-count mismatch between the roles would otherwise block the host threads of the test process for good."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from helpers import rel_l2, tile_states
from oracle import ttt_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ttt-video-dit_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/amdclang++"
NAN = float("nan")


class LinParams(ctypes.Structure):            # wv::Lin16Params (csrc/ttt_wave_types.h)
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("XQ", "XK", "XV", "eta", "ln_w", "ln_b", "W1", "b1", "W1c", "b1c", "out", "dOut", "dW1_last", "db1_last",
                 "scratch_w", "scratch_b", "dln_w", "dln_b", "dW1", "db1", "deta", "dXQ", "dXK", "dXV")] + \
               [(n, ctypes.c_int) for n in ("NH", "NC", "G", "K")] + [("eps", ctypes.c_float)]


class ChunkParams(ctypes.Structure):          # wv::Lin16ChunkParams
    _fields_ = [("p", LinParams), ("step0", ctypes.c_int), ("NCs", ctypes.c_int), ("W1f", ctypes.c_void_p), ("b1f", ctypes.c_void_p)]


# run in a child first: one step and three steps of one (b, h) on zero inputs - enough for a barrier-count mismatch to hang
_PROBE = r"""
import ctypes, sys
lib = ctypes.CDLL(sys.argv[1])
nbytes = lib.emul_lin_chunk_params_size()
for steps in (1, 3):
    bufs = [ctypes.create_string_buffer(64 * 64 * 4 * 4) for _ in range(11)]
    raw = (ctypes.c_char * nbytes)()
    ptrs = ctypes.cast(raw, ctypes.POINTER(ctypes.c_void_p))
    for k in range(11):
        ptrs[k] = ctypes.addressof(bufs[k])
    ints = ctypes.cast(ctypes.byref(raw, 24 * 8), ctypes.POINTER(ctypes.c_int))
    ints[0], ints[1], ints[2], ints[3] = 1, steps, 2, 2            # NH, NC, G, K
    ctypes.cast(ctypes.byref(raw, 24 * 8 + 16), ctypes.POINTER(ctypes.c_float))[0] = 1e-8
    tail = ctypes.cast(ctypes.byref(raw, 24 * 8 + 24), ctypes.POINTER(ctypes.c_int))
    tail[0], tail[1] = 0, steps                                     # step0, NCs ; no final-state buffers
    assert lib.emul_lin16_split_forward_part(raw, 1, None, 0) == 0
    assert lib.emul_lin16_split_chain_alone_part(raw, 1, None, 0) == 0
print("ok")
"""


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    build = os.path.join(HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "liblin16_split_emul.so")
    srcs = [os.path.join(HERE, "emul", f) for f in ("lin16_split_emul.cpp", "wave_emul.h")] + \
           [os.path.join(CSRC, f) for f in ("ttt_lin16_split_body.h", "ttt_lin16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run([CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                        "-I", CSRC, "-I", os.path.join(HERE, "emul"), srcs[0], "-o", so], check=True, timeout=300)
    # layout of the raw parameter block the probe fills by offset
    assert ctypes.sizeof(LinParams) == 24 * 8 + 24 and ChunkParams.step0.offset == 24 * 8 + 24
    probe = subprocess.run([sys.executable, "-c", _PROBE, so], capture_output=True, text=True, timeout=120)
    assert probe.returncode == 0 and probe.stdout.strip() == "ok", probe.stderr[-2000:]
    lib = ctypes.CDLL(so)
    assert lib.emul_lin_chunk_params_size() == ctypes.sizeof(ChunkParams)
    return lib


B, NH, NC, CS = 1, 2, 7, 16
_CASE = []


def _case():
    """bf16-valued inputs of the 7-step scan, as the tensors the body reads (as tests/test_emul_lin_parts_cpu.py makes them); made once"""
    if not _CASE:
        d = O.make_inputs("linear", B, NH, NC, CS, 64, seed=41 + CS)
        for k in ("XQ", "XK", "XV", "eta"):
            d[k] = d[k].to(torch.bfloat16).to(torch.float32)
        bf = lambda x: x.to(torch.bfloat16).contiguous()
        st = tile_states(d, B)
        t = dict(XQ=bf(d["XQ"]), XK=bf(d["XK"]), XV=bf(d["XV"]), eta=bf(d["eta"][:, :, :, -1, :, None]),
                 ln_w=d["ln_w"].float().contiguous(), ln_b=d["ln_b"].float().contiguous(),
                 W1=st["W1"].float().contiguous(), b1=st["b1"].float().contiguous())
        _CASE.append((d, t))
    return _CASE[0]


def _run(lib, G, cuts, split, final=True, chain_alone=False):
    """the scan as consecutive parts of the given lengths, the state carried IN PLACE -> out, checkpoints, final state.  Every buffer
    starts as NaN."""
    _, t = _case()
    K = -(-NC // G)
    cks = (torch.full((B, NH, K, 64, 64), NAN), torch.full((B, NH, K, 1, 64), NAN))
    out = torch.full((B, NH, NC, CS, 64), NAN, dtype=torch.bfloat16)
    state = [t["W1"].clone(), t["b1"].clone()]
    msg = ctypes.create_string_buffer(256)
    s0 = 0
    for ns in cuts:
        c = ChunkParams()
        for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=state[0], b1=state[1],
                         W1c=cks[0], b1c=cks[1], out=out).items():
            setattr(c.p, n, v.data_ptr())
        c.p.NH, c.p.NC, c.p.G, c.p.K, c.p.eps = NH, ns, G, K, 1e-8
        c.step0, c.NCs = s0, NC
        c.W1f, c.b1f = (state[0].data_ptr(), state[1].data_ptr()) if final else (None, None)
        if chain_alone:
            races = lib.emul_lin16_split_chain_alone_part(ctypes.byref(c), B * NH, msg, 256)
        elif split:
            races = lib.emul_lin16_split_forward_part(ctypes.byref(c), B * NH, msg, 256)
        else:
            races = lib.emul_lin16_forward_part(ctypes.byref(c), B * NH)
        assert races == 0, f"LDS race between the roles in the part [{s0}, {s0 + ns}): {msg.value.decode()}"
        s0 += ns
    return out, cks, state


def test_lds_map(emul):
    """two private regions of the one-wave scan's size and two slots of 8 448 bytes (8 KiB of operand fragments + the bias row): two
    workgroups fit the 160 KiB of a compute unit"""
    assert emul.emul_lin16_split_slot_bytes() == 8448
    assert emul.emul_lin16_split_lds_bytes() == 2 * emul.emul_lin16_wave_lds_bytes() + 2 * 8448
    assert 2 * emul.emul_lin16_split_lds_bytes() <= 160 * 1024


@pytest.mark.parametrize("G", [7, 2, 3])
def test_emulated_split_scan_is_the_one_wave_scan(emul, G):
    """A scan of 7 steps cut as (7), (3, 4), (1, 1, 5), (6, 1), the state carried in place: out, both checkpoints and the final state
    of every cutting are the bits of the emulated one-wave ``lin16::forward_part`` of the same cutting, with 0 LDS races (asserted per
    part in ``_run``), every NaN-pre-filled buffer fully written, and the uncut run within the suite's 1e-2 of the fp64 oracle."""
    d, t = _case()
    for cuts in ((7,), (3, 4), (1, 1, 5), (6, 1)):
        out0, cks0, st0 = _run(emul, G, cuts, split=False)
        out, cks, st = _run(emul, G, cuts, split=True)
        assert not torch.isnan(out.float()).any() and not any(torch.isnan(x).any() for x in (*cks, *st)), cuts
        assert torch.equal(out, out0), cuts
        for name, c, c0 in zip(("W1c", "b1c"), cks, cks0):
            assert torch.equal(c, c0), (cuts, name)
        for name, s, s0 in zip(("W1", "b1"), st, st0):
            assert torch.equal(s, s0), (cuts, name)
        assert not torch.equal(st[0], t["W1"]) and not torch.equal(st[1], t["b1"]), "the state did not move"
        if cuts == (7,):
            d64 = {k: v.double() for k, v in d.items()}
            s64 = tile_states(d64, B)
            ro, rc, _ = O.linear_forward(d64["XQ"], d64["XK"], d64["XV"], d64["eta"][:, :, :, -1, :, None], d64["ln_w"], d64["ln_b"],
                                         s64["W1"], s64["b1"], G)
            assert rel_l2(out, ro) < 1e-2
            for c, r in zip(cks, rc):
                assert rel_l2(c, r) < 1e-2


def test_final_state_of_a_part_is_the_next_checkpoint(emul):
    """The state that leaves the part [0, 6) at G = 3 is checkpoint 2 of the uncut run (the state entering step 6), bit for bit; with no
    final-state buffers the state arrays keep the initial state."""
    _, t = _case()
    _, cks0, _ = _run(emul, 3, (7,), split=True)
    _, _, st = _run(emul, 3, (6,), split=True)
    assert torch.equal(st[0], cks0[0][:, :, 2]) and torch.equal(st[1], cks0[1][:, :, 2])
    _, _, kept = _run(emul, 3, (6,), split=True, final=False)
    assert torch.equal(kept[0], t["W1"]) and torch.equal(kept[1], t["b1"])


def test_chain_alone_keeps_the_chain_and_writes_no_output(emul):
    """the bench tool's chain-alone arm: checkpoints and the final state are the split scan's, ``out`` is never written"""
    out, cks, st = _run(emul, 3, (7,), split=True, chain_alone=True)
    _, cks0, st0 = _run(emul, 3, (7,), split=True)
    assert torch.isnan(out.float()).all()
    assert all(torch.equal(a, b) for a, b in zip((*cks, *st), (*cks0, *st0)))
