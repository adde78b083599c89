"""The third stage of the TTT-Linear backward over ranges of checkpoint groups at mini-batches of 64 (csrc/ttt_lin64_body.h) on the wave
emulator of tests/emul: ``front_groups`` runs the half of every reverse step that stands in front of barrier A - one SINGLE wave per
(b, h, step, 16-row token block) - and leaves a record per step; ``chain_groups`` is the walk that remains, a workgroup of four waves
under the emulator's LDS race detector, and reads the records.  However the K groups are cut into ranges, recompute -> front -> chain
gives the BITS of the one-call ``lin64::backward()`` in all eight gradients, and a range done by ``sweep_groups`` hands over to a range
done by front + chain and back.  The same bodies are instantiated with the device backend in csrc/ttt_mfma16.hip
(linear_front_cs64_groups_kernel, linear_chain_cs64_groups_kernel).  Inputs, checkpoints and the one-call reference are those of
tests/test_emul_lin_bwd_parts_cpu.py at CS = 64, made once."""
import ctypes
import os
import subprocess

import pytest
import torch

import test_emul_lin_bwd_parts_cpu as P
from test_emul_cpu import Params
from test_emul_lin_bwd_parts_cpu import B, GRADS, GUARD, NC, NH, PartParams, _call, _common, _cuttings, _grads, _guarded, _set

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ttt-video-dit_amd", "csrc")
CS = 64
REC = 77824
GS = sorted({G for cs, G in P.CASES if cs == CS}, reverse=True)          # every G the parts tests use at CS = 64


class FrontParams(ctypes.Structure):           # wv::Lin16BwdFrontParams (csrc/ttt_wave_types.h)
    _fields_ = [("q", PartParams), ("records", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(P.CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    build = os.path.join(HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "liblin64_bwd_front_emul.so")
    srcs = [os.path.join(HERE, "emul", f) for f in ("lin64_bwd_front_emul.cpp", "wave_emul.h")] + \
           [os.path.join(CSRC, f) for f in ("ttt_lin64_body.h", "ttt_lin16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([P.CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", CSRC, "-I", os.path.join(HERE, "emul"), srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.emul_lin_params_size() == ctypes.sizeof(Params)
    assert lib.emul_lin_bwd_part_params_size() == ctypes.sizeof(PartParams)          # the existing structs keep their layout
    assert lib.emul_lin_bwd_front_params_size() == ctypes.sizeof(FrontParams)
    assert lib.emul_lin_part_slot_bytes() == 16 * 1024 + 256
    assert lib.emul_lin_front_block_record_bytes() == 19456 == 64 * (32 + 16 + 32 + 192 + 32)
    assert lib.emul_lin_front_record_bytes() == REC == 4 * 19456
    assert lib.emul_lin_chain_lds_bytes() <= 160 * 1024
    return lib


def test_the_cases_are_those_of_the_parts_tests():
    assert GS == [3, 2] and NC == 7


def _front_parts(lib, G, cuts, upfront=False, stop_after=None, skip_front=False, sweep=()):
    """the backward as ranges of `cuts` groups each, walked from the LAST range to the first: recompute -> front -> chain per range,
    dW1 / db1 carried IN PLACE in the output buffers (which start as the upstream gradients; everything else starts as NaN), one
    ln_carry.  upfront: every range is recomputed and fronted into its own region of one large slot / record workspace before the
    first chain; otherwise each range has workspaces of its own size.  stop_after: chain only that many ranges (without `upfront`, the
    front of the others does not run either).  skip_front: the records stay NaN.  sweep: the ranges (counted in walking order) that
    sweep_groups does in place of front + chain.  The front is called without dW1_last, db1_last and ln_carry, the chain without XV,
    dOut and dXQ.  -> gradients, [dW1 after each range]"""
    _, t, cks = P._case(lib, CS, G)
    K = -(-NC // G)
    assert sum(cuts) == K
    keep = {k: v.clone() for k, v in t.items()}
    keep_ck = [c.clone() for c in cks]
    g = _grads(CS)
    g["dW1"].copy_(t["dW1_last"]); g["db1"].copy_(t["db1_last"])
    slot_floats = lambda nk: B * NH * nk * (G + 1) * lib.emul_lin_part_slot_bytes() // 4
    rec_floats = lambda nk: B * NH * nk * G * REC // 4
    carry_all, carry = _guarded(B * NH * lib.emul_lin_part_carry_floats(CS))
    ranges, k_end = [], K
    for nk in reversed(cuts):
        ranges.append((k_end - nk, nk))
        k_end -= nk

    def spaces_of(floats):
        if upfront:               # one large workspace, a region per range
            whole, view = _guarded(sum(floats(nk) for _, nk in ranges))
            offs = [sum(floats(nk) for _, nk in ranges[:n]) for n in range(len(ranges))]
            return [(whole, view[o:o + floats(nk)]) for o, (_, nk) in zip(offs, ranges)]
        return [_guarded(floats(nk)) for _, nk in ranges]

    slot_spaces, rec_spaces = spaces_of(slot_floats), spaces_of(rec_floats)

    def part(k0, nk, ws):
        q = PartParams()
        _set(q.p, G, K, dW1_last=g["dW1"], db1_last=g["db1"], **_common(t, cks, g))
        q.k0, q.nk, q.slots, q.ln_carry = k0, nk, ws.data_ptr(), carry.data_ptr()
        return q

    def front_part(k0, nk, ws, rs, chain):
        f = FrontParams()
        f.q = part(k0, nk, ws)
        f.records = rs.data_ptr()
        if chain:
            f.q.p.XV = f.q.p.dOut = f.q.p.dXQ = None
        else:
            f.q.p.dW1_last = f.q.p.db1_last = f.q.ln_carry = None
        return f

    def steps(k0, nk):
        return min((k0 + nk) * G, NC) - k0 * G

    def prepare(n):
        (k0, nk), ws, rs = ranges[n], slot_spaces[n][1], rec_spaces[n][1]
        _call(lib.emul_lin_recompute_groups, CS, part(k0, nk, ws), B * NH * nk, f"the recompute of groups [{k0}, {k0 + nk})")
        if skip_front or n in sweep:
            return
        _call(lib.emul_lin_front_groups, CS, front_part(k0, nk, ws, rs, False), B * NH * steps(k0, nk) * 4, f"the front of groups [{k0}, {k0 + nk})")
        # the records in use - [B*NH][nk][steps of the group] - are fully overwritten
        r = rs.view(B * NH, nk, G, REC // 4)
        for j in range(nk):
            used = min((k0 + j + 1) * G, NC) - (k0 + j) * G
            assert not torch.isnan(r[:, j, :used]).any(), f"the front left part of a record of group {k0 + j} unwritten"
            assert torch.isnan(r[:, j, used:]).all(), "a record beyond the steps of a ragged group was written"

    if upfront:
        for n in range(len(ranges)):
            prepare(n)
    trail = []
    for n, (k0, nk) in enumerate(ranges):
        if stop_after is not None and n == stop_after:
            break
        if not upfront:
            prepare(n)
        if n in sweep:
            _call(lib.emul_lin_sweep_groups, CS, part(k0, nk, slot_spaces[n][1]), B * NH, f"the sweep of groups [{k0}, {k0 + nk})")
        else:
            _call(lib.emul_lin_chain_groups, CS, front_part(k0, nk, slot_spaces[n][1], rec_spaces[n][1], True), B * NH,
                  f"the chain of groups [{k0}, {k0 + nk})")
        trail.append(g["dW1"].clone())
    for whole, _ in slot_spaces + rec_spaces + [(carry_all, None)]:
        assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[-GUARD:]).all(), "write outside a workspace"
    for k, v in t.items():
        assert torch.equal(v, keep[k]), f"input {k} was written"
    assert all(torch.equal(a, b) for a, b in zip(cks, keep_ck)), "a checkpoint was written"
    return g, trail


@pytest.mark.parametrize("G", GS)
def test_emulated_front_and_chain_are_the_one_call_backward(emul, G):
    """7 steps at G = 3 (odd, last group of one step) and 2 (even, ragged): every cutting of the K groups - one range, one group per
    range, (K - 1, 1), (1, K - 1) -, with per-range workspaces and (one group per range) with every range recomputed and fronted up
    front into one large workspace, gives the bits of the emulated one-call lin64::backward() in all eight gradients; no LDS race in
    the chain (``_call`` asserts it); the front overwrites every record in use and nothing else; nothing lands outside the workspaces."""
    ref = P._one_call(emul, CS, G)
    K = -(-NC // G)
    for cuts in _cuttings(K):
        for upfront in ((False, True) if cuts == (1,) * K and K > 1 else (False,)):
            g, _ = _front_parts(emul, G, cuts, upfront)
            for name in GRADS:
                assert torch.equal(g[name], ref[name]), (cuts, upfront, name)


@pytest.mark.parametrize("G", GS)
def test_sweep_ranges_and_chain_ranges_hand_over_to_each_other(emul, G):
    """one group per range, every other range by sweep_groups and the rest by front + chain, starting with either: the bits of the one
    call.  The carries (dW1 / db1 in place, ln_carry) are the same whichever stage wrote them."""
    ref = P._one_call(emul, CS, G)
    K = -(-NC // G)
    for first in (0, 1):
        g, _ = _front_parts(emul, G, (1,) * K, sweep=tuple(range(first, K, 2)))
        for name in GRADS:
            assert torch.equal(g[name], ref[name]), (first, name)
    g, _ = _front_parts(emul, G, (K - 1, 1), sweep=(0,))
    for name in GRADS:
        assert torch.equal(g[name], ref[name]), ("sweep, chain", name)
    g, _ = _front_parts(emul, G, (K - 1, 1), sweep=(1,))
    for name in GRADS:
        assert torch.equal(g[name], ref[name]), ("chain, sweep", name)


def test_the_chain_reads_the_records(emul):
    """a chain over NaN-filled records (the front skipped) gives NaN gradients: it does not rebuild what the front computes"""
    G = 3
    g, _ = _front_parts(emul, G, (-(-NC // G),), skip_front=True)
    for name in ("dln_w", "dln_b", "dW1", "db1", "deta", "dXK", "dXV"):
        assert torch.isnan(g[name].float()).all(), name
    assert torch.isnan(g["dXQ"].float()).all(), "dXQ is the front's to write"


def test_a_walk_that_stops_leaves_the_rest_untouched(emul):
    """Chaining only the groups [k0, K), k0 > 0: deta / dXK / dXV of the steps in front of group k0 and dln_w / dln_b stay NaN, those of
    the walked steps are final; dXQ is final for exactly the groups whose front has run; dW1 / db1 are the carried state - the state
    a sweep of the same range hands on."""
    G = 2
    ref = P._one_call(emul, CS, G)
    K = -(-NC // G)
    k0 = 1
    s0 = k0 * G
    g, trail = _front_parts(emul, G, (k0, K - k0), stop_after=1)
    assert torch.isnan(g["dln_w"]).all() and torch.isnan(g["dln_b"]).all()
    for name in ("deta", "dXQ", "dXK", "dXV"):
        assert torch.isnan(g[name][:, :, :s0].float()).all(), name
        assert torch.equal(g[name][:, :, s0:], ref[name][:, :, s0:]), name
    up, _ = _front_parts(emul, G, (k0, K - k0), upfront=True, stop_after=1)           # every front has run, one chain
    assert torch.equal(up["dXQ"], ref["dXQ"])
    for name in ("deta", "dXK", "dXV"):
        assert torch.isnan(up[name][:, :, :s0].float()).all(), name
    assert not torch.isnan(g["dW1"]).any() and not torch.isnan(g["db1"]).any()
    assert not torch.equal(g["dW1"], ref["dW1"]), "the carried state is not yet the result"
    _, sweep_trail = P._parts(emul, CS, G, (k0, K - k0), stop_after=1)
    assert torch.equal(sweep_trail[0], trail[0])
