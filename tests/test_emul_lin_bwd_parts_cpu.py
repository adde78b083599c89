"""The TTT-Linear backward over RANGES of checkpoint groups at both MFMA geometries (mini-batches of 16: csrc/ttt_lin16_body.h, one wave
per unit of work; of 64: csrc/ttt_lin64_body.h, four waves) on the wave emulator of tests/emul: ``recompute_groups`` re-runs the groups
[k0, k0 + nk) from their checkpoints into a slot workspace, ``sweep_groups`` walks them in reverse from a carried gradient state.
However the K groups are cut into ranges, the eight gradients are the BITS of the one-call ``backward()`` of the same body: the
step functions of the parts are its steps, statement by statement, and a slot holds the operands the one call keeps in its scratch.  The same bodies are
instantiated with the device backend in csrc/ttt_mfma16.hip (linear_recompute16_groups_kernel, linear_sweep16_groups_kernel and their
_cs64_ counterparts)."""
import ctypes
import os
import subprocess

import pytest
import torch

from helpers import rel_l2, tile_states
from oracle import ttt_oracle as O
from test_emul_cpu import Params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "ttt-video-dit_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/amdclang++"
def _one_call_bound():
    """the bound of the one-call emulator tests on every gradient, read from their assertions (a literal in both, no name to import):
    test_emul_cpu.py::test_emulated_linear_backward_vs_oracle and test_emul_lin64_cpu.py::test_emulated_linear_cs64_vs_oracle"""
    import inspect
    import re
    import test_emul_cpu
    import test_emul_lin64_cpu
    found = [re.findall(r"assert all\(v < ([0-9.e-]+) for v in (?:errs|gerrs)\.values\(\)\)", inspect.getsource(f))
             for f in (test_emul_cpu.test_emulated_linear_backward_vs_oracle, test_emul_lin64_cpu.test_emulated_linear_cs64_vs_oracle)]
    bounds = {float(found[0][-1]), float(found[1][-1])}         # (the CS = 64 test: outputs first, gradients last)
    assert len(bounds) == 1, found
    return bounds.pop()


GRAD_BOUND = _one_call_bound()
GRADS = ("dln_w", "dln_b", "dW1", "db1", "deta", "dXQ", "dXK", "dXV")


class PartParams(ctypes.Structure):           # wv::Lin16BwdPartParams (csrc/ttt_wave_types.h)
    _fields_ = [("p", Params), ("k0", ctypes.c_int), ("nk", ctypes.c_int), ("slots", ctypes.c_void_p), ("ln_carry", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    build = os.path.join(HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "liblin_bwd_parts_emul.so")
    srcs = [os.path.join(HERE, "emul", f) for f in ("lin_bwd_parts_emul.cpp", "wave_emul.h")] + \
           [os.path.join(CSRC, f) for f in ("ttt_lin64_body.h", "ttt_lin16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", CSRC, "-I", os.path.join(HERE, "emul"), srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.emul_lin_params_size() == ctypes.sizeof(Params)
    assert lib.emul_lin_bwd_part_params_size() == ctypes.sizeof(PartParams)
    assert lib.emul_lin_part_slot_bytes() == 16 * 1024 + 256
    return lib


B, NH, NC = 1, 2, 7
GUARD = 64              # floats of NaN on either side of the slot workspace and of ln_carry
_CASE = {}


def _nan(*s, dt=torch.float32):
    return torch.full(s, float("nan"), dtype=dt)


def _call(fn, CS, p, n, what):
    msg = ctypes.create_string_buffer(256)
    races = fn(CS, ctypes.byref(p), n, msg, 256)
    assert races == 0, f"LDS race between the waves in {what}: {msg.value.decode()}"


def _set(p, G, K, **tensors):
    for n, v in tensors.items():
        setattr(p, n, v.data_ptr())
    p.NH, p.NC, p.G, p.K, p.eps = NH, NC, G, K, 1e-8


def _case(lib, CS, G):
    """bf16-valued inputs of the 7-step scan, non-zero upstream gradients of the final state, and the emulated forward's checkpoints
    at this group size; made once per (CS, G)"""
    if CS not in _CASE:
        d = O.make_inputs("linear", B, NH, NC, CS, 64, seed=57 + CS)
        for k in ("XQ", "XK", "XV", "eta", "dOut"):
            d[k] = d[k].to(torch.bfloat16).to(torch.float32)
        bf = lambda x: x.to(torch.bfloat16).contiguous()
        st = tile_states(d, B)
        g = torch.Generator().manual_seed(5 + CS)
        t = dict(XQ=bf(d["XQ"]), XK=bf(d["XK"]), XV=bf(d["XV"]), eta=bf(d["eta"][:, :, :, -1, :, None]), dOut=bf(d["dOut"]),
                 ln_w=d["ln_w"].float().contiguous(), ln_b=d["ln_b"].float().contiguous(),
                 W1=st["W1"].float().contiguous(), b1=st["b1"].float().contiguous(),
                 dW1_last=0.05 * torch.randn(B, NH, 64, 64, generator=g), db1_last=0.05 * torch.randn(B, NH, 1, 64, generator=g))
        _CASE[CS] = (d, t)
    d, t = _CASE[CS]
    if (CS, G) not in _CASE:
        K = -(-NC // G)
        cks = (_nan(B, NH, K, 64, 64), _nan(B, NH, K, 1, 64))
        out = _nan(B, NH, NC, CS, 64, dt=torch.bfloat16)
        p = Params()
        _set(p, G, K, XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=t["W1"], b1=t["b1"],
             W1c=cks[0], b1c=cks[1], out=out)
        _call(lib.emul_lin_forward, CS, p, B * NH, "the forward")
        assert not any(torch.isnan(c).any() for c in cks)
        _CASE[CS, G] = cks
    return d, t, _CASE[CS, G]


def _grads(CS):
    return dict(dln_w=_nan(B, NH, 1, 64), dln_b=_nan(B, NH, 1, 64), dW1=_nan(B, NH, 64, 64), db1=_nan(B, NH, 1, 64),
                deta=_nan(B, NH, NC, CS, 1, dt=torch.bfloat16), dXQ=_nan(B, NH, NC, CS, 64, dt=torch.bfloat16),
                dXK=_nan(B, NH, NC, CS, 64, dt=torch.bfloat16), dXV=_nan(B, NH, NC, CS, 64, dt=torch.bfloat16))


def _common(t, cks, g):
    return dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1c=cks[0], b1c=cks[1], dOut=t["dOut"],
                dln_w=g["dln_w"], dln_b=g["dln_b"], dW1=g["dW1"], db1=g["db1"], deta=g["deta"], dXQ=g["dXQ"], dXK=g["dXK"], dXV=g["dXV"])


_ONE_CALL = {}


def _one_call(lib, CS, G):
    """the emulated one-call backward() of the same body, made once per (CS, G)"""
    if (CS, G) not in _ONE_CALL:
        _, t, cks = _case(lib, CS, G)
        g = _grads(CS)
        scr_w, scr_b = _nan(B * NH * G * 64 * 64), _nan(B * NH * G * 64)
        p = Params()
        _set(p, G, -(-NC // G), dW1_last=t["dW1_last"], db1_last=t["db1_last"], scratch_w=scr_w, scratch_b=scr_b, **_common(t, cks, g))
        _call(lib.emul_lin_backward, CS, p, B * NH, "the one-call backward")
        assert not any(torch.isnan(v.float()).any() for v in g.values())
        _ONE_CALL[CS, G] = g
    return _ONE_CALL[CS, G]


def _guarded(n_floats):
    buf = _nan(n_floats + 2 * GUARD)
    return buf, buf[GUARD:GUARD + n_floats]


def _parts(lib, CS, G, cuts, upfront=False, stop_after=None):
    """the backward as ranges of `cuts` groups each, walked from the LAST range to the first: recompute then sweep per range, dW1 / db1
    carried IN PLACE in the output buffers (which start as the upstream gradients; everything else starts as NaN), one ln_carry.
    upfront: every range is recomputed into its own region of one large workspace before the first sweep; otherwise each range has
    a workspace of its own size.  stop_after: sweep only that many ranges.  -> gradients, [dW1 after each sweep]"""
    _, t, cks = _case(lib, CS, G)
    K = -(-NC // G)
    assert sum(cuts) == K
    keep = {k: v.clone() for k, v in t.items()}
    keep_ck = [c.clone() for c in cks]
    g = _grads(CS)
    g["dW1"].copy_(t["dW1_last"]); g["db1"].copy_(t["db1_last"])
    slot_floats = lambda nk: B * NH * nk * (G + 1) * lib.emul_lin_part_slot_bytes() // 4
    carry_all, carry = _guarded(B * NH * lib.emul_lin_part_carry_floats(CS))
    ranges, k_end = [], K
    for nk in reversed(cuts):
        ranges.append((k_end - nk, nk))
        k_end -= nk
    if upfront:               # one large workspace, a region per range
        whole, view = _guarded(sum(slot_floats(nk) for _, nk in ranges))
        offs = [sum(slot_floats(nk) for _, nk in ranges[:n]) for n in range(len(ranges))]
        spaces = [(whole, view[o:o + slot_floats(nk)]) for o, (_, nk) in zip(offs, ranges)]
    else:
        spaces = [_guarded(slot_floats(nk)) for _, nk in ranges]

    def part(k0, nk, ws):
        q = PartParams()
        _set(q.p, G, K, dW1_last=g["dW1"], db1_last=g["db1"], **_common(t, cks, g))
        q.k0, q.nk, q.slots, q.ln_carry = k0, nk, ws.data_ptr(), carry.data_ptr()
        return q

    if upfront:
        for (k0, nk), (_, ws) in zip(ranges, spaces):
            _call(lib.emul_lin_recompute_groups, CS, part(k0, nk, ws), B * NH * nk, f"the recompute of groups [{k0}, {k0 + nk})")
    trail = []
    for n, ((k0, nk), (_, ws)) in enumerate(zip(ranges, spaces)):
        if stop_after is not None and n == stop_after:
            break
        if not upfront:
            _call(lib.emul_lin_recompute_groups, CS, part(k0, nk, ws), B * NH * nk, f"the recompute of groups [{k0}, {k0 + nk})")
        _call(lib.emul_lin_sweep_groups, CS, part(k0, nk, ws), B * NH, f"the sweep of groups [{k0}, {k0 + nk})")
        trail.append(g["dW1"].clone())
    for whole, _ in spaces + [(carry_all, None)]:
        assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[-GUARD:]).all(), "write outside a workspace"
    for k, v in t.items():
        assert torch.equal(v, keep[k]), f"input {k} was written"
    assert all(torch.equal(a, b) for a, b in zip(cks, keep_ck)), "a checkpoint was written"
    return g, trail


def _cuttings(K):
    return sorted({(K,), (1,) * K, (K - 1, 1), (1, K - 1)} - {(0, 1), (1, 0)})


CASES = [(16, 7), (16, 3), (16, 2), (16, 1), (64, 3), (64, 2)]


@pytest.mark.parametrize("CS,G", CASES)
def test_emulated_backward_in_parts_is_the_one_call_backward(emul, CS, G):
    """7 steps at G = 7 (one group), 3 (odd, last group of one step), 2 (even, ragged), 1: every cutting of the K groups - one range, one
    group per range, (K - 1, 1), (1, K - 1) -, with per-range workspaces (and, one group per range, with everything recomputed up front
    into one large workspace), gives the bits of the
    emulated one-call backward() in all eight gradients; nothing is written outside the workspaces; no LDS race at CS = 64.  The one
    call holds the bound of the one-call emulator tests against the fp64 oracle (with the same non-zero upstream gradients), and
    bit equality gives the parts that bound."""
    ref = _one_call(emul, CS, G)
    K = -(-NC // G)
    for cuts in _cuttings(K):
        for upfront in ((False, True) if cuts == (1,) * K and K > 1 else (False,)):      # up front: the cutting with the most ranges
            g, _ = _parts(emul, CS, G, cuts, upfront)
            for name in GRADS:
                assert torch.equal(g[name], ref[name]), (cuts, upfront, name)
    d, t, _ = _case(emul, CS, G)
    d64 = {k: v.double() for k, v in d.items()}
    s64 = tile_states(d64, B)
    le = d64["eta"][:, :, :, -1, :, None]
    _, rc, _ = O.linear_forward(d64["XQ"], d64["XK"], d64["XV"], le, d64["ln_w"], d64["ln_b"], s64["W1"], s64["b1"], G)
    rg = O.linear_backward(d64["XQ"], d64["XK"], d64["XV"], le, d64["ln_w"], d64["ln_b"], rc, G, d64["dOut"],
                           dst_last=(t["dW1_last"].double(), t["db1_last"].double()))
    rg["deta"] = rg["dlast_eta"]
    errs = {k: rel_l2(ref[k], rg[k].reshape(ref[k].shape)) for k in GRADS}
    print(f"emulated one-call backward CS={CS} G={G}", {k: round(v, 5) for k, v in errs.items()})
    assert all(v < GRAD_BOUND for v in errs.values()), errs


@pytest.mark.parametrize("CS,G", [(16, 3), (64, 2)])
def test_a_walk_that_stops_leaves_the_rest_untouched(emul, CS, G):
    """Sweeping only the groups [k0, K), k0 > 0: the gradients of the steps in front of group k0 and dln_w / dln_b (written by the range
    that holds group 0 only) stay NaN, those of the swept steps are final, and dW1 / db1 are the carried state - the same bits however
    [k0, K) itself was cut - from which the remaining ranges arrive at the one-call result."""
    ref = _one_call(emul, CS, G)
    K = -(-NC // G)
    k0 = 1
    g, trail = _parts(emul, CS, G, (k0, K - k0), stop_after=1)
    s0 = k0 * G
    assert torch.isnan(g["dln_w"]).all() and torch.isnan(g["dln_b"]).all()
    for name in ("deta", "dXQ", "dXK", "dXV"):
        assert torch.isnan(g[name][:, :, :s0].float()).all(), name
        assert torch.equal(g[name][:, :, s0:], ref[name][:, :, s0:]), name
    assert not torch.isnan(g["dW1"]).any() and not torch.isnan(g["db1"]).any()
    assert not torch.equal(g["dW1"], ref["dW1"]), "the carried state is not yet the result"
    # the same carried state from [k0, K) swept one group at a time, and the full walk continues from it to the one-call bits
    _, fine = _parts(emul, CS, G, (k0,) + (1,) * (K - k0))
    assert torch.equal(fine[K - k0 - 1], trail[0])
    full, coarse = _parts(emul, CS, G, (k0, K - k0))
    assert torch.equal(coarse[0], trail[0]) and torch.equal(full["dW1"], ref["dW1"])
