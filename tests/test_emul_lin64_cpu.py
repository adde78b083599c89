"""The workgroup-level kernel bodies of csrc/ttt_lin64_body.h (TTT-Linear, mini-batches of 64: four waves per (b, h), the state and
the token rows split between them) executed on the CPU by the wave emulator of tests/emul (256 host threads per scan; its LDS race
detector watches every exchange between the waves that uses the tracked loads and stores - all but the L_WHI slot, which goes through
raw pointers like a scratch slot), against the fp64 oracle, the reference-executed golden and, one step at a time,
the comparison of tests/scan_cases.py.  The same template bodies are instantiated with the device backend in csrc/ttt_mfma16.hip
(linear_fwd_cs64_kernel / linear_bwd_cs64_kernel)."""
import ctypes
import os
import subprocess

import pytest
import torch

import scan_cases as C
from helpers import SCAN_TOL, load_golden, op_inputs, rel_l2, tile_states
from oracle import ttt_oracle as O
from test_emul_cpu import Params
from test_kernels_gpu import check_vs_golden

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ttt-video-dit_amd", "csrc")
CS = 64


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(C.CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    build = os.path.join(HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "liblin64_emul.so")
    srcs = [os.path.join(HERE, "emul", f) for f in ("lin64_emul.cpp", "wave_emul.h")] + \
           [os.path.join(CSRC, f) for f in ("ttt_lin64_body.h", "ttt_lin16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([C.CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", CSRC, "-I", os.path.join(HERE, "emul"), srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.emul_lin64_params_size() == ctypes.sizeof(Params)
    assert lib.emul_lin64_lds_bytes(0) <= lib.emul_lin64_lds_bytes(1) <= 160 * 1024
    return lib


def _call(fn, p, n_bh):
    msg = ctypes.create_string_buffer(256)
    races = fn(ctypes.byref(p), n_bh, msg, 256)
    assert races == 0, f"LDS race between the waves of a scan: {msg.value.decode()}"


def _forward(lib, t, G):
    """t: XQ XK XV eta [.., 64, 1] (bf16), ln_w ln_b [NH, 64], W1 b1 [B, NH, ..] (fp32) -> out, {W1, b1} checkpoints"""
    B, NH, NC = t["XQ"].shape[:3]
    K = -(-NC // G)
    cks = dict(W1=torch.full((B, NH, K, 64, 64), float("nan")), b1=torch.full((B, NH, K, 1, 64), float("nan")))
    out = torch.full((B, NH, NC, CS, 64), float("nan"), dtype=torch.bfloat16)
    p = Params()
    for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=t["W1"], b1=t["b1"],
                     W1c=cks["W1"], b1c=cks["b1"], out=out).items():
        setattr(p, n, v.data_ptr())
    p.NH, p.NC, p.G, p.K, p.eps = NH, NC, G, K, 1e-8
    _call(lib.emul_lin64_forward, p, B * NH)
    return out, cks


def _backward(lib, t, G, cks, dOut):
    B, NH, NC = t["XQ"].shape[:3]
    K = -(-NC // G)
    nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt)
    g = dict(dln_w=nan(B, NH, 1, 64), dln_b=nan(B, NH, 1, 64), dW1=nan(B, NH, 64, 64), db1=nan(B, NH, 1, 64),
             dlast_eta=nan(B, NH, NC, CS, 1, dt=torch.bfloat16), dXQ=nan(B, NH, NC, CS, 64, dt=torch.bfloat16),
             dXK=nan(B, NH, NC, CS, 64, dt=torch.bfloat16), dXV=nan(B, NH, NC, CS, 64, dt=torch.bfloat16))
    dWl, dbl = torch.zeros(B, NH, 64, 64), torch.zeros(B, NH, 1, 64)
    # the scratch of the tensor contract: W1_init_group [B, NH, G, 64, 64] fp32 = G x 16 KiB, b1_init_group [B, NH, G, 1, 64], between guards
    guard = 64
    scr_w, scr_b = nan(B * NH * G * 64 * 64 + 2 * guard), nan(B * NH * G * 64 + 2 * guard)
    p = Params()
    for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1c=cks["W1"], b1c=cks["b1"],
                     dOut=dOut, dW1_last=dWl, db1_last=dbl, scratch_w=scr_w[guard:], scratch_b=scr_b[guard:], dln_w=g["dln_w"],
                     dln_b=g["dln_b"], dW1=g["dW1"], db1=g["db1"], deta=g["dlast_eta"], dXQ=g["dXQ"], dXK=g["dXK"], dXV=g["dXV"]).items():
        setattr(p, n, v.data_ptr())
    p.NH, p.NC, p.G, p.K, p.eps = NH, NC, G, K, 1e-8
    _call(lib.emul_lin64_backward, p, B * NH)
    for s in (scr_w, scr_b):
        assert torch.isnan(s[:guard]).all() and torch.isnan(s[-guard:]).all(), "write outside the documented scratch"
    return g


def _tensors(d, B):
    bf = lambda x: x.to(torch.bfloat16).contiguous()
    st = tile_states(d, B)
    return dict(XQ=bf(d["XQ"]), XK=bf(d["XK"]), XV=bf(d["XV"]), eta=bf(d["eta"][:, :, :, -1, :, None]),
                ln_w=d["ln_w"].float().contiguous(), ln_b=d["ln_b"].float().contiguous(),
                W1=st["W1"].float().contiguous(), b1=st["b1"].float().contiguous())


def _run(lib, d, G):
    B = d["XQ"].shape[0]
    t = _tensors(d, B)
    keep = {k: v.clone() for k, v in t.items()}
    out, cks = _forward(lib, t, G)
    g = _backward(lib, t, G, cks, d["dOut"].to(torch.bfloat16).contiguous())
    for k, v in t.items():
        assert torch.equal(v, keep[k]), f"input {k} was written"
    return out, cks, g


_ORACLE = {}


def _oracle(shape):
    """inputs (bf16-valued activations) and the fp64 oracle's results for a shape, computed once"""
    if shape not in _ORACLE:
        B, NH, NC, G = shape
        d = O.make_inputs("linear", B, NH, NC, CS, 64, seed=99 + NC)
        for k in ("XQ", "XK", "XV", "eta", "dOut"):
            d[k] = d[k].to(torch.bfloat16).to(torch.float32)
        d64 = {k: v.double() for k, v in d.items()}
        st = tile_states(d64, B)
        le = d64["eta"][:, :, :, -1, :, None]
        out, cks, _ = O.linear_forward(d64["XQ"], d64["XK"], d64["XV"], le, d64["ln_w"], d64["ln_b"], st["W1"], st["b1"], G)
        g = O.linear_backward(d64["XQ"], d64["XK"], d64["XV"], le, d64["ln_w"], d64["ln_b"], cks, G, d64["dOut"])
        _ORACLE[shape] = (d, out, cks, g)
    return _ORACLE[shape]


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 4, 2), (1, 2, 7, 3)])
def test_emulated_linear_cs64_vs_oracle(emul, shape):
    """forward scan and reverse sweep vs the fp64 oracle on the same bf16-rounded inputs: a single step, even groups, a ragged last
    group with an odd group size.  Bounds of the device parity tests: outputs / checkpoints 1e-2, gradients 3e-2."""
    d, ro, rc, rg = _oracle(shape)
    out, cks, g = _run(emul, d, shape[3])
    errs = {"XQW": rel_l2(out, ro), "W1c": rel_l2(cks["W1"], rc[0]), "b1c": rel_l2(cks["b1"], rc[1])}
    gerrs = {k: rel_l2(g[k], rg[k].reshape(g[k].shape)) for k in g}
    print("emulated linear CS=64", shape, {k: round(v, 5) for k, v in {**errs, **gerrs}.items()})
    assert all(v < 1e-2 for v in errs.values()), errs
    assert all(v < 3e-2 for v in gerrs.values()), gerrs


def test_emulated_linear_cs64_vs_reference_golden(emul):
    """against the results of the executed reference (tests/golden/op_lin_f64_cs64.pt) on its inputs rounded to bf16"""
    gold = load_golden("op_lin_f64_cs64.pt")
    d = op_inputs(gold)
    out, _, g = _run(emul, d, gold["G"])
    check_vs_golden(gold, out, g, 1.5e-2, 4e-2)


def _scan_case_run(lib, regime):
    kind, cs, B, NH, NC, G, seed = C.MFMA_CASES["lin64_b2"]
    assert (kind, cs) == ("linear", CS)
    c = C.scan_case(kind, B, NH, C.run_steps(kind, NC, G), cs, seed, regime)
    t = {k: c[k].to(torch.bfloat16).contiguous() for k in ("XQ", "XK", "XV", "eta")}
    t.update({k: c[k].float().contiguous() for k in ("ln_w", "ln_b", "W1", "b1")})
    out, cks = _forward(lib, t, G)
    return c, out, cks, G


@pytest.mark.parametrize("regime", ["base", "high"])
def test_emulated_linear_cs64_one_step_at_a_time(emul, regime):
    """the case ``lin64_b2`` of the device file (B = 2 x 3 heads, a state per batch element, G = 1): every step's state delta and
    output against the fp64 step from the scan's own checkpoint, at SCAN_TOL"""
    c, out, cks, G = _scan_case_run(emul, regime)
    assert not torch.isnan(out.float()).any() and not any(torch.isnan(v).any() for v in cks.values())
    C.assert_initial_state(c, cks)
    m = C.compare(c, out, cks, G, None)
    print(f"emulated lin64_b2 {regime}: {C.fmt(m)}")
    bad = {k: (v, SCAN_TOL[k]) for k, v in m.items() if not v < SCAN_TOL[k]}
    assert not bad, bad
