"""Inputs, runners and comparisons for the MFMA TTT-MLP backward at mini-batches of 16 (csrc/ttt_mlp16_bwd_body.h), shared by
tests/test_emul_mlp16_bwd_cpu.py (the body on the wave emulator) and tests/test_mlp_cs16_bwd_mfma_gpu.py (the device kernel).

A ``run`` is a callable (t, cks, up, G) -> (g, scratch): t = XQ XK XV eta dOut (bf16) and ln_w ln_b [NH, 64] fp32, cks = the four
checkpoint tensors [B, NH, K, ...] fp32, up = (dW1, db1, dW2, db2)_last fp32; g = the ten gradients, scratch = the four *_init_group
buffers [B, NH, G, ...].  Every output starts as NaN, the scratch lies between NaN guards, the inputs must come back unchanged.

Bounds (what tests/test_kernels_gpu.py applies to this geometry's forward and to the CS = 64 MFMA backward): rel-L2
against the fp64 oracle on the same bf16-rounded inputs, 1e-2 for outputs and checkpoints, 3e-2 for each of the ten gradients.

Seeds: 141 + NC for the five shapes, 500 + NC for the chain cases.  No draw had a near-constant LayerNorm row; no seed was replaced."""
import ctypes
import os
import subprocess

import torch

import scan_cases as C
from helpers import rel_l2
from oracle import ttt_oracle as O

F, H, CS = 64, 256, 16
TOL_OUT, TOL_G = 1e-2, 3e-2
SHAPES = [(1, 1, 1, 1), (1, 2, 5, 2), (2, 3, 9, 4), (1, 2, 7, 3), (1, 2, 6, 6)]       # (B, NH, NC, G)
CHAIN = ((11, 4), (7, 3), (3, 1))                                                       # (NC, G) at B = 2, NH = 3
CHAIN_B, CHAIN_NH = 2, 3
GRADS = ("dXQ", "dXK", "dXV", "dlast_eta", "dW1", "db1", "dW2", "db2", "dln_w", "dln_b")
EXACT = ("dXQ", "dXK", "dXV", "dlast_eta", "dW1", "db1", "dW2", "db2")
STATE_SHAPES = ((F, H), (1, H), (H, F), (1, F))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "ttt-video-dit_amd", "csrc")


def seed_of(shape):
    return 141 + shape[2]


def case(B, NH, NC, seed):
    """scan_cases.scan_case (bf16-valued activations, ln_w / ln_b per head, a state per (b, h)) plus a bf16-valued dOut; fp64"""
    c = C.scan_case("mlp", B, NH, NC, CS, seed)
    g = torch.Generator().manual_seed(seed + 200003)
    c["dOut"] = torch.randn(B, NH, NC, CS, F, generator=g, dtype=torch.float64).bfloat16().double()
    return c


def host_tensors(c):
    t = {k: c[k].to(torch.bfloat16).contiguous() for k in ("XQ", "XK", "XV", "eta", "dOut")}
    t.update({k: c[k].float().contiguous() for k in ("ln_w", "ln_b", "W1", "b1", "W2", "b2")})
    return t


def oracle_forward(c, G):
    out, cks, _ = O.mlp_forward(c["XQ"], c["XK"], c["XV"], c["eta"], c["ln_w"], c["ln_b"], c["W1"], c["b1"], c["W2"], c["b2"], G)
    return out, cks


def oracle_backward(c, cks, G, up):
    return O.mlp_backward(c["XQ"], c["XK"], c["XV"], c["eta"], c["ln_w"], c["ln_b"], tuple(k.double().cpu() for k in cks), G, c["dOut"],
                          dst_last=tuple(u.double().cpu() for u in up))


def upstream(c, cks, G, seed):
    """(dW1, db1, dW2, db2)_last drawn per (b, h), each (b, h) scaled to the norm of the call's own contribution (the oracle's state
    gradient with zero upstream), as scan_bwd_cases.bwd_case does; fp32"""
    B, NH = c["XQ"].shape[:2]
    zero = tuple(torch.zeros(B, NH, *s, dtype=torch.float64) for s in STATE_SHAPES)
    own = oracle_backward(c, cks, G, zero)
    g = torch.Generator().manual_seed(seed + 300007)
    up = []
    for s, name in zip(STATE_SHAPES, ("dW1", "db1", "dW2", "db2")):
        x = torch.randn(B, NH, *s, generator=g, dtype=torch.float64)
        n = lambda v: v.flatten(2).norm(dim=-1)[:, :, None, None]
        up.append((x * (n(own[name]) / n(x))).float().contiguous())
    return tuple(up)


def errors(g, ref):
    """whole-tensor rel-L2 of the ten gradients, and of dW1 / db1 / dW2 per 32-hidden-unit slice (the share of one wave)"""
    e = {k: rel_l2(g[k].cpu(), ref[k].reshape(g[k].shape)) for k in GRADS}
    for w in range(H // 32):
        s = slice(32 * w, 32 * w + 32)
        e[f"dW1[w{w}]"] = rel_l2(g["dW1"].cpu()[..., s], ref["dW1"][..., s])
        e[f"db1[w{w}]"] = rel_l2(g["db1"].cpu()[..., s], ref["db1"][..., s])
        e[f"dW2[w{w}]"] = rel_l2(g["dW2"].cpu()[..., s, :], ref["dW2"][..., s, :])
    return e


def check_call(tag, run, c, cks, up, G):
    """one backward call from the checkpoints ``cks`` against the fp64 oracle from the same checkpoints and upstream"""
    t = host_tensors(c)
    g, scratch = run(t, cks, up, G)
    assert not any(torch.isnan(g[k].float()).any() for k in GRADS), (tag, [k for k in GRADS if torch.isnan(g[k].float()).any()])
    e = errors(g, oracle_backward(c, cks, G, up))
    print(f"{tag}: " + "  ".join(f"{k} {v:.3g}" for k, v in e.items()))
    bad = {k: v for k, v in e.items() if not v < TOL_G}
    assert not bad, (tag, bad)
    return g, scratch


def chain(run, t, cks, up, NC, G):
    """K one-group calls in place of the call over K groups, from the last group to the first, chained through the four state
    gradients; dln_w / dln_b: the sum of the calls' partials in call order"""
    K = -(-NC // G)
    parts, dln = {k: [None] * K for k in ("dXQ", "dXK", "dXV", "dlast_eta")}, None
    for k in reversed(range(K)):
        lo, hi = k * G, min((k + 1) * G, NC)
        tk = {n: (v[:, :, lo:hi].contiguous() if n in ("XQ", "XK", "XV", "eta", "dOut") else v) for n, v in t.items()}
        g, _ = run(tk, tuple(c[:, :, k:k + 1].contiguous() for c in cks), up, G)
        up = tuple(g[n].clone() for n in ("dW1", "db1", "dW2", "db2"))
        for n in parts:
            parts[n][k] = g[n]
        dln = (g["dln_w"].clone(), g["dln_b"].clone()) if dln is None else (dln[0] + g["dln_w"], dln[1] + g["dln_b"])
    out = {n: torch.cat(v, 2) for n, v in parts.items()}
    out.update(dW1=up[0], db1=up[1], dW2=up[2], db2=up[3], dln_w=dln[0], dln_b=dln[1])
    return out


def check_chain(tag, run, c, cks, up, G, dln_tol):
    t = host_tensors(c)
    NC = c["XQ"].shape[2]
    whole, _ = run(t, cks, up, G)
    parts = chain(run, t, cks, up, NC, G)
    assert not any(torch.isnan(whole[k].float()).any() for k in GRADS), tag
    same = {k: torch.equal(whole[k], parts[k]) for k in EXACT}
    dln = max(float(((whole[k] - parts[k]).double().flatten(2).norm(dim=-1) / parts[k].double().flatten(2).norm(dim=-1)).max())
              for k in ("dln_w", "dln_b"))
    print(f"{tag}: whole call vs chain of {-(-NC // G)} one-group calls: equal bits {same}  dln {dln:.3g}")
    assert all(same.values()), (tag, same)
    assert dln < dln_tol, (tag, dln, dln_tol)


# ------------------------------------------------------------------------------------------------ the wave emulator
_PTRS = ("XQ", "XK", "XV", "eta", "ln_w", "ln_b", "W1c", "b1c", "W2c", "b2c", "dOut", "dW1_last", "db1_last", "dW2_last", "db2_last",
         "W1s", "b1s", "W2s", "b2s", "dln_w", "dln_b", "dW1", "db1", "dW2", "db2", "deta", "dXQ", "dXK", "dXV")


class BwdParams(ctypes.Structure):            # wv::Mlp16BwdParams (csrc/ttt_wave_types.h)
    _fields_ = [(n, ctypes.c_void_p) for n in _PTRS] + [(n, ctypes.c_int) for n in ("NH", "NC", "G", "K")] + [("eps", ctypes.c_float)]


class FwdParams(ctypes.Structure):            # wv::Mlp16Params
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("XQ", "XK", "XV", "eta", "ln_w", "ln_b", "W1", "b1", "W2", "b2", "W1c", "b1c", "W2c", "b2c", "out")] + \
               [(n, ctypes.c_int) for n in ("NH", "NC", "G", "K")] + [("eps", ctypes.c_float)]


def build_emul():
    build = os.path.join(HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libmlp16_bwd_emul.so")
    srcs = [os.path.join(HERE, "emul", f) for f in ("mlp16_bwd_emul.cpp", "wave_emul.h")] + \
           [os.path.join(CSRC, f) for f in ("ttt_mlp16_bwd_body.h", "ttt_mlp16_body.h", "ttt_lin16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([C.CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", CSRC, "-I", os.path.join(HERE, "emul"), srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.emul_mlp16_bwd_params_size() == ctypes.sizeof(BwdParams)
    assert lib.emul_mlp16_params_size() == ctypes.sizeof(FwdParams)
    assert lib.emul_mlp16_bwd_lds_bytes() <= 160 * 1024
    return lib


def _nan(*s, dt=torch.float32, device="cpu"):
    return torch.full(s, float("nan"), dtype=dt, device=device)


def outputs(B, NH, NC, device="cpu"):
    bf = torch.bfloat16
    return dict(dln_w=_nan(B, NH, 1, F, device=device), dln_b=_nan(B, NH, 1, F, device=device), dW1=_nan(B, NH, F, H, device=device),
                db1=_nan(B, NH, 1, H, device=device), dW2=_nan(B, NH, H, F, device=device), db2=_nan(B, NH, 1, F, device=device),
                dlast_eta=_nan(B, NH, NC, CS, 1, dt=bf, device=device), dXQ=_nan(B, NH, NC, CS, F, dt=bf, device=device),
                dXK=_nan(B, NH, NC, CS, F, dt=bf, device=device), dXV=_nan(B, NH, NC, CS, F, dt=bf, device=device))


GUARD = 64


def guarded_scratch(B, NH, G, device="cpu"):
    """the four *_init_group buffers [B, NH, G, ...] as views into NaN-filled storage with GUARD floats on either side"""
    raw = [_nan(B * NH * G * a * b + 2 * GUARD, device=device) for a, b in STATE_SHAPES]
    return raw, [r[GUARD:-GUARD].view(B, NH, G, a, b) for r, (a, b) in zip(raw, STATE_SHAPES)]


def check_guards(raw):
    for r in raw:
        assert torch.isnan(r[:GUARD]).all() and torch.isnan(r[-GUARD:]).all(), "write outside the documented scratch"


def emul_forward(lib, t, G):
    B, NH, NC = t["XQ"].shape[:3]
    K = -(-NC // G)
    cks = tuple(_nan(B, NH, K, a, b) for a, b in STATE_SHAPES)
    out = _nan(B, NH, NC, CS, F, dt=torch.bfloat16)
    p = FwdParams()
    for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=t["W1"], b1=t["b1"], W2=t["W2"],
                     b2=t["b2"], W1c=cks[0], b1c=cks[1], W2c=cks[2], b2c=cks[3], out=out).items():
        assert v.is_contiguous()
        setattr(p, n, v.data_ptr())
    p.NH, p.NC, p.G, p.K, p.eps = NH, NC, G, K, 1e-8
    msg = ctypes.create_string_buffer(256)
    assert lib.emul_mlp16_forward(ctypes.byref(p), B * NH, msg, 256) == 0, msg.value.decode()
    return out, cks


def emul_run(lib):
    def run(t, cks, up, G):
        B, NH, NC = t["XQ"].shape[:3]
        K = cks[0].shape[2]
        assert K == -(-NC // G)
        g = outputs(B, NH, NC)
        raw, scr = guarded_scratch(B, NH, G)
        ins = dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1c=cks[0], b1c=cks[1], W2c=cks[2],
                   b2c=cks[3], dOut=t["dOut"], dW1_last=up[0], db1_last=up[1], dW2_last=up[2], db2_last=up[3])
        keep = {k: v.clone() for k, v in ins.items()}
        p = BwdParams()
        for n, v in dict(ins, W1s=scr[0], b1s=scr[1], W2s=scr[2], b2s=scr[3], dln_w=g["dln_w"], dln_b=g["dln_b"], dW1=g["dW1"], db1=g["db1"],
                         dW2=g["dW2"], db2=g["db2"], deta=g["dlast_eta"], dXQ=g["dXQ"], dXK=g["dXK"], dXV=g["dXV"]).items():
            assert v.is_contiguous()
            setattr(p, n, v.data_ptr())
        p.NH, p.NC, p.G, p.K, p.eps = NH, NC, G, K, 1e-8
        msg = ctypes.create_string_buffer(256)
        races = lib.emul_mlp16_backward(ctypes.byref(p), B * NH, msg, 256)
        assert races == 0, f"LDS race between the waves of the backward: {msg.value.decode()}"
        check_guards(raw)
        for k, v in ins.items():
            assert torch.equal(v, keep[k]), f"input {k} was written"
        return g, scr
    return run
