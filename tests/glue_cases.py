"""Seeded inputs of the glue kernels (csrc/ttt_prepost.hip) and their fp64 oracle results with gradients, shared by the sensitivity
table (tests/test_glue_oracle_cpu.py) and the device tests (tests/test_prepost_oracle_gpu.py).  Every input is a bf16 value (fp32
parameters: bf16-representable), so the kernels and the oracle see the same numbers."""
import math

import torch

from oracle import glue_oracle as G


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(*shape, g, sc=1.0):
    return (sc * torch.randn(*shape, generator=g)).bfloat16()


def pre_case(B, L, NH, seed=0):
    g = _gen(seed)
    D = NH * 64
    d = {"q": _bf(B, L, D, g=g), "k": _bf(B, L, D, g=g), "v": _bf(B, L, D, g=g, sc=0.5),
         "ln_w": _bf(NH, 64, g=g, sc=0.3).float() + 1, "ln_b": _bf(NH, 64, g=g, sc=0.2).float()}
    d.update({n: _bf(B, NH, L, 64, g=g) for n in ("dXQ", "dXK", "dXV")})
    return d


def pre_oracle(d, rope, src, pos, NH, dtype=torch.float64, heads=None, **mut):
    """oracle forward + backward on (a head subset of) a pre case: {XQ, XK, XV, dq, dk, dv, dln_w, dln_b}"""
    hs = list(range(NH)) if heads is None else list(heads)
    cols = torch.cat([torch.arange(h * 64, (h + 1) * 64) for h in hs])
    x = [d[n].index_select(2, cols).to(dtype).requires_grad_(True) for n in ("q", "k", "v")]
    w, b = (d[n][hs].to(dtype).requires_grad_(True) for n in ("ln_w", "ln_b"))
    outs = G.pre(*x, w, b, None if rope is None else rope.to(dtype), src, pos, len(hs), **mut)
    gr = [d[n][:, hs].to(dtype) for n in ("dXQ", "dXK", "dXV")]
    gx = torch.autograd.grad(outs, x + [w, b], gr)
    r = dict(zip(("XQ", "XK", "XV"), (o.detach() for o in outs)))
    r.update(zip(("dq", "dk", "dv", "dln_w", "dln_b"), gx))
    return r


def post_case(B, L, NH, seed=0):
    """Y rows (one token, all heads) of RMS 1e-3 .. 1: the small ones make eps matter"""
    g = _gen(seed)
    D = NH * 64
    sc = torch.exp(torch.empty(B, 1, L, 1).uniform_(math.log(1e-3), 0.0, generator=g))
    return {"Y": (sc * torch.randn(B, NH, L, 64, generator=g)).bfloat16(), "w": _bf(D, g=g, sc=0.3).float() + 1,
            "b": _bf(D, g=g, sc=0.2).float(), "dOut": _bf(B, L, D, g=g)}


def post_oracle(d, src, eps, dtype=torch.float64, **mut):
    Y, w, b = (d[n].to(dtype).requires_grad_(True) for n in ("Y", "w", "b"))
    out = G.post(Y, w, b, src, eps, **mut)
    gY, gw, gb = torch.autograd.grad(out, (Y, w, b), d["dOut"].to(dtype))
    return {"out": out.detach(), "dY": gY, "dw": gw, "db": gb}


def gate_case(B, L, D, seed=0):
    g = _gen(seed)
    return {"res": _bf(B, L, D, g=g), "y": _bf(B, L, D, g=g), "at": _bf(D, g=g, sc=0.5).float(), "av": _bf(D, g=g, sc=0.5).float(),
            "g": _bf(B, L, D, g=g)}


def gate_oracle(d, n_text, dtype=torch.float64, **mut):
    res, y, at, av = (d[n].to(dtype).requires_grad_(True) for n in ("res", "y", "at", "av"))
    out = G.gate(res, y, at, av, n_text, **mut)
    gy, gt, gv = torch.autograd.grad(out, (y, at, av), d["g"].to(dtype))
    # the kernel's partials are d/d tanh(alpha): the chain rule's 1 - tanh^2 is applied by the caller
    return {"out": out.detach(), "dy": gy, "dtanh_t": gt / (1 - torch.tanh(at.detach()) ** 2),
            "dtanh_v": gv / (1 - torch.tanh(av.detach()) ** 2)}


def adaln_case(B, Lt, Lv, D, seed=0):
    """distinct modulation per batch and group; shift / scale bf16 values as the modulation Linear produces them"""
    g = _gen(seed)
    d = {"vid": _bf(B, Lv, D, g=g, sc=2.0), "text": _bf(B, Lt, D, g=g), "w": _bf(D, g=g, sc=0.2).float() + 1,
         "b": _bf(D, g=g, sc=0.1).float(), "dout": _bf(B, Lt + Lv, D, g=g)}
    d.update({n: _bf(B, D, g=g, sc=0.3).float() for n in ("sh_v", "sc_v", "sh_t", "sc_t", "g_v", "g_t")})
    d.update({"y": _bf(B, Lt + Lv, D, g=g), "dvid": _bf(B, Lv, D, g=g), "dtext": _bf(B, Lt, D, g=g)})
    return d


ADALN_NAMES = ("vid", "text", "w", "b", "sh_v", "sc_v", "sh_t", "sc_t")


def adaln_oracle(d, eps, dtype=torch.float64):
    x = [d[n].to(dtype).requires_grad_(True) for n in ADALN_NAMES]
    out = G.adaln(*x, eps)
    gr = torch.autograd.grad(out, x, d["dout"].to(dtype), allow_unused=True)
    r = {"out": out.detach()}
    r.update(("d" + n, t if t is not None else torch.zeros_like(x[i])) for i, (n, t) in enumerate(zip(ADALN_NAMES, gr)))
    return r


def resgate_oracle(d, dtype=torch.float64):
    x = [d[n].to(dtype).requires_grad_(True) for n in ("vid", "text", "y", "g_v", "g_t")]
    ov, ot = G.resgate(*x)
    gr = torch.autograd.grad((ov, ot), x[2:], (d["dvid"].to(dtype), d["dtext"].to(dtype)), allow_unused=True)
    r = {"ovid": ov.detach(), "otext": ot.detach()}
    r.update(("d" + n, t if t is not None else torch.zeros_like(x[2 + i])) for i, (n, t) in enumerate(zip(("y", "g_v", "g_t"), gr)))
    return r
