"""TTT-Linear at mini-batches of 64: the opt-in MFMA scan / sweep (csrc/ttt_lin64_body.h) against the generic kernels, alternated from
iteration to iteration inside one process, forward and backward timed separately (one event pair per call).

    python tools/lin64_bench.py [--nh 48] [--nc 282] [--batch 1] [--g 16] [--iters 10] [--warmup 2] [--json FILE]

The generic kernels are what ``auto`` runs for this geometry, so the ratio is the opt-in path against the default one."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ttt-video-dit_amd"))
import test_time_training as e  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nh", type=int, default=48)
ap.add_argument("--nc", type=int, default=282)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--g", type=int, default=16, help="checkpoint group size (ModelConfig.scan_checkpoint_group_size)")
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = "cuda:0"
B, NH, NC, CS, F, G = a.batch, a.nh, a.nc, 64, 64, a.g
K = -(-NC // G)
torch.manual_seed(0)
n = lambda *s: torch.randn(*s, device=dev)
XQ = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XK = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XV, dOut = n(B, NH, NC, CS, F).bfloat16(), n(B, NH, NC, CS, F).bfloat16()
le = (1.0 * torch.sigmoid(n(B, NH, NC, CS, 1)) / (F * CS)).bfloat16()
lw, lb = torch.ones(NH, F, device=dev), torch.zeros(NH, F, device=dev)
W1, b1 = 0.02 * n(B, NH, F, F), torch.zeros(B, NH, 1, F, device=dev)
f32 = lambda *s: torch.empty(*s, device=dev)
IMPLS = ("generic", "mfma")
buf = {}
for impl in IMPLS:
    buf[impl] = dict(out=torch.empty_like(XQ), cks=(f32(B, NH, K, F, F), f32(B, NH, K, 1, F)), scr=(f32(B, NH, G, F, F), f32(B, NH, G, 1, F)),
                     up=(torch.zeros(B, NH, F, F, device=dev), torch.zeros(B, NH, 1, F, device=dev)),
                     g=(f32(B, NH, 1, F), f32(B, NH, 1, F), f32(B, NH, F, F), f32(B, NH, 1, F),
                        torch.empty(B, NH, NC, CS, 1, device=dev, dtype=torch.bfloat16), torch.empty_like(XQ), torch.empty_like(XQ), torch.empty_like(XQ)))


def fwd(impl):
    b = buf[impl]
    e.ttt_linear_forward_impl(impl, XQ, XK, XV, le, lw, lb, W1, b1, *b["cks"], b["out"], G)


def bwd(impl):
    b = buf[impl]
    e.ttt_linear_backward_impl(impl, XQ, XK, XV, le, lw, lb, *b["cks"], *b["up"], dOut, *b["scr"], *b["g"], G)


def timed(fn, impl):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn(impl)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


ms = {(d, impl): [] for d in ("fwd", "bwd") for impl in IMPLS}
for it in range(a.warmup + a.iters):
    for impl in (IMPLS if it % 2 == 0 else IMPLS[::-1]):       # alternate, and alternate who goes first
        tf, tb = timed(fwd, impl), timed(bwd, impl)
        if it >= a.warmup:
            ms["fwd", impl].append(tf)
            ms["bwd", impl].append(tb)
res = {"geometry": dict(B=B, NH=NH, NC=NC, CS=CS, F=F, G=G), "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
for d in ("fwd", "bwd"):
    for impl in IMPLS:
        v = ms[d, impl]
        res[f"{d}_{impl}_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "us_per_step": statistics.median(v) * 1e3 / NC}
    res[f"{d}_mfma_over_generic"] = res[f"{d}_mfma_ms"]["median"] / res[f"{d}_generic_ms"]["median"]
rel = lambda x, y: float((x.float() - y.float()).norm() / y.float().norm())
res["rel_l2_mfma_vs_generic"] = {"out": rel(buf["mfma"]["out"], buf["generic"]["out"]), "dXK": rel(buf["mfma"]["g"][6], buf["generic"]["g"][6]),
                                 "dW1": rel(buf["mfma"]["g"][2], buf["generic"]["g"][2])}
line = json.dumps(res)
print(line)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(line + "\n")
