"""TTT-MLP backward at mini-batches of 16: the opt-in MFMA backward (csrc/ttt_mlp16_bwd_body.h) against the generic kernels, alternated
from iteration to iteration inside one process from the same MFMA forward's checkpoints, one HIP event pair per call.

    timeout -k 10 600 python tools/mlp16_bwd_bench.py [--nh 48] [--nc 1128] [--batch 1] [--g 16] [--iters 6] [--warmup 1]
                                                       [--budget-s 240] [--json FILE]

The generic kernels are what ``auto`` runs for this call, so the ratio is the opt-in path against the default one.  Nobody had
measured the generic leg at this geometry: a first call of each leg is timed on its own, and the iteration count is cut down so that
the generic leg stays inside ``--budget-s`` seconds (at least one timed iteration of each).  Run it under ``timeout -k 10``."""
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
ap.add_argument("--nc", type=int, default=1128, help="mini-batches of 16: 1128 = the 3 s video, 3216 = the 9 s video")
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--g", type=int, default=16, help="checkpoint group size (ModelConfig.scan_checkpoint_group_size)")
ap.add_argument("--iters", type=int, default=6)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--budget-s", type=float, default=240.0, help="wall-clock budget of the generic leg")
ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = "cuda:0"
B, NH, NC, CS, F, G = a.batch, a.nh, a.nc, 16, 64, a.g
H, K = 4 * F, -(-NC // G)
torch.manual_seed(0)
n = lambda *s: torch.randn(*s, device=dev)
XQ = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XK = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XV, dOut = n(B, NH, NC, CS, F).bfloat16(), n(B, NH, NC, CS, F).bfloat16()
le = (0.1 * torch.sigmoid(n(B, NH, NC, CS, 1)) / F).bfloat16()
lw, lb = torch.ones(1, NH, 1, F, device=dev), torch.zeros(1, NH, 1, F, device=dev)
state = (0.02 * n(B, NH, F, H), torch.zeros(B, NH, 1, H, device=dev), 0.02 * n(B, NH, H, F), torch.zeros(B, NH, 1, F, device=dev))
f32 = lambda *s: torch.empty(*s, device=dev)
bf = lambda *s: torch.empty(*s, device=dev, dtype=torch.bfloat16)
out = torch.empty_like(XQ)
cks = (f32(B, NH, K, F, H), f32(B, NH, K, 1, H), f32(B, NH, K, H, F), f32(B, NH, K, 1, F))
e.ttt_forward(XQ, XK, XV, le, lw, lb, *state, *cks, out, G)              # the MFMA forward scan: both legs start from its checkpoints
up = tuple(torch.zeros_like(s) for s in state)
IMPLS = ("generic", "mfma")
buf = {impl: dict(scr=(f32(B, NH, G, F, H), f32(B, NH, G, 1, H), f32(B, NH, G, H, F), f32(B, NH, G, 1, F)),
                  g=(f32(B, NH, 1, F), f32(B, NH, 1, F), f32(B, NH, F, H), f32(B, NH, 1, H), f32(B, NH, H, F), f32(B, NH, 1, F),
                     bf(B, NH, NC, CS, 1), torch.empty_like(XQ), torch.empty_like(XQ), torch.empty_like(XQ))) for impl in IMPLS}


def bwd(impl):
    b = buf[impl]
    e.ttt_backward_impl(impl, XQ, XK, XV, le, lw, lb, *cks, out, *b["scr"], *[None] * 12, *up, dOut, *b["g"], G)


def timed(impl):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    bwd(impl)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


first = {impl: timed(impl) for impl in IMPLS}                  # (also the first-call warm-up of each leg)
iters = max(1, min(a.iters, int(a.budget_s * 1e3 / max(first["generic"], 1e-3)) - a.warmup))
warmup = a.warmup if iters > 1 else 0
ms = {impl: [] for impl in IMPLS}
for it in range(warmup + iters):
    for impl in (IMPLS if it % 2 == 0 else IMPLS[::-1]):       # alternate, and alternate who goes first
        t = timed(impl)
        if it >= warmup:
            ms[impl].append(t)
res = {"geometry": dict(B=B, NH=NH, NC=NC, CS=CS, F=F, G=G), "iters": iters, "warmup": warmup, "first_call_ms": first,
       "device": torch.cuda.get_device_name(0)}
for impl in IMPLS:
    v = ms[impl]
    res[f"bwd_{impl}_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "us_per_step": statistics.median(v) * 1e3 / NC}
res["bwd_mfma_over_generic"] = res["bwd_mfma_ms"]["median"] / res["bwd_generic_ms"]["median"]
res["mfma_slowest_faster_than_generic_fastest"] = res["bwd_mfma_ms"]["max"] < res["bwd_generic_ms"]["min"]
rel = lambda x, y: float((x.float() - y.float()).norm() / y.float().norm())
names = ("dln_w", "dln_b", "dW1", "db1", "dW2", "db2", "dlast_eta", "dXQ", "dXK", "dXV")
res["rel_l2_mfma_vs_generic"] = {k: rel(x, y) for k, x, y in zip(names, buf["mfma"]["g"], buf["generic"]["g"])}
line = json.dumps(res)
print(line)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(line + "\n")
