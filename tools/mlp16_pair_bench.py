"""TTT-MLP forward scan at mini-batches of 16: the opt-in pair form (csrc/ttt_mlp16_pair_body.h: a state workgroup and an output
workgroup per (b, h)) against the one-workgroup kernel, alternated from iteration to iteration inside one process on the same inputs,
one HIP event pair per call.

    timeout -k 10 300 python tools/mlp16_pair_bench.py [--batch 2] [--nh 48] [--nc 3216] [--g NC] [--iters 7] [--warmup 2] [--json FILE]

The yardstick is the one-workgroup arm of the same process: the pair "wins" when its slowest iteration beats that arm's fastest.
``--nc 3216`` = the 9 s video, ``--nc 21948`` = the 63 s video (the sampler runs one checkpoint group: ``--g`` defaults to NC).  One JSON
line; outputs and checkpoints of the two arms are compared bit for bit.  Run it under ``timeout -k 10``."""
import argparse
import ctypes
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
ap.add_argument("--nc", type=int, default=3216, help="mini-batches of 16: 3216 = the 9 s video, 21948 = the 63 s video")
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--g", type=int, default=0, help="checkpoint group size; 0 = NC (sampling: one group)")
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--json", default=None)
ap.add_argument("--lib", default=None, help="another build of libttt_hip.so for the whole run (e.g. one with another ring depth)")
a = ap.parse_args()
if a.lib:
    e._LIB_PATH = os.path.abspath(a.lib)
dev = "cuda:0"
B, NH, NC, CS, F = a.batch, a.nh, a.nc, 16, 64
G = a.g or NC
H, K = 4 * F, -(-NC // G)
torch.manual_seed(0)
n = lambda *s: torch.randn(*s, device=dev)
XQ = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XK = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XV = n(B, NH, NC, CS, F).bfloat16()
le = (0.1 * torch.sigmoid(n(B, NH, NC, CS, 1)) / F).bfloat16()
lw, lb = torch.ones(1, NH, 1, F, device=dev), torch.zeros(1, NH, 1, F, device=dev)
state = (0.02 * n(B, NH, F, H), torch.zeros(B, NH, 1, H, device=dev), 0.02 * n(B, NH, H, F), torch.zeros(B, NH, 1, F, device=dev))
f32 = lambda *s: torch.empty(*s, device=dev)
ARMS = ("one_workgroup", "pair")
buf = {arm: dict(out=torch.empty_like(XQ), cks=(f32(B, NH, K, F, H), f32(B, NH, K, 1, H), f32(B, NH, K, H, F), f32(B, NH, K, 1, F)))
       for arm in ARMS}
paired = []


def scan(arm):
    b = buf[arm]
    if arm == "pair":
        paired.append(e.ttt_forward_pair16(XQ, XK, XV, le, lw, lb, *state, *b["cks"], b["out"], G))
    else:
        e.ttt_forward(XQ, XK, XV, le, lw, lb, *state, *b["cks"], b["out"], G)


def timed(arm):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    scan(arm)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


# the ring depth the library was built with, from its workspace formula: 256 bytes of flag words + RING records per (b, h)
ring = (e.load_library().ttt_hip_mlp_forward_pair16_workspace(ctypes.byref(e._dims(1, 1, 1, CS, F, 1, torch.bfloat16))) - 256) // (64 * 1024 + 1024 + 256)
ms = {arm: [] for arm in ARMS}
for it in range(a.warmup + a.iters):
    for arm in (ARMS if it % 2 == 0 else ARMS[::-1]):          # alternate, and alternate who goes first
        t = timed(arm)
        if it >= a.warmup:
            ms[arm].append(t)
res = {"geometry": dict(B=B, NH=NH, NC=NC, CS=CS, F=F, G=G), "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
       "ring": ring, "pairs_ran": all(paired), "hand_over_error": e.sweep_error()}
for arm in ARMS:
    v = ms[arm]
    res[f"scan_{arm}_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "us_per_step": statistics.median(v) * 1e3 / NC}
res["pair_over_one_workgroup"] = res["scan_pair_ms"]["median"] / res["scan_one_workgroup_ms"]["median"]
res["pair_slowest_faster_than_one_workgroup_fastest"] = res["scan_pair_ms"]["max"] < res["scan_one_workgroup_ms"]["min"]
res["same_bits"] = bool(torch.equal(buf["pair"]["out"], buf["one_workgroup"]["out"]) and
                        all(torch.equal(x, y) for x, y in zip(buf["pair"]["cks"], buf["one_workgroup"]["cks"])))
line = json.dumps(res)
print(line)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(line + "\n")
