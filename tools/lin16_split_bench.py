"""TTT-Linear forward scan at mini-batches of 16: the opt-in two-wave form (csrc/ttt_lin16_split_body.h: a chain wave and an output
wave per (b, h), hand-over through LDS) against the one-wave kernel, alternated from iteration to iteration inside one process on the
same inputs, one HIP event pair per call.

    timeout -k 10 600 python tools/lin16_split_bench.py [--nc 3216] [--batch 1 2] [--nh 48] [--g 16] [--iters 15] [--warmup 3]
                                                        [--chain-alone] [--json FILE]

The yardstick is the one-wave arm of the same process: the split "wins" when its slowest iteration beats that arm's fastest.
``--nc 3216`` = the 9 s video, ``--nc 21948`` = the 63 s video.  ``--chain-alone`` adds a third arm: the split kernel with the output
role's work removed (its barriers stay; ``out`` is not written) - what the chain role alone costs, i.e. the floor of the two-wave form.
One JSON line with an entry per batch size - median (fastest - slowest) ms per scan, microseconds per step, and the count of output /
checkpoint elements that differ from the one-wave arm -, also written to ``--json`` (default profiles/r21_lin16_split_nc<NC>.json).
Run it under ``timeout -k 10``."""
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
ap.add_argument("--nc", type=int, default=3216, help="mini-batches of 16: 3216 = the 9 s video, 21948 = the 63 s video")
ap.add_argument("--batch", type=int, nargs="+", default=[1, 2])
ap.add_argument("--g", type=int, default=16, help="checkpoint group size; 0 = NC (sampling: one group)")
ap.add_argument("--iters", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--chain-alone", action="store_true", help="a third arm: the split kernel without the output role's work")
ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = "cuda:0"
NH, NC, CS, F = a.nh, a.nc, 16, 64
G = a.g or NC
K = -(-NC // G)
ARMS = ("one_wave", "split") + (("chain_alone",) if a.chain_alone else ())


def bench(B):
    torch.manual_seed(0)
    n = lambda *s: torch.randn(*s, device=dev)
    XQ = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
    XK = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
    XV = n(B, NH, NC, CS, F).bfloat16()
    le = (0.1 * torch.sigmoid(n(B, NH, NC, CS, 1)) / F).bfloat16()
    lw, lb = torch.ones(NH, F, device=dev), torch.zeros(NH, F, device=dev)
    state = (0.02 * n(B, NH, F, F), torch.zeros(B, NH, 1, F, device=dev))
    buf = {arm: dict(out=torch.zeros_like(XQ), cks=(torch.zeros(B, NH, K, F, F, device=dev), torch.zeros(B, NH, K, 1, F, device=dev)))
           for arm in ARMS}

    def scan(arm):
        b = buf[arm]
        args = (XQ, XK, XV, le, lw, lb, *state, *b["cks"], b["out"], G)
        if arm == "one_wave":
            e.ttt_linear_forward_impl(None, *args)
        elif arm == "split":
            e.ttt_linear_forward_split16(None, *args)
        else:
            e.debug_option("lin_split16_chain_alone", 1)
            try:
                e.ttt_linear_forward_split16(None, *args)
            finally:
                e.debug_option("lin_split16_chain_alone", 0)

    def timed(arm):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        scan(arm)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    ms = {arm: [] for arm in ARMS}
    for it in range(a.warmup + a.iters):
        order = ARMS[it % len(ARMS):] + ARMS[:it % len(ARMS)]          # alternate, and rotate who goes first
        for arm in order:
            t = timed(arm)
            if it >= a.warmup:
                ms[arm].append(t)
    res = {"B": B}
    for arm in ARMS:
        v = ms[arm]
        res[f"scan_{arm}_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "us_per_step": statistics.median(v) * 1e3 / NC}
    one = buf["one_wave"]
    differ = lambda x, y: int((x != y).sum().item())
    res["split_differing_elements"] = {"out": differ(buf["split"]["out"], one["out"]),
                                       "checkpoints": sum(differ(x, y) for x, y in zip(buf["split"]["cks"], one["cks"]))}
    if a.chain_alone:      # (its `out` is never written)
        res["chain_alone_differing_elements"] = {"checkpoints": sum(differ(x, y) for x, y in zip(buf["chain_alone"]["cks"], one["cks"]))}
        res["chain_alone_over_one_wave"] = res["scan_chain_alone_ms"]["median"] / res["scan_one_wave_ms"]["median"]
    res["split_over_one_wave"] = res["scan_split_ms"]["median"] / res["scan_one_wave_ms"]["median"]
    res["split_slowest_faster_than_one_wave_fastest"] = res["scan_split_ms"]["max"] < res["scan_one_wave_ms"]["min"]
    return res


out = {"geometry": dict(NH=NH, NC=NC, CS=CS, F=F, G=G), "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
       "arms": list(ARMS), "batches": [bench(B) for B in a.batch]}
out["split_calls"] = dict(e.linear_split16_calls)
line = json.dumps(out)
print(line)
path = a.json or os.path.join(ROOT, "profiles", f"r21_lin16_split_nc{NC}.json")
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    f.write(line + "\n")
