"""TTT-MLP backward at mini-batches of 16: the one-call MFMA backward (``ttt_backward_impl("mfma", ...)``) against the backward in parts
(``mlp_tk.backward_in_parts``: the recompute of the next range of checkpoint groups on a side stream beside the reverse walk of the
current one) at 1, 2, 4, 8 and 16 groups per part, alternated from iteration to iteration inside one process, one event pair per
backward; and the two new kernels alone on one stream, per range size - over a window of the LAST ``max(parts)`` groups of the sequence
(all groups at once would need 20 GB of slots at NC = 3216) every range of the window is recomputed, launch behind launch, into its
own region of one workspace, then every range is walked, the last first (not alternated: the walks always run right behind those
recomputes).  One group per range is the one call's own grid (B * NH workgroups per launch, one launch behind the other), so that
recompute time against the one call's time is the share of its chain the recompute was.

    python tools/mlp16_bwd_parts_bench.py [--nc 1128] [--nh 48] [--batch 1] [--g 16] [--parts 1 2 4 8 16] [--iters 7] [--warmup 2]
                                          [--parent-lib libttt_hip.so of the parent commit] [--dump PREFIX] [--json FILE]

The gradients of every cutting are compared with the one call's: they must be equal.  ``--parent-lib``: the one-call backward of another
build of the library (the commit before the two halves became kernels of their own) joins the alternation, called through its C ABI on
the same inputs; its ten results are counted element by element against this build's.  ``--dump PREFIX``: the one call's ten results go
to PREFIX_this.pt (and the parent build's to PREFIX_parent.pt)."""
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
from ttt_amd.models.ssm.mlp_tk import backward_in_parts, part_ranges  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--nh", type=int, default=48)
ap.add_argument("--nc", type=int, default=1128)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--g", type=int, default=16, help="checkpoint group size (ModelConfig.scan_checkpoint_group_size)")
ap.add_argument("--parts", type=int, nargs="*", default=[1, 2, 4, 8, 16], help="checkpoint groups per part")
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--dump", default=None)
ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = "cuda:0"
B, NH, NC, CS, F, H, G = a.batch, a.nh, a.nc, 16, 64, 256, a.g
K = -(-NC // G)
BF = torch.bfloat16
NAMES = ("dln_w", "dln_b", "dW1", "db1", "dW2", "db2", "deta", "dXQ", "dXK", "dXV")
assert e.resolved_impl(B, NH, NC, CS, F, G, BF, mlp=True, backward=True, impl="mfma") == "mfma"
torch.manual_seed(0)
n = lambda *s: torch.randn(*s, device=dev)
XQ = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XK = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XV, dOut = n(B, NH, NC, CS, F).bfloat16(), n(B, NH, NC, CS, F).bfloat16()
le = (1.0 * torch.sigmoid(n(B, NH, NC, CS, 1)) / (F * CS)).bfloat16()
lw, lb = torch.ones(1, NH, 1, F, device=dev), torch.zeros(1, NH, 1, F, device=dev)
state = (0.02 * n(B, NH, F, H), torch.zeros(B, NH, 1, H, device=dev), 0.02 * n(B, NH, H, F), torch.zeros(B, NH, 1, F, device=dev))
f32 = lambda *s: torch.empty(*s, device=dev)
STATE = ((F, H), (1, H), (H, F), (1, F))
cks = tuple(f32(B, NH, K, *s) for s in STATE)
assert e.resolved_impl(B, NH, NC, CS, F, G, BF, mlp=True, backward=False) == "mfma"
e.ttt_forward(XQ, XK, XV, le, lw, lb, *state, *cks, torch.empty_like(XQ), G)
scr = tuple(f32(B, NH, G, *s) for s in STATE)
up = tuple(torch.zeros(B, NH, *s, device=dev) for s in STATE)


def grads():
    return (f32(B, NH, 1, F), f32(B, NH, 1, F), *(f32(B, NH, *s) for s in STATE),
            torch.empty(B, NH, NC, CS, 1, device=dev, dtype=BF), torch.empty_like(XQ), torch.empty_like(XQ), torch.empty_like(XQ))


def tensors(g, scratch=True):
    return (XQ, XK, XV, le, lw, lb, *cks, dOut, *(scr if scratch else (None,) * 4), *(None,) * 12, *up, dOut, *g)


variants = {"one_call": lambda g: e.ttt_backward_impl("mfma", *tensors(g), G)}
for gpp in a.parts:
    variants[f"parts_{gpp}"] = (lambda gpp: lambda g: backward_in_parts(e, gpp, tensors(g, False), G))(gpp)
if a.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    parent.ttt_hip_mlp_backward.restype, parent.ttt_hip_mlp_backward.argtypes = e._PROTOTYPES["ttt_hip_mlp_backward"]
    parent.ttt_hip_mlp_backward_workspace.restype, parent.ttt_hip_mlp_backward_workspace.argtypes = e._PROTOTYPES["ttt_hip_mlp_backward_workspace"]
    parent.ttt_hip_last_error.restype = ctypes.c_char_p
    dims = e._dims(B, NH, NC, CS, F, G, BF, "mfma")
    pws_bytes = parent.ttt_hip_mlp_backward_workspace(ctypes.byref(dims))
    pws = torch.empty(max(pws_bytes, 16), dtype=torch.uint8, device=dev)

    def one_call_parent(g):
        args = e._MlpBwd(*[None if t is None else t.data_ptr() for t in tensors(g)])
        rc = parent.ttt_hip_mlp_backward(ctypes.byref(dims), ctypes.byref(args), pws.data_ptr() if pws_bytes else None, pws_bytes,
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, parent.ttt_hip_last_error()

    variants["one_call_parent"] = one_call_parent

# the two new kernels alone, on one stream, per range size, over the last `window` groups of the sequence
window = min(max(a.parts), K)
alone = sorted({min(gpp, window) for gpp in a.parts})
slots_win = torch.empty(e.mlp_backward_parts_slots(B, NH, NC, CS, F, G, window, impl="mfma"), dtype=torch.uint8, device=dev)
carry = torch.empty(e.mlp_backward_parts_carry(B, NH, NC, CS, F, G, impl="mfma") // 4, device=dev)
rec_args = (None, XK, XV, le, lw, lb, *cks) + (None,) * 32
window_steps = NC - (K - window) * G


def window_ranges(nk):
    """[(k0, nk, region of slots_win)] of the window cut into ranges of nk groups, the last range first"""
    out, ofs = [], 0
    for k0, n in part_ranges(window, nk):
        nbytes = e.mlp_backward_parts_slots(B, NH, NC, CS, F, G, n, impl="mfma")
        out.append((K - window + k0, n, slots_win[ofs:ofs + nbytes]))
        ofs += nbytes
    return out


def recompute_alone(nk):
    rngs = window_ranges(nk)

    def run(g):
        for k0, n, ws in rngs:
            e.ttt_recompute_groups(*rec_args, G, k0, n, ws, impl="mfma")
    return run


def sweep_alone(nk):       # (dW1 .. db2 carried in place from zeros, set outside the timed window)
    rngs = window_ranges(nk)

    def run(g):
        for k0, n, ws in rngs:
            e.ttt_sweep_groups(XQ, XK, XV, le, lw, lb, *(None,) * 21, *g[2:6], dOut, *g, G, k0, n, ws, carry, impl="mfma")
    return run


for nk in alone:
    variants[f"recompute_alone_{nk}"] = recompute_alone(nk)
    variants[f"sweep_alone_{nk}"] = sweep_alone(nk)


def timed(fn, g):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn(g)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


names = list(variants)
alternated = [v for v in names if "_alone_" not in v]
singles = [v for v in names if "_alone_" in v]                       # recompute_alone_n directly in front of sweep_alone_n
out = {v: (grads() if v in alternated else None) for v in names}
g_alone = grads()
ms = {v: [] for v in names}
for it in range(a.warmup + a.iters):
    order = alternated if it % 2 == 0 else alternated[::-1]           # alternate, and alternate who goes first
    for v in list(order) + singles:
        if v.startswith("sweep_alone_"):
            for t in g_alone[2:6]:
                t.zero_()
            torch.cuda.synchronize()
        t = timed(variants[v], out[v] if v in alternated else g_alone)
        if it >= a.warmup:
            ms[v].append(t)
res = {"geometry": dict(B=B, NH=NH, NC=NC, CS=CS, F=F, G=G, K=K), "iters": a.iters, "warmup": a.warmup,
       "device": torch.cuda.get_device_name(0), "slot_bytes": 132352}
for v in names:
    res[f"{v}_ms"] = {"median": statistics.median(ms[v]), "min": min(ms[v]), "max": max(ms[v])}
    if v in alternated:
        res[f"{v}_ms"]["us_per_step"] = statistics.median(ms[v]) * 1e3 / NC
for nk in alone:      # per step of the window (the sequence's last group may be ragged)
    for half in ("recompute", "sweep"):
        res[f"{half}_alone_{nk}_ms"].update(window_groups=window, steps=window_steps, launches=len(part_ranges(window, nk)),
                                            us_per_step=res[f"{half}_alone_{nk}_ms"]["median"] * 1e3 / window_steps)
# the one call's grid (one group at a time on B * NH workgroups, launch behind launch): the recompute's share of its chain
r1, s1 = (res[f"{h}_alone_{alone[0]}_ms"]["us_per_step"] for h in ("recompute", "sweep"))
c1 = res["one_call_ms"]["us_per_step"]
res["recompute_share_of_chain"] = {"range_groups": alone[0], "recompute_us_per_step": r1, "sweep_us_per_step": s1, "one_call_us_per_step": c1,
                                   "recompute_over_one_call": r1 / c1, "one_call_minus_sweep_over_one_call": (c1 - s1) / c1}
for v in alternated:
    if v != "one_call":
        res[f"{v}_over_one_call"] = res[f"{v}_ms"]["median"] / res["one_call_ms"]["median"]
cut = [v for v in alternated if v.startswith("parts_")]
best = min(cut, key=lambda v: res[f"{v}_ms"]["median"])
res["best_cutting"] = best
res["best_cutting_slowest_beats_one_call_fastest"] = res[f"{best}_ms"]["max"] < res["one_call_ms"]["min"]
res["equal_to_one_call"] = {v: all(torch.equal(x, y) for x, y in zip(out[v], out["one_call"])) for v in cut}
if a.parent_lib:      # another build's code: elements that differ from this build's one call, per gradient
    res["parent_differing_elements"] = {k: [int((x != y).sum()), x.numel()] for k, x, y in zip(NAMES, out["one_call_parent"], out["one_call"])}
if a.dump:
    os.makedirs(os.path.dirname(os.path.abspath(a.dump)), exist_ok=True)
    torch.save({k: x.cpu() for k, x in zip(NAMES, out["one_call"])}, a.dump + "_this.pt")
    if a.parent_lib:
        torch.save({k: x.cpu() for k, x in zip(NAMES, out["one_call_parent"])}, a.dump + "_parent.pt")
line = json.dumps(res)
print(line)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(line + "\n")
assert all(res["equal_to_one_call"].values()), res["equal_to_one_call"]
