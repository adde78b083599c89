"""TTT-Linear backward: the one call against the backward in parts (``linear_hip.backward_in_parts``: the recompute of the next range of
checkpoint groups on a side stream beside the reverse walk of the current one) at 2, 4, 8 and 16 groups per part, alternated from
iteration to iteration inside one process, one event pair per backward; and the two new kernels alone on one stream - the recompute
of ALL groups at once and the reverse walk over all groups (not alternated: the walk always runs right behind that recompute).

    python tools/lin_bwd_parts_bench.py [--cs 16] [--nc 1128] [--nh 48] [--batch 1] [--g 16] [--iters 7] [--warmup 2]
                                        [--parent-lib libttt_hip.so of the parent commit] [--json FILE]

CS = 64 runs the opt-in MFMA kernels (impl "mfma").  ``--parent-lib``: the one-call backward of another build of the library (the
commit before the per-step code was factored out of the one-call kernels) joins the alternation, called through its C ABI.
The gradients of every variant of this build are compared with the one call's: they must be equal.  The parent build's are
counted element by element (another compilation of the same arithmetic: its fused multiply-adds need not fall the same way)."""
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
from ttt_amd.models.ssm.linear_hip import backward_in_parts  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cs", type=int, default=16, choices=(16, 64))
ap.add_argument("--nh", type=int, default=48)
ap.add_argument("--nc", type=int, default=1128)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--g", type=int, default=16, help="checkpoint group size (ModelConfig.scan_checkpoint_group_size)")
ap.add_argument("--parts", type=int, nargs="*", default=[2, 4, 8, 16], help="checkpoint groups per part")
ap.add_argument("--iters", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--json", default=None)
a = ap.parse_args()
dev = "cuda:0"
B, NH, NC, CS, F, G = a.batch, a.nh, a.nc, a.cs, 64, a.g
impl = "mfma" if CS == 64 else None
K = -(-NC // G)
assert e.resolved_impl(B, NH, NC, CS, F, G, torch.bfloat16, mlp=False, backward=True, impl=impl) == "mfma"
torch.manual_seed(0)
n = lambda *s: torch.randn(*s, device=dev)
XQ = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XK = torch.nn.functional.normalize(n(B, NH, NC, CS, F), dim=-1).bfloat16()
XV, dOut = n(B, NH, NC, CS, F).bfloat16(), n(B, NH, NC, CS, F).bfloat16()
le = (1.0 * torch.sigmoid(n(B, NH, NC, CS, 1)) / (F * CS)).bfloat16()
lw, lb = torch.ones(NH, F, device=dev), torch.zeros(NH, F, device=dev)
W1, b1 = 0.02 * n(B, NH, F, F), torch.zeros(B, NH, 1, F, device=dev)
f32 = lambda *s: torch.empty(*s, device=dev)
cks = (f32(B, NH, K, F, F), f32(B, NH, K, 1, F))
e.ttt_linear_forward_impl(impl, XQ, XK, XV, le, lw, lb, W1, b1, *cks, torch.empty_like(XQ), G)
scr = (f32(B, NH, G, F, F), f32(B, NH, G, 1, F))
up = (torch.zeros(B, NH, F, F, device=dev), torch.zeros(B, NH, 1, F, device=dev))


def grads():
    return (f32(B, NH, 1, F), f32(B, NH, 1, F), f32(B, NH, F, F), f32(B, NH, 1, F),
            torch.empty(B, NH, NC, CS, 1, device=dev, dtype=torch.bfloat16), torch.empty_like(XQ), torch.empty_like(XQ), torch.empty_like(XQ))


def tensors(g):
    return (XQ, XK, XV, le, lw, lb, *cks, *up, dOut, *scr, *g)


variants = {"one_call": lambda g: e.ttt_linear_backward_impl(impl, *tensors(g), G)}
for gpp in a.parts:
    if K > gpp:
        variants[f"parts_{gpp}"] = (lambda gpp: lambda g: backward_in_parts(e, impl, gpp, tensors(g), G))(gpp)
if a.parent_lib:
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    parent.ttt_hip_linear_backward.restype, parent.ttt_hip_linear_backward.argtypes = e._PROTOTYPES["ttt_hip_linear_backward"]
    parent.ttt_hip_last_error.restype = ctypes.c_char_p
    dims = e._dims(B, NH, NC, CS, F, G, torch.bfloat16, impl)

    def one_call_parent(g):
        args = e._LinBwd(*[t.data_ptr() for t in tensors(g)])
        rc = parent.ttt_hip_linear_backward(ctypes.byref(dims), ctypes.byref(args), None, 0, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, parent.ttt_hip_last_error()

    variants["one_call_parent"] = one_call_parent
# the two new kernels alone, on one stream: all K groups recomputed at once, then one reverse walk over all of them
slots_all = torch.empty(e.linear_backward_parts_slots(B, NH, NC, CS, F, G, K, impl=impl), dtype=torch.uint8, device=dev)
carry = torch.empty(e.linear_backward_parts_carry(B, NH, NC, CS, F, G, impl=impl) // 4, device=dev)
rec_args = (None, XK, XV, le, lw, lb, *cks) + (None,) * 13


def recompute_all(g):
    e.ttt_linear_recompute_groups(impl, *rec_args, G, 0, K, slots_all)


def sweep_all(g):       # (dW1 / db1 carried in place; zeroed outside the timed window)
    e.ttt_linear_sweep_groups(impl, XQ, XK, XV, le, lw, lb, None, None, g[2], g[3], dOut, None, None, *g, G, 0, K, slots_all, carry)


variants["recompute_all_groups"] = recompute_all
variants["sweep_all_groups"] = sweep_all           # (runs behind recompute_all_groups in every iteration)


def timed(fn, g):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn(g)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


names = list(variants)
alternated = [v for v in names if not v.endswith("_all_groups")]
out = {v: grads() for v in names}
ms = {v: [] for v in names}
for it in range(a.warmup + a.iters):
    order = alternated if it % 2 == 0 else alternated[::-1]           # alternate, and alternate who goes first
    for v in list(order) + ["recompute_all_groups", "sweep_all_groups"]:
        if v == "sweep_all_groups":
            out[v][2].zero_(); out[v][3].zero_()
        t = timed(variants[v], out[v])
        if it >= a.warmup:
            ms[v].append(t)
res = {"geometry": dict(B=B, NH=NH, NC=NC, CS=CS, F=F, G=G, K=K), "iters": a.iters, "warmup": a.warmup,
       "device": torch.cuda.get_device_name(0), "slots_bytes_all_groups": slots_all.numel()}
for v in names:
    res[f"{v}_ms"] = {"median": statistics.median(ms[v]), "min": min(ms[v]), "max": max(ms[v]),
                      "us_per_step": statistics.median(ms[v]) * 1e3 / NC}
for v in names:
    if v != "one_call":
        res[f"{v}_over_one_call"] = res[f"{v}_ms"]["median"] / res["one_call_ms"]["median"]
res["equal_to_one_call"] = {v: all(torch.equal(x, y) for x, y in zip(out[v], out["one_call"]))
                            for v in names if v not in ("one_call", "recompute_all_groups", "one_call_parent")}
if a.parent_lib:      # another build's code: elements that differ from this build's one call, per gradient
    res["parent_differing_elements"] = {k: [int((x != y).sum()), x.numel()] for k, x, y in
                                        zip(("dln_w", "dln_b", "dW1", "db1", "deta", "dXQ", "dXK", "dXV"), out["one_call_parent"], out["one_call"])}
line = json.dumps(res)
print(line)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(line + "\n")
assert all(res["equal_to_one_call"].values()), res["equal_to_one_call"]
