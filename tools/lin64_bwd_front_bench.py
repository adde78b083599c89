"""TTT-Linear backward at mini-batches of 64 on the opt-in MFMA kernels (``impl="mfma"``): the one call, the backward in parts
(``linear_hip.backward_in_parts``) and the backward in parts with the front / chain stage of include/ttt_hip_lin64_bwd_front.h
(``front=True``: the carry-free half of every reverse step beside the recompute on the side stream, one wave per 16-row token block; the
shorter four-wave chain on the caller's stream), at 2 and 4 checkpoint groups per part, alternated from iteration to iteration inside
one process, one event pair per backward; and the four part kernels alone on one stream over ALL groups - recompute, front, the
existing walk (sweep) and the chain (not alternated: each runs behind the kernels whose output it reads).

    python tools/lin64_bwd_front_bench.py [--nc 804] [--nh 48] [--batch 1] [--g 16] [--iters 15] [--warmup 3]
                                          [--parent-lib libttt_hip.so of the parent commit] [--json FILE]

Before anything is timed, every arm's eight gradients are compared with the one call's, element by element: 0 may differ.  With
``--parent-lib`` the one-call backward of another build of the library (the parent commit's) is called through its C ABI and must give
this build's one-call bits as well (the one-call kernel is the same machine code)."""
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
ap.add_argument("--nh", type=int, default=48)
ap.add_argument("--nc", type=int, default=804)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--g", type=int, default=16, help="checkpoint group size (ModelConfig.scan_checkpoint_group_size)")
ap.add_argument("--parts", type=int, nargs="*", default=[2, 4], help="checkpoint groups per part")
ap.add_argument("--iters", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--json", default=None)
a = ap.parse_args()
assert a.iters >= 15 and a.warmup >= 3, "at least 3 warm-up and 15 timed iterations"
dev = "cuda:0"
B, NH, NC, CS, F, G = a.batch, a.nh, a.nc, 64, 64, a.g
impl = "mfma"
K = -(-NC // G)
GRADS = ("dln_w", "dln_b", "dW1", "db1", "deta", "dXQ", "dXK", "dXV")
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
        variants[f"parts_front_{gpp}"] = (lambda gpp: lambda g: backward_in_parts(e, impl, gpp, tensors(g), G, front=True))(gpp)
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
# the four part kernels alone, on one stream, over all K groups: recompute -> front -> walk (sweep) -> chain
slots_all = torch.empty(e.linear_backward_parts_slots(B, NH, NC, CS, F, G, K, impl=impl), dtype=torch.uint8, device=dev)
records_all = torch.empty(e.linear_backward_front64_records(B, NH, NC, CS, F, G, K, impl=impl), dtype=torch.uint8, device=dev)
carry = torch.empty(e.linear_backward_parts_carry(B, NH, NC, CS, F, G, impl=impl) // 4, device=dev)
ALONE = ("recompute_all_groups", "front_all_groups", "sweep_all_groups", "chain_all_groups")
variants["recompute_all_groups"] = lambda g: e.ttt_linear_recompute_groups(impl, None, XK, XV, le, lw, lb, *cks, *(None,) * 13, G, 0, K, slots_all)
variants["front_all_groups"] = lambda g: e.ttt_linear_front64_groups(impl, XQ, XK, XV, None, lw, lb, None, None, None, None, dOut, *(None,) * 7,
                                                                   g[5], None, None, G, 0, K, slots_all, records_all)
# (dW1 / db1 carried in place; zeroed outside the timed window)
variants["sweep_all_groups"] = lambda g: e.ttt_linear_sweep_groups(impl, XQ, XK, XV, le, lw, lb, None, None, g[2], g[3], dOut, None, None, *g,
                                                                   G, 0, K, slots_all, carry)
variants["chain_all_groups"] = lambda g: e.ttt_linear_chain64_groups(impl, XQ, XK, None, le, lw, lb, None, None, g[2], g[3], None, None, None,
                                                                   g[0], g[1], g[2], g[3], g[4], None, g[6], g[7], G, 0, K, slots_all,
                                                                   records_all, carry)


def timed(fn, g):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn(g)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


names = list(variants)
alternated = [v for v in names if v not in ALONE]
out = {v: grads() for v in names}
out["chain_all_groups"] = out["front_all_groups"]          # the front writes dXQ, the chain the other seven


def run_all(it, ms=None):
    order = alternated if it % 2 == 0 else alternated[::-1]           # alternate, and alternate who goes first
    for v in list(order) + list(ALONE):
        if v in ("sweep_all_groups", "chain_all_groups"):
            out[v][2].zero_(); out[v][3].zero_()
        t = timed(variants[v], out[v])
        if ms is not None:
            ms[v].append(t)


# ---- the bits first: 0 differing elements of all eight gradients between every arm and the one call
run_all(0)
differing = {v: {k: int((x != y).sum()) for k, x, y in zip(GRADS, out[v], out["one_call"])}
             for v in names if v not in ("one_call", "recompute_all_groups", "front_all_groups")}
print(json.dumps({"differing_elements_vs_one_call": differing}))
assert all(c == 0 for d in differing.values() for c in d.values()), differing
ms = {v: [] for v in names}
for it in range(1, a.warmup + a.iters):
    run_all(it, ms if it >= a.warmup else None)
res = {"geometry": dict(B=B, NH=NH, NC=NC, CS=CS, F=F, G=G, K=K), "iters": a.iters, "warmup": a.warmup,
       "device": torch.cuda.get_device_name(0), "slots_bytes_all_groups": slots_all.numel(), "records_bytes_all_groups": records_all.numel(),
       "records_bytes_per_workspace": {str(gpp): e.linear_backward_front64_records(B, NH, NC, CS, F, G, gpp, impl=impl) for gpp in a.parts}}
for v in names:
    res[f"{v}_ms"] = {"median": statistics.median(ms[v]), "min": min(ms[v]), "max": max(ms[v]), "n": len(ms[v]),
                      "us_per_step": statistics.median(ms[v]) * 1e3 / NC}
for v in names:
    if v != "one_call":
        res[f"{v}_over_one_call"] = res[f"{v}_ms"]["median"] / res["one_call_ms"]["median"]
for gpp in a.parts:
    if f"parts_front_{gpp}_ms" in res:
        res[f"parts_front_{gpp}_over_parts_{gpp}"] = res[f"parts_front_{gpp}_ms"]["median"] / res[f"parts_{gpp}_ms"]["median"]
res["chain_over_sweep_all_groups"] = res["chain_all_groups_ms"]["median"] / res["sweep_all_groups_ms"]["median"]
res["differing_elements_vs_one_call"] = differing
line = json.dumps(res)
print(line)
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        f.write(line + "\n")
