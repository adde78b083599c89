"""Runners and layouts for the TTT-MLP backward at mini-batches of 16 IN PARTS (recompute_groups / sweep_groups of
csrc/ttt_mlp16_bwd_body.h), shared by tests/test_emul_mlp16_bwd_parts_cpu.py (the bodies on the wave emulator) and
tests/test_mlp16_bwd_parts_gpu.py (the device kernels).  Inputs, seeds and the one-call runners are those of tests/mlp16_bwd_cases.py.

A walk takes the host tensors ``t``, the checkpoints ``cks``, the upstream state gradient ``up``, G and a cutting ``cuts`` of the K
checkpoint groups (group counts, first range first) and returns (g, spaces, carry): the ten gradients, the slot workspace of every
range (in walk order, the LAST range first) and ln_carry.  Every output starts as NaN except dW1 .. db2, which start as the upstream
(carried in place); every workspace and the carry start as NaN between NaN guards."""
import ctypes
import os
import subprocess

import torch

import mlp16_bwd_cases as M
import scan_cases as C

SLOT_FLOATS = 64 * 256 + 256 + 256 * 64 + 64          # W1, b1, W2, b2 of one slot
SLOT_BYTES = 4 * SLOT_FLOATS                            # 132 352
CARRY_FLOATS = 2 * 16 * 64                              # per (b, h)
GUARD = 64
_OFS = (0, 64 * 256, 64 * 256 + 256, 64 * 256 + 256 + 256 * 64, SLOT_FLOATS)


class PartParams(ctypes.Structure):            # wv::Mlp16BwdPartParams (csrc/ttt_wave_types.h)
    _fields_ = [("p", M.BwdParams), ("k0", ctypes.c_int), ("nk", ctypes.c_int), ("slots", ctypes.c_void_p), ("ln_carry", ctypes.c_void_p)]


def cuttings(K):
    """every cutting of K groups into ranges (the compositions of K), as tuples of group counts"""
    if K == 0:
        return [()]
    return [(n,) + rest for n in range(1, K + 1) for rest in cuttings(K - n)]


def ranges(K, cuts):
    """(k0, nk) of the cutting, the LAST range first"""
    assert sum(cuts) == K and all(n > 0 for n in cuts)
    out, k1 = [], K
    for nk in reversed(cuts):
        out.append((k1 - nk, nk))
        k1 -= nk
    return out


def guarded(n_floats, device="cpu"):
    buf = torch.full((n_floats + 2 * GUARD,), float("nan"), device=device)
    return buf, buf[GUARD:GUARD + n_floats]


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def slot_fields(view, B, NH, nk, G):
    """the slot workspace [B*NH][nk][G] of one range as its four state arrays [B, NH, nk, G, ...]"""
    s = view[:B * NH * nk * G * SLOT_FLOATS].view(B, NH, nk, G, SLOT_FLOATS)
    return tuple(s[..., _OFS[i]:_OFS[i + 1]].reshape(B, NH, nk, G, a, b) for i, (a, b) in enumerate(M.STATE_SHAPES))


def group_steps(NC, G, k):
    return min(G, NC - k * G)


def check_slots(tag, spaces, rngs, cks1, B, NH, NC, G):
    """slot j of group k holds the bits of checkpoint k G + j of a forward with G = 1; what a ragged last group leaves unused is NaN"""
    for view, (k0, nk) in zip(spaces, rngs):
        for name, f, c1 in zip(("W1", "b1", "W2", "b2"), slot_fields(view.cpu(), B, NH, nk, G), cks1):
            for k in range(k0, k0 + nk):
                n = group_steps(NC, G, k)
                assert torch.equal(f[:, :, k - k0, :n], c1[:, :, k * G:k * G + n]), (tag, name, k)
                assert torch.isnan(f[:, :, k - k0, n:]).all(), (tag, name, k, "a slot past the group's last step was written")


# ------------------------------------------------------------------------------------------------ the wave emulator
def build_emul():
    build = os.path.join(M.HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libmlp16_bwd_parts_emul.so")
    srcs = [os.path.join(M.HERE, "emul", f) for f in ("mlp16_bwd_parts_emul.cpp", "wave_emul.h")] + \
           [os.path.join(M.CSRC, f) for f in ("ttt_mlp16_bwd_body.h", "ttt_mlp16_body.h", "ttt_lin16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([C.CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", M.CSRC, "-I", os.path.join(M.HERE, "emul"), srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.emul_mlp16_bwd_part_params_size() == ctypes.sizeof(PartParams)
    assert lib.emul_mlp16_part_slot_bytes() == SLOT_BYTES
    assert lib.emul_mlp16_part_carry_floats() == CARRY_FLOATS
    return lib


def emul_walk(lib):
    def walk(t, cks, up, G, cuts):
        B, NH, NC = t["XQ"].shape[:3]
        K = cks[0].shape[2]
        rngs = ranges(K, cuts)
        g = M.outputs(B, NH, NC)
        for n, u in zip(("dW1", "db1", "dW2", "db2"), up):
            g[n].copy_(u)
        ins = dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1c=cks[0], b1c=cks[1], W2c=cks[2],
                   b2c=cks[3], dOut=t["dOut"])
        keep = {k: v.clone() for k, v in ins.items()}
        spaces = [guarded(B * NH * nk * G * SLOT_FLOATS) for _, nk in rngs]
        carry_all, carry = guarded(B * NH * CARRY_FLOATS)
        for (k0, nk), (_, ws) in zip(rngs, spaces):
            q = PartParams()
            for n, v in dict(ins, dW1_last=g["dW1"], db1_last=g["db1"], dW2_last=g["dW2"], db2_last=g["db2"], dln_w=g["dln_w"],
                             dln_b=g["dln_b"], dW1=g["dW1"], db1=g["db1"], dW2=g["dW2"], db2=g["db2"], deta=g["dlast_eta"], dXQ=g["dXQ"],
                             dXK=g["dXK"], dXV=g["dXV"]).items():
                assert v.is_contiguous()
                setattr(q.p, n, v.data_ptr())
            q.p.NH, q.p.NC, q.p.G, q.p.K, q.p.eps = NH, NC, G, K, 1e-8
            q.k0, q.nk, q.slots, q.ln_carry = k0, nk, ws.data_ptr(), carry.data_ptr()
            msg = ctypes.create_string_buffer(256)
            races = lib.emul_mlp16_recompute_groups(ctypes.byref(q), B * NH * nk, msg, 256)
            assert races == 0, f"LDS race in the recompute of groups [{k0}, {k0 + nk}): {msg.value.decode()}"
            races = lib.emul_mlp16_sweep_groups(ctypes.byref(q), B * NH, msg, 256)
            assert races == 0, f"LDS race in the sweep of groups [{k0}, {k0 + nk}): {msg.value.decode()}"
        for buf, _ in spaces + [(carry_all, carry)]:
            assert guards_intact(buf), f"{cuts}: write outside a workspace"
        for k, v in ins.items():
            assert torch.equal(v, keep[k]), f"input {k} was written"
        return g, [v for _, v in spaces], carry
    return walk


# ------------------------------------------------------------------------------------------------ the device
def device_walk(e, two_streams, device="cuda"):
    """the walk over ``ttt_recompute_groups`` / ``ttt_sweep_groups``: on one stream with a workspace per range, or with the schedule
    of ``mlp_tk.backward_in_parts`` - the recompute of the next range on the pipeline's side stream into one of two workspaces, events
    both ways"""
    def walk(t, cks, up, G, cuts):
        B, NH, NC = t["XQ"].shape[:3]
        K = cks[0].shape[2]
        rngs = ranges(K, cuts)
        assert e.get_impl() == "auto"
        assert e.resolved_impl(B, NH, NC, M.CS, M.F, G, torch.bfloat16, mlp=True, backward=True, impl="mfma") == "mfma"
        ins = {k: t[k].to(device) for k in ("XQ", "XK", "XV", "eta", "dOut", "ln_w", "ln_b")}
        ins.update({f"ck{i}": c.to(device) for i, c in enumerate(cks)})
        keep = {k: v.clone() for k, v in ins.items()}
        g = M.outputs(B, NH, NC, device=device)
        for n, u in zip(("dW1", "db1", "dW2", "db2"), up):
            g[n].copy_(u)
        lw, lb = ins["ln_w"].reshape(1, NH, 1, M.F), ins["ln_b"].reshape(1, NH, 1, M.F)
        ck = [ins[f"ck{i}"] for i in range(4)]
        st = [g[n] for n in ("dW1", "db1", "dW2", "db2")]
        rec = (None, ins["XK"], ins["XV"], ins["eta"], lw, lb, *ck) + (None,) * 32
        swp = (ins["XQ"], ins["XK"], ins["XV"], ins["eta"], lw, lb) + (None,) * 21 + \
              (*st, ins["dOut"], g["dln_w"], g["dln_b"], *st, g["dlast_eta"], g["dXQ"], g["dXK"], g["dXV"])
        nbytes = lambda nk: e.mlp_backward_parts_slots(B, NH, NC, M.CS, M.F, G, nk, impl="mfma")
        assert nbytes(1) == B * NH * G * SLOT_BYTES
        if two_streams:
            spaces = [guarded(nbytes(max(nk for _, nk in rngs)) // 4, device) for _ in range(2)]
        else:
            spaces = [guarded(nbytes(nk) // 4, device) for _, nk in rngs]
        carry_all, carry = guarded(e.mlp_backward_parts_carry(B, NH, NC, M.CS, M.F, G, impl="mfma") // 4, device)
        assert carry.numel() == B * NH * CARRY_FLOATS
        slots = lambda n: spaces[n % len(spaces)][1]
        torch.cuda.synchronize()
        if not two_streams:
            for n, (k0, nk) in enumerate(rngs):
                e.ttt_recompute_groups(*rec, G, k0, nk, slots(n), impl="mfma")
                e.ttt_sweep_groups(*swp, G, k0, nk, slots(n), carry, impl="mfma")
        else:
            from ttt_amd.models.ssm.pipeline import side_stream
            main, side = torch.cuda.current_stream(), side_stream(device)          # the stream the shipped schedule uses
            ready, swept = [torch.cuda.Event() for _ in rngs], [torch.cuda.Event() for _ in rngs]

            def recompute(n):
                with torch.cuda.stream(side):
                    if n >= 2:
                        side.wait_event(swept[n - 2])
                    e.ttt_recompute_groups(*rec, G, *rngs[n], slots(n), impl="mfma")
                    ready[n].record(side)

            side.wait_stream(main)
            recompute(0)
            for n, (k0, nk) in enumerate(rngs):
                if n + 1 < len(rngs):
                    recompute(n + 1)
                main.wait_event(ready[n])
                e.ttt_sweep_groups(*swp, G, k0, nk, slots(n), carry, impl="mfma")
                swept[n].record(main)
            main.wait_stream(side)
        torch.cuda.synchronize()
        for buf, _ in spaces + [(carry_all, carry)]:
            assert guards_intact(buf), f"{cuts}: write outside a workspace"
        for k, v in ins.items():
            assert torch.equal(v, keep[k]), f"input {k} was written"
        return {k: v.cpu() for k, v in g.items()}, [v.cpu() for _, v in spaces], carry.cpu()
    return walk
