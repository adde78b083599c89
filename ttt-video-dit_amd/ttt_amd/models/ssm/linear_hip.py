"""``HipLinear`` (alias ``TritonLinear``): autograd boundary around the TTT-Linear scan kernels.

Signature of the reference's ``TritonLinear.apply(ttt_norm_weight, ttt_norm_bias, W1, b1, XQ, XV,
XK, eta, checkpoint_group_size)`` (``ttt/models/ssm/linear_triton.py:14-26``; call site
``ttt_layer.py:371-381``).  The Triton kernels it replaces (``kernels/linear_forward.py``,
``linear_backward.py``) are re-implemented as HIP for gfx950 behind ``test_time_training``.
Activations may be bf16 or fp32 (the Triton path accepts both); state and checkpoints are fp32.
"""
from __future__ import annotations

import math
import os

import torch

_F32 = torch.float32


def _ext():
    import test_time_training
    return test_time_training


def _cs64_impl_default():
    v = os.environ.get("TTT_LINEAR_CS64_IMPL", "auto")
    if v not in ("auto", "mfma"):
        raise ValueError(f"TTT_LINEAR_CS64_IMPL: expected 'auto' or 'mfma', got {v!r}")
    return v


def _backward_parts_default():
    v = os.environ.get("TTT_LINEAR_BACKWARD_PARTS", "0")
    if not v.isdigit():
        raise ValueError(f"TTT_LINEAR_BACKWARD_PARTS: expected a non-negative integer (checkpoint groups per part, 0 = off), got {v!r}")
    return int(v)


def _backward_front_default():
    v = os.environ.get("TTT_LINEAR_BACKWARD_FRONT", "0")
    if v not in ("0", "1"):
        raise ValueError(f"TTT_LINEAR_BACKWARD_FRONT: expected '0' (off) or '1', got {v!r}")
    return int(v)


def _backward_front64_default():
    v = os.environ.get("TTT_LINEAR_BACKWARD_FRONT64", "0")
    if v not in ("0", "1"):
        raise ValueError(f"TTT_LINEAR_BACKWARD_FRONT64: expected '0' (off) or '1', got {v!r}")
    return int(v)


def _cs16_scan_split_default():
    v = os.environ.get("TTT_LINEAR_CS16_SCAN_SPLIT", "0")
    if v not in ("0", "1"):
        raise ValueError(f"TTT_LINEAR_CS16_SCAN_SPLIT: expected '0' (off) or '1', got {v!r}")
    return int(v)


def scan_split_applies(ext, impl, XQ, G):
    """``HipLinear.cs16_scan_split`` is on and this forward is what the two-wave scan serves: bf16, head dim 64, mini-batches of 16, on
    the MFMA scan, with an extension that has the entry.  Off (the default): nothing is asked of the extension."""
    v = HipLinear.cs16_scan_split
    if v not in (0, 1) or isinstance(v, bool):
        raise ValueError(f"HipLinear.cs16_scan_split: expected 0 or 1, got {v!r}")
    B, NH, NC, CS, F = XQ.shape
    if v == 0 or CS != 16 or F != 64 or XQ.dtype != torch.bfloat16 or not hasattr(ext, "ttt_linear_forward_chunk_split16"):
        return False
    return ext.resolved_impl(B, NH, NC, CS, F, int(G), XQ.dtype, mlp=False, backward=False, impl=impl) == "mfma"


def linear_forward_chunk_call(ext, impl, XQ, G):
    """the binding's TTT-Linear forward over a part of the sequence for this call: ``ttt_linear_forward_chunk`` unless the split switch
    applies (same arguments, same bits)"""
    return ext.ttt_linear_forward_chunk_split16 if scan_split_applies(ext, impl, XQ, G) else ext.ttt_linear_forward_chunk


def backward_in_parts(ext, impl, gpp, tensors, G, front=False):
    """``ttt_linear_backward`` as ranges of ``gpp`` checkpoint groups, walked from the last range to the first (the entries of
    include/ttt_hip_bwd_parts.h), on the schedule of ``pipeline.run_in_parts``: the recompute of the range to be swept next runs on the
    side stream into one of two slot workspaces while the caller's stream sweeps the current range.  ``tensors``: the 21 of
    ``ttt_linear_backward`` - the ``*_init_group`` scratch is not used; dW1 / db1 are carried IN PLACE in the output buffers, which
    start as copies of the upstream gradients of the final state (zeros in ``HipLinear.backward``).  The workspaces are allocated on
    the caller's stream and not handed to ``record_stream``: the side stream is joined into the caller's stream before this returns,
    so nothing allocated on that stream later can run before the side stream's last use of them (``record_stream`` would only defer
    the allocator's reuse of the blocks).
    ``front`` (mini-batches of 16, include/ttt_hip_lin_bwd_front.h): the side stream also runs, behind the recompute of a range, the
    half of its reverse steps that does not depend on the carried gradients (``ttt_linear_front_groups``, into one of two record
    workspaces), and the caller's stream walks the range with ``ttt_linear_chain_groups`` instead of the sweep.  At mini-batches of 64
    ``front`` takes the entries of include/ttt_hip_lin64_bwd_front.h (``ttt_linear_front64_groups``, ``ttt_linear_chain64_groups``,
    ``linear_backward_front64_records``) on the same schedule with the same arguments."""
    from ttt_amd.models.ssm.pipeline import part_ranges, run_in_parts
    (XQ, XK, XV, last_eta, ln_w, ln_b, W1c, b1c, uW1, ub1, dOut, _, _, d_lnw, d_lnb, dW1, db1, d_eta, dQ, dK, dV) = tensors
    B, NH, NC, CS, F = XQ.shape
    dev = XQ.device
    ranges = part_ranges(math.ceil(NC / G), gpp)
    sets = range(min(2, len(ranges)))
    space = lambda nbytes: [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in sets]
    slots = space(ext.linear_backward_parts_slots(B, NH, NC, CS, F, G, ranges[0][1], XQ.dtype, impl=impl))
    carry = torch.empty(ext.linear_backward_parts_carry(B, NH, NC, CS, F, G, XQ.dtype, impl=impl) // 4, dtype=_F32, device=dev)
    dW1.copy_(uW1); db1.copy_(ub1)
    rec_args = (None, XK, XV, last_eta, ln_w, ln_b, W1c, b1c) + (None,) * 13
    if front:
        if CS == 64:
            records_bytes, front_groups, chain_groups = ext.linear_backward_front64_records, ext.ttt_linear_front64_groups, ext.ttt_linear_chain64_groups
        else:
            records_bytes, front_groups, chain_groups = ext.linear_backward_front_records, ext.ttt_linear_front_groups, ext.ttt_linear_chain_groups
        records = space(records_bytes(B, NH, NC, CS, F, G, ranges[0][1], XQ.dtype, impl=impl))
        front_args = (XQ, XK, XV, None, ln_w, ln_b, None, None, None, None, dOut) + (None,) * 7 + (dQ, None, None)
        walk_args = (XQ, XK, None, last_eta, ln_w, ln_b, None, None, dW1, db1, None, None, None, d_lnw, d_lnb, dW1, db1, d_eta, None, dK, dV)
    else:
        walk_args = (XQ, XK, XV, last_eta, ln_w, ln_b, None, None, dW1, db1, dOut, None, None, d_lnw, d_lnb, dW1, db1, d_eta, dQ, dK, dV)

    def side_work(n, p):
        ext.ttt_linear_recompute_groups(impl, *rec_args, G, *ranges[n], slots[p])
        if front:
            front_groups(impl, *front_args, G, *ranges[n], slots[p], records[p])

    def main_work(n, p):
        if front:
            chain_groups(impl, *walk_args, G, *ranges[n], slots[p], records[p], carry)
        else:
            ext.ttt_linear_sweep_groups(impl, *walk_args, G, *ranges[n], slots[p], carry)

    run_in_parts(dev, ranges, side_work, main_work)


class HipLinear(torch.autograd.Function):
    sharded_mode = False
    # Kernels of the calls at mini-batches of 64 with bf16 activations and head_dim 64: "auto" = what the library's selector picks
    # (the generic fp32-arithmetic kernels), "mfma" = the opt-in MFMA scan and sweep (csrc/ttt_lin64_body.h).  Every other call
    # is untouched.  Default from the environment variable TTT_LINEAR_CS64_IMPL, read once at import.
    cs64_impl = _cs64_impl_default()
    # The backward in parts: 0 = one call (default), n > 0 = ranges of n checkpoint groups, the recompute of the next range on the
    # pipeline's side stream beside the reverse walk of the current one (``backward_in_parts``) - where the call runs the MFMA sweep,
    # has at least two ranges and the extension has the entries; every other call is the one call.  Same bits either way.  Default
    # from the environment variable TTT_LINEAR_BACKWARD_PARTS, read once at import.
    backward_parts = _backward_parts_default()
    # With the backward in parts selected, at mini-batches of 16: 1 = the carry-free half of every reverse step runs as a kernel of its
    # own beside the recompute (``ttt_linear_front_groups``) and the caller's stream walks the shorter chain (``ttt_linear_chain_groups``),
    # 0 (default) = the sweep.  Read only where ``backward_parts`` selects the in-parts path and the extension has the entries; every
    # other call is what it is without it.  Same bits either way.  Default from the environment variable TTT_LINEAR_BACKWARD_FRONT, read
    # once at import.
    backward_front = _backward_front_default()
    # The same at mini-batches of 64 (``ttt_linear_front64_groups`` / ``ttt_linear_chain64_groups``, csrc/ttt_lin64_body.h): 0 (default) or
    # 1.  Read only where ``backward_parts`` selects the in-parts path at mini-batches of 64 with ``cs64_impl == "mfma"`` and the
    # extension has the entries; ``backward_front`` keeps meaning mini-batches of 16 only.  Same bits either way.  The record
    # workspaces are large (two of B * NH * backward_parts * G * 77 824 bytes).  Default from the environment variable
    # TTT_LINEAR_BACKWARD_FRONT64, read once at import.
    backward_front64 = _backward_front64_default()
    # The forward scan at mini-batches of 16 with its output path on a second wave (csrc/ttt_lin16_split_body.h): 0 (default) = the
    # one-wave scan, 1 = the two-wave form - in one piece here and in the parts of pipeline.py (the chunk picker of
    # ``pipeline.LINEAR_SCAN``) - where the call is bf16, head dim 64, mini-batches of 16, resolves to the MFMA scan and the extension
    # has the entry (``scan_split_applies``); every other call is what it is without it.  Same bits either way, so the backward needs
    # nothing.  Default from the environment variable TTT_LINEAR_CS16_SCAN_SPLIT, read once at import.
    cs16_scan_split = _cs16_scan_split_default()

    @staticmethod
    def _impl(CS, F, act):
        if HipLinear.cs64_impl == "mfma" and CS == 64 and F == 64 and act == torch.bfloat16:
            return "mfma"
        if HipLinear.cs64_impl not in ("auto", "mfma"):
            raise ValueError(f"HipLinear.cs64_impl: expected 'auto' or 'mfma', got {HipLinear.cs64_impl!r}")
        return None

    @staticmethod
    def _in_parts(ext, impl, XQ, G):
        gpp = HipLinear.backward_parts
        if not isinstance(gpp, int) or gpp < 0:
            raise ValueError(f"HipLinear.backward_parts: expected a non-negative integer, got {gpp!r}")
        B, NH, NC, CS, F = XQ.shape
        if gpp == 0 or math.ceil(NC / G) <= gpp or not hasattr(ext, "ttt_linear_sweep_groups"):
            return False
        return ext.resolved_impl(B, NH, NC, CS, F, G, XQ.dtype, mlp=False, backward=True, impl=impl) == "mfma"

    @staticmethod
    def _with_front(ext, XQ, impl=None):
        v = HipLinear.backward_front
        if v not in (0, 1) or isinstance(v, bool):
            raise ValueError(f"HipLinear.backward_front: expected 0 or 1, got {v!r}")
        if XQ.shape[3] == 64 and impl == "mfma" and hasattr(ext, "ttt_linear_chain64_groups"):
            v64 = HipLinear.backward_front64
            if v64 not in (0, 1) or isinstance(v64, bool):
                raise ValueError(f"HipLinear.backward_front64: expected 0 or 1, got {v64!r}")
            return v64 == 1
        return v == 1 and XQ.shape[3] == 16 and hasattr(ext, "ttt_linear_chain_groups")

    @staticmethod
    def forward(ctx, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, XQ_batch, XV_batch, XK_batch, eta_batch,
                checkpoint_group_size):
        ext = _ext()
        B, NH, NC, CS, F = XQ_batch.shape
        G = int(checkpoint_group_size)
        K = math.ceil(NC / G)
        dev, act = XQ_batch.device, XQ_batch.dtype
        XQ, XV, XK = XQ_batch.contiguous(), XV_batch.contiguous(), XK_batch.contiguous()
        last_eta = eta_batch.to(act)[:, :, :, -1, :, None].contiguous()   # kernels/linear_forward.py:90-101
        ln_w = ttt_norm_weight.reshape(NH, F).to(_F32).contiguous()
        ln_b = ttt_norm_bias.reshape(NH, F).to(_F32).contiguous()
        # the backward runs the family the forward ran ; None: the plain call, which is all that the oracle-backed stand-in of
        # the CPU tests (oracle/cpu_ext.py) provides
        ctx.impl = HipLinear._impl(CS, F, act)
        from ttt_amd.models.ssm.pipeline import injected
        pre = injected("scan_lin")            # (a pipelined forward: the scan has walked the sequence part by part already, on the
        if pre is not None:                   # same kernel family: TTTBase._pipeline_plan asks with this call's selector)
            out, W1c, b1c = pre
        else:
            out = torch.empty(B, NH, NC, CS, F, device=dev, dtype=act)
            W1c = torch.empty(B, NH, K, F, F, device=dev, dtype=_F32)
            b1c = torch.empty(B, NH, K, 1, F, device=dev, dtype=_F32)
            W1, b1 = W1_init.to(_F32).contiguous(), b1_init.to(_F32).contiguous()
            if scan_split_applies(ext, ctx.impl, XQ, G):
                fwd = lambda *a: ext.ttt_linear_forward_split16(ctx.impl, *a)
            else:
                fwd = ext.ttt_linear_forward if ctx.impl is None else (lambda *a: ext.ttt_linear_forward_impl(ctx.impl, *a))
            fwd(XQ, XK, XV, last_eta, ln_w, ln_b, W1, b1, W1c, b1c, out, G)
        ctx.save_for_backward(XQ, XV, XK, last_eta, ln_w, ln_b, W1c, b1c)
        ctx.G = G
        ctx.eta_shape = tuple(eta_batch.shape)
        ctx.param_dtypes = (ttt_norm_weight.dtype, W1_init.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ext = _ext()
        XQ, XV, XK, last_eta, ln_w, ln_b, W1c, b1c = ctx.saved_tensors
        B, NH, NC, CS, F = XQ.shape
        G, dev, act = ctx.G, XQ.device, XQ.dtype
        e32 = lambda *s: torch.empty(*s, device=dev, dtype=_F32)
        up = (torch.zeros(B, NH, F, F, device=dev, dtype=_F32), torch.zeros(B, NH, 1, F, device=dev, dtype=_F32))
        grp = (e32(B, NH, G, F, F), e32(B, NH, G, 1, F))
        d_lnw, d_lnb = e32(B, NH, 1, F), e32(B, NH, 1, F)
        dW1, db1 = e32(B, NH, F, F), e32(B, NH, 1, F)
        d_eta = torch.empty(B, NH, NC, CS, 1, device=dev, dtype=act)
        dQ, dK, dV = (torch.empty_like(XQ) for _ in range(3))
        tensors = (XQ, XK, XV, last_eta, ln_w, ln_b, W1c, b1c, *up, grad_out.to(act).contiguous(), *grp,
                   d_lnw, d_lnb, dW1, db1, d_eta, dQ, dK, dV)
        if HipLinear._in_parts(ext, ctx.impl, XQ, G):
            backward_in_parts(ext, ctx.impl, int(HipLinear.backward_parts), tensors, G, front=HipLinear._with_front(ext, XQ, ctx.impl))
        else:
            bwd = ext.ttt_linear_backward if ctx.impl is None else (lambda *a: ext.ttt_linear_backward_impl(ctx.impl, *a))
            bwd(*tensors, G)
        ln_dt, st_dt = ctx.param_dtypes
        row = d_eta.transpose(-2, -1)
        rows = ctx.eta_shape[-2]
        d_eta_full = row if rows == 1 else torch.nn.functional.pad(row, (0, 0, rows - 1, 0))  # linear_backward.py:134-135
        return (d_lnw.sum(0).squeeze(1).to(ln_dt), d_lnb.sum(0).squeeze(1).to(ln_dt), dW1.to(st_dt), db1.to(st_dt),
                dQ, dV, dK, d_eta_full.to(act), None)


TritonLinear = HipLinear  # reference class name (ttt/models/ssm/linear_triton.py:12)
