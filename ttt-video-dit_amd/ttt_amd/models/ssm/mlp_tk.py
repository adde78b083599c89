"""``TkMLP``: autograd boundary around the TTT-MLP scan kernels.

Same signature and return contract as the reference's ``ttt/models/ssm/mlp_tk.py`` (``TkMLP.apply(
ttt_norm_weight, ttt_norm_bias, W1, b1, W2, b2, XQ, XV, XK, eta, checkpoint_group_size)`` ->
``[B,NH,NC,CS,F]``; 11 gradients, last None), and the same division of labour: Python allocates
every buffer, the extension ``test_time_training`` (here: HIP for gfx950) only computes.

Differences from the reference wrapper, on purpose:
  * the eta gradient is padded with CS-1 rows instead of a hard-coded 63 (mlp_tk.py:280 assumes
    CS=64 although every eval config uses 16 - SURVEY.md hazard C3);
  * ``eta`` may also be given directly as its last row ``[B,NH,NC,1,CS]`` so callers need not
    materialise the 64x redundant tile; the gradient then has that shape too.
"""
from __future__ import annotations

import functools
import math
import os

import torch

from ttt_amd.models.ssm.pipeline import part_ranges, run_in_parts  # noqa: F401  (part_ranges: tools and tests import it from here)

_BF16, _F32 = torch.bfloat16, torch.float32
CS16_BWD_IMPLS = ("auto", "mfma")


def _check_cs16_bwd_impl(value):
    if value not in CS16_BWD_IMPLS:
        raise ValueError(f"TkMLP.cs16_bwd_impl / TTT_MLP_CS16_BWD_IMPL: expected 'auto' or 'mfma', got {value!r}")
    return value


def _check_cs16_scan_pair(value):
    if isinstance(value, str) and value.strip() in ("0", "1"):
        value = int(value)
    if isinstance(value, bool) or value not in (0, 1):
        raise ValueError(f"TTTBase.cs16_scan_pair / TTT_MLP_CS16_SCAN_PAIR: expected 0 or 1, got {value!r}")
    return int(value)


def _cs16_backward_parts_default():
    v = os.environ.get("TTT_MLP_CS16_BACKWARD_PARTS", "0")
    if not v.isdigit():
        raise ValueError(f"TTT_MLP_CS16_BACKWARD_PARTS: expected a non-negative integer (checkpoint groups per part, 0 = off), got {v!r}")
    return int(v)


def _ext():
    import test_time_training  # the HIP extension (raises if its library is missing)
    return test_time_training


def backward_in_parts(ext, gpp, tensors, G):
    """``ttt_backward_impl("mfma", ...)`` at mini-batches of 16 as ranges of ``gpp`` checkpoint groups, walked from the last range to
    the first (the entries of include/ttt_hip_mlp_bwd_parts.h), on the schedule of ``pipeline.run_in_parts``: the recompute of the range
    to be swept next runs on the side stream into one of two slot workspaces while the caller's stream sweeps the current range.
    ``tensors``: the 42 of ``ttt_backward`` - the sixteen re-materialisation buffers are not used (None is fine); dW1 .. db2 are
    carried IN PLACE in the output buffers, which start as copies of the upstream gradients of the final state.  The side stream is
    joined into the caller's stream before this returns (so the workspaces, allocated on the caller's stream, are not reused before
    it is done)."""
    XQ, XK, XV, last_eta, ln_w, ln_b, W1c, b1c, W2c, b2c = tensors[:10]
    up, dOut, (d_lnw, d_lnb), d_state, (d_eta, dQ, dK, dV) = tensors[27:31], tensors[31], tensors[32:34], tensors[34:38], tensors[38:42]
    B, NH, NC, CS, F = XQ.shape
    dev = XQ.device
    ranges = part_ranges(math.ceil(NC / G), gpp)
    nbytes = ext.mlp_backward_parts_slots(B, NH, NC, CS, F, G, ranges[0][1], XQ.dtype, impl="mfma")
    slots = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(min(2, len(ranges)))]
    carry = torch.empty(ext.mlp_backward_parts_carry(B, NH, NC, CS, F, G, XQ.dtype, impl="mfma") // 4, dtype=_F32, device=dev)
    for d, u in zip(d_state, up):
        d.copy_(u)
    rec_args = (None, XK, XV, last_eta, ln_w, ln_b, W1c, b1c, W2c, b2c) + (None,) * 32
    sweep_args = (XQ, XK, XV, last_eta, ln_w, ln_b) + (None,) * 21 + (*d_state, dOut, d_lnw, d_lnb, *d_state, d_eta, dQ, dK, dV)
    run_in_parts(dev, ranges,
                 lambda n, p: ext.ttt_recompute_groups(*rec_args, G, *ranges[n], slots[p], impl="mfma"),
                 lambda n, p: ext.ttt_sweep_groups(*sweep_args, G, *ranges[n], slots[p], carry, impl="mfma"))


def _scan_pair_applies(ext, XQ, G):
    """``TTTBase.cs16_scan_pair`` is on and this forward is what the pair scan serves: bf16, head dim 64, mini-batches of 16, on the
    MFMA scan.  Off (the default): nothing is asked of the extension."""
    from ttt_amd.models.ssm.ttt_layer import TTTBase
    if not _check_cs16_scan_pair(TTTBase.cs16_scan_pair):
        return False
    B, NH, NC, CS, F = XQ.shape
    if CS != 16 or F != 64 or XQ.dtype != _BF16:
        return False
    return ext.resolved_impl(B, NH, NC, CS, F, int(G), _BF16, mlp=True, backward=False) == "mfma"


def mlp_forward_call(ext, XQ, G):
    """the binding's TTT-MLP forward for this call: ``ttt_forward`` unless the pair switch applies (same arguments, same bits)"""
    return ext.ttt_forward_pair16 if _scan_pair_applies(ext, XQ, G) else ext.ttt_forward


def mlp_forward_chunk_call(ext, XQ, G):
    """... and its forward over a part of the sequence: ``ttt_forward_chunk`` unless the pair switch applies"""
    return ext.ttt_forward_chunk_pair16 if _scan_pair_applies(ext, XQ, G) else ext.ttt_forward_chunk


def _last_row(eta: torch.Tensor, act_dtype) -> torch.Tensor:
    # mlp_tk.py:104-105 : cast, take the last row of the [CS,CS] tile, as a column [.., CS, 1]
    return eta.to(act_dtype)[:, :, :, -1, :, None].contiguous()


class TkMLP(torch.autograd.Function):
    sharded_mode = False  # head-sharded tensor parallel (next row): op is head-local
    # the backward at mini-batches of 16 (head dim 64, bf16): "auto" - what the library resolves, the generic kernels - or "mfma" -
    # the opt-in MFMA backward of csrc/ttt_mlp16_bwd_body.h.  Read by this backward and by FusedPreScanMLP's; ignored at every
    # other geometry (like HipLinear._impl).  The forward call is not affected.
    cs16_bwd_impl = _check_cs16_bwd_impl(os.environ.get("TTT_MLP_CS16_BWD_IMPL", "auto"))

    @staticmethod
    def bwd_impl(CS, F, act_dtype):
        """the ``impl`` of ``ttt_backward_impl`` for a backward at this geometry: None (the global selector) unless the switch applies"""
        value = _check_cs16_bwd_impl(TkMLP.cs16_bwd_impl)
        return "mfma" if value == "mfma" and CS == 16 and F == 64 and act_dtype == _BF16 else None

    # That MFMA backward in parts: 0 = one call (default), n > 0 = ranges of n checkpoint groups, the recompute of the next range on
    # the pipeline's side stream beside the reverse walk of the current one (``backward_in_parts``).  Applies only where ``bwd_impl``
    # returns "mfma" (so ``cs16_bwd_impl`` must be "mfma" too); ignored everywhere else.  Same bits either way.  Default from the
    # environment variable TTT_MLP_CS16_BACKWARD_PARTS, read once at import.
    cs16_backward_parts = _cs16_backward_parts_default()

    @staticmethod
    def bwd_parts(impl):
        """checkpoint groups per part for a backward whose ``bwd_impl`` is ``impl``: 0 = the one call"""
        gpp = TkMLP.cs16_backward_parts
        if not isinstance(gpp, int) or isinstance(gpp, bool) or gpp < 0:
            raise ValueError(f"TkMLP.cs16_backward_parts: expected a non-negative integer, got {gpp!r}")
        return gpp if impl == "mfma" else 0

    @staticmethod
    def bwd_call(ext, impl):
        """the binding's backward for that ``impl``: ``ttt_backward`` itself unless the switch applies; in parts where
        ``cs16_backward_parts`` applies too (same 42 tensors + G)"""
        if impl is None:
            return ext.ttt_backward
        gpp = TkMLP.bwd_parts(impl)
        if gpp:
            return lambda *a: backward_in_parts(ext, gpp, a[:-1], a[-1])
        return functools.partial(ext.ttt_backward_impl, impl)

    @staticmethod
    def forward(ctx, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W2_init, b2_init,
                XQ_batch, XV_batch, XK_batch, eta_batch, checkpoint_group_size):
        ext = _ext()
        B, NH, NC, CS, F = XQ_batch.shape
        G = int(checkpoint_group_size)
        K = math.ceil(NC / G)
        dev, act = XQ_batch.device, XQ_batch.dtype
        if act != _BF16:
            raise AssertionError("TTT-MLP kernel must run in mixed-precision bfloat16.")  # mlp_tk.py:89

        XQ, XV, XK = XQ_batch.contiguous(), XV_batch.contiguous(), XK_batch.contiguous()
        last_eta = _last_row(eta_batch, act)
        ln_w = ttt_norm_weight.reshape(1, NH, 1, F).to(_F32).contiguous()
        ln_b = ttt_norm_bias.reshape(1, NH, 1, F).to(_F32).contiguous()
        state = [t.to(_F32).contiguous() for t in (W1_init, b1_init, W2_init, b2_init)]

        out = torch.empty(B, NH, NC, CS, F, device=dev, dtype=act)
        cks = (torch.empty(B, NH, K, F, 4 * F, device=dev, dtype=_F32), torch.empty(B, NH, K, 1, 4 * F, device=dev, dtype=_F32),
               torch.empty(B, NH, K, 4 * F, F, device=dev, dtype=_F32), torch.empty(B, NH, K, 1, F, device=dev, dtype=_F32))
        mlp_forward_call(ext, XQ, G)(XQ, XK, XV, last_eta, ln_w, ln_b, *state, *cks, out, G)

        ctx.save_for_backward(XQ, XV, XK, last_eta, ln_w, ln_b, *cks)   # XQW is not an input of the backward arithmetic
        ctx.G = G
        ctx.eta_shape = tuple(eta_batch.shape)
        ctx.param_dtypes = (ttt_norm_weight.dtype, W1_init.dtype)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ext = _ext()
        XQ, XV, XK, last_eta, ln_w, ln_b, W1c, b1c, W2c, b2c = ctx.saved_tensors
        B, NH, NC, CS, F = XQ.shape
        G, H, dev = ctx.G, 4 * XQ.shape[-1], XQ.device
        z32 = lambda *s: torch.zeros(*s, device=dev, dtype=_F32)
        e32 = lambda *s: torch.empty(*s, device=dev, dtype=_F32)
        e16 = lambda *s: torch.empty(*s, device=dev, dtype=_BF16)

        up = (z32(B, NH, F, H), z32(B, NH, 1, H), z32(B, NH, H, F), z32(B, NH, 1, F))  # final state is not an output
        g_out = grad_out.to(_BF16).contiguous()
        out = g_out                 # placeholder for the ABI's XQW slot (mlp_tk.py:236): same shape / dtype, never read
        # re-materialisation scratch, shapes/dtypes of mlp_tk.py:192-210 (the backward in parts keeps its state in its own workspaces)
        impl = TkMLP.bwd_impl(CS, F, XQ.dtype)
        remat = (None,) * 16 if TkMLP.bwd_parts(impl) else (
                 e32(B, NH, G, F, H), e32(B, NH, G, 1, H), e32(B, NH, G, H, F), e32(B, NH, G, 1, F),
                 e16(B, NH, G, CS, F), e32(B, NH, G, CS, 1),
                 e16(B, NH, G, CS, H), e16(B, NH, G, CS, H), e16(B, NH, G, CS, H), e16(B, NH, G, CS, H),
                 e16(B, NH, G, CS, F), e16(B, NH, G, CS, H), e16(B, NH, G, CS, F), e16(B, NH, G, CS, F), e16(B, NH, G, CS, F),
                 e32(B, NH, G, CS, 1))
        d_lnw, d_lnb = e32(B, NH, 1, F), e32(B, NH, 1, F)       # per batch element, summed below
        d_state = (e32(B, NH, F, H), e32(B, NH, 1, H), e32(B, NH, H, F), e32(B, NH, 1, F))
        d_eta = torch.empty(B, NH, NC, CS, 1, device=dev, dtype=_BF16)
        dQ, dK, dV = (torch.empty_like(XQ) for _ in range(3))

        TkMLP.bwd_call(ext, impl)(XQ, XK, XV, last_eta, ln_w, ln_b, W1c, b1c, W2c, b2c, out, *remat, *up,
                                   g_out, d_lnw, d_lnb, *d_state, d_eta, dQ, dK, dV, G)

        ln_dt, st_dt = ctx.param_dtypes
        d_lnw = d_lnw.sum(dim=0).squeeze(1).to(ln_dt)
        d_lnb = d_lnb.sum(dim=0).squeeze(1).to(ln_dt)
        row = d_eta.transpose(-2, -1)                              # [B,NH,NC,1,CS]
        rows = ctx.eta_shape[-2]
        d_eta_full = row if rows == 1 else torch.nn.functional.pad(row, (0, 0, rows - 1, 0))
        act = XQ.dtype
        return (d_lnw, d_lnb, *(g.to(st_dt) for g in d_state), dQ.to(act), dV.to(act), dK.to(act), d_eta_full.to(act), None)
