"""CPU oracle of the TTT layer's glue kernels (TEST INFRASTRUCTURE ONLY - imported by tests/, never by the product path).

Restates in plain fp64 tensor statements what ``csrc/ttt_prepost.hip`` computes, from the maths and from the module's unfused
path: ``TTTBase.process_input`` / ``ln_reconstruction_target`` / ``_token_maps`` (``ssm/ttt_layer.py``), ``apply_rotary_emb``
(``ssm/utils.py``), ``post_norm`` + the inverse token map, ``SeqModelingBlock._gate``, ``modulate`` and the gated residuals
(``cogvideo/dit.py``, ``cogvideo/utils.py``).  Pinned to that unfused path by ``tests/test_glue_oracle_cpu.py``, which the
reference-executed ``mod_*.pt`` goldens pin in turn (``test_modules_cpu.py``, ``test_parity_r2_cpu.py``).

``round_bf16=True`` rounds to bf16 exactly where the bf16 module (and the kernels) round: after the L2 normalisation, after the
rotation, after the LayerNorm of AdaLN, after the gate product of the residual gates, at every output.  Each rounding is
straight-through (``x + (bf16(x) - x).detach()``), so fp64 autograd of these statements gives the gradients the kernels compute.
"""
import torch

NORM_EPS = 1e-12      # F.normalize
TGT_EPS = 1e-8        # ln_reconstruction_target: eps added to the unbiased std


def rb(x, on=True):
    """straight-through bf16 rounding"""
    return x + (x.to(torch.bfloat16).to(x.dtype) - x).detach() if on else x


def _rows(x, src):
    return x if src is None else x.index_select(1, src.long())


def rotate(y, rope, pos, sin_sign=1.0):
    """rotate adjacent (even, odd) pairs of y [B, L, NH, F] by rope[pos[t]] ([n, F/2, 2] (cos, sin)); pos < 0: unrotated"""
    p = pos.long()
    cs = rope.to(y.dtype)[p.clamp_min(0)]                               # [L, F/2, 2]
    c, s = cs[None, :, None, :, 0], sin_sign * cs[None, :, None, :, 1]
    a, b = y[..., 0::2], y[..., 1::2]
    r = torch.stack((a * c - b * s, a * s + b * c), dim=-1).flatten(-2)
    return r, (p >= 0)[None, :, None, None]


def pre(q_raw, k_raw, v_raw, ln_w, ln_b, rope, src, pos, NH, round_bf16=True, *, unbiased=True, sin_sign=1.0):
    """q_raw, k_raw, v_raw [B, Lin, NH*F]; ln_w, ln_b [NH, F]; rope [n, F/2, 2] or None; src, pos [L] (or None: identity /
    no rotation) -> XQ, XK, XV [B, NH, L, F] in scan order: position t reads token src[t], rotated by rope[pos[t]].
    ``unbiased`` / ``sin_sign``: mutation switches for the sensitivity table of the tests."""
    B, Lin, D = q_raw.shape
    F = D // NH
    L = Lin if src is None else src.numel()
    heads = lambda x: _rows(x, src).reshape(B, L, NH, F)
    q, k, v = heads(q_raw), heads(k_raw), heads(v_raw)

    def norm_rope(x):
        y = rb(x / x.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS), round_bf16)
        if pos is None or rope is None:
            return y
        r, rot = rotate(y, rope, pos, sin_sign)
        return torch.where(rot, rb(r, round_bf16), y)

    q, k = norm_rope(q), norm_rope(k)
    d = v - k
    d = d - d.mean(dim=-1, keepdim=True)
    sd = (d.square().sum(dim=-1, keepdim=True) / (F - 1 if unbiased else F)).sqrt()
    t = ln_w.to(d.dtype).view(1, 1, NH, F) * (d / (sd + TGT_EPS)) + ln_b.to(d.dtype).view(1, 1, NH, F) + k
    out = lambda x: rb(x, round_bf16).permute(0, 2, 1, 3)
    return out(q), out(k), out(t)


def layernorm(x, w, b, eps, eps_in_sqrt=True):
    xc = x - x.mean(dim=-1, keepdim=True)
    var = xc.square().mean(dim=-1, keepdim=True)
    den = (var + eps).sqrt() if eps_in_sqrt else var.sqrt() + eps
    return xc / den * w.to(x.dtype) + b.to(x.dtype)


def post(Y, w, b, src, eps, round_bf16=True, *, eps_in_sqrt=True):
    """Y [B, NH, L, F] in scan order -> LayerNorm over D = NH*F as [B, L, D] in token order: position t lands on token src[t]."""
    B, NH, L, F = Y.shape
    y = layernorm(Y.permute(0, 2, 1, 3).reshape(B, L, NH * F), w, b, eps, eps_in_sqrt)
    if src is not None:
        y = torch.zeros_like(y).index_copy(1, src.long(), y)
    return rb(y, round_bf16)


def gate(res, y, alpha_text, alpha_video, n_text, round_bf16=True):
    """res + tanh(alpha) * y with the text gate on tokens [0, n_text) and the video gate on the rest (res, y [B, L, D])."""
    L = res.shape[1]
    sel = torch.cat((torch.tanh(alpha_text).expand(min(n_text, L), -1), torch.tanh(alpha_video).expand(L - min(n_text, L), -1)))
    return rb(res + sel * y, round_bf16)


def adaln(vid, text, w, b, shift_v, scale_v, shift_t, scale_t, eps, round_bf16=True):
    """[modulate(LN(text), shift_t, scale_t) | modulate(LN(vid), shift_v, scale_v)] as [B, Lt + Lv, D]; modulate(x, sh, sc) =
    sh + x * (1 + sc) with [B, D] modulation; ``1 + sc`` and the LayerNorm output are bf16 values in the bf16 module."""
    def one(x, sh, sc):
        return sh[:, None] + rb(layernorm(x, w, b, eps), round_bf16) * rb(1 + sc, round_bf16)[:, None]
    return rb(torch.cat((one(text, shift_t, scale_t), one(vid, shift_v, scale_v)), dim=1), round_bf16)


def resgate(vid, text, y, gate_v, gate_t, round_bf16=True):
    """(vid + gate_v * y[:, Lt:], text + gate_t * y[:, :Lt]) with y = [text | video] and [B, D] gates."""
    Lt = text.shape[1]
    ov = vid + rb(gate_v[:, None] * y[:, Lt:], round_bf16)
    ot = text + rb(gate_t[:, None] * y[:, :Lt], round_bf16)
    return rb(ov, round_bf16), rb(ot, round_bf16)
