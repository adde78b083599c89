"""Pins ``oracle/glue_oracle.py`` (the fp64 statement of the fused pre / post / gate / AdaLN / residual-gate kernels) to the module's
unfused path on CPU tensors, and fixes the tolerances of ``tests/test_prepost_oracle_gpu.py`` with a sensitivity table: for every
metric the GPU file asserts, the distance a correct fp32 kernel can have (the oracle in fp32 vs fp64) and the distance of a set of
plausible kernel bugs (the oracle with one statement changed).  The unfused path is itself pinned to the reference-executed
``mod_*.pt`` goldens (``test_modules_cpu.py``, ``test_parity_r2_cpu.py``)."""
import pytest
import torch

from helpers import glue_maps, rel_l2, row_rel_err, scene_meta, ulp_stats
from oracle import glue_oracle as G

# (text_length, scenes, frames, H, W): single scene without / with text, three scenes (scene 0 owns the remainder frame)
CASES = {"1scene": (0, 1, 4, 4, 8), "1scene_text": (32, 1, 4, 4, 8), "3scene": (16, 3, 7, 4, 4)}


def _wrapper(NH, meta, CS):
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm.ttt_layer import TTTWrapper
    cfg = ModelConfig(model_dim=NH * 64, num_heads=NH, num_layers=1, mini_batch_size=CS, latent_height=meta.latent_height,
                      latent_width=meta.latent_width, compressed_num_frames=meta.num_frames)
    torch.manual_seed(0)
    m = TTTWrapper(cfg)
    m.ttt.use_kernel = False
    with torch.no_grad():
        m.ttt.ttt_norm_weight.copy_((1 + 0.3 * torch.randn_like(m.ttt.ttt_norm_weight)).bfloat16())
        m.ttt.ttt_norm_bias.copy_((0.2 * torch.randn_like(m.ttt.ttt_norm_bias)).bfloat16())
        m.ttt.post_norm.weight.copy_((1 + 0.3 * torch.randn(NH * 64)).bfloat16())
        m.ttt.post_norm.bias.copy_((0.2 * torch.randn(NH * 64)).bfloat16())
    return m


def _raws(B, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [(s * torch.randn(B, L, D, generator=g)).bfloat16() for s in (1.0, 1.0, 0.5)]


def _module_pre(m, raws, meta, reverse):
    """XQ, XK, XV [B, NH, L, F] from the module's process_input (projections replaced by the given raw tensors; the time
    reversal is applied to its inputs as TTTBase.forward does)."""
    from ttt_amd.models.ssm.ttt_layer import flip_sequence
    if reverse:
        raws = [flip_sequence(r, meta) for r in raws]
    t = m.ttt
    t.get_qkv_projections = lambda h: tuple(raws)
    out = t.process_input(raws[0], m.freqs_cis, meta)
    del t.get_qkv_projections
    B, NH, NC, CS, F = out["XQ"].shape
    return [out[k].reshape(B, NH, NC * CS, F) for k in ("XQ", "XK", "XV")]


def _module_post(m, Y, meta, reverse):
    """the unfused tail: post_norm on the scan output [B, NH, L, F], undo the scene interleave, undo the time reversal"""
    from ttt_amd.models.ssm.ttt_layer import flip_sequence
    B, NH, L, F = Y.shape
    y = m.ttt.post_norm(Y.permute(0, 2, 1, 3).reshape(B, L, NH * F))
    if meta.is_multiscene:
        y = m.ttt.undo_interleave(y, meta)
    return flip_sequence(y, meta) if reverse else y


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("reverse", [False, True])
def test_pre_post_oracle_matches_unfused_module_fp64(case, reverse):
    """fp64 inputs: the oracle (round_bf16=False) == process_input / post_norm tail of the module, forward and every gradient, to
    the fp32 precision of the module's ``.float()`` casts (rotation, LN target)"""
    meta = scene_meta(*CASES[case])
    L, src, pos, rope = glue_maps(meta, reverse)
    NH, B = 3, 2
    m = _wrapper(NH, meta, 16).double()
    assert int(pos.max()) + 1 == rope.shape[0]                      # the last row of the RoPE table is used
    raws = [r.double().requires_grad_(True) for r in _raws(B, L, NH * 64, 1)]
    got = _module_pre(m, raws, meta, reverse)
    g = torch.Generator().manual_seed(2)
    dout = [torch.randn(x.shape, generator=g, dtype=torch.float64) for x in got]
    params = (m.ttt.ttt_norm_weight, m.ttt.ttt_norm_bias)
    gm = torch.autograd.grad(got, raws + list(params), dout)
    raws2 = [r.detach().clone().requires_grad_(True) for r in raws]
    lw, lb = (p.detach().clone().requires_grad_(True) for p in params)
    want = G.pre(*raws2, lw, lb, rope.double(), src, pos, NH, round_bf16=False)
    go = torch.autograd.grad(want, raws2 + [lw, lb], dout)
    for a, b in zip(got, want):
        assert rel_l2(a, b) < 1e-6 and row_rel_err(a, b, (0, 1, 2)) < 1e-5, (rel_l2(a, b), row_rel_err(a, b, (0, 1, 2)))
    for i, (a, b) in enumerate(zip(gm, go)):
        assert rel_l2(a, b) < 1e-6, (i, rel_l2(a, b))

    Y = torch.randn(B, NH, L, 64, generator=g, dtype=torch.float64).requires_grad_(True)
    y = _module_post(m, Y, meta, reverse)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    pn = m.ttt.post_norm
    gm = torch.autograd.grad(y, (Y, pn.weight, pn.bias), dy)
    Y2, w, b = (t.detach().clone().requires_grad_(True) for t in (Y, pn.weight, pn.bias))
    yo = G.post(Y2, w, b, src, pn.eps, round_bf16=False)
    go = torch.autograd.grad(yo, (Y2, w, b), dy)
    assert rel_l2(yo, y) < 1e-12
    assert all(rel_l2(a, b) < 1e-12 for a, b in zip(go, gm))


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("reverse", [False, True])
def test_pre_post_oracle_rounding_matches_bf16_module(case, reverse):
    """round_bf16=True: the oracle in fp64 on bf16 inputs == the module's unfused path run on bf16 CPU tensors.  Unrotated (text)
    rows of XQ / XK and the post output agree to 1 bf16 ulp per element.  The module divides by a bf16-rounded norm (F.normalize),
    the oracle and the kernel by the exact one: a 1-ulp difference of the normalised values that the rotation and the LN target
    carry on, so those are held to 4 ulps at the row's scale (floor: the RMS) and 1 % of the elements beyond 1 ulp."""
    meta = scene_meta(*CASES[case])
    L, src, pos, rope = glue_maps(meta, reverse)
    NH, B = 3, 2
    m = _wrapper(NH, meta, 16).to(torch.bfloat16)
    raws = _raws(B, L, NH * 64, 3)
    with torch.no_grad():
        got = _module_pre(m, raws, meta, reverse)
    f = lambda t: t.detach().double()
    want = G.pre(*map(f, raws), f(m.ttt.ttt_norm_weight), f(m.ttt.ttt_norm_bias), rope.double(), src, pos, NH)
    text = pos < 0
    for i, (a, b) in enumerate(zip(got, want)):
        frac, mx = ulp_stats(a, b, floor=float(b.square().mean().sqrt()))
        assert frac < 1e-2 and mx <= 4, (i, frac, mx)
        if i < 2 and bool(text.any()):
            assert ulp_stats(a[:, :, text], b[:, :, text])[1] <= 1, i
    g = torch.Generator().manual_seed(4)
    Y = (0.1 * torch.randn(B, NH, L, 64, generator=g)).bfloat16()
    with torch.no_grad():
        y = _module_post(m, Y, meta, reverse)
    pn = m.ttt.post_norm
    assert ulp_stats(y, G.post(f(Y), f(pn.weight), f(pn.bias), src, pn.eps))[1] <= 1


@pytest.mark.parametrize("n_text", [0, 1, 40, 96])
def test_gate_adaln_resgate_oracle_matches_module_fp64(n_text):
    """fp64: the oracle (round_bf16=False) == SeqModelingBlock._gate with its SSMGating modules, modulate(LayerNorm) + concat and
    the gated residuals of TransformerLayer, forward and gradients"""
    from types import SimpleNamespace
    from ttt_amd.models.cogvideo.dit import SeqModelingBlock, SSMGating
    from ttt_amd.models.cogvideo.utils import modulate
    g = torch.Generator().manual_seed(n_text)
    B, L, D = 2, 96, 128
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)
    res, y, dout = r(B, L, D), r(B, L, D), torch.randn(B, L, D, generator=g, dtype=torch.float64)
    gt, gv = (SSMGating(SimpleNamespace(model_dim=D, gating_alpha_init=0.1)).double() for _ in range(2))
    with torch.no_grad():
        gt.gating_alpha.normal_(generator=g); gv.gating_alpha.normal_(generator=g)
    ins = (res, y, gt.gating_alpha, gv.gating_alpha)
    got = SeqModelingBlock._gate(None, gt, gv, res, y, n_text)
    want = G.gate(res, y, gt.gating_alpha, gv.gating_alpha, n_text, round_bf16=False)
    assert rel_l2(got, want) < 1e-14
    for a, b in zip(torch.autograd.grad(got, ins, dout), torch.autograd.grad(want, ins, dout)):
        assert rel_l2(a, b) < 1e-14

    Lt, Lv = n_text, L - n_text
    ln = torch.nn.LayerNorm(D, eps=1e-6).double()
    with torch.no_grad():
        ln.weight.normal_(generator=g); ln.bias.normal_(generator=g)
    vid, text = r(B, Lv, D), r(B, Lt, D)
    mods = [r(B, D) for _ in range(6)]                              # sh_v, sc_v, sh_t, sc_t, g_v, g_t
    ins = [vid, text, ln.weight, ln.bias] + mods
    got = torch.cat((modulate(ln(text), mods[2], mods[3]), modulate(ln(vid), mods[0], mods[1])), dim=1)
    want = G.adaln(vid, text, ln.weight, ln.bias, *mods[:4], ln.eps, round_bf16=False)
    assert rel_l2(got, want) < 1e-14
    for a, b in zip(torch.autograd.grad(got, ins, dout, allow_unused=True), torch.autograd.grad(want, ins, dout, allow_unused=True)):
        assert (a is None and b is None) or rel_l2(a, b) < 1e-14
    got = (vid + mods[4].unsqueeze(1) * y[:, Lt:], text + mods[5].unsqueeze(1) * y[:, :Lt])
    want = G.resgate(vid, text, y, mods[4], mods[5], round_bf16=False)
    assert all(rel_l2(a, b) < 1e-14 for a, b in zip(got, want) if b.numel())


# ------------------------------------------------------------------------------------------------ sensitivity table
def _dist(metric, a, b, row_dims):
    """distance of a result (a kernel's, or the oracle's in fp32 or mutated) from the fp64 oracle; bf16 outputs (every tensor that
    is not a parameter-gradient sum) are rounded first, as the kernels write them"""
    if metric == "psum":
        return rel_l2(a, b)
    a = a.bfloat16()
    if metric == "row":
        return row_rel_err(a, b.bfloat16(), row_dims)
    return ulp_stats(a, b)[0 if metric == "ulp_frac" else 1]


ROWS = {"XQ": (0, 1, 2), "XK": (0, 1, 2), "XV": (0, 1, 2), "dq": (0, 1), "dk": (0, 1), "dv": (0, 1), "out": (0, 1), "dY": (0, 1, 2),
        "dy": (0, 1), "dvid": (0, 1), "dtext": (0, 1), "ovid": (0, 1), "otext": (0, 1)}
PSUM = ("dln_w", "dln_b", "dw", "db", "dtanh_t", "dtanh_v", "dsh_v", "dsc_v", "dsh_t", "dsc_t", "dg_v", "dg_t")


def _fp32_error(metric, want, got):
    """largest distance of the oracle in fp32 from the oracle in fp64 over the tensors the metric is asserted on"""
    keys = PSUM if metric == "psum" else [k for k in want if k in ROWS]
    return max(_dist(metric, got[k], want[k], ROWS.get(k)) for k in keys if k in want)


def sensitivity_table():
    """{metric: (fp32 error, threshold, {mutation: distance})} on a 3-scene, 4-head, batch-2 sequence (the GPU file's kinds of
    inputs at a CPU-sized length)"""
    from collections import defaultdict
    from helpers import GLUE_TOL
    import glue_cases as C
    B, NH = 2, 4
    meta = scene_meta(32, 3, 10, 4, 8)
    L, src, pos, rope = glue_maps(meta)
    pc, qc, gc, ac = C.pre_case(B, L, NH, 5), C.post_case(B, L, NH, 6), C.gate_case(B, L, 512, 7), C.adaln_case(B, 96, 320, 512, 8)
    n_text, eps = meta.seq_text_length, 1e-6
    runs = {  # (fp64, fp32) oracle results per kernel
        "pre": [C.pre_oracle(pc, rope, src, pos, NH, dt) for dt in (torch.float64, torch.float32)],
        "post": [C.post_oracle(qc, src, eps, dt) for dt in (torch.float64, torch.float32)],
        "gate": [C.gate_oracle(gc, n_text, dt) for dt in (torch.float64, torch.float32)],
        "adaln": [C.adaln_oracle(ac, eps, dt) for dt in (torch.float64, torch.float32)],
        "resgate": [C.resgate_oracle(ac, dt) for dt in (torch.float64, torch.float32)],
    }
    last = pos.clone()
    last[int(pos.argmax())] = -1
    mutations = {   # name: (metric it must trip, fp64 oracle result of the mutated kernel, reference result, key)
        "biased std": ("ulp_frac", C.pre_oracle(pc, rope, src, pos, NH, unbiased=False), runs["pre"][0], "XV"),
        "biased std (dln_w)": ("psum", C.pre_oracle(pc, rope, src, pos, NH, unbiased=False), runs["pre"][0], "dln_w"),
        "sign of sin": ("row", C.pre_oracle(pc, rope, src, pos, NH, sin_sign=-1.0), runs["pre"][0], "XQ"),
        "pos off by one text token": ("row", C.pre_oracle(pc, rope, src, (pos - 1).clamp_min(-1), NH), runs["pre"][0], "XK"),
        "no RoPE on the last video token": ("row", C.pre_oracle(pc, rope, src, last, NH), runs["pre"][0], "XQ"),
        "post: src and inverse src swapped": ("row", C.post_oracle(qc, torch.argsort(src), eps), runs["post"][0], "out"),
        "post: eps outside the sqrt": ("row", C.post_oracle(qc, src, eps, eps_in_sqrt=False), runs["post"][0], "out"),
        "gate: text gate on token n_text": ("row", C.gate_oracle(gc, n_text + 1), runs["gate"][0], "out"),
        "gate: text gate on token n_text (dalpha)": ("psum", C.gate_oracle(gc, n_text + 1), runs["gate"][0], "dtanh_t"),
    }
    table = {}
    for metric, tol in GLUE_TOL.items():
        err = max(_fp32_error(metric, want, got) for want, got in runs.values())
        table[metric] = (err, tol, {})
    for name, (metric, mut, ref, key) in mutations.items():
        table[metric][2][name] = _dist(metric, mut[key], ref[key], ROWS.get(key))
    return table


def test_sensitivity_table():
    """every threshold >= 10x the fp32 arithmetic's distance from fp64, every mutation >= 10x its threshold (ulp_max has no
    mutation of its own: the fraction and row metrics catch the mutations that move elements by more than a few ulps)"""
    table = sensitivity_table()
    for metric, (err, tol, muts) in table.items():
        print(f"{metric:9s} fp32 {err:.3g}  threshold {tol:.3g}  " + ", ".join(f"{k}: {v:.3g}" for k, v in muts.items()))
    for metric, (err, tol, muts) in table.items():
        assert 10 * err <= tol, (metric, err, tol)
        for name, v in muts.items():
            assert v >= 10 * tol, (metric, name, v, tol)
