"""The opt-in MFMA TTT-MLP backward at mini-batches of 16 (csrc/ttt_mfma16.hip: mlp_bwd16_kernel) on the device, through
``ttt_backward_impl("mfma", ...)`` from the MFMA forward's checkpoints: the fp64 oracle with a nonzero upstream state gradient, the
generic kernels on the same call, a call over K groups against K chained one-group calls, the recomputed slots against the forward's
checkpoints, determinism, and the layer switch ``TkMLP.cs16_bwd_impl`` through the autograd boundary and a TTT-MLP module.  Cases,
bounds and seeds: tests/mlp16_bwd_cases.py (every case was first run on the wave emulator, tests/test_emul_mlp16_bwd_cpu.py)."""
import pytest
import torch

import mlp16_bwd_cases as M
from helpers import SCAN_BWD_TOL_GENERIC, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ext():
    import test_time_training as e
    e.load_library()
    return e


def device_forward(e, t, G):
    B, NH, NC = t["XQ"].shape[:3]
    K = -(-NC // G)
    d = {k: v.to(DEV) for k, v in t.items()}
    cks = tuple(torch.full((B, NH, K, a, b), float("nan"), device=DEV) for a, b in M.STATE_SHAPES)
    out = torch.full((B, NH, NC, M.CS, M.F), float("nan"), device=DEV, dtype=torch.bfloat16)
    lw, lb = d["ln_w"].reshape(1, NH, 1, M.F), d["ln_b"].reshape(1, NH, 1, M.F)
    assert e.resolved_impl(B, NH, NC, M.CS, M.F, G, torch.bfloat16, mlp=True, backward=False) == "mfma"
    e.ttt_forward(d["XQ"], d["XK"], d["XV"], d["eta"], lw, lb, d["W1"], d["b1"], d["W2"], d["b2"], *cks, out, G)
    torch.cuda.synchronize()
    return out.cpu(), tuple(c.cpu() for c in cks)


def device_run(e, impl):
    """``run`` of mlp16_bwd_cases over ``ttt_backward_impl(impl, ...)``: host tensors in, host results out"""
    def run(t, cks, up, G):
        B, NH, NC = t["XQ"].shape[:3]
        assert e.resolved_impl(B, NH, NC, M.CS, M.F, G, torch.bfloat16, mlp=True, backward=True, impl=impl) == impl
        ins = {k: t[k].to(DEV) for k in ("XQ", "XK", "XV", "eta", "dOut", "ln_w", "ln_b")}
        ins.update({f"ck{i}": c.to(DEV) for i, c in enumerate(cks)})
        ins.update({f"up{i}": u.to(DEV) for i, u in enumerate(up)})
        keep = {k: v.clone() for k, v in ins.items()}
        g = M.outputs(B, NH, NC, device=DEV)
        raw, scr = M.guarded_scratch(B, NH, G, device=DEV)
        lw, lb = ins["ln_w"].reshape(1, NH, 1, M.F), ins["ln_b"].reshape(1, NH, 1, M.F)
        e.ttt_backward_impl(impl, ins["XQ"], ins["XK"], ins["XV"], ins["eta"], lw, lb, *[ins[f"ck{i}"] for i in range(4)], ins["dOut"],
                            *scr, *[None] * 12, *[ins[f"up{i}"] for i in range(4)], ins["dOut"], g["dln_w"], g["dln_b"], g["dW1"],
                            g["db1"], g["dW2"], g["db2"], g["dlast_eta"], g["dXQ"], g["dXK"], g["dXV"], G)
        torch.cuda.synchronize()
        M.check_guards(raw)
        for k, v in ins.items():
            assert torch.equal(v, keep[k]), f"input {k} was written"
        assert e.get_impl() == "auto"
        return {k: v.cpu() for k, v in g.items()}, [s.cpu() for s in scr]
    return run


_CASES = {}


def _case(e, B, NH, NC, G, seed):
    key = (B, NH, NC, G, seed)
    if key not in _CASES:
        c = M.case(B, NH, NC, seed)
        out, cks = device_forward(e, M.host_tensors(c), G)
        _CASES[key] = (c, out, cks, M.upstream(c, cks, G, seed))
    return _CASES[key]


@pytest.mark.parametrize("shape", M.SHAPES)
def test_mfma_mlp_cs16_backward_vs_oracle_and_generic(shape):
    """the five shapes of the emulator test: the ten gradients (and dW1 / db1 / dW2 per 32-hidden-unit slice) within 3e-2 of the fp64
    oracle from the MFMA forward's checkpoints with a nonzero upstream; NaN-initialised outputs, guarded scratch, inputs unchanged;
    the generic kernels on the same call agree within 3e-2"""
    e = ext()
    B, NH, NC, G = shape
    c, out, cks, up = _case(e, B, NH, NC, G, M.seed_of(shape))
    ro, rc = M.oracle_forward(c, G)
    errs = {"XQW": rel_l2(out, ro), **{f"ck{i}": rel_l2(a, b) for i, (a, b) in enumerate(zip(cks, rc))}}
    assert all(v < M.TOL_OUT for v in errs.values()), errs
    g, _ = M.check_call(f"mfma mlp CS=16 backward {shape}", device_run(e, "mfma"), c, cks, up, G)
    gg, _ = device_run(e, "generic")(M.host_tensors(c), cks, up, G)
    vs = {k: rel_l2(g[k], gg[k].double()) for k in M.GRADS}
    print(f"mfma vs generic {shape}: " + "  ".join(f"{k} {v:.3g}" for k, v in vs.items()))
    assert all(v < M.TOL_G for v in vs.values()), vs


@pytest.mark.parametrize("NC,G", M.CHAIN)
def test_mfma_whole_call_is_the_chain_of_its_groups(NC, G):
    e = ext()
    c, _, cks, up = _case(e, M.CHAIN_B, M.CHAIN_NH, NC, G, 500 + NC)
    M.check_chain(f"mfma mlp CS=16 chain NC={NC} G={G}", device_run(e, "mfma"), c, cks, up, G, SCAN_BWD_TOL_GENERIC["dln"])


def test_mfma_recompute_leaves_the_forward_states_in_the_scratch():
    """the slots of group 0 after a backward with G = 3 hold the bits of the checkpoints of a forward with G = 1"""
    e = ext()
    B, NH, NC, G = 1, 2, 7, 3
    c, _, cks, up = _case(e, B, NH, NC, G, M.seed_of((B, NH, NC, G)))
    t = M.host_tensors(c)
    _, scr = device_run(e, "mfma")(t, cks, up, G)
    _, cks1 = device_forward(e, t, 1)
    for name, s, k1 in zip(("W1", "b1", "W2", "b2"), scr, cks1):
        assert torch.equal(s[:, :, :G], k1[:, :, :G]), name


def test_mfma_backward_is_deterministic():
    e = ext()
    shape = (2, 3, 9, 4)
    c, _, cks, up = _case(e, *shape, M.seed_of(shape))
    run = device_run(e, "mfma")
    a, _ = run(M.host_tensors(c), cks, up, shape[3])
    b, _ = run(M.host_tensors(c), cks, up, shape[3])
    for k in M.GRADS:
        assert torch.equal(a[k], b[k]), k


def _tk_grads(c, G, impl):
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    t = M.host_tensors(c)
    leaves = [t[k].to(DEV).requires_grad_(True) for k in ("ln_w", "ln_b", "W1", "b1", "W2", "b2", "XQ", "XV", "XK")]
    eta = t["eta"].to(DEV).transpose(-2, -1).contiguous().requires_grad_(True)          # the last row [B, NH, NC, 1, CS]
    old = TkMLP.cs16_bwd_impl
    TkMLP.cs16_bwd_impl = impl
    try:
        out = TkMLP.apply(*leaves, eta, G)
        out.backward(t["dOut"].to(DEV))
        torch.cuda.synchronize()
    finally:
        TkMLP.cs16_bwd_impl = old
    return out.detach().cpu(), [x.grad.cpu() for x in leaves + [eta]]


def test_autograd_switch_mfma_vs_auto():
    """``TkMLP.apply`` at (2, 3, 9, 4) with the switch at "mfma" against "auto": equal forward bits, all ten gradients within 3e-2"""
    ext()
    shape = (2, 3, 9, 4)
    c = M.case(*shape[:3], M.seed_of(shape))
    o0, g0 = _tk_grads(c, shape[3], "auto")
    o1, g1 = _tk_grads(c, shape[3], "mfma")
    assert torch.equal(o0, o1)
    errs = [rel_l2(a, b.double()) for a, b in zip(g1, g0)]
    print("TkMLP mfma vs auto:", [f"{v:.3g}" for v in errs])
    assert len(errs) == 10 and all(v < M.TOL_G for v in errs), errs


def test_module_fused_path_switch_mfma_vs_auto():
    """a TTT-MLP module at mini-batch 16 (the fused pre / scan path) with grad enabled: every parameter and input gradient with the
    switch at "mfma" within 3e-2 of the default path.  Four heads: the gradient of the learnable-lr bias has one entry per head, each
    the sum over all tokens of a signed, bf16-rounded d eta; with two heads one cancelling sum decides the rel-L2 of the whole
    tensor (measured 3.7e-2 there, every other gradient under 5e-3)."""
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    from ttt_amd.models.ssm.ttt_layer import TTTWrapper
    ext()
    scenes, tl, frames, tpf = 1, 32, 4, 64
    cfg = ModelConfig(model_dim=256, num_heads=4, num_layers=1, mini_batch_size=16, latent_height=8, latent_width=8,
                      compressed_num_frames=frames, ssm_layer="ttt_mlp", scan_checkpoint_group_size=4, ttt_base_lr=1.0)
    torch.manual_seed(0)
    m = TTTWrapper(cfg)
    m.ttt.init_weights()
    m = m.to(DEV).to(torch.bfloat16)
    m.init_freqs()
    meta = SequenceMetadata(text_length=tl, seq_text_length=tl * scenes, num_frames=frames, num_chunks=scenes, tokens_per_frame=tpf,
                            latent_height=8, latent_width=8, t_emb=None)
    L = scenes * tl + frames * tpf
    g = torch.Generator(device=DEV).manual_seed(11)
    x0 = torch.randn(2, L, 256, device=DEV, generator=g).bfloat16()
    dy = torch.randn(2, L, 256, device=DEV, generator=g).bfloat16()

    def grads(impl):
        old = TkMLP.cs16_bwd_impl
        TkMLP.cs16_bwd_impl = impl
        try:
            m.zero_grad(set_to_none=True)
            x = x0.clone().requires_grad_(True)
            y = m(x, meta, False)
            y.backward(dy)
            torch.cuda.synchronize()
        finally:
            TkMLP.cs16_bwd_impl = old
        out = {"x": x.grad.float().cpu()}
        out.update({n: p.grad.float().cpu() for n, p in m.named_parameters() if p.grad is not None})
        return y.detach().float().cpu(), out

    y0, g0 = grads("auto")
    y1, g1 = grads("mfma")
    assert torch.equal(y0, y1) and set(g0) == set(g1) and len(g0) > 5
    errs = {n: rel_l2(g1[n], g0[n].double()) for n in g0 if float(g0[n].norm()) > 0}
    print("module mfma vs auto:", {n: round(v, 5) for n, v in errs.items()})
    assert all(v < M.TOL_G for v in errs.values()), errs
