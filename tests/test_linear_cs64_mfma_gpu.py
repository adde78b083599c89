"""The opt-in MFMA TTT-Linear kernels at mini-batches of 64 (csrc/ttt_lin64_body.h: linear_fwd_cs64_kernel / linear_bwd_cs64_kernel)
on the device, requested per call with ``impl="mfma"``: against the fp64 oracle and the generic kernels, one step at a time, for
determinism and head equivariance, at the 3 s head geometry, and through ``HipLinear.cs64_impl`` at the layer level.  ``auto`` must
keep resolving the geometry to the generic kernels."""
import math

import pytest
import torch

import scan_cases as C
from helpers import SCAN_TOL, load_golden, rel_l2, tile_states
from oracle import ttt_oracle as O
from test_kernels_gpu import _per_head, check_vs_oracle, oracle_on, round_acts
from test_scan_oracle_gpu import assert_written_inside, guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def ext():
    import test_time_training as e
    e.load_library()
    return e


def run_lin64(e, d, G, impl):
    """forward + backward through the binding with ``impl=`` per call; every output a NaN buffer between NaN guards; the inputs and
    the initial state must come back unchanged"""
    XQ, XK, XV, dOut = (d[k].to(DEV, BF).contiguous() for k in ("XQ", "XK", "XV", "dOut"))
    B, NH, NC, CS, F = XQ.shape
    K = math.ceil(NC / G)
    last_eta = d["eta"][:, :, :, -1, :, None].to(DEV, BF).contiguous()
    ln_w, ln_b = d["ln_w"].to(DEV, torch.float32).contiguous(), d["ln_b"].to(DEV, torch.float32).contiguous()
    st = {k: v.to(DEV, torch.float32) for k, v in tile_states(d, B).items()}
    ins = dict(XQ=XQ, XK=XK, XV=XV, dOut=dOut, last_eta=last_eta, ln_w=ln_w, ln_b=ln_b, W1=st["W1"], b1=st["b1"])
    keep = {k: v.clone() for k, v in ins.items()}
    f32 = torch.float32
    bufs = {"out": guarded((B, NH, NC, CS, F), BF), "W1c": guarded((B, NH, K, F, F), f32), "b1c": guarded((B, NH, K, 1, F), f32)}
    out, cks = bufs["out"][1], (bufs["W1c"][1], bufs["b1c"][1])
    e.ttt_linear_forward_impl(impl, XQ, XK, XV, last_eta, ln_w, ln_b, st["W1"], st["b1"], *cks, out, G)
    gb = {"dln_w": guarded((B, NH, 1, F), f32), "dln_b": guarded((B, NH, 1, F), f32), "dW1": guarded((B, NH, F, F), f32),
          "db1": guarded((B, NH, 1, F), f32), "dlast_eta": guarded((B, NH, NC, CS, 1), BF), "dXQ": guarded((B, NH, NC, CS, F), BF),
          "dXK": guarded((B, NH, NC, CS, F), BF), "dXV": guarded((B, NH, NC, CS, F), BF)}
    scr = {"W1_init_group": guarded((B, NH, G, F, F), f32), "b1_init_group": guarded((B, NH, G, 1, F), f32)}
    g = {k: v[1] for k, v in gb.items()}
    z = lambda *s: torch.zeros(s, device=DEV, dtype=f32)
    e.ttt_linear_backward_impl(impl, XQ, XK, XV, last_eta, ln_w, ln_b, *cks, z(B, NH, F, F), z(B, NH, 1, F), dOut,
                          scr["W1_init_group"][1], scr["b1_init_group"][1], g["dln_w"], g["dln_b"], g["dW1"], g["db1"],
                          g["dlast_eta"], g["dXQ"], g["dXK"], g["dXV"], G)
    torch.cuda.synchronize()
    assert_written_inside({**bufs, **gb}, f"linear CS=64 {impl} {(B, NH, NC, G)}")
    for name, (buf, _) in scr.items():       # opaque scratch: only its bounds are checked
        assert bool(torch.isnan(buf[:256]).all()) and bool(torch.isnan(buf[-256:]).all()), f"write outside {name}"
    for k, v in ins.items():
        assert torch.equal(v, keep[k]), f"{k} was written"
    assert e.get_impl() == "auto"
    return out, cks, g


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 2, 4, 2), (2, 3, 7, 3), (1, 5, 11, 3)])
def test_mfma_linear_cs64_vs_oracle_and_generic(shape):
    """forced ``mfma`` forward + backward vs the fp64 oracle on the same bf16-rounded inputs (1e-2 / 3e-2) and vs the
    generic kernels at the same bounds: a single step, even groups, B > 1 with a ragged last group, an odd head count"""
    e = ext()
    B, NH, NC, G = shape
    assert e.resolved_impl(B, NH, NC, 64, 64, G, BF, mlp=False, backward=False, impl="mfma") == "mfma"
    assert e.resolved_impl(B, NH, NC, 64, 64, G, BF, mlp=False, backward=True, impl="mfma") == "mfma"
    d = round_acts(O.make_inputs("linear", B, NH, NC, 64, 64, seed=99 + NC), BF)
    out, cks, g = run_lin64(e, d, G, "mfma")
    ro, rc, rg = oracle_on(d, G, "linear")
    errs = check_vs_oracle(out, cks, g, ro, rc, rg, 1e-2, 3e-2, what=f"mfma linear CS=64 {shape}")
    print("mfma linear cs64 errors", shape, {k: round(v[0], 5) for k, v in errs.items()})
    og, cg, gg = run_lin64(e, d, G, "generic")
    assert rel_l2(out, og) < 1e-2 and rel_l2(cks[0], cg[0]) < 1e-2 and rel_l2(cks[1], cg[1]) < 1e-2
    for k in g:
        assert rel_l2(g[k], gg[k]) < 3e-2, k


def _scan(e, regime):
    kind, CS, B, NH, NC, G, seed = C.MFMA_CASES["lin64_b2"]
    c = C.scan_case(kind, B, NH, C.run_steps(kind, NC, G), CS, seed, regime)
    n, K = c["XQ"].shape[2], -(-c["XQ"].shape[2] // G)
    X = [c[k].to(DEV, BF).contiguous() for k in ("XQ", "XK", "XV", "eta")]
    ln = [c[k].reshape(NH, 64).to(DEV, torch.float32).contiguous() for k in ("ln_w", "ln_b")]
    st = [c[k].to(DEV, torch.float32).contiguous() for k in C.STATE[kind]]
    bufs = {"out": guarded((B, NH, n, CS, 64), BF), "W1": guarded((B, NH, K, 64, 64), torch.float32),
            "b1": guarded((B, NH, K, 1, 64), torch.float32)}
    e.ttt_linear_forward_impl("mfma", *X, *ln, *st, bufs["W1"][1], bufs["b1"][1], bufs["out"][1], G)
    torch.cuda.synchronize()
    assert_written_inside(bufs, f"lin64_b2 mfma {regime}")
    for s, k in zip(st, C.STATE[kind]):
        assert torch.equal(s.cpu().double(), c[k]), f"the initial state {k} was written"
    return c, bufs["out"][1].cpu(), {k: bufs[k][1].cpu() for k in C.STATE[kind]}, G


@pytest.mark.parametrize("regime", ["base", "high"])
def test_mfma_linear_cs64_scan_one_step_at_a_time(regime):
    """the case ``lin64_b2`` with ``impl="mfma"``: every step's state delta and output against the fp64 step from the scan's own
    checkpoint at SCAN_TOL; in the high regime every must-catch mutation written into the oracle side must fail its metric"""
    e = ext()
    c, out, cks, G = _scan(e, regime)
    C.assert_initial_state(c, cks)
    m = C.compare(c, out, cks, G, None)
    print(f"lin64_b2 mfma {regime}: {C.fmt(m)}")
    bad = {k: (v, SCAN_TOL[k]) for k, v in m.items() if not v < SCAN_TOL[k]}
    assert not bad, bad
    if regime == "high":
        for mut, metric in C.MUTATIONS.items():
            if metric is None or mut == "no_b2":
                continue
            mm = C.compare(c, out, cks, G, None, how=mut)
            print(f"lin64_b2 mfma {mut:20s} {metric}: {mm[metric]:.3g} (threshold {SCAN_TOL[metric]:.3g})")
            assert mm[metric] > SCAN_TOL[metric], (mut, mm)


def test_mfma_linear_cs64_deterministic_and_head_equivariant():
    """two runs give equal bits; a head permutation of the inputs permutes outputs and gradients exactly"""
    e = ext()
    NH, G = 5, 3
    d = round_acts(O.make_inputs("linear", 1, NH, 8, 64, 64, seed=6), BF)
    o1, c1, g1 = run_lin64(e, d, G, "mfma")
    o2, c2, g2 = run_lin64(e, d, G, "mfma")
    assert torch.equal(o1, o2) and torch.equal(c1[0], c2[0]) and torch.equal(c1[1], c2[1])
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    perm = torch.randperm(NH, generator=torch.Generator().manual_seed(1))
    hp = {k: (v[:, perm] if k in ("XQ", "XK", "XV", "eta", "dOut") else v[perm]) for k, v in d.items()}
    op, _, gp = run_lin64(e, hp, G, "mfma")
    assert torch.equal(op, o1[:, perm])
    for k in ("dXQ", "dXK", "dXV", "dlast_eta", "dW1", "db1", "dln_w", "dln_b"):
        assert torch.equal(gp[k], g1[k][:, perm]), k


def test_mfma_linear_cs64_training_geometry():
    """NH = 48, NC = 282 (3 s of video at mini-batches of 64), G = the training config's group size: everything finite; head by
    head agreement with the generic kernels over the first 8 mini-batches"""
    from ttt_amd.models.configs import ModelConfig
    e = ext()
    NH, NC, G = 48, 282, int(ModelConfig.__dataclass_fields__["scan_checkpoint_group_size"].default)
    d = round_acts(O.make_inputs("linear", 1, NH, NC, 64, 64, seed=4), BF)
    out, _, g = run_lin64(e, d, G, "mfma")
    assert torch.isfinite(out.float()).all() and all(torch.isfinite(v.float()).all() for v in g.values())
    head = {k: (v[:, :, :8] if k in ("XQ", "XK", "XV", "eta", "dOut") else v) for k, v in d.items()}
    o_m, _, g_m = run_lin64(e, head, G, "mfma")
    o_g, _, g_g = run_lin64(e, head, G, "generic")
    assert _per_head(o_m, o_g).max() < 1e-2
    for k in ("dXQ", "dXK", "dXV", "dW1"):
        err = _per_head(g_m[k], g_g[k])
        print("linear cs64", k, "per-head rel-L2 vs generic: median %.2e max %.2e" % (err.median().item(), err.max().item()))
        assert err.max() < 3e-2, k


def test_layer_with_cs64_impl_switch():
    """a small TTT-Linear layer (bf16, mini_batch_size 64, 2 heads, L = 4 x 64 video tokens + 64 text tokens) forward + backward with
    ``HipLinear.cs64_impl`` = "mfma" and "auto": outputs within 1e-2, input / parameter gradients within 3e-2.  The "mfma" arm must
    hand ``impl="mfma"`` to the scan and to the sweep, the "auto" arm must not, and the two families never give equal bits"""
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm.linear_hip import HipLinear
    from ttt_amd.models.ssm.ttt_layer import TTTWrapper
    e = ext()
    gold = load_golden("mod_lin_cfg1.pt")
    assert gold["cfg"]["mini_batch_size"] == 64 and gold["cfg"]["num_heads"] == 2
    m = TTTWrapper(ModelConfig(**gold["cfg"]))
    m.load_state_dict(gold["state_dict"], strict=True)
    m = m.to(DEV).to(BF)
    meta = SequenceMetadata(t_emb=torch.zeros(1, 512, device=DEV), text_length=64, seq_text_length=64, num_frames=8, num_chunks=1,
                            tokens_per_frame=32, latent_height=4, latent_width=8)
    gen = torch.Generator().manual_seed(11)
    L = 4 * 64 + 64
    x0, dy = torch.randn(1, L, 128, generator=gen), torch.randn(1, L, 128, generator=gen)
    res, old, asked = {}, HipLinear.cs64_impl, {"mfma": [], "auto": []}
    real = e.ttt_linear_forward_impl, e.ttt_linear_backward_impl
    try:
        for impl in ("mfma", "auto"):
            HipLinear.cs64_impl = impl
            e.ttt_linear_forward_impl = lambda sel, *a, _to=asked[impl]: (_to.append(("fwd", sel, a[0].shape[3])), real[0](sel, *a))[1]
            e.ttt_linear_backward_impl = lambda sel, *a, _to=asked[impl]: (_to.append(("bwd", sel, a[0].shape[3])), real[1](sel, *a))[1]
            m.zero_grad(set_to_none=True)
            x = x0.to(DEV, BF).requires_grad_(True)
            y = m(x, meta)
            y.backward(dy.to(DEV, BF))
            torch.cuda.synchronize()
            res[impl] = (y.detach(), x.grad.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    finally:
        HipLinear.cs64_impl = old
        e.ttt_linear_forward_impl, e.ttt_linear_backward_impl = real
    assert asked["mfma"] == [("fwd", "mfma", 64), ("bwd", "mfma", 64)], asked
    assert all(sel is None for _, sel, _ in asked["auto"]), asked
    assert not torch.equal(res["mfma"][0], res["auto"][0]) and not torch.equal(res["mfma"][1], res["auto"][1])
    assert res["auto"][2], "no parameter gradient"
    errs = {"y": rel_l2(res["mfma"][0], res["auto"][0]), "dx": rel_l2(res["mfma"][1], res["auto"][1])}
    for k, v in res["auto"][2].items():
        errs[k] = rel_l2(res["mfma"][2][k], v)
    print("layer cs64_impl mfma vs auto:", {k: round(v, 5) for k, v in errs.items()})
    assert errs["y"] < 1e-2, errs
    bad = {k: v for k, v in errs.items() if not v < 3e-2}
    assert not bad, (bad, errs)


@pytest.mark.parametrize("backward", [False, True])
def test_auto_still_resolves_cs64_linear_to_generic(backward):
    e = ext()
    assert e.get_impl() == "auto"
    assert e.resolved_impl(1, 48, 282, 64, 64, 16, BF, mlp=False, backward=backward) == "generic"
    assert e.resolved_impl(1, 48, 282, 64, 64, 16, BF, mlp=False, backward=backward, impl="auto") == "generic"
