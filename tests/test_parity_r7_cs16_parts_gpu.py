"""The sampling forward in parts, on the device: the TTT-MLP scan at mini-batches of 16 continued from a state
(``ttt_hip_mlp_forward_chunk`` at CS = 16, csrc/ttt_mlp16_body.h ``forward_part``) and the layer forward that uses it under
``no_grad`` (ttt_amd/models/ssm/pipeline.py, ``TTTBase._pipeline_plan``)."""
import pytest
import torch

from helpers import rel_l2
from oracle import ttt_oracle as O
from test_kernels_gpu import DEV, ext, round_acts
from test_parity_r2_gpu import check_per_head

pytestmark = pytest.mark.gpu


def _dev_inputs(d, NH):
    XQ, XK, XV = (d[k].to(DEV, torch.bfloat16).contiguous() for k in ("XQ", "XK", "XV"))
    le = d["eta"][:, :, :, -1, :, None].to(DEV, torch.bfloat16).contiguous()
    lw, lb = d["ln_w"].reshape(1, NH, 1, 64).to(DEV), d["ln_b"].reshape(1, NH, 1, 64).to(DEV)
    B = XQ.shape[0]
    st = [d[k].unsqueeze(0).expand(B, *d[k].shape).to(DEV, torch.float32).contiguous() for k in ("W1", "b1", "W2", "b2")]
    return XQ, XK, XV, le, lw, lb, st


def _bufs(B, NH, NC, K):
    nan = lambda *s: torch.full(s, float("nan"), device=DEV, dtype=torch.float32)
    cks = (nan(B, NH, K, 64, 256), nan(B, NH, K, 1, 256), nan(B, NH, K, 256, 64), nan(B, NH, K, 1, 64))
    return cks, torch.full((B, NH, NC, 16, 64), float("nan"), device=DEV, dtype=torch.bfloat16)


def _one_call_and_parts(e, d, B, NH, NC, G, cuts):
    """-> (out, cks) of ttt_forward, (out, cks, final state) of ONE chunk call over [0, NC), the same of the parts `cuts`"""
    XQ, XK, XV, le, lw, lb, st = _dev_inputs(d, NH)
    K = -(-NC // G)
    cks0, out0 = _bufs(B, NH, NC, K)
    e.ttt_forward(XQ, XK, XV, le, lw, lb, *st, *cks0, out0, G)
    res = [(out0, cks0, None)]
    for cc in ((0, NC), cuts):
        cks, out = _bufs(B, NH, NC, K)
        state = [t.clone() for t in st]                      # carried in place: every part replaces it
        for s0, s1 in zip(cc[:-1], cc[1:]):
            e.ttt_forward_chunk(XQ, XK, XV, le, lw, lb, *state, *cks, out, G, s0, s1 - s0)
        res.append((out, cks, state))
    torch.cuda.synchronize()
    return res


def _assert_same_bits(res, what):
    (out0, cks0, _), (out1, cks1, st1), (outp, cksp, stp) = res
    assert not torch.isnan(outp.float()).any() and not any(torch.isnan(t).any() for t in cksp + tuple(stp)), what
    assert torch.equal(out1, out0) and all(torch.equal(a, b) for a, b in zip(cks1, cks0)), f"{what}: one chunk call over [0, NC) vs ttt_forward"
    assert torch.equal(outp, out0), f"{what}: output"
    for n, a, b in zip(("W1c", "b1c", "W2c", "b2c"), cksp, cks0):
        assert torch.equal(a, b), f"{what}: checkpoint {n}"
    for n, a, b in zip(("W1", "b1", "W2", "b2"), stp, st1):
        assert torch.equal(a, b), f"{what}: final state {n}"
    assert not any(torch.equal(a, b) for a, b in zip(stp, [c[:, :, 0] for c in cks0])), "the state did not move"


def test_cs16_scan_in_parts_small_off_group_boundaries():
    """B = 2, NH = 3, 11 steps, G = 3 (ragged last group), cut at 1, 2, 7: no cut on a group boundary but 0, parts of one step -
    output, all four checkpoints and the final state carry the bits of the one-call forward."""
    e = ext()
    B, NH, NC, G = 2, 3, 11, 3
    d = round_acts(O.make_inputs("mlp", B, NH, NC, 16, 64, seed=811), torch.bfloat16)
    assert e.resolved_impl(B, NH, NC, 16, 64, G, torch.bfloat16, mlp=True, backward=False) == "mfma"
    _assert_same_bits(_one_call_and_parts(e, d, B, NH, NC, G, (0, 1, 2, 7, 11)), "NC=11 G=3")


def test_cs16_scan_in_parts_at_63s_length_bits_and_oracle():
    """The geometry of test_mfma_cs16_at_63s_length_vs_oracle (B = 1, NH = 2, 21 948 mini-batches of 16, ONE checkpoint group):
    parts of whole multiples of the 256-step quantum plus the ragged tail (188 steps), the state carried in place - output, the
    checkpoint and the final state ``torch.equal`` to the one-call forward (on the device the two orientations of W2 come from
    mirrored MFMA calls; a restart fills both from one array - this is the check that they are exact transposes there).  Then the
    run in parts against the fp64 oracle at the tolerances of that test (1e-2 / 3e-2 per head), whole and last tenth."""
    e = ext()
    NH, NC = 2, 21948
    G = NC
    d = round_acts(O.make_inputs("mlp", 1, NH, NC, 16, 64, seed=5000 + NC), torch.bfloat16)
    assert e.resolved_impl(1, NH, NC, 16, 64, G, torch.bfloat16, mlp=True, backward=False) == "mfma"
    q = 256
    cuts = (0, 12 * q, 24 * q, 25 * q, 60 * q, 85 * q, NC)
    assert NC - 85 * q == 188
    res = _one_call_and_parts(e, d, 1, NH, NC, G, cuts)
    _assert_same_bits(res, f"NC={NC} G=NC")
    out = res[2][0]
    d64 = {k: v.double() for k, v in d.items()}
    ro, _, _ = O.mlp_forward(d64["XQ"], d64["XK"], d64["XV"], d64["eta"][:, :, :, -1, :, None], d64["ln_w"], d64["ln_b"],
                             *[d64[k].unsqueeze(0) for k in ("W1", "b1", "W2", "b2")], G)
    tail = NC - NC // 10
    print(f"mlp CS=16 NC={NC} in {len(cuts) - 1} parts: whole {rel_l2(out, ro):.2e}, last tenth {rel_l2(out[:, :, tail:], ro[:, :, tail:]):.2e}")
    check_per_head(f"TTT-mlp CS=16 MFMA forward in parts NC={NC}", out, (), {}, ro, (), {}, 1e-2, 3e-2)
    check_per_head(f"TTT-mlp CS=16 MFMA forward in parts NC={NC}, last tenth", out[:, :, tail:], (), {}, ro[:, :, tail:], (), {}, 1e-2, 3e-2)


def test_cs16_forward_chunk_refuses_parts_outside_the_sequence():
    e = ext()
    B, NH, NC, G = 1, 2, 5, 5
    d = round_acts(O.make_inputs("mlp", B, NH, NC, 16, 64, seed=3), torch.bfloat16)
    XQ, XK, XV, le, lw, lb, st = _dev_inputs(d, NH)
    cks, out = _bufs(B, NH, NC, 1)
    for s0, ns in ((-1, 2), (0, 0), (3, 3), (5, 1)):
        with pytest.raises(RuntimeError, match=r"inside \[0, NC\)"):
            e.ttt_forward_chunk(XQ, XK, XV, le, lw, lb, *st, *cks, out, G, s0, ns)
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()                     # nothing was launched


# ------------------------------------------------------------------------------------------------------------- layer level
def _count_calls(monkeypatch, e):
    from ttt_amd.models.ssm import pipeline
    calls = {"prepass": 0, "chunk": 0, "one_call": 0}
    orig_prepass, orig_chunk, orig_fwd = pipeline.prepass, e.ttt_forward_chunk, e.ttt_forward

    def prepass(*a, **k):
        calls["prepass"] += 1
        return orig_prepass(*a, **k)

    def chunk(*a):
        calls["chunk"] += 1
        return orig_chunk(*a)

    def one_call(*a):
        calls["one_call"] += 1
        return orig_fwd(*a)

    monkeypatch.setattr(pipeline, "prepass", prepass)
    monkeypatch.setattr(e, "ttt_forward_chunk", chunk)
    monkeypatch.setattr(e, "ttt_forward", one_call)
    return calls


def test_cs16_layer_forward_pipelined_under_no_grad(monkeypatch):
    """A TTT-MLP layer at mini-batches of 16 with the sampling settings (one checkpoint group), 3 interleaved scenes, 33 888 tokens =
    2 118 mini-batches (>= pipeline.CS16_MIN_STEPS), batch 2, both scan directions.  Under ``no_grad`` the DEFAULT forward is the
    pipeline: the pre-pass ran, the scans arrived as chunk launches, no one-call forward; against the one-piece forward
    (pipeline_parts = 0) rel-L2 < 1e-2 (the figure of the same comparison at CS = 64, tests/test_parity_r6_gpu.py: the scan parts carry
    the one-call bits, the GEMMs run per token run).  With grad enabled the same layer makes no chunk launch."""
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm import pipeline
    from ttt_amd.models.ssm.ttt_layer import TTTWrapper
    e = ext()
    scenes, tl, frames, tpf = 3, 32, 66, 512
    cfg = ModelConfig(model_dim=128, num_heads=2, num_layers=1, mini_batch_size=16, latent_height=16, latent_width=32,
                      compressed_num_frames=frames, ssm_layer="ttt_mlp", scan_checkpoint_group_size=10 ** 6, ttt_base_lr=1.0)
    torch.manual_seed(0)
    m = TTTWrapper(cfg)
    m.ttt.init_weights()
    m = m.to(DEV).to(torch.bfloat16)
    m.init_freqs()
    meta = SequenceMetadata(text_length=tl, seq_text_length=tl * scenes, num_frames=frames, num_chunks=scenes, tokens_per_frame=tpf,
                            latent_height=16, latent_width=32, t_emb=None)
    meta.init_multiscene_offsets()
    L = scenes * tl + frames * tpf
    assert L % 16 == 0 and L // 16 >= pipeline.CS16_MIN_STEPS
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(2, L, 128, device=DEV, generator=g).bfloat16()
    assert m.ttt.pipeline_parts >= 2, "the library default must be the pipelined forward"
    calls = _count_calls(monkeypatch, e)
    for reverse in (False, True):
        before = dict(calls)
        with torch.no_grad():
            y1 = m(x, meta, reverse)
        torch.cuda.synchronize()
        assert calls["prepass"] == before["prepass"] + 1 and calls["chunk"] >= before["chunk"] + 2 and calls["one_call"] == before["one_call"], calls
        saved = m.ttt.pipeline_parts
        m.ttt.pipeline_parts = 0
        try:
            before = dict(calls)
            with torch.no_grad():
                y0 = m(x, meta, reverse)
            torch.cuda.synchronize()
        finally:
            m.ttt.pipeline_parts = saved
        assert calls["chunk"] == before["chunk"] and calls["one_call"] == before["one_call"] + 1, calls
        err = rel_l2(y1, y0.double())
        print(f"CS=16 layer forward, reverse={reverse}: pipelined vs one piece rel-L2 {err:.2e} (equal: {torch.equal(y1, y0)})", calls)
        assert torch.isfinite(y1.float()).all() and float(y0.float().norm()) > 0
        assert err < 1e-2, err
    before = dict(calls)
    y = m(x.clone().requires_grad_(True), meta, False)          # grad enabled: one piece
    torch.cuda.synchronize()
    assert y.requires_grad
    assert calls["chunk"] == before["chunk"] and calls["prepass"] == before["prepass"], calls


def test_cs16_denoising_step_default_vs_one_piece(monkeypatch):
    """One denoising step (the classifier-free-guidance pair as a batch of two) of a small DiT through the DPM-Solver++ sampler of
    ttt_amd/models/cogvideo/sampling.py, TTT-MLP at mini-batches of 16, 3 scenes (37 frames of 960 tokens in attention segments of
    12 + 1 frames, 3 x 32 text tokens: 35 616 tokens = 2 226 mini-batches): the default (pipelined: 2 layers
    x 2 directions pre-passes, no one-call scan) against pipeline_parts = 0, rel-L2 < 1e-2."""
    from ttt_amd.models.cogvideo.dit import DiffusionTransformer
    from ttt_amd.models.cogvideo.sampling import DiscreteDenoiser, VPSDEDPMPP2MSampler
    from ttt_amd.models.configs import ModelConfig
    e = ext()
    frames, scenes, tl = 37, 3, 32
    cfg = ModelConfig(model_dim=512, num_heads=8, num_layers=2, mini_batch_size=16, latent_height=24, latent_width=40,
                      compressed_num_frames=frames, ssm_layer="ttt_mlp", adapter_method="sft", time_embed_dim=512, text_dim=64,
                      scan_checkpoint_group_size=10 ** 6)
    torch.manual_seed(0)
    net = DiffusionTransformer(cfg)
    with torch.no_grad():
        for _, p in net.named_parameters():
            if p.ndim >= 2:
                p.normal_(0, 0.02)
    net = net.to(DEV).to(torch.bfloat16).eval()
    for mod in net.modules():
        if hasattr(mod, "init_freqs"):
            mod.init_freqs()
    g = torch.Generator(device=DEV).manual_seed(7)
    noise = torch.randn(1, frames, 16, 48, 80, device=DEV, generator=g)
    text = torch.randn(1, scenes, tl, 64, device=DEV, generator=g).bfloat16()
    neg = torch.randn(1, scenes, tl, 64, device=DEV, generator=g).bfloat16()

    def step():
        sampler = VPSDEDPMPP2MSampler(denoiser=DiscreteDenoiser(net, num_idx=1000, quantize_c_noise=False, dtype=torch.bfloat16),
                                      discretization_config={"shift_scale": 1.0}, guider_config={"scale": 6, "exp": 5, "num_steps": 1},
                                      device=DEV, num_steps=1)
        torch.manual_seed(99)
        with torch.no_grad():
            out = sampler(noise, {"crossattn": text}, {"crossattn": neg})
        torch.cuda.synchronize()
        return out

    calls = _count_calls(monkeypatch, e)
    o1 = step()
    assert calls["prepass"] == 4 and calls["chunk"] >= 8 and calls["one_call"] == 0, calls
    for mod in net.modules():
        if hasattr(mod, "pipeline_parts"):
            mod.pipeline_parts = 0
    o0 = step()
    assert calls["prepass"] == 4 and calls["one_call"] == 4, calls
    err = rel_l2(o1, o0.double())
    print(f"CS=16 denoising step, default vs one piece: rel-L2 {err:.2e} (equal: {torch.equal(o1, o0)})", calls)
    assert torch.isfinite(o1).all() and err < 1e-2, err
