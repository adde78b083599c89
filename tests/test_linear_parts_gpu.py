"""TTT-Linear forward in parts, on the device: the MFMA scans at mini-batches of 16 and of 64 continued from a state
(``ttt_hip_linear_forward_chunk`` of include/ttt_hip_parts.h; ``forward_part`` of csrc/ttt_lin16_body.h / ttt_lin64_body.h) and the
opt-in layer forward that uses them (``TTTBase.linear_pipeline_parts``, ttt_amd/models/ssm/pipeline.py)."""
import pytest
import torch

from helpers import rel_l2
from oracle import ttt_oracle as O
from test_kernels_gpu import DEV, ext, round_acts
from test_scan_oracle_gpu import GUARD, assert_written_inside, guarded

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------- scan level
def _dev_inputs(d, B):
    X = [d[k].to(DEV, BF).contiguous() for k in ("XQ", "XK", "XV")]
    le = d["eta"][:, :, :, -1, :, None].to(DEV, BF).contiguous()
    ln = [d[k].to(DEV, torch.float32).contiguous() for k in ("ln_w", "ln_b")]
    st = [d[k].unsqueeze(0).expand(B, *d[k].shape).to(DEV, torch.float32).contiguous() for k in ("W1", "b1")]
    return X, le, ln, st


def _bufs(B, NH, NC, CS, K):
    return {"out": guarded((B, NH, NC, CS, 64), BF), "W1c": guarded((B, NH, K, 64, 64), torch.float32),
            "b1c": guarded((B, NH, K, 1, 64), torch.float32)}


def _walk(e, impl, X, le, ln, st, G, B, NH, NC, CS, cuts):
    """the scan as the parts the cuts make, the state (between guards too) carried in place -> out, W1c, b1c, final state.  A walk that
    stops short of NC leaves the rest of its buffers NaN: the guards and the written / unwritten steps of the output are checked then."""
    bufs = _bufs(B, NH, NC, CS, -(-NC // G))
    bufs["W1"], bufs["b1"] = guarded(tuple(st[0].shape), torch.float32), guarded(tuple(st[1].shape), torch.float32)
    state = [bufs["W1"][1], bufs["b1"][1]]
    state[0].copy_(st[0]), state[1].copy_(st[1])
    for s0, s1 in zip(cuts[:-1], cuts[1:]):
        e.ttt_linear_forward_chunk(impl, *X, le, *ln, *state, bufs["W1c"][1], bufs["b1c"][1], bufs["out"][1], G, s0, s1 - s0)
    torch.cuda.synchronize()
    if cuts[-1] == NC:
        assert_written_inside(bufs, f"parts {cuts}")
    else:
        for name, (buf, view) in bufs.items():
            assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"parts {cuts}: write outside {name}"
        out = bufs["out"][1]
        assert not torch.isnan(out[:, :, :cuts[-1]].float()).any() and bool(torch.isnan(out[:, :, cuts[-1]:].float()).all())
    return bufs["out"][1], bufs["W1c"][1], bufs["b1c"][1], state


@pytest.mark.parametrize("CS,impl,B,NH,NC,G,cuts", [(16, None, 2, 5, 11, 3, (0, 1, 2, 7, 11)), (64, "mfma", 2, 3, 7, 3, (0, 1, 2, 6, 7))])
def test_linear_scan_in_parts_carries_the_one_call_bits(CS, impl, B, NH, NC, G, cuts):
    """CS = 16 under the global selector (auto): 10 scans = a ragged last workgroup of the four-scans-per-workgroup kernel, no cut on a
    checkpoint-group boundary, a ragged last group.  CS = 64 on request.  One chunk call over [0, NC) and the parts each carry the bits
    of the one-call forward (output, both checkpoints), their final states are equal, the state that leaves [0, 6) is checkpoint 2,
    the state moved, and nothing is written outside the guards around the outputs, the checkpoints and the carried state."""
    e = ext()
    assert e.get_impl() == "auto"
    assert e.resolved_impl(B, NH, NC, CS, 64, G, BF, mlp=False, backward=False, impl=impl) == "mfma"
    d = round_acts(O.make_inputs("linear", B, NH, NC, CS, 64, seed=900 + CS), BF)
    X, le, ln, st = _dev_inputs(d, B)
    keep = [t.clone() for t in st]
    one = _bufs(B, NH, NC, CS, -(-NC // G))
    e.ttt_linear_forward_impl(impl, *X, le, *ln, *st, one["W1c"][1], one["b1c"][1], one["out"][1], G)
    torch.cuda.synchronize()
    assert_written_inside(one, "one call")
    assert torch.equal(st[0], keep[0]) and torch.equal(st[1], keep[1]), "the one-call forward wrote its initial state"
    out0, W1c0, b1c0 = (one[k][1] for k in ("out", "W1c", "b1c"))
    whole = _walk(e, impl, X, le, ln, st, G, B, NH, NC, CS, (0, NC))
    parts = _walk(e, impl, X, le, ln, st, G, B, NH, NC, CS, cuts)
    for what, (out, W1c, b1c, state) in (("one chunk call over [0, NC)", whole), (f"parts {cuts}", parts)):
        assert torch.equal(out, out0), f"{what}: output"
        assert torch.equal(W1c, W1c0) and torch.equal(b1c, b1c0), f"{what}: checkpoints"
    assert torch.equal(parts[3][0], whole[3][0]) and torch.equal(parts[3][1], whole[3][1]), "final state"
    assert not torch.equal(whole[3][0], keep[0]) and not torch.equal(whole[3][1], keep[1]), "the state did not move"
    assert 6 < NC and 6 // G == 2
    head = _walk(e, impl, X, le, ln, st, G, B, NH, NC, CS, (0, 6))
    assert torch.equal(head[3][0], W1c0[:, :, 2]) and torch.equal(head[3][1], b1c0[:, :, 2]), "the state leaving [0, 6) is checkpoint 2"


@pytest.mark.parametrize("CS,impl", [(16, None), (64, "mfma")])
def test_linear_forward_chunk_refuses_parts_outside_the_sequence(CS, impl):
    e = ext()
    B, NH, NC, G = 1, 2, 5, 2
    d = round_acts(O.make_inputs("linear", B, NH, NC, CS, 64, seed=3), BF)
    X, le, ln, st = _dev_inputs(d, B)
    bufs = _bufs(B, NH, NC, CS, 3)
    for s0, ns in ((-1, 2), (0, 0), (3, 3), (5, 1), (2 ** 31 - 1, 2)):
        with pytest.raises(RuntimeError, match=r"inside \[0, NC\)"):
            e.ttt_linear_forward_chunk(impl, *X, le, *ln, *st, bufs["W1c"][1], bufs["b1c"][1], bufs["out"][1], G, s0, ns)
    if CS == 64:        # under auto the generic kernels would run this geometry: they do not continue from a state
        with pytest.raises(RuntimeError, match="only the MFMA scan"):
            e.ttt_linear_forward_chunk(None, *X, le, *ln, *st, bufs["W1c"][1], bufs["b1c"][1], bufs["out"][1], G, 0, 2)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(buf.float()).all()) for buf, _ in bufs.values())          # nothing was launched


# ------------------------------------------------------------------------------------------------------------- layer level
def _count_calls(monkeypatch, e):
    from ttt_amd.models.ssm import pipeline
    calls = {"prepass": 0, "chunk": 0, "one_call": 0, "chunk_impl": set()}
    orig = pipeline.prepass, e.ttt_linear_forward_chunk, e.ttt_linear_forward, e.ttt_linear_forward_impl

    def prepass(*a, **k):
        calls["prepass"] += 1
        return orig[0](*a, **k)

    def chunk(impl, *a):
        calls["chunk"] += 1
        calls["chunk_impl"].add(impl)
        return orig[1](impl, *a)

    def one_call(*a):
        calls["one_call"] += 1
        return orig[3](None, *a)

    def one_call_impl(*a):
        calls["one_call"] += 1
        return orig[3](*a)

    monkeypatch.setattr(pipeline, "prepass", prepass)
    monkeypatch.setattr(e, "ttt_linear_forward_chunk", chunk)
    monkeypatch.setattr(e, "ttt_linear_forward", one_call)
    monkeypatch.setattr(e, "ttt_linear_forward_impl", one_call_impl)
    return calls


def _layer(CS, G, L, scenes):
    """a TTT-Linear TTTWrapper (model_dim 128, 2 heads, bf16) and the metadata of a sequence of L tokens: ``scenes`` x 32 text tokens (one
    scene: 64) + frames of 32 tokens"""
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm.ttt_layer import TTTWrapper
    tl = 64 if scenes == 1 else 32
    frames = (L - scenes * tl) // 32
    assert scenes * tl + frames * 32 == L and L % CS == 0
    cfg = ModelConfig(model_dim=128, num_heads=2, num_layers=1, mini_batch_size=CS, latent_height=4, latent_width=8,
                      compressed_num_frames=frames, ssm_layer="ttt_linear", scan_checkpoint_group_size=G, ttt_base_lr=1.0)
    torch.manual_seed(0)
    m = TTTWrapper(cfg)
    m.ttt.init_weights()
    m = m.to(DEV).to(BF)
    m.init_freqs()
    meta = SequenceMetadata(text_length=tl, seq_text_length=tl * scenes, num_frames=frames, num_chunks=scenes, tokens_per_frame=32,
                            latent_height=4, latent_width=8, t_emb=None)
    if scenes > 1:
        meta.init_multiscene_offsets()
    return m, meta


def _run(m, meta, x0, dy, reverse, grad):
    """forward (+ backward) -> y, dx, {parameter: gradient}"""
    m.zero_grad(set_to_none=True)
    if not grad:
        with torch.no_grad():
            y = m(x0, meta, reverse)
        torch.cuda.synchronize()
        return y, None, {}
    x = x0.clone().requires_grad_(True)
    y = m(x, meta, reverse)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), x.grad.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _parts_vs_one_piece(monkeypatch, CS, G, L, scenes, switch, grad, want_parts=True):
    """the layer with the switch on against the switch-off run, both scan directions: the pre-pass ran and the scan arrived as >= 2 chunk
    launches and no one-call forward (``want_parts`` False: the other way round); output within 1e-2, input / parameter gradients within
    3e-2 (the project's bounds, SURVEY.md 8c, as in test_layer_with_cs64_impl_switch).  Switch off: never a chunk launch."""
    e = ext()
    m, meta = _layer(CS, G, L, scenes)
    assert m.ttt.linear_pipeline_parts == 0, "the switch must be off by default"
    gen = torch.Generator().manual_seed(11)
    x0, dy = (torch.randn(1, L, 128, generator=gen).to(DEV, BF) for _ in range(2))
    calls = _count_calls(monkeypatch, e)
    for reverse in (False, True):
        before = dict(calls)
        y0, dx0, g0 = _run(m, meta, x0, dy, reverse, grad)
        assert calls["chunk"] == before["chunk"] and calls["prepass"] == before["prepass"] and calls["one_call"] == before["one_call"] + 1, calls
        m.ttt.linear_pipeline_parts = switch
        try:
            before = dict(calls)
            y1, dx1, g1 = _run(m, meta, x0, dy, reverse, grad)
        finally:
            m.ttt.linear_pipeline_parts = 0
        if not want_parts:
            assert calls["chunk"] == before["chunk"] and calls["prepass"] == before["prepass"] and calls["one_call"] == before["one_call"] + 1, calls
        else:
            assert calls["prepass"] == before["prepass"] + 1 and calls["chunk"] >= before["chunk"] + 2 and calls["one_call"] == before["one_call"], calls
        assert torch.isfinite(y1.float()).all() and float(y0.float().norm()) > 0
        errs = {"y": rel_l2(y1, y0.double())}
        if grad:
            assert g0 and sorted(g0) == sorted(g1), "parameter gradients"
            errs["dx"] = rel_l2(dx1, dx0.double())
            errs.update({k: rel_l2(g1[k], v.double()) for k, v in g0.items()})
        print(f"TTT-Linear layer CS={CS} G={G} scenes={scenes} reverse={reverse} grad={grad}: parts vs one piece",
              {k: float(f"{v:.2e}") for k, v in errs.items()}, {k: v for k, v in calls.items()})
        assert errs["y"] < 1e-2, errs
        bad = {k: v for k, v in errs.items() if not v < 3e-2}
        assert not bad, (bad, errs)
    return calls


@pytest.mark.parametrize("scenes", [1, 3])
def test_layer_in_parts_cs16_with_grad(monkeypatch, scenes):
    """(a) mini-batches of 16, G = 4, 640 tokens = 40 steps = 10 checkpoint groups, switch = 3, grad enabled: parts of whole groups; the
    MFMA backward reads the checkpoints the parts wrote"""
    calls = _parts_vs_one_piece(monkeypatch, 16, 4, 640, scenes, 3, grad=True)
    assert calls["chunk"] == 2 * 3 and calls["chunk_impl"] == {None}, calls


@pytest.mark.parametrize("scenes", [1, 3])
def test_layer_in_parts_cs16_one_group_no_grad(monkeypatch, scenes):
    """(b) the same under ``no_grad`` with ONE checkpoint group (sampling) and a step quantum of 8: the any-step cut at small size - 40
    steps = 5 quanta -> 2 parts"""
    from ttt_amd.models.ssm import pipeline
    monkeypatch.setattr(pipeline, "LIN_QUANTUM", 8)
    calls = _parts_vs_one_piece(monkeypatch, 16, 10 ** 6, 640, scenes, 3, grad=False)
    assert calls["chunk"] == 2 * 2, calls


@pytest.mark.parametrize("scenes", [1, 3])
def test_layer_in_parts_cs64_on_request(monkeypatch, scenes):
    """(c) mini-batches of 64 with ``HipLinear.cs64_impl = "mfma"``, G = 2, 704 tokens = 11 steps = 6 groups (the last one ragged),
    switch = 3, grad enabled; with "auto" the generic kernels run the scan and the layer stays one piece whatever the switch says"""
    from ttt_amd.models.ssm.linear_hip import HipLinear
    monkeypatch.setattr(HipLinear, "cs64_impl", "mfma")
    calls = _parts_vs_one_piece(monkeypatch, 64, 2, 704, scenes, 3, grad=True)
    assert calls["chunk"] == 2 * 3 and calls["chunk_impl"] == {"mfma"}, calls
    monkeypatch.setattr(HipLinear, "cs64_impl", "auto")
    _parts_vs_one_piece(monkeypatch, 64, 2, 704, scenes, 3, grad=True, want_parts=False)
