"""The TTT-MLP forward scan at mini-batches of 16 as a PAIR of workgroups per (b, h), on the device (``ttt_forward_pair16`` /
``ttt_forward_chunk_pair16`` -> ``ttt_hip_mlp_forward_chunk_pair16`` -> mlp_pair16_kernel, csrc/ttt_mlp16_pair_body.h).  Role A runs the
state chain of ``mlp16::forward_part`` and publishes the updated state per step; role B (another CU) runs the output path from those
records with the same calls in the same order.  So the pair form must return the BITS of the one-workgroup kernel (``ttt_forward`` /
``ttt_forward_chunk``) - outputs, all four checkpoint tensors, the state a part hands on - which the other GPU tests tie to the fp64
oracle."""
import pytest
import torch

from helpers import rel_l2
from oracle import ttt_oracle as O
from test_kernels_gpu import DEV, ext, round_acts
from test_parity_r7_cs16_parts_gpu import _bufs, _dev_inputs

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _inputs(B, NH, NC, seed):
    d = round_acts(O.make_inputs("mlp", B, NH, NC, 16, 64, seed=seed), BF16)
    return d, _dev_inputs(d, NH)


def _one_workgroup(e, t, B, NH, NC, G, cuts=None):
    XQ, XK, XV, le, lw, lb, st = t
    cks, out = _bufs(B, NH, NC, -(-NC // G))
    state = None
    if cuts is None:
        e.ttt_forward(XQ, XK, XV, le, lw, lb, *st, *cks, out, G)
    else:
        state = [s.clone() for s in st]
        for s0, s1 in zip(cuts[:-1], cuts[1:]):
            e.ttt_forward_chunk(XQ, XK, XV, le, lw, lb, *state, *cks, out, G, s0, s1 - s0)
    return out, cks, state


def _pair(e, t, B, NH, NC, G, cuts=None):
    """-> out, checkpoints, final state (parts only), [paired of every launch]"""
    XQ, XK, XV, le, lw, lb, st = t
    cks, out = _bufs(B, NH, NC, -(-NC // G))
    state = None
    if cuts is None:
        paired = [e.ttt_forward_pair16(XQ, XK, XV, le, lw, lb, *st, *cks, out, G)]
    else:
        state = [s.clone() for s in st]                      # carried in place; one workspace (the stream's) serves every launch
        paired = [e.ttt_forward_chunk_pair16(XQ, XK, XV, le, lw, lb, *state, *cks, out, G, s0, s1 - s0) for s0, s1 in zip(cuts[:-1], cuts[1:])]
    return out, cks, state, paired


def _assert_bits(got, want, what):
    out, cks = got[0], got[1]
    assert not torch.isnan(out.float()).any() and not any(torch.isnan(c).any() for c in cks), what
    assert torch.equal(out, want[0]), f"{what}: output"
    for n, a, b in zip(("W1c", "b1c", "W2c", "b2c"), cks, want[1]):
        assert torch.equal(a, b), f"{what}: checkpoint {n}"


# (1, 5, 1, 1): role B starts at block 8 ; (1, 2, 3, 16): NC < RING, NC < G ; (2, 3, 37, 4): ragged last group, nine ring wraps ;
# (1, 8, 600, 600): long enough for back-pressure ; (2, 48, 64, 16): the sampler's 192 workgroups
@pytest.mark.parametrize("B,NH,NC,G", [(1, 5, 1, 1), (1, 2, 3, 16), (2, 3, 37, 4), (1, 8, 600, 600), (2, 48, 64, 16)])
def test_pair16_has_the_bits_of_the_one_workgroup_scan(B, NH, NC, G):
    e = ext()
    assert e.resolved_impl(B, NH, NC, 16, 64, G, BF16, mlp=True, backward=False) == "mfma"
    _, t = _inputs(B, NH, NC, 40 + NC)
    want = _one_workgroup(e, t, B, NH, NC, G)
    for rep in range(2):                    # twice: the flag words are re-zeroed in front of every launch
        got = _pair(e, t, B, NH, NC, G)
        torch.cuda.synchronize()
        assert e.sweep_error() == 0
        assert got[3] == [True], "the pairs fit the device: they must have run"
        _assert_bits(got, want, f"run {rep}")
    # ... and the state behind the last step (fp32: a last-bit difference on the chain shows here long before it shows in bf16 outputs)
    want, got = _one_workgroup(e, t, B, NH, NC, G, (0, NC)), _pair(e, t, B, NH, NC, G, (0, NC))
    torch.cuda.synchronize()
    assert e.sweep_error() == 0 and got[3] == [True]
    for n, a, b in zip(("W1", "b1", "W2", "b2"), got[2], want[2]):
        assert torch.equal(a, b), f"final state {n}"


def test_pair16_in_parts_hands_on_the_same_state():
    """(1, 6, 45, 8) cut at 7, 8, 31: cuts on and off the group boundaries, a part of one step, the state in place and one workspace
    reused across the launches - outputs, checkpoints and the final state of the one-workgroup chunks"""
    e = ext()
    B, NH, NC, G, cuts = 1, 6, 45, 8, (0, 7, 8, 31, 45)
    _, t = _inputs(B, NH, NC, 7)
    want = _one_workgroup(e, t, B, NH, NC, G, cuts)
    got = _pair(e, t, B, NH, NC, G, cuts)
    torch.cuda.synchronize()
    assert e.sweep_error() == 0 and got[3] == [True] * 4
    _assert_bits(got, want, "parts")
    for n, a, b in zip(("W1", "b1", "W2", "b2"), got[2], want[2]):
        assert not torch.isnan(a).any() and torch.equal(a, b), f"final state {n}"
    assert not torch.equal(got[2][0], t[6][0]), "the state did not move"
    _assert_bits(got, _one_workgroup(e, t, B, NH, NC, G), "parts vs the one-call scan")


def test_pair16_that_does_not_fit_the_device_runs_the_one_workgroup_kernel():
    """both workgroups of every pair must be resident: with B * NH rounded up to 8, plus B * NH, just above the compute units the
    launch function enqueues the one-workgroup kernel and says so - same bits, no error"""
    e = ext()
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    n = next(n for n in range(1, 4096) if ((n + 7) & ~7) + n > cus)
    assert ((n - 1 + 7) & ~7) + n - 1 <= cus
    B, NH, NC, G = 1, n, 4, 2
    _, t = _inputs(B, NH, NC, 19)
    want = _one_workgroup(e, t, B, NH, NC, G)
    got = _pair(e, t, B, NH, NC, G)
    torch.cuda.synchronize()
    assert e.sweep_error() == 0 and got[3] == [False]
    _assert_bits(got, want, f"fallback at {n} (b, h) on {cus} compute units")


def test_pair16_on_a_side_stream_beside_a_busy_chip():
    """What the pipelined layer forward does: the scan on a side stream while GEMMs fill the other CUs (role-B workgroups are
    dispatched when CUs come free: role A runs up to RING steps ahead and waits) - same bits, no hand-over error."""
    e = ext()
    B, NH, NC, G = 2, 48, 96, 16
    _, t = _inputs(B, NH, NC, 23)
    want = _one_workgroup(e, t, B, NH, NC, G)
    a = torch.randn(8192, 8192, device=DEV, dtype=BF16)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(6):
        a @ a                                # ~ 0.9 ms each on the whole chip
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = _pair(e, t, B, NH, NC, G)
    for _ in range(12):
        a @ a
    torch.cuda.synchronize()
    assert e.sweep_error() == 0 and got[3] == [True]
    _assert_bits(got, want, "busy chip")


def test_pair16_vs_oracle():
    e = ext()
    B, NH, NC, G = 1, 4, 21, 4
    d, t = _inputs(B, NH, NC, 123)
    out, cks, _, paired = _pair(e, t, B, NH, NC, G)
    torch.cuda.synchronize()
    assert e.sweep_error() == 0 and paired == [True]
    d64 = {k: v.double() for k, v in d.items()}
    ro, rc, _ = O.mlp_forward(d64["XQ"], d64["XK"], d64["XV"], d64["eta"][:, :, :, -1, :, None], d64["ln_w"], d64["ln_b"],
                              *[d64[k].unsqueeze(0) for k in ("W1", "b1", "W2", "b2")], G)
    assert rel_l2(out, ro) < 1e-2
    for c, r in zip(cks, rc):
        assert rel_l2(c, r) < 1e-2


@pytest.mark.parametrize("piped", [False, True])
def test_layer_switch_keeps_the_bits(monkeypatch, piped):
    """The TTT-MLP layer under ``no_grad`` at mini-batches of 16 (the layer of test_cs16_layer_forward_pipelined_under_no_grad: 3
    scenes, 2 118 mini-batches, batch 2), one piece and pipelined: ``TTTBase.cs16_scan_pair`` = 1 reaches the pair entries - and only
    them - and returns the bits of the switch at 0."""
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm import pipeline
    from ttt_amd.models.ssm.ttt_layer import TTTBase, TTTWrapper
    e = ext()
    scenes, tl, frames, tpf = 3, 32, 66, 512
    cfg = ModelConfig(model_dim=128, num_heads=2, num_layers=1, mini_batch_size=16, latent_height=16, latent_width=32,
                      compressed_num_frames=frames, ssm_layer="ttt_mlp", scan_checkpoint_group_size=10 ** 6, ttt_base_lr=1.0)
    torch.manual_seed(0)
    m = TTTWrapper(cfg)
    m.ttt.init_weights()
    m = m.to(DEV).to(BF16)
    m.init_freqs()
    meta = SequenceMetadata(text_length=tl, seq_text_length=tl * scenes, num_frames=frames, num_chunks=scenes, tokens_per_frame=tpf,
                            latent_height=16, latent_width=32, t_emb=None)
    meta.init_multiscene_offsets()
    L = scenes * tl + frames * tpf
    assert L // 16 >= pipeline.CS16_MIN_STEPS
    x = torch.randn(2, L, 128, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11)).bfloat16()
    m.ttt.pipeline_parts = 5 if piped else 0
    calls = {}
    for name in ("ttt_forward", "ttt_forward_chunk", "ttt_forward_pair16", "ttt_forward_chunk_pair16"):
        def counted(*a, _f=getattr(e, name), _n=name):
            r = _f(*a)
            calls[_n] = calls.get(_n, 0) + 1
            assert r is not False, "the pairs of four (b, h) fit the device"
            return r
        monkeypatch.setattr(e, name, counted)
    ys = []
    for on in (0, 1):
        monkeypatch.setattr(TTTBase, "cs16_scan_pair", on)
        calls.clear()
        with torch.no_grad():
            ys.append(m(x, meta, False))
        torch.cuda.synchronize()
        want = ("ttt_forward_chunk" if piped else "ttt_forward") + ("_pair16" if on else "")
        assert list(calls) == [want] and (calls[want] >= 2 if piped else calls[want] == 1), calls
    assert e.sweep_error() == 0
    assert torch.isfinite(ys[1].float()).all() and float(ys[0].float().norm()) > 0
    assert torch.equal(ys[0], ys[1])
