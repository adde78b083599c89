"""The plan of the TTT-Linear layer's forward in parts (``TTTBase.linear_pipeline_parts``, ``TTTBase._pipeline_plan`` for ``TTTLinear``;
ttt_amd/models/ssm/pipeline.py): off by default, and when it is on the parts cover the scan exactly once, in order - whole checkpoint
groups where groups are plentiful, multiples of the step quantum where they are not (the TTT-Linear MFMA scans continue from any step)."""
import pytest
import torch


def _layer_and_meta(CS, steps, G, scenes=1):
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm.ttt_layer import TTTLinear
    cfg = ModelConfig(model_dim=128, num_heads=2, num_layers=1, mini_batch_size=CS, latent_height=4, latent_width=4,
                      compressed_num_frames=4, ssm_layer="ttt_linear", scan_checkpoint_group_size=G)
    layer = TTTLinear(cfg)
    L = CS * steps
    tl = 16
    frames = (L - scenes * tl) // 16
    meta = SequenceMetadata(text_length=tl, seq_text_length=tl * scenes, num_frames=frames, num_chunks=scenes, tokens_per_frame=16,
                            latent_height=4, latent_width=4, t_emb=None)
    if scenes > 1:
        meta.init_multiscene_offsets()
    x = torch.zeros(1, 1, 128).expand(1, L, 128)          # (the plan looks at x's shape, dtype and device only)
    return layer, meta, x, L


def _check_cover(parts, NC, CS, L, unit):
    at, seen = 0, torch.zeros(L, dtype=torch.int32)
    for c, (s0, ns, runs) in enumerate(parts):
        assert s0 == at and ns >= 1 and s0 % unit == 0
        assert ns % unit == 0 or c == len(parts) - 1
        assert sum(r1 - r0 for r0, r1 in runs) == ns * CS
        for r0, r1 in runs:
            seen[r0:r1] += 1
        at += ns
    assert at == NC and bool((seen == 1).all())


@pytest.fixture
def mfma(monkeypatch):
    import test_time_training as ext
    asked = []

    def resolved(*a, **k):
        asked.append(k)
        return "mfma"
    monkeypatch.setattr(ext, "resolved_impl", resolved)
    monkeypatch.delenv("TTT_PIPELINE_WEIGHTS", raising=False)
    return asked


def test_switch_is_off_by_default(mfma, monkeypatch):
    monkeypatch.delenv("TTT_LINEAR_PIPELINE_PARTS", raising=False)
    layer, meta, x, L = _layer_and_meta(16, 64, 4)
    assert layer.linear_pipeline_parts == 0
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            assert layer._pipeline_plan(x, meta, L, False, False) is None
    layer.linear_pipeline_parts = 1
    assert layer._pipeline_plan(x, meta, L, False, False) is None
    layer.pipeline_parts = 5                              # the TTT-MLP switch does not turn a TTT-Linear layer on
    layer.linear_pipeline_parts = 0
    assert layer._pipeline_plan(x, meta, L, False, False) is None
    monkeypatch.setenv("TTT_LINEAR_PIPELINE_PARTS", "3")
    assert _layer_and_meta(16, 64, 4)[0].linear_pipeline_parts == 3


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("CS,steps,G,scenes,n", [(16, 40, 4, 1, 3), (64, 23, 3, 1, 3), (16, 75, 2, 3, 4), (64, 10, 2, 1, 2)])
def test_parts_are_whole_groups_when_groups_are_plentiful(mfma, CS, steps, G, scenes, n, reverse):
    """ceil(NC / G) >= 2 n: the requested number of parts, each a whole number of checkpoint groups but for the ragged tail, with grad
    enabled and without; the question to the library carries HipLinear's selector for this call"""
    from ttt_amd.models.ssm.linear_hip import HipLinear
    layer, meta, x, L = _layer_and_meta(CS, steps, G, scenes)
    layer.linear_pipeline_parts = n
    NC = L // CS
    assert -(-NC // G) >= 2 * n
    for grad in (torch.no_grad, torch.enable_grad):
        with grad():
            parts = layer._pipeline_plan(x, meta, L, reverse, False)
        assert parts is not None and len(parts) == n
        _check_cover(parts, NC, CS, L, G)
    assert mfma and all(k["mlp"] is False and k["backward"] is False and k["impl"] == HipLinear._impl(CS, 64, torch.bfloat16) for k in mfma)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("CS,steps,scenes,n", [(16, 2048, 1, 3), (64, 500, 1, 4), (16, 1027, 1, 2), (16, 1536, 3, 8)])
def test_parts_are_multiples_of_the_quantum_when_there_is_one_group(mfma, CS, steps, scenes, n, reverse):
    """G >= NC (sampling: one checkpoint group): cuts at multiples of LIN_QUANTUM steps = one 4 096-token row block, at least two quanta
    per part on average - fewer parts than asked for when the scan is short"""
    from ttt_amd.models.ssm import pipeline
    layer, meta, x, L = _layer_and_meta(CS, steps, 10 ** 6, scenes)
    layer.linear_pipeline_parts = n
    NC, q = L // CS, pipeline.lin_quantum(CS)
    assert pipeline.LIN_QUANTUM is None and q == 4096 // CS
    with torch.no_grad():
        parts = layer._pipeline_plan(x, meta, L, reverse, False)
    want = min(n, -(-NC // q) // 2)
    assert want >= 2 and parts is not None and len(parts) == want
    _check_cover(parts, NC, CS, L, q)


def test_quantum_override(mfma, monkeypatch):
    from ttt_amd.models.ssm import pipeline
    monkeypatch.setattr(pipeline, "LIN_QUANTUM", 8)
    layer, meta, x, L = _layer_and_meta(16, 40, 10 ** 6)
    layer.linear_pipeline_parts = 3
    parts = layer._pipeline_plan(x, meta, L, False, False)
    assert parts is not None and len(parts) == 2            # five quanta: two parts of at least two
    _check_cover(parts, 40, 16, L, 8)


def test_layer_stays_one_piece(mfma, monkeypatch):
    """a head shard, a scan too short for two parts of two units, and whatever the MFMA scan does not run"""
    import test_time_training as ext
    from ttt_amd.infra import remat_cache
    layer, meta, x, L = _layer_and_meta(16, 40, 4)
    layer.linear_pipeline_parts = 3
    assert layer._pipeline_plan(x, meta, L, False, False) is not None
    assert layer._pipeline_plan(x, meta, L, False, True) is None                    # heads_only
    monkeypatch.setattr(remat_cache, "replaying", lambda kind: kind == "scan")
    assert layer._pipeline_plan(x, meta, L, False, False) is None                   # a replay gets its scan result handed back
    monkeypatch.undo()
    short, meta_s, x_s, L_s = _layer_and_meta(16, 6, 2)                              # three groups, 6 steps: n = min(3, 3 // 2) < 2
    short.linear_pipeline_parts = 3
    assert short._pipeline_plan(x_s, meta_s, L_s, False, False) is None
    monkeypatch.setattr(ext, "resolved_impl", lambda *a, **k: "generic")           # e.g. mini-batches of 64 with cs64_impl = "auto"
    assert layer._pipeline_plan(x, meta, L, False, False) is None
