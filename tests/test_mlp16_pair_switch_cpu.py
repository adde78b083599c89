"""The layer switch of the pair scan, ``TTTBase.cs16_scan_pair`` / ``TTT_MLP_CS16_SCAN_PAIR`` (no device needed): parsing and validation,
and - with an extension that only records its calls - which entry of the binding a TTT-MLP forward reaches: on = the pair entries at
mini-batches of 16 (bf16, head dim 64, MFMA scan) and only there, off = today's calls, in one piece (``TkMLP``, ``FusedPreScanMLP``)
and in the parts of pipeline.py (the chunk getter of ``pipeline.MLP_SCAN``)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


class RecordingExt:
    """stands in for ``test_time_training``: every scan entry records its name and the call's trailing integers"""

    def __init__(self, resolves="mfma"):
        self.calls, self.asked, self.resolves = [], [], resolves

    def resolved_impl(self, B, NH, NC, CS, F, G, act_dtype=BF16, mlp=True, backward=False, *, impl=None):
        self.asked.append((B, NH, NC, CS, F, G, act_dtype, mlp, backward))
        return self.resolves

    def _scan(name, n_ints):
        def fn(self, *a):
            assert len(a) == 15 + n_ints and all(isinstance(t, torch.Tensor) for t in a[:15])
            self.calls.append((name, *a[15:]))
            return True
        return fn

    ttt_forward = _scan("ttt_forward", 1)
    ttt_forward_pair16 = _scan("ttt_forward_pair16", 1)
    ttt_forward_chunk = _scan("ttt_forward_chunk", 3)
    ttt_forward_chunk_pair16 = _scan("ttt_forward_chunk_pair16", 3)

    def pre_forward(self, *a, **k):
        self.calls.append(("pre_forward",))


@pytest.fixture
def switch():
    from ttt_amd.models.ssm.ttt_layer import TTTBase
    old = TTTBase.cs16_scan_pair
    yield TTTBase
    TTTBase.cs16_scan_pair = old


def test_default_is_off_and_values_are_validated(switch):
    from ttt_amd.models.ssm import mlp_tk
    assert mlp_tk._check_cs16_scan_pair("0") == 0 and mlp_tk._check_cs16_scan_pair("1") == 1
    assert mlp_tk._check_cs16_scan_pair(0) == 0 and mlp_tk._check_cs16_scan_pair(1) == 1
    for bad in ("2", "on", "", "mfma", 2, -1, None, True, 1.5):
        with pytest.raises(ValueError, match="TTT_MLP_CS16_SCAN_PAIR"):
            mlp_tk._check_cs16_scan_pair(bad)
    # a wrong value set on the class is refused at the call that reads it
    switch.cs16_scan_pair = "pair"
    with pytest.raises(ValueError, match="cs16_scan_pair"):
        mlp_tk.mlp_forward_call(RecordingExt(), torch.zeros(1, 2, 3, 16, 64, dtype=BF16), 1)


def test_environment_variable_sets_the_default():
    code = "from ttt_amd.models.ssm.ttt_layer import TTTBase; print(TTTBase.cs16_scan_pair)"
    env = {k: v for k, v in os.environ.items() if k != "TTT_MLP_CS16_SCAN_PAIR"}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "ttt-video-dit_amd"), ROOT, env.get("PYTHONPATH", "")])
    run = lambda e: subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True)
    r = run(env)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stderr[-400:]
    r = run({**env, "TTT_MLP_CS16_SCAN_PAIR": "1"})
    assert r.returncode == 0 and r.stdout.strip() == "1", r.stderr[-400:]
    r = run({**env, "TTT_MLP_CS16_SCAN_PAIR": "yes"})
    assert r.returncode != 0 and "TTT_MLP_CS16_SCAN_PAIR" in r.stderr


def test_switch_selects_only_the_cs16_bf16_mfma_geometry(switch):
    from ttt_amd.models.ssm import mlp_tk
    x16 = torch.zeros(1, 2, 3, 16, 64, dtype=BF16)
    fake = RecordingExt()
    switch.cs16_scan_pair = 0
    assert mlp_tk.mlp_forward_call(fake, x16, 4) == fake.ttt_forward
    assert mlp_tk.mlp_forward_chunk_call(fake, x16, 4) == fake.ttt_forward_chunk
    assert fake.asked == [], "off: nothing is asked of the extension"
    switch.cs16_scan_pair = 1
    assert mlp_tk.mlp_forward_call(fake, x16, 4) == fake.ttt_forward_pair16
    assert mlp_tk.mlp_forward_chunk_call(fake, x16, 4) == fake.ttt_forward_chunk_pair16
    assert fake.asked[-1] == (1, 2, 3, 16, 64, 4, BF16, True, False)
    for other in (torch.zeros(1, 2, 3, 64, 64, dtype=BF16), torch.zeros(1, 2, 3, 16, 32, dtype=BF16), torch.zeros(1, 2, 3, 16, 64)):
        assert mlp_tk.mlp_forward_call(fake, other, 4) == fake.ttt_forward
        assert mlp_tk.mlp_forward_chunk_call(fake, other, 4) == fake.ttt_forward_chunk
    generic = RecordingExt(resolves="generic")           # (set_impl("generic"): the scan does not resolve to the MFMA kernels)
    assert mlp_tk.mlp_forward_call(generic, x16, 4) == generic.ttt_forward
    assert mlp_tk.mlp_forward_chunk_call(generic, x16, 4) == generic.ttt_forward_chunk


def _tk_inputs(CS, NC=3, B=1, NH=2, F=64):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    return (z(NH, F), z(NH, F), z(B, NH, F, 4 * F), z(B, NH, 1, 4 * F), z(B, NH, 4 * F, F), z(B, NH, 1, F),
            z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, 1, CS, dt=BF16), 2)


@pytest.mark.parametrize("grad", [False, True])
def test_one_piece_forward_reaches_the_pair_entry_only_when_on(switch, monkeypatch, grad):
    from ttt_amd.models.ssm import fused, mlp_tk
    fake = RecordingExt()
    monkeypatch.setattr(mlp_tk, "_ext", lambda: fake)
    monkeypatch.setattr(fused, "_ext", lambda: fake)

    def forwards(CS):
        fake.calls.clear()
        with torch.set_grad_enabled(grad):
            mlp_tk.TkMLP.apply(*_tk_inputs(CS))
            B, NH, NC, F = 1, 2, 3, 64
            raw = [torch.zeros(B, NC * CS, NH * F, dtype=BF16) for _ in range(3)]
            st = _tk_inputs(CS)[2:6]
            fused.FusedPreScanMLP.apply(*raw, torch.zeros(NH, F), torch.zeros(NH, F), None, None, None, NH, *st,
                                        torch.zeros(B, NH, NC, 1, CS, dtype=BF16), 2)
        return [c for c in fake.calls if c[0] != "pre_forward"]

    switch.cs16_scan_pair = 0
    assert forwards(16) == [("ttt_forward", 2)] * 2 and forwards(64) == [("ttt_forward", 2)] * 2
    switch.cs16_scan_pair = 1
    assert forwards(16) == [("ttt_forward_pair16", 2)] * 2
    assert forwards(64) == [("ttt_forward", 2)] * 2


def test_scan_parts_reach_the_pair_chunk_entry_only_when_on(switch):
    from ttt_amd.models.ssm import pipeline
    fake = RecordingExt()
    part = pipeline.MLP_SCAN.chunk(fake, None)

    def walk(CS):
        fake.calls.clear()
        t = [torch.zeros(1, 2, 9, CS, 64, dtype=BF16)] + [torch.zeros(1)] * 14
        for s0, ns in ((0, 4), (4, 5)):
            part(*t, 7, s0, ns)
        return list(fake.calls)

    switch.cs16_scan_pair = 0
    assert walk(16) == [("ttt_forward_chunk", 7, 0, 4), ("ttt_forward_chunk", 7, 4, 5)] == walk(64)
    assert fake.asked == []
    switch.cs16_scan_pair = 1
    assert walk(16) == [("ttt_forward_chunk_pair16", 7, 0, 4), ("ttt_forward_chunk_pair16", 7, 4, 5)]
    assert fake.asked[-1][:6] == (1, 2, 9, 16, 64, 7)
    assert walk(64) == [("ttt_forward_chunk", 7, 0, 4), ("ttt_forward_chunk", 7, 4, 5)]
