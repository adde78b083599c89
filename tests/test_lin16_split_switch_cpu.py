"""The layer switch of the two-wave TTT-Linear forward scan, ``HipLinear.cs16_scan_split`` / ``TTT_LINEAR_CS16_SCAN_SPLIT`` (no device
needed): parsing and validation, and - with an extension that only counts its calls - which entry of the binding a TTT-Linear forward
reaches: on = the split entries at mini-batches of 16 (bf16, head dim 64, MFMA scan, an extension that has them) and only there, off =
today's calls, in one piece (``HipLinear.forward``) and in the parts of pipeline.py (the chunk picker of ``pipeline.LINEAR_SCAN``)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


class CountingExt:
    """stands in for ``test_time_training``: every scan entry records its name, the selector and the call's trailing integers"""

    def __init__(self, resolves="mfma"):
        self.calls, self.asked, self.resolves = [], [], resolves

    def resolved_impl(self, B, NH, NC, CS, F, G, act_dtype=BF16, mlp=True, backward=False, *, impl=None):
        self.asked.append((B, NH, NC, CS, F, G, act_dtype, mlp, backward, impl))
        return self.resolves

    def _scan(name, n_ints, with_impl=True):
        def fn(self, *a):
            impl, a = (a[0], a[1:]) if with_impl else (None, a)
            assert len(a) == 11 + n_ints and all(isinstance(t, torch.Tensor) for t in a[:11])
            self.calls.append((name, impl, *a[11:]))
        return fn

    ttt_linear_forward = _scan("ttt_linear_forward", 1, with_impl=False)
    ttt_linear_forward_impl = _scan("ttt_linear_forward_impl", 1)
    ttt_linear_forward_chunk = _scan("ttt_linear_forward_chunk", 3)


class CountingExtWithSplit(CountingExt):
    ttt_linear_forward_split16 = CountingExt._scan("ttt_linear_forward_split16", 1)
    ttt_linear_forward_chunk_split16 = CountingExt._scan("ttt_linear_forward_chunk_split16", 3)


@pytest.fixture
def switch():
    from ttt_amd.models.ssm.linear_hip import HipLinear
    old = HipLinear.cs16_scan_split, HipLinear.cs64_impl
    yield HipLinear
    HipLinear.cs16_scan_split, HipLinear.cs64_impl = old


def test_switch_is_off_by_default_and_read_from_the_environment():
    code = "from ttt_amd.models.ssm.linear_hip import HipLinear; print('split', HipLinear.cs16_scan_split)"
    env = {k: v for k, v in os.environ.items() if k != "TTT_LINEAR_CS16_SCAN_SPLIT"}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "ttt-video-dit_amd"), ROOT])
    run = lambda e: subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True)
    r = run(env)
    assert r.returncode == 0 and "split 0" in r.stdout, r.stderr[-400:]
    r = run({**env, "TTT_LINEAR_CS16_SCAN_SPLIT": "0"})
    assert r.returncode == 0 and "split 0" in r.stdout, r.stderr[-400:]
    r = run({**env, "TTT_LINEAR_CS16_SCAN_SPLIT": "1"})
    assert r.returncode == 0 and "split 1" in r.stdout, r.stderr[-400:]
    for bad in ("2", "on", "", "mfma"):
        r = run({**env, "TTT_LINEAR_CS16_SCAN_SPLIT": bad})
        assert r.returncode != 0 and "TTT_LINEAR_CS16_SCAN_SPLIT: expected '0' (off) or '1'" in r.stderr, (bad, r.stderr[-400:])


def test_bad_values_of_the_attribute_raise_at_the_call_that_reads_it(switch):
    from ttt_amd.models.ssm import linear_hip
    x16 = torch.zeros(1, 2, 3, 16, 64, dtype=BF16)
    for bad in ("1", "on", 2, -1, None, True, 1.5):
        switch.cs16_scan_split = bad
        with pytest.raises(ValueError, match="HipLinear.cs16_scan_split: expected 0 or 1"):
            linear_hip.scan_split_applies(CountingExtWithSplit(), None, x16, 4)
        with pytest.raises(ValueError, match="HipLinear.cs16_scan_split"):
            linear_hip.linear_forward_chunk_call(CountingExtWithSplit(), None, x16, 4)


def test_switch_selects_only_the_cs16_bf16_mfma_geometry(switch):
    from ttt_amd.models.ssm import linear_hip
    x16 = torch.zeros(1, 2, 3, 16, 64, dtype=BF16)
    fake = CountingExtWithSplit()
    switch.cs16_scan_split = 0
    assert not linear_hip.scan_split_applies(fake, None, x16, 4)
    assert linear_hip.linear_forward_chunk_call(fake, None, x16, 4) == fake.ttt_linear_forward_chunk
    assert fake.asked == [], "off: nothing is asked of the extension"
    switch.cs16_scan_split = 1
    assert linear_hip.scan_split_applies(fake, None, x16, 4)
    assert linear_hip.linear_forward_chunk_call(fake, None, x16, 4) == fake.ttt_linear_forward_chunk_split16
    assert fake.asked[-1] == (1, 2, 3, 16, 64, 4, BF16, False, False, None)
    for other in (torch.zeros(1, 2, 3, 64, 64, dtype=BF16), torch.zeros(1, 2, 3, 16, 32, dtype=BF16), torch.zeros(1, 2, 3, 16, 64)):
        for impl in (None, "mfma"):
            assert not linear_hip.scan_split_applies(fake, impl, other, 4)
            assert linear_hip.linear_forward_chunk_call(fake, impl, other, 4) == fake.ttt_linear_forward_chunk
    generic = CountingExtWithSplit(resolves="generic")    # (set_impl("generic"): the scan does not resolve to the MFMA kernels)
    assert linear_hip.linear_forward_chunk_call(generic, None, x16, 4) == generic.ttt_linear_forward_chunk
    without = CountingExt()                                # an extension without the entry
    assert linear_hip.linear_forward_chunk_call(without, None, x16, 4) == without.ttt_linear_forward_chunk
    assert without.asked == []


def _inputs(CS, F=64, act=BF16, NC=3, B=1, NH=2):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    return (z(NH, F), z(NH, F), z(B, NH, F, F), z(B, NH, 1, F), z(B, NH, NC, CS, F, dt=act), z(B, NH, NC, CS, F, dt=act),
            z(B, NH, NC, CS, F, dt=act), z(B, NH, NC, CS, CS, dt=act), 2)


@pytest.mark.parametrize("grad", [False, True])
def test_one_piece_forward_reaches_the_split_entry_only_when_on(switch, monkeypatch, grad):
    from ttt_amd.models.ssm import linear_hip

    def forwards(fake, *a, **k):
        monkeypatch.setattr(linear_hip, "_ext", lambda: fake)
        fake.calls.clear()
        with torch.set_grad_enabled(grad):
            linear_hip.HipLinear.apply(*_inputs(*a, **k))
        return list(fake.calls)

    fake = CountingExtWithSplit()
    switch.cs16_scan_split = 0
    assert forwards(fake, 16) == [("ttt_linear_forward", None, 2)] == forwards(fake, 64)
    assert fake.asked == [], "default off never reaches the new binding, and asks nothing"
    switch.cs16_scan_split = 1
    assert forwards(fake, 16) == [("ttt_linear_forward_split16", None, 2)]
    assert forwards(fake, 64) == [("ttt_linear_forward", None, 2)]
    assert forwards(fake, 16, F=32) == [("ttt_linear_forward", None, 2)]
    assert forwards(fake, 16, act=torch.float32) == [("ttt_linear_forward", None, 2)]
    switch.cs64_impl = "mfma"
    assert forwards(fake, 64) == [("ttt_linear_forward_impl", "mfma", 2)]
    assert forwards(fake, 16) == [("ttt_linear_forward_split16", None, 2)]
    switch.cs64_impl = "auto"
    assert forwards(CountingExt(), 16) == [("ttt_linear_forward", None, 2)], "an extension without the entry takes today's path"
    assert forwards(CountingExtWithSplit(resolves="generic"), 16) == [("ttt_linear_forward", None, 2)]


def test_scan_parts_reach_the_split_chunk_entry_only_when_on(switch):
    from ttt_amd.models.ssm import pipeline

    def walk(fake, CS, impl=None, act=BF16, F=64):
        part = pipeline.LINEAR_SCAN.chunk(fake, impl)
        fake.calls.clear()
        t = [torch.zeros(1, 2, 9, CS, F, dtype=act)] + [torch.zeros(1)] * 10
        for s0, ns in ((0, 4), (4, 1), (5, 4)):
            part(*t, 7, s0, ns)
        return list(fake.calls)

    parts = lambda name, impl=None: [(name, impl, 7, 0, 4), (name, impl, 7, 4, 1), (name, impl, 7, 5, 4)]
    fake = CountingExtWithSplit()
    switch.cs16_scan_split = 0
    assert walk(fake, 16) == parts("ttt_linear_forward_chunk") == walk(fake, 64)
    assert fake.asked == []
    switch.cs16_scan_split = 1
    assert walk(fake, 16) == parts("ttt_linear_forward_chunk_split16"), "every part of a pipelined forward"
    assert fake.asked[-1][:6] == (1, 2, 9, 16, 64, 7)
    assert walk(fake, 64, "mfma") == parts("ttt_linear_forward_chunk", "mfma")
    assert walk(fake, 16, act=torch.float32) == parts("ttt_linear_forward_chunk")
    assert walk(fake, 16, F=32) == parts("ttt_linear_forward_chunk")
    assert walk(CountingExt(), 16) == parts("ttt_linear_forward_chunk")


def test_oracle_backed_stand_in_has_no_entry_and_runs_todays_call(switch):
    """oracle/cpu_ext.py does not have the entry: with the switch on, the layer's forward is the call of the switch off, bit for bit"""
    from oracle import cpu_ext
    from oracle import ttt_oracle as O
    cpu_ext.install()
    try:
        import test_time_training as fake
        assert not hasattr(fake, "ttt_linear_forward_chunk_split16") and not hasattr(fake, "ttt_linear_forward_split16")
        B, NH, NC, CS, F, G = 1, 2, 5, 16, 64, 2
        d = O.make_inputs("linear", B, NH, NC, CS, F, seed=3)
        st = [d[k].unsqueeze(0).expand(B, *d[k].shape) for k in ("W1", "b1")]
        outs = []
        for v in (0, 1):
            switch.cs16_scan_split = v
            with torch.no_grad():
                outs.append(switch.apply(d["ln_w"], d["ln_b"], *st, d["XQ"], d["XV"], d["XK"], d["eta"], G))
        assert torch.equal(*outs)
    finally:
        cpu_ext.uninstall()
