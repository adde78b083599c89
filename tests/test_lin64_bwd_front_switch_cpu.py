"""``HipLinear.backward_front64`` / ``TTT_LINEAR_BACKWARD_FRONT64`` (ttt_amd/models/ssm/linear_hip.py), the switch of the front / chain
stage of the TTT-Linear backward in parts at mini-batches of 64, without a device: parsing and validation, and - with an extension
that only records its calls and stand-ins for the two streams and their events (tests/helpers.py) - which entries
``HipLinear.backward`` reaches, in which order and on which stream.  The switch applies only at mini-batches of 64 with
``cs64_impl == "mfma"`` and ``backward_parts > 0``; ``backward_front`` keeps meaning mini-batches of 16 only."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import fake_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
SLOT, REC16, REC64 = 16 * 1024 + 256, 19456, 77824


def _import_with(value):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "ttt-video-dit_amd"), ROOT]))
    for name in ("TTT_LINEAR_BACKWARD_FRONT64", "TTT_LINEAR_BACKWARD_FRONT", "TTT_LINEAR_BACKWARD_PARTS"):
        env.pop(name, None)
    if value is not None:
        env["TTT_LINEAR_BACKWARD_FRONT64"] = value
    code = ("from ttt_amd.models.ssm.linear_hip import HipLinear; "
            "print('front64', HipLinear.backward_front64, 'front', HipLinear.backward_front, 'parts', HipLinear.backward_parts)")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


def test_switch_is_off_by_default_and_read_from_the_environment():
    """all three defaults are off; the variable is read once, at import, and selects nothing by itself"""
    r = _import_with(None)
    assert r.returncode == 0 and "front64 0 front 0 parts 0" in r.stdout, r.stderr
    r = _import_with("0")
    assert r.returncode == 0 and "front64 0 front 0 parts 0" in r.stdout, r.stderr
    r = _import_with("1")
    assert r.returncode == 0 and "front64 1 front 0 parts 0" in r.stdout, r.stderr
    for bad in ("2", "on", ""):
        r = _import_with(bad)
        assert r.returncode != 0 and "TTT_LINEAR_BACKWARD_FRONT64: expected '0' (off) or '1'" in r.stderr, (bad, r.stderr)
    from ttt_amd.models.ssm import linear_hip
    old = os.environ.get("TTT_LINEAR_BACKWARD_FRONT64")
    os.environ["TTT_LINEAR_BACKWARD_FRONT64"] = "1"              # after the import: not read again
    try:
        assert linear_hip.HipLinear.backward_front64 == 0
    finally:
        if old is None:
            del os.environ["TTT_LINEAR_BACKWARD_FRONT64"]
        else:
            os.environ["TTT_LINEAR_BACKWARD_FRONT64"] = old


class RecordingExt:
    """stands in for ``test_time_training``: every TTT-Linear scan entry records its name, the stream it was issued on and its integers"""

    def __init__(self, log, current):
        self.log, self.current, self.spaces = log, current, []

    def resolved_impl(self, B, NH, NC, CS, F, G, act_dtype=BF16, mlp=False, backward=False, *, impl=None):
        return "mfma" if impl == "mfma" or CS == 16 else "generic"

    def ttt_linear_forward(self, *a):
        pass

    def ttt_linear_forward_impl(self, impl, *a):
        pass

    def ttt_linear_backward(self, *a):
        assert len(a) == 22
        self.log.append(("one_call", self.current[0], None))

    def ttt_linear_backward_impl(self, impl, *a):
        assert len(a) == 22
        self.log.append(("one_call", self.current[0], impl))

    def linear_backward_parts_slots(self, B, NH, NC, CS, F, G, nk, act_dtype=BF16, *, impl=None):
        return B * NH * nk * (G + 1) * SLOT

    def linear_backward_parts_carry(self, B, NH, NC, CS, F, G, act_dtype=BF16, *, impl=None):
        return B * NH * 8 * (64 if CS == 16 else 256) * 4

    def linear_backward_front_records(self, B, NH, NC, CS, F, G, nk, act_dtype=BF16, *, impl=None):
        assert CS == 16
        return B * NH * nk * G * REC16

    def linear_backward_front64_records(self, B, NH, NC, CS, F, G, nk, act_dtype=BF16, *, impl=None):
        assert CS == 64 and impl == "mfma"
        return B * NH * nk * G * REC64

    def _space(self, t):
        if not any(s is t for s in self.spaces):
            self.spaces.append(t)
        return next(i for i, s in enumerate(self.spaces) if s is t)

    def _groups(self, name, n_extra, needed, impl, a, cs=None):
        assert len(a) == 21 + 1 + n_extra
        assert all((a[i] is not None) == (i in needed) for i in range(21)), f"{name} is given what it needs and nothing else"
        XK = a[1]
        if cs is not None:
            assert XK.shape[3] == cs and (impl == "mfma" or cs == 16)
        G, k0, nk = a[21:24]
        if n_extra >= 4 and name != "sweep":
            records = a[25]
            per = REC64 if XK.shape[3] == 64 else REC16
            assert records.numel() * records.element_size() >= XK.shape[0] * XK.shape[1] * nk * G * per
        self.log.append((name, self.current[0], G, k0, nk))

    RECOMPUTE = (1, 2, 3, 4, 5, 6, 7)
    SWEEP = (0, 1, 2, 3, 4, 5, 8, 9, 10, 13, 14, 15, 16, 17, 18, 19, 20)
    FRONT = (0, 1, 2, 4, 5, 10, 18)
    CHAIN = (0, 1, 3, 4, 5, 8, 9, 13, 14, 15, 16, 17, 19, 20)

    def ttt_linear_recompute_groups(self, impl, *a):
        self._groups("recompute", 3, self.RECOMPUTE, impl, a)

    def ttt_linear_sweep_groups(self, impl, *a):
        self._groups("sweep", 4, self.SWEEP, impl, a)

    def ttt_linear_front_groups(self, impl, *a):
        self._groups("front16", 4, self.FRONT, impl, a, cs=16)

    def ttt_linear_chain_groups(self, impl, *a):
        self._groups("chain16", 5, self.CHAIN, impl, a, cs=16)

    def ttt_linear_front64_groups(self, impl, *a):
        self._groups("front64", 4, self.FRONT, impl, a, cs=64)

    def ttt_linear_chain64_groups(self, impl, *a):
        self._groups("chain64", 5, self.CHAIN, impl, a, cs=64)


@pytest.fixture
def fake(monkeypatch):
    from ttt_amd.models.ssm import linear_hip
    log, current = fake_streams(monkeypatch)
    ext = RecordingExt(log, current)
    monkeypatch.setattr(linear_hip, "_ext", lambda: ext)
    return ext


@pytest.fixture
def switch():
    from ttt_amd.models.ssm.linear_hip import HipLinear
    old = HipLinear.backward_parts, HipLinear.backward_front, HipLinear.backward_front64, HipLinear.cs64_impl
    yield HipLinear
    HipLinear.backward_parts, HipLinear.backward_front, HipLinear.backward_front64, HipLinear.cs64_impl = old


def _backward(CS, NC=9, G=2, B=1, NH=2, F=64):
    from ttt_amd.models.ssm.linear_hip import HipLinear
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt).requires_grad_(True)
    out = HipLinear.apply(z(NH, F), z(NH, F), z(B, NH, F, F), z(B, NH, 1, F), z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, CS, F, dt=BF16),
                          z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, CS, CS, dt=BF16), G)
    out.backward(torch.zeros_like(out))


def _scan_calls(log):
    return [c for c in log if c[0] in ("recompute", "sweep", "front16", "chain16", "front64", "chain64", "one_call")]


def test_schedule_with_the_front_at_mini_batches_of_64(switch, fake):
    """NC = 9, G = 2: K = 5 groups in ranges of 2 -> [3, 5), [1, 3), [0, 1).  Per range the side stream issues recompute -> front, the
    caller's stream the chain; the side work of range n + 1 is issued before the chain of range n; events as in
    ``pipeline.run_in_parts``"""
    switch.cs64_impl, switch.backward_parts, switch.backward_front64 = "mfma", 2, 1
    _backward(64)
    sync = [c for c in fake.log if c[0] in ("wait_stream", "wait_event", "record", "recompute", "front64", "chain64", "sweep", "one_call")]
    ready, swept = (0, 1, 2), (3, 4, 5)                  # the events in the order they were made
    assert sync == [
        ("wait_stream", "side", "main"),
        ("recompute", "side", 2, 3, 2), ("front64", "side", 2, 3, 2), ("record", "side", ready[0]),
        ("recompute", "side", 2, 1, 2), ("front64", "side", 2, 1, 2), ("record", "side", ready[1]),
        ("wait_event", "main", ready[0]), ("chain64", "main", 2, 3, 2), ("record", "main", swept[0]),
        ("wait_event", "side", swept[0]), ("recompute", "side", 2, 0, 1), ("front64", "side", 2, 0, 1), ("record", "side", ready[2]),
        ("wait_event", "main", ready[1]), ("chain64", "main", 2, 1, 2), ("record", "main", swept[1]),
        ("wait_event", "main", ready[2]), ("chain64", "main", 2, 0, 1), ("record", "main", swept[2]),
        ("wait_stream", "main", "side")]


def test_the_switch_applies_only_at_64_with_mfma_and_parts(switch, fake):
    names = lambda: sorted({c[0] for c in _scan_calls(fake.log)})
    # off by default: parts at CS = 64 sweep
    switch.cs64_impl, switch.backward_parts = "mfma", 2
    assert switch.backward_front64 == 0
    _backward(64)
    assert names() == ["recompute", "sweep"]
    # backward_front = 1 alone changes nothing at CS = 64
    fake.log.clear()
    switch.backward_front = 1
    _backward(64)
    assert names() == ["recompute", "sweep"]
    # ... and backward_front64 = 1 changes nothing at CS = 16: the CS = 16 front stays behind its own switch
    fake.log.clear()
    switch.backward_front, switch.backward_front64 = 0, 1
    _backward(16)
    assert names() == ["recompute", "sweep"]
    fake.log.clear()
    switch.backward_front = 1
    _backward(16)
    assert names() == ["chain16", "front16", "recompute"]
    # without backward_parts: the one call
    fake.log.clear()
    switch.backward_parts, switch.backward_front = 0, 0
    _backward(64)
    assert _scan_calls(fake.log) == [("one_call", "main", "mfma")]
    # under "auto" the CS = 64 backward is the generic one call whatever the switches say
    fake.log.clear()
    switch.cs64_impl, switch.backward_parts = "auto", 2
    _backward(64)
    assert _scan_calls(fake.log) == [("one_call", "main", None)]
    # one range only: the one call
    fake.log.clear()
    switch.cs64_impl, switch.backward_parts = "mfma", 8
    _backward(64)
    assert _scan_calls(fake.log) == [("one_call", "main", "mfma")]


def test_an_extension_without_the_entries_sweeps(switch, fake, monkeypatch):
    monkeypatch.delattr(RecordingExt, "ttt_linear_chain64_groups")
    switch.cs64_impl, switch.backward_parts, switch.backward_front64 = "mfma", 2, 1
    _backward(64)
    assert sorted({c[0] for c in _scan_calls(fake.log)}) == ["recompute", "sweep"]


def test_a_wrong_value_on_the_class_is_refused_where_it_is_read(switch, fake):
    switch.cs64_impl, switch.backward_parts = "mfma", 2
    for bad in (2, -1, "1", 0.5, None, True):
        switch.backward_front64 = bad
        with pytest.raises(ValueError, match="HipLinear.backward_front64: expected 0 or 1"):
            _backward(64)
    switch.backward_parts = 0                     # not read where the in-parts path is not selected
    _backward(64)
    switch.backward_parts = 2                     # ... nor at mini-batches of 16
    _backward(16)
