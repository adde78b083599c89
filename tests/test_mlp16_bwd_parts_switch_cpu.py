"""The layer switch of the TTT-MLP backward in parts at mini-batches of 16, ``TkMLP.cs16_backward_parts`` /
``TTT_MLP_CS16_BACKWARD_PARTS`` (ttt_amd/models/ssm/mlp_tk.py), without a device: parsing and validation, the range cutting, and - with
an extension that only records its calls and stand-ins for the two streams and their events - the schedule of ``backward_in_parts``:
which entries ``TkMLP.backward`` and ``FusedPreScanMLP.backward`` reach, in which order, on which stream, into which workspace."""
import os
import subprocess
import sys

import pytest
import torch

from helpers import fake_streams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
SLOT = 132352


def _import_with(value):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "ttt-video-dit_amd"), ROOT]))
    env.pop("TTT_MLP_CS16_BACKWARD_PARTS", None)
    if value is not None:
        env["TTT_MLP_CS16_BACKWARD_PARTS"] = value
    code = "from ttt_amd.models.ssm.mlp_tk import TkMLP; print('parts', TkMLP.cs16_backward_parts)"
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


def test_switch_is_off_by_default_and_read_from_the_environment():
    r = _import_with(None)
    assert r.returncode == 0 and "parts 0" in r.stdout, r.stderr
    r = _import_with("4")
    assert r.returncode == 0 and "parts 4" in r.stdout, r.stderr
    for bad in ("-1", "two", "1.5", ""):
        r = _import_with(bad)
        assert r.returncode != 0 and "TTT_MLP_CS16_BACKWARD_PARTS: expected a non-negative integer" in r.stderr, (bad, r.stderr)


@pytest.fixture
def switch():
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    old = TkMLP.cs16_backward_parts, TkMLP.cs16_bwd_impl
    yield TkMLP
    TkMLP.cs16_backward_parts, TkMLP.cs16_bwd_impl = old


def test_a_wrong_value_on_the_class_is_refused_where_it_is_read(switch):
    assert switch.cs16_backward_parts == 0
    for bad in (-2, "2", 1.5, None, True):
        switch.cs16_backward_parts = bad
        with pytest.raises(ValueError, match="TkMLP.cs16_backward_parts: expected a non-negative integer"):
            switch.bwd_parts("mfma")
    switch.cs16_backward_parts = 3
    assert switch.bwd_parts("mfma") == 3 and switch.bwd_parts(None) == 0


def test_range_cutting_covers_every_group_once_last_range_first():
    from ttt_amd.models.ssm.mlp_tk import part_ranges
    assert part_ranges(5, 2) == [(3, 2), (1, 2), (0, 1)]
    assert part_ranges(4, 2) == [(2, 2), (0, 2)]
    assert part_ranges(3, 8) == [(0, 3)] and part_ranges(1, 1) == [(0, 1)]
    for K in range(1, 20):
        for gpp in range(1, 22):
            r = part_ranges(K, gpp)
            groups = [k for k0, nk in r for k in range(k0 + nk - 1, k0 - 1, -1)]
            assert groups == list(range(K - 1, -1, -1)), (K, gpp, r)
            assert all(0 < nk <= gpp for _, nk in r) and len(r) == -(-K // gpp)
            assert r[0][1] == max(nk for _, nk in r), "the workspaces are sized for the first range walked"


# ------------------------------------------------------------------------------------------------ the recorded schedule
class RecordingExt:
    """stands in for ``test_time_training``: every scan entry records its name, the stream it was issued on and its integers"""

    def __init__(self, log, current):
        self.log, self.current, self.spaces = log, current, []

    def resolved_impl(self, B, NH, NC, CS, F, G, act_dtype=BF16, mlp=True, backward=False, *, impl=None):
        return "mfma" if impl == "mfma" or not backward else "generic"

    def ttt_forward(self, *a):
        pass

    def pre_forward(self, *a, **k):
        pass

    def pre_backward_partials(self, NH):
        return 1

    def pre_backward(self, *a, **k):
        pass

    def ttt_backward(self, *a):
        assert len(a) == 43
        self.log.append(("ttt_backward", self.current[0], a[-1]))

    def ttt_backward_impl(self, impl, *a):
        assert len(a) == 43
        self.log.append(("ttt_backward_impl", self.current[0], impl, a[-1], a[11] is not None))

    def mlp_backward_parts_slots(self, B, NH, NC, CS, F, G, nk, act_dtype=BF16, *, impl=None):
        assert impl == "mfma"
        return B * NH * nk * G * SLOT

    def mlp_backward_parts_carry(self, B, NH, NC, CS, F, G, act_dtype=BF16, *, impl=None):
        assert impl == "mfma"
        return B * NH * 8192

    def _space(self, slots):
        if not any(s is slots for s in self.spaces):
            self.spaces.append(slots)
        return next(i for i, s in enumerate(self.spaces) if s is slots)

    def ttt_recompute_groups(self, *a, impl=None):
        assert len(a) == 42 + 4 and impl == "mfma"
        needed = (1, 2, 3, 4, 5, 6, 7, 8, 9)
        assert all((a[i] is not None) == (i in needed) for i in range(42)), "the recompute is given what it needs and nothing else"
        G, k0, nk, slots = a[42:]
        assert slots.numel() * slots.element_size() >= a[1].shape[0] * a[1].shape[1] * nk * G * SLOT
        self.log.append(("recompute", self.current[0], G, k0, nk, self._space(slots)))

    def ttt_sweep_groups(self, *a, impl=None):
        assert len(a) == 42 + 5 and impl == "mfma"
        assert all(a[i] is None for i in range(6, 27)), "no checkpoints, no XQW, none of the sixteen *_group buffers"
        assert all(a[i] is not None for i in list(range(6)) + list(range(27, 42)))
        assert all(a[27 + i] is a[34 + i] for i in range(4)), "the state gradient is carried in place"
        G, k0, nk, slots, carry = a[42:]
        assert carry.dtype == torch.float32 and carry.numel() * 4 == a[0].shape[0] * a[0].shape[1] * 8192
        self.log.append(("sweep", self.current[0], G, k0, nk, self._space(slots)))


@pytest.fixture
def fake(monkeypatch):
    from ttt_amd.models.ssm import fused, mlp_tk
    log, current = fake_streams(monkeypatch)
    ext = RecordingExt(log, current)
    monkeypatch.setattr(mlp_tk, "_ext", lambda: ext)
    monkeypatch.setattr(fused, "_ext", lambda: ext)
    return ext


def _tk_backward(CS, NC, G, B=1, NH=2, F=64):
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt).requires_grad_(True)
    out = TkMLP.apply(z(NH, F), z(NH, F), z(B, NH, F, 4 * F), z(B, NH, 1, 4 * F), z(B, NH, 4 * F, F), z(B, NH, 1, F),
                      z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, 1, CS, dt=BF16), G)
    out.backward(torch.zeros_like(out))


def _fused_backward(CS, NC, G, B=1, NH=2, F=64):
    from ttt_amd.models.ssm.fused import FusedPreScanMLP
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt).requires_grad_(True)
    raw = [z(B, NC * CS, NH * F, dt=BF16) for _ in range(3)]
    out = FusedPreScanMLP.apply(*raw, z(NH, F), z(NH, F), None, None, None, NH, z(B, NH, F, 4 * F), z(B, NH, 1, 4 * F),
                                z(B, NH, 4 * F, F), z(B, NH, 1, F), z(B, NH, NC, 1, CS, dt=BF16), G)
    out.backward(torch.zeros_like(out))


def _scan_calls(log):
    return [c for c in log if c[0] in ("recompute", "sweep", "ttt_backward", "ttt_backward_impl")]


@pytest.mark.parametrize("backward", [_tk_backward, _fused_backward], ids=["TkMLP", "FusedPreScanMLP"])
def test_schedule_of_the_backward_in_parts(switch, fake, backward):
    """NC = 9, G = 2: K = 5 groups in ranges of 2 -> [3, 5), [1, 3), [0, 1).  The recompute of range n + 1 is issued (on the side
    stream) before the sweep of range n (on the caller's stream); the two workspaces alternate; a sweep waits for its recompute's
    event, the recompute of range n + 2 for the event of sweep n, which read the workspace it writes; the side stream first waits for
    the caller's stream and is joined into it at the end."""
    switch.cs16_bwd_impl, switch.cs16_backward_parts = "mfma", 2
    backward(16, 9, 2)
    log = fake.log
    assert _scan_calls(log) == [("recompute", "side", 2, 3, 2, 0), ("recompute", "side", 2, 1, 2, 1), ("sweep", "main", 2, 3, 2, 0),
                                ("recompute", "side", 2, 0, 1, 0), ("sweep", "main", 2, 1, 2, 1), ("sweep", "main", 2, 0, 1, 0)]
    assert len(fake.spaces) == 2
    sync = [c for c in log if c[0] in ("wait_stream", "wait_event", "record", "recompute", "sweep")]
    ready, swept = (0, 1, 2), (3, 4, 5)                  # the events in the order they were made
    assert sync == [
        ("wait_stream", "side", "main"),
        ("recompute", "side", 2, 3, 2, 0), ("record", "side", ready[0]),
        ("recompute", "side", 2, 1, 2, 1), ("record", "side", ready[1]),
        ("wait_event", "main", ready[0]), ("sweep", "main", 2, 3, 2, 0), ("record", "main", swept[0]),
        ("wait_event", "side", swept[0]), ("recompute", "side", 2, 0, 1, 0), ("record", "side", ready[2]),
        ("wait_event", "main", ready[1]), ("sweep", "main", 2, 1, 2, 1), ("record", "main", swept[1]),
        ("wait_event", "main", ready[2]), ("sweep", "main", 2, 0, 1, 0), ("record", "main", swept[2]),
        ("wait_stream", "main", "side")]


@pytest.mark.parametrize("backward", [_tk_backward, _fused_backward], ids=["TkMLP", "FusedPreScanMLP"])
def test_one_range_and_off(switch, fake, backward):
    """more groups per part than the sequence has: one range, one workspace; 0: the one call with its *_init_group scratch"""
    switch.cs16_bwd_impl, switch.cs16_backward_parts = "mfma", 8
    backward(16, 9, 2)
    assert _scan_calls(fake.log) == [("recompute", "side", 2, 0, 5, 0), ("sweep", "main", 2, 0, 5, 0)] and len(fake.spaces) == 1
    fake.log.clear()
    switch.cs16_backward_parts = 0
    backward(16, 9, 2)
    assert _scan_calls(fake.log) == [("ttt_backward_impl", "main", "mfma", 2, True)]


@pytest.mark.parametrize("backward", [_tk_backward, _fused_backward], ids=["TkMLP", "FusedPreScanMLP"])
def test_switch_is_ignored_unless_the_backward_is_the_mfma_one(switch, fake, backward):
    """``cs16_bwd_impl`` = "auto": ``bwd_impl`` is None and the one call runs whatever the parts switch says; at mini-batches of 64
    too, with either ``cs16_bwd_impl``"""
    switch.cs16_backward_parts = 2
    switch.cs16_bwd_impl = "auto"
    backward(16, 9, 2)
    assert _scan_calls(fake.log) == [("ttt_backward", "main", 2)]
    for impl in ("auto", "mfma"):
        fake.log.clear()
        switch.cs16_bwd_impl = impl
        backward(64, 5, 2)
        assert _scan_calls(fake.log) == [("ttt_backward", "main", 2)]
    assert not any(c[0] in ("wait_stream", "wait_event", "record") for c in fake.log)
