"""The schedule of the TTT-Linear backward in parts (``linear_hip.backward_in_parts`` behind ``HipLinear.backward_parts`` /
``backward_front``), without a device: with an extension that only records its calls and stand-ins for the two streams and their
events - which entries ``HipLinear.backward`` reaches, in which order, on which stream, into which workspace, with which tensors."""
import pytest
import torch

from helpers import fake_streams

BF16 = torch.bfloat16
SLOT, RECORD = 16 * 1024 + 256, 19456
ENTRIES = ("ttt_linear_recompute_groups", "ttt_linear_sweep_groups", "ttt_linear_front_groups", "ttt_linear_chain_groups")


class RecordingExt:
    """stands in for ``test_time_training``: every scan entry records its name, the stream it was issued on and its integers.
    ``without``: entries this extension does not have."""

    def __init__(self, log, current, without=()):
        self.log, self.current, self.slot_spaces, self.record_spaces = log, current, [], []
        for name in ENTRIES:
            if name not in without:
                setattr(self, name, getattr(self, "_" + name))

    def resolved_impl(self, B, NH, NC, CS, F, G, act_dtype=BF16, mlp=True, backward=False, *, impl=None):
        return "mfma"

    def ttt_linear_forward(self, *a):
        assert len(a) == 12

    def ttt_linear_backward(self, *a):
        assert len(a) == 22 and all(t is not None for t in a)
        self.log.append(("ttt_linear_backward", self.current[0], a[-1]))

    def linear_backward_parts_slots(self, B, NH, NC, CS, F, G, nk, act_dtype=BF16, *, impl=None):
        return B * NH * nk * (G + 1) * SLOT

    def linear_backward_parts_carry(self, B, NH, NC, CS, F, G, act_dtype=BF16, *, impl=None):
        return B * NH * 8 * (64 if CS == 16 else 256) * 4

    def linear_backward_front_records(self, B, NH, NC, CS, F, G, nk, act_dtype=BF16, *, impl=None):
        return B * NH * nk * G * RECORD if CS == 16 else 0

    @staticmethod
    def _space(spaces, t):
        if not any(s is t for s in spaces):
            spaces.append(t)
        return next(i for i, s in enumerate(spaces) if s is t)

    def _entry(self, name, a, n_tail, given):
        """``a``: impl, the 21 tensors, G, k0, nk and ``n_tail`` workspaces; ``given``: the fields that are tensors - the rest is None"""
        import test_time_training as binding
        assert len(a) == 1 + 21 + 3 + n_tail and a[0] is None
        tensors, (G, k0, nk), tail = a[1:22], a[22:25], a[25:]
        assert all((t is not None) == (f in given) for f, t in zip(binding.LIN_BWD_FIELDS, tensors)), f"{name}: what it touches, nothing else"
        B, NH = tensors[1].shape[:2]
        assert tail[0].numel() * tail[0].element_size() >= self.linear_backward_parts_slots(B, NH, 0, 16, 64, G, nk)
        return tensors, tail, (name, self.current[0], G, k0, nk, self._space(self.slot_spaces, tail[0]))

    def _carried(self, tensors, carry):
        assert tensors[8] is tensors[15] and tensors[9] is tensors[16], "dW1 / db1 are carried in place"
        B, NH, _, CS, _ = tensors[0].shape
        assert carry.dtype == torch.float32 and carry.numel() * 4 == self.linear_backward_parts_carry(B, NH, 0, CS, 64, 0)

    def _records(self, tensors, records, G, nk):
        B, NH = tensors[0].shape[:2]
        assert records.numel() * records.element_size() >= self.linear_backward_front_records(B, NH, 0, 16, 64, G, nk)
        return self._space(self.record_spaces, records)

    def _ttt_linear_recompute_groups(self, *a):
        import test_time_training as binding
        _, _, call = self._entry("recompute", a, 1, binding._LIN_RECOMPUTE_FIELDS)
        self.log.append(call)

    def _ttt_linear_sweep_groups(self, *a):
        import test_time_training as binding
        tensors, tail, call = self._entry("sweep", a, 2, set(binding.LIN_BWD_FIELDS) - binding._LIN_SWEEP_UNUSED)
        self._carried(tensors, tail[1])
        self.log.append(call)

    def _ttt_linear_front_groups(self, *a):
        import test_time_training as binding
        tensors, tail, call = self._entry("front", a, 2, binding._LIN_FRONT_FIELDS)
        self.log.append(call + (self._records(tensors, tail[1], call[2], call[4]),))

    def _ttt_linear_chain_groups(self, *a):
        import test_time_training as binding
        tensors, tail, call = self._entry("chain", a, 3, set(binding.LIN_BWD_FIELDS) - binding._LIN_CHAIN_UNUSED)
        self._carried(tensors, tail[2])
        self.log.append(call + (self._records(tensors, tail[1], call[2], call[4]),))


@pytest.fixture
def switches():
    from ttt_amd.models.ssm.linear_hip import HipLinear
    old = HipLinear.backward_parts, HipLinear.backward_front, HipLinear.cs64_impl
    yield HipLinear
    HipLinear.backward_parts, HipLinear.backward_front, HipLinear.cs64_impl = old


def _fake(monkeypatch, without=()):
    from ttt_amd.models.ssm import linear_hip
    log, current = fake_streams(monkeypatch)
    ext = RecordingExt(log, current, without)
    monkeypatch.setattr(linear_hip, "_ext", lambda: ext)
    return ext


def _backward(CS, NC=9, G=2, B=1, NH=2, F=64):
    from ttt_amd.models.ssm.linear_hip import HipLinear
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt).requires_grad_(True)
    out = HipLinear.apply(z(NH, F), z(NH, F), z(B, NH, F, F), z(B, NH, 1, F), z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, CS, F, dt=BF16),
                          z(B, NH, NC, CS, F, dt=BF16), z(B, NH, NC, CS, CS, dt=BF16), G)
    out.backward(torch.zeros_like(out))


def _scan_calls(log):
    return [c for c in log if c[0] in ("recompute", "sweep", "front", "chain", "ttt_linear_backward")]


def _sync(log):
    return [c for c in log if c[0] in ("wait_stream", "wait_event", "record", "recompute", "sweep", "front", "chain")]


def test_schedule_of_the_backward_in_parts(switches, monkeypatch):
    """NC = 9, G = 2: K = 5 groups in ranges of 2 -> [3, 5), [1, 3), [0, 1).  The recompute of range n + 1 is issued (on the side
    stream) before the sweep of range n (on the caller's stream); the two workspaces alternate; a sweep waits for its recompute's
    event, the recompute of range n + 2 for the event of sweep n, which read the workspace it writes; the side stream first waits for
    the caller's stream and is joined into it at the end.  (The log of tests/test_mlp16_bwd_parts_switch_cpu.py.)"""
    ext = _fake(monkeypatch)
    switches.backward_parts, switches.backward_front = 2, 0
    _backward(16)
    ready, swept = (0, 1, 2), (3, 4, 5)                  # the events in the order they were made
    assert _sync(ext.log) == [
        ("wait_stream", "side", "main"),
        ("recompute", "side", 2, 3, 2, 0), ("record", "side", ready[0]),
        ("recompute", "side", 2, 1, 2, 1), ("record", "side", ready[1]),
        ("wait_event", "main", ready[0]), ("sweep", "main", 2, 3, 2, 0), ("record", "main", swept[0]),
        ("wait_event", "side", swept[0]), ("recompute", "side", 2, 0, 1, 0), ("record", "side", ready[2]),
        ("wait_event", "main", ready[1]), ("sweep", "main", 2, 1, 2, 1), ("record", "main", swept[1]),
        ("wait_event", "main", ready[2]), ("sweep", "main", 2, 0, 1, 0), ("record", "main", swept[2]),
        ("wait_stream", "main", "side")]
    assert len(ext.slot_spaces) == 2 and not ext.record_spaces


def test_schedule_with_the_front(switches, monkeypatch):
    """the same, ``backward_front`` = 1: the front of a range is issued on the side stream right behind its recompute, in front of the
    ``ready`` record; the chain takes the sweep's place; the record workspaces alternate with the slot workspaces"""
    ext = _fake(monkeypatch)
    switches.backward_parts, switches.backward_front = 2, 1
    _backward(16)
    ready, swept = (0, 1, 2), (3, 4, 5)
    assert _sync(ext.log) == [
        ("wait_stream", "side", "main"),
        ("recompute", "side", 2, 3, 2, 0), ("front", "side", 2, 3, 2, 0, 0), ("record", "side", ready[0]),
        ("recompute", "side", 2, 1, 2, 1), ("front", "side", 2, 1, 2, 1, 1), ("record", "side", ready[1]),
        ("wait_event", "main", ready[0]), ("chain", "main", 2, 3, 2, 0, 0), ("record", "main", swept[0]),
        ("wait_event", "side", swept[0]), ("recompute", "side", 2, 0, 1, 0), ("front", "side", 2, 0, 1, 0, 0), ("record", "side", ready[2]),
        ("wait_event", "main", ready[1]), ("chain", "main", 2, 1, 2, 1, 1), ("record", "main", swept[1]),
        ("wait_event", "main", ready[2]), ("chain", "main", 2, 0, 1, 0, 0), ("record", "main", swept[2]),
        ("wait_stream", "main", "side")]
    assert len(ext.slot_spaces) == 2 and len(ext.record_spaces) == 2


def test_one_range_is_the_one_call(switches, monkeypatch):
    """more groups per part than the sequence has (K <= gpp): the one call, no stream or event traffic"""
    ext = _fake(monkeypatch)
    switches.backward_parts, switches.backward_front = 8, 1
    _backward(16)
    assert ext.log == [("ttt_linear_backward", "main", 2)]


def test_the_front_is_for_mini_batches_of_16(switches, monkeypatch):
    ext = _fake(monkeypatch)
    switches.backward_parts, switches.backward_front = 2, 1
    _backward(64)
    assert [c[0] for c in _scan_calls(ext.log)] == ["recompute", "recompute", "sweep", "recompute", "sweep", "sweep"]
    assert len(ext.slot_spaces) == 2 and not ext.record_spaces


def test_an_extension_without_the_entries(switches, monkeypatch):
    """no chain entry: the sweep; no sweep entry: the one call"""
    switches.backward_parts, switches.backward_front = 2, 1
    ext = _fake(monkeypatch, without=("ttt_linear_chain_groups",))
    _backward(16)
    assert [c[0] for c in _scan_calls(ext.log)] == ["recompute", "recompute", "sweep", "recompute", "sweep", "sweep"]
    ext = _fake(monkeypatch, without=("ttt_linear_sweep_groups",))
    _backward(16)
    assert ext.log == [("ttt_linear_backward", "main", 2)]
