"""``HipLinear.backward_parts`` (ttt_amd/models/ssm/linear_hip.py), the switch of the TTT-Linear backward in parts, without a GPU: off
by default, a malformed value refused, and with an extension that has no part entries - the oracle-backed stand-in of
oracle/cpu_ext.py - the one call runs whatever the switch says."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import cpu_ext
from oracle import ttt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _import_with(value):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "ttt-video-dit_amd"), ROOT]))
    env.pop("TTT_LINEAR_BACKWARD_PARTS", None)
    if value is not None:
        env["TTT_LINEAR_BACKWARD_PARTS"] = value
    code = "from ttt_amd.models.ssm.linear_hip import HipLinear; print('parts', HipLinear.backward_parts)"
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


def test_switch_is_off_by_default_and_read_from_the_environment():
    r = _import_with(None)
    assert r.returncode == 0 and "parts 0" in r.stdout, r.stderr
    r = _import_with("4")
    assert r.returncode == 0 and "parts 4" in r.stdout, r.stderr
    for bad in ("-1", "two", "1.5", ""):
        r = _import_with(bad)
        assert r.returncode != 0 and "TTT_LINEAR_BACKWARD_PARTS: expected a non-negative integer" in r.stderr, (bad, r.stderr)


def _grads(parts):
    from ttt_amd.models.ssm.linear_hip import HipLinear
    B, NH, NC, CS, F, G = 1, 2, 5, 16, 64, 2
    d = O.make_inputs("linear", B, NH, NC, CS, F, seed=3)
    leaves = [d[k].clone().requires_grad_(True) for k in ("ln_w", "ln_b", "W1", "b1", "XQ", "XV", "XK", "eta")]
    st = [p.unsqueeze(0).expand(B, *p.shape) for p in leaves[2:4]]
    old = HipLinear.backward_parts
    HipLinear.backward_parts = parts
    try:
        out = HipLinear.apply(leaves[0], leaves[1], *st, *leaves[4:], G)
        out.backward(d["dOut"])
    finally:
        HipLinear.backward_parts = old
    return [t.grad for t in leaves]


def test_stand_in_without_the_part_entries_runs_the_one_call():
    cpu_ext.install()
    try:
        import test_time_training as fake
        assert not hasattr(fake, "ttt_linear_sweep_groups")
        calls = []
        one_call = fake.ttt_linear_backward
        fake.ttt_linear_backward = lambda *a: (calls.append(1), one_call(*a))[1]
        try:
            off, on = _grads(0), _grads(1)
        finally:
            fake.ttt_linear_backward = one_call
        assert len(calls) == 2
        assert all(torch.equal(a, b) for a, b in zip(off, on))
        from ttt_amd.models.ssm.linear_hip import HipLinear
        with pytest.raises(ValueError, match="HipLinear.backward_parts: expected a non-negative integer"):
            _grads(-2)
        assert HipLinear.backward_parts == 0
    finally:
        cpu_ext.uninstall()
