"""``HipLinear.backward_front`` (ttt_amd/models/ssm/linear_hip.py), the switch of the front / chain stage of the TTT-Linear backward in
parts, without a GPU: off by default, read from TTT_LINEAR_BACKWARD_FRONT, anything but "0" / "1" refused with the variable's name, and
with an extension that has no part entries - the oracle-backed stand-in of oracle/cpu_ext.py - the one call runs whatever the switch
says."""
import os
import subprocess
import sys

import torch

from oracle import cpu_ext
from oracle import ttt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _import_with(value):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "ttt-video-dit_amd"), ROOT]))
    for name in ("TTT_LINEAR_BACKWARD_FRONT", "TTT_LINEAR_BACKWARD_PARTS"):
        env.pop(name, None)
    if value is not None:
        env["TTT_LINEAR_BACKWARD_FRONT"] = value
    code = "from ttt_amd.models.ssm.linear_hip import HipLinear; print('front', HipLinear.backward_front, 'parts', HipLinear.backward_parts)"
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)


def test_switch_is_off_by_default_and_read_from_the_environment():
    r = _import_with(None)
    assert r.returncode == 0 and "front 0 parts 0" in r.stdout, r.stderr
    r = _import_with("0")
    assert r.returncode == 0 and "front 0 parts 0" in r.stdout, r.stderr
    r = _import_with("1")
    assert r.returncode == 0 and "front 1 parts 0" in r.stdout, r.stderr          # (it selects nothing by itself)
    for bad in ("2", "on", ""):
        r = _import_with(bad)
        assert r.returncode != 0 and "TTT_LINEAR_BACKWARD_FRONT: expected '0' (off) or '1'" in r.stderr, (bad, r.stderr)


def _grads(parts, front):
    from ttt_amd.models.ssm.linear_hip import HipLinear
    B, NH, NC, CS, F, G = 1, 2, 5, 16, 64, 2
    d = O.make_inputs("linear", B, NH, NC, CS, F, seed=3)
    leaves = [d[k].clone().requires_grad_(True) for k in ("ln_w", "ln_b", "W1", "b1", "XQ", "XV", "XK", "eta")]
    st = [p.unsqueeze(0).expand(B, *p.shape) for p in leaves[2:4]]
    old = HipLinear.backward_parts, HipLinear.backward_front
    HipLinear.backward_parts, HipLinear.backward_front = parts, front
    try:
        out = HipLinear.apply(leaves[0], leaves[1], *st, *leaves[4:], G)
        out.backward(d["dOut"])
    finally:
        HipLinear.backward_parts, HipLinear.backward_front = old
    return [t.grad for t in leaves]


def test_stand_in_without_the_part_entries_runs_the_one_call():
    cpu_ext.install()
    try:
        import test_time_training as fake
        assert not hasattr(fake, "ttt_linear_sweep_groups") and not hasattr(fake, "ttt_linear_chain_groups")
        calls = []
        one_call = fake.ttt_linear_backward
        fake.ttt_linear_backward = lambda *a: (calls.append(1), one_call(*a))[1]
        try:
            off, front_only, both = _grads(0, 0), _grads(0, 1), _grads(1, 1)
        finally:
            fake.ttt_linear_backward = one_call
        assert len(calls) == 3
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(off, front_only, both))
        from ttt_amd.models.ssm.linear_hip import HipLinear
        assert HipLinear.backward_front == 0 and HipLinear.backward_parts == 0
    finally:
        cpu_ext.uninstall()
