"""The REFERENCE's own autograd wrapper on top of this repo's extension interface, replayed from a stored fixture.

``ttt/models/ssm/mlp_tk.py`` does ``import test_time_training`` and calls ``ttt_forward`` with 15 tensors + G
(mlp_tk.py:116-133) and ``ttt_backward`` with 42 tensors + G (mlp_tk.py:227-275).  tests/golden/reference_tkmlp.pt holds, at
seeded sample positions, what that very code - ``TkMLP.apply`` - returned when it ran against the CPU stand-in of the extension
(oracle/cpu_ext.py: the same positional-buffer contract as the ctypes binding, backed by the oracle; TEST INFRASTRUCTURE), and
what the reference's ops path (``ops/ttt_mlp.py``) returns on the same inputs (tests/golden/gen_reference_tkmlp_golden.py).
Here this repo's wrapper (ttt_amd/models/ssm/mlp_tk.py) runs on the same stand-in and inputs, and the ops path runs as the
oracle's restatement of it (``oracle.ttt_oracle.scan_dual``, fp32 on the bf16-rounded activations), pinned to the reference's
values at the stored positions: the wrapper returns what the reference's wrapper returned, output and all ten gradients agree
with the ops path within the bf16 op-boundary tolerance, and the buffers have the shapes the interface documents.
The real binding's signatures (``ttt-video-dit_amd/test_time_training/__init__.py``) are checked for the same arity, so what
passes here is what the reference would call on the GPU box.
"""
import inspect
import os

import pytest
import torch

from helpers import load_golden, rel_l2
from oracle import cpu_ext as fake_ext
from oracle import ttt_oracle as O


def test_real_binding_has_the_reference_arity():
    """16 / 43 positional parameters: what mlp_tk.py:116-133 / 227-275 pass (the Linear pair: 12 / 22)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_ttt_binding_sig", os.path.join(root, "ttt-video-dit_amd", "test_time_training", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                     # importing does not load the library
    n = lambda f: len(inspect.signature(f).parameters)
    assert (n(mod.ttt_forward), n(mod.ttt_backward), n(mod.ttt_linear_forward), n(mod.ttt_linear_backward)) == (16, 43, 12, 22)


@pytest.mark.parametrize("B,NH,NC,G", [(1, 2, 5, 2), (2, 3, 4, 4)])
def test_reference_tkmlp_apply_on_this_interface(B, NH, NC, G):
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    gold = load_golden("reference_tkmlp.pt")[f"{B}-{NH}-{NC}-{G}"]
    assert gold["G"] == G
    d = O.make_inputs(**gold["gen"])
    for k, ref in gold["input_checksums"].items():
        got = float(d[k].double().abs().sum())
        assert abs(got - ref) <= 1e-9 * max(1.0, abs(ref)), f"input RNG drift in {k}: {got} vs {ref}"
    CS, F = gold["gen"]["CS"], gold["gen"]["Fd"]
    tile = lambda w: torch.tile(w.unsqueeze(0), dims=(B, 1, 1, 1))
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("ln_w", "ln_b", "W1", "b1", "W2", "b2", "XQ", "XV", "XK", "eta")}

    def run(fn, cast):
        for v in leaves.values():
            v.grad = None
        a = {k: (cast(v) if k in ("XQ", "XV", "XK", "eta") else v) for k, v in leaves.items()}
        st = [tile(a[k]) for k in ("W1", "b1", "W2", "b2")]
        out = fn(a, st)
        out.float().backward(d["dOut"])
        grads = {k: v.grad.detach().clone() for k, v in leaves.items()}
        grads["eta"] = grads["eta"].sum(-2)
        return out.detach().float(), grads

    fake_ext.install()
    try:        # this repo's wrapper: returns the kernel layout [B,NH,NC,CS,F]
        out_k, g_k = run(lambda a, st: TkMLP.apply(a["ln_w"], a["ln_b"], *st, a["XQ"], a["XV"], a["XK"], a["eta"], G), lambda t: t.to(torch.bfloat16))
    finally:
        fake_ext.uninstall()
    # the reference ops path (restated by the oracle) on the bf16-rounded activations, fp32 arithmetic
    out_o, g_o = run(lambda a, st: O.scan_dual("mlp", a["XQ"], a["XK"], a["XV"], a["eta"], a["ln_w"], a["ln_b"], *st, checkpoint_group_size=G)[0],
                     lambda t: t.to(torch.bfloat16).float())
    assert out_k.shape == (B, NH, NC, CS, F)
    pos = gold["pos"]
    at = lambda t, k: t.reshape(-1)[pos[k].long()]
    # the restated ops path is the reference's at the stored positions (same statements, fp32: reassociation only)
    perrs = {"out": rel_l2(at(out_o, "out"), gold["ops"]["out"]), **{k: rel_l2(at(g_o[k], k), v) for k, v in gold["ops"]["grads"].items()}}
    assert set(perrs) == {"out", *g_o} and all(v < 5e-4 for v in perrs.values()), perrs
    # what the reference's wrapper returned on this interface: the same output and activation / eta gradients; its parameter
    # gradients went through bf16 (this wrapper keeps them in fp32): within bf16 rounding
    assert rel_l2(at(out_k, "out"), gold["wrapper"]["out"]) < 1e-6
    werrs = {k: rel_l2(at(g_k[k], k), v) for k, v in gold["wrapper"]["grads"].items()}
    assert set(werrs) == set(g_k), werrs
    bad = {k: v for k, v in werrs.items() if not v < (5e-3 if k in ("ln_w", "ln_b", "W1", "b1", "W2", "b2") else 1e-6)}
    assert not bad, (bad, werrs)
    # the whole tensors against the ops path
    assert rel_l2(out_k, out_o) < 1e-2
    errs = {k: rel_l2(g_k[k], g_o[k]) for k in g_o}
    bad = {k: v for k, v in errs.items() if not v < 3e-2}
    assert not bad, (bad, errs)
