"""The two-wave TTT-Linear forward scan at mini-batches of 16 on the device (``ttt_hip_linear_forward_chunk_split16`` of
include/ttt_hip_lin_split16.h; ``lin16::split::forward_part`` of csrc/ttt_lin16_split_body.h: the chain role on wave 0, the output role
on wave 1) against the one-wave scan of the same build - the bits, not a tolerance -, its refusals, and the layer switch
``HipLinear.cs16_scan_split`` in one piece and in the parts of the pipelined forward."""
import pytest
import torch

from helpers import rel_l2
from oracle import ttt_oracle as O
from test_kernels_gpu import DEV, ext, round_acts
from test_linear_parts_gpu import _bufs, _dev_inputs, _layer, _run
from test_scan_oracle_gpu import GUARD, assert_written_inside, guarded

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _walk(e, X, le, ln, st, G, B, NH, NC, cuts):
    """the split scan as the parts the cuts make, the state (between guards too) carried in place -> out, W1c, b1c, final state"""
    bufs = _bufs(B, NH, NC, 16, -(-NC // G))
    bufs["W1"], bufs["b1"] = guarded(tuple(st[0].shape), torch.float32), guarded(tuple(st[1].shape), torch.float32)
    state = [bufs["W1"][1], bufs["b1"][1]]
    state[0].copy_(st[0]), state[1].copy_(st[1])
    for s0, s1 in zip(cuts[:-1], cuts[1:]):
        e.ttt_linear_forward_chunk_split16(None, *X, le, *ln, *state, bufs["W1c"][1], bufs["b1c"][1], bufs["out"][1], G, s0, s1 - s0)
    torch.cuda.synchronize()
    if cuts[-1] == NC:
        assert_written_inside(bufs, f"parts {cuts}")
    else:
        for name, (buf, view) in bufs.items():
            assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"parts {cuts}: write outside {name}"
        out = bufs["out"][1]
        assert not torch.isnan(out[:, :, :cuts[-1]].float()).any() and bool(torch.isnan(out[:, :, cuts[-1]:].float()).all())
    return bufs["out"][1], bufs["W1c"][1], bufs["b1c"][1], state


def _one_wave_and_one_call_split(e, X, le, ln, st, G, B, NH, NC):
    """(out, W1c, b1c) of ``ttt_linear_forward_impl(None, ...)`` and of the one-call split form, each between guards"""
    res = []
    keep = [t.clone() for t in st]
    for fwd in (e.ttt_linear_forward_impl, e.ttt_linear_forward_split16):
        b = _bufs(B, NH, NC, 16, -(-NC // G))
        fwd(None, *X, le, *ln, *st, b["W1c"][1], b["b1c"][1], b["out"][1], G)
        torch.cuda.synchronize()
        assert_written_inside(b, fwd.__name__)
        assert torch.equal(st[0], keep[0]) and torch.equal(st[1], keep[1]), f"{fwd.__name__} wrote its initial state"
        res.append(tuple(b[k][1] for k in ("out", "W1c", "b1c")))
    return res


@pytest.mark.parametrize("B,NH,NC,G,cuttings", [(2, 5, 11, 3, ((0, 1, 2, 7, 11), (0, 11))), (1, 1, 1, 1, ((0, 1),))])
def test_split_scan_carries_the_one_wave_bits(B, NH, NC, G, cuttings):
    """out, W1c, b1c of the one-call split form and of every cutting are the bits of ``ttt_linear_forward_impl(None, ...)``; the final
    states are equal across cuttings; the state leaving [0, 6) is checkpoint 2; the state moved; nothing is written outside the guards;
    the one-call form did not write its initial state."""
    e = ext()
    assert e.get_impl() == "auto"
    assert e.resolved_impl(B, NH, NC, 16, 64, G, BF, mlp=False, backward=False) == "mfma"
    d = round_acts(O.make_inputs("linear", B, NH, NC, 16, 64, seed=916), BF)
    X, le, ln, st = _dev_inputs(d, B)
    before = dict(e.linear_split16_calls)
    (out0, W1c0, b1c0), (out1, W1c1, b1c1) = _one_wave_and_one_call_split(e, X, le, ln, st, G, B, NH, NC)
    assert torch.equal(out1, out0), "one call: output"
    assert torch.equal(W1c1, W1c0) and torch.equal(b1c1, b1c0), "one call: checkpoints"
    walks = [_walk(e, X, le, ln, st, G, B, NH, NC, cuts) for cuts in cuttings]
    for cuts, (out, W1c, b1c, state) in zip(cuttings, walks):
        assert torch.equal(out, out0), f"parts {cuts}: output"
        assert torch.equal(W1c, W1c0) and torch.equal(b1c, b1c0), f"parts {cuts}: checkpoints"
        assert torch.equal(state[0], walks[0][3][0]) and torch.equal(state[1], walks[0][3][1]), f"parts {cuts}: final state"
        assert not torch.equal(state[0], st[0]) and not torch.equal(state[1], st[1]), "the state did not move"
    assert e.linear_split16_calls["whole"] == before["whole"] + 1
    assert e.linear_split16_calls["chunk"] == before["chunk"] + sum(len(c) - 1 for c in cuttings)
    # the final state against the one-wave chunk entry's
    ref = [t.clone() for t in st]
    b = _bufs(B, NH, NC, 16, -(-NC // G))
    e.ttt_linear_forward_chunk(None, *X, le, *ln, *ref, b["W1c"][1], b["b1c"][1], b["out"][1], G, 0, NC)
    torch.cuda.synchronize()
    assert torch.equal(walks[0][3][0], ref[0]) and torch.equal(walks[0][3][1], ref[1]), "final state of the one-wave scan"
    if NC > 6:
        assert 6 // G == 2
        head = _walk(e, X, le, ln, st, G, B, NH, NC, (0, 6))
        assert torch.equal(head[3][0], W1c0[:, :, 2]) and torch.equal(head[3][1], b1c0[:, :, 2]), "the state leaving [0, 6) is checkpoint 2"


def test_split_scan_many_workgroups():
    """B = 2, NH = 48, NC = 300, G = 16: 96 workgroups and 150 reuses of each slot.  The bits of the one-wave kernel, and the 1e-2
    rel-L2 against the fp64 oracle of tests/test_kernels_gpu.py::test_mfma_linear_cs16_vs_oracle (output and checkpoints)."""
    e = ext()
    B, NH, NC, G = 2, 48, 300, 16
    d = round_acts(O.make_inputs("linear", B, NH, NC, 16, 64, seed=317), BF)
    X, le, ln, st = _dev_inputs(d, B)
    (out0, W1c0, b1c0), (out1, W1c1, b1c1) = _one_wave_and_one_call_split(e, X, le, ln, st, G, B, NH, NC)
    assert torch.equal(out1, out0) and torch.equal(W1c1, W1c0) and torch.equal(b1c1, b1c0)
    ro, rc, _ = O.linear_forward(*(d[k].double() for k in ("XQ", "XK", "XV")), d["eta"].double()[:, :, :, -1, :, None], d["ln_w"].double(),
                                 d["ln_b"].double(), *(d[k].double().unsqueeze(0).expand(B, *d[k].shape) for k in ("W1", "b1")), G)
    errs = {"XQW": rel_l2(out1, ro), "ck0": rel_l2(W1c1, rc[0]), "ck1": rel_l2(b1c1, rc[1])}
    print("split16 many workgroups vs fp64 oracle", {k: float(f"{v:.3e}") for k, v in errs.items()})
    assert all(v < 1e-2 for v in errs.values()), errs


def test_split_scan_refusals_leave_the_buffers_untouched():
    """mini-batches of 64 (auto and on request), fp32, F != 64, the generic kernels, a range not inside [0, NC): RuntimeError naming the
    entry, and nothing launched - the NaN-filled buffers stay NaN"""
    e = ext()
    B, NH, NC, G = 1, 2, 5, 2
    touched = []

    def refused(CS, F, act, impl, s0, ns, match):
        d = O.make_inputs("linear", B, NH, NC, CS, F, seed=3)
        X = [d[k].to(DEV, act).contiguous() for k in ("XQ", "XK", "XV")]
        le = d["eta"][:, :, :, -1, :, None].to(DEV, act).contiguous()
        ln = [d[k].to(DEV, torch.float32).contiguous() for k in ("ln_w", "ln_b")]
        st = [torch.full((B, NH, F, F), float("nan"), device=DEV), torch.full((B, NH, 1, F), float("nan"), device=DEV)]
        bufs = [torch.full((B, NH, 3, F, F), float("nan"), device=DEV), torch.full((B, NH, 3, 1, F), float("nan"), device=DEV),
                torch.full((B, NH, NC, CS, F), float("nan"), device=DEV, dtype=act)]
        with pytest.raises(RuntimeError, match=match):
            e.ttt_linear_forward_chunk_split16(impl, *X, le, *ln, *st, *bufs, G, s0, ns)
        if (s0, ns) == (0, NC):
            with pytest.raises(RuntimeError, match=match):
                e.ttt_linear_forward_split16(impl, *X, le, *ln, *st, *bufs, G)
        touched.extend(st + bufs)

    serves = r"linear_forward_chunk_split16: the two-wave scan serves"
    refused(64, 64, BF, None, 0, NC, serves)
    refused(64, 64, BF, "mfma", 0, NC, serves)
    refused(16, 64, torch.float32, None, 0, NC, serves)
    refused(16, 32, BF, None, 0, NC, serves)
    refused(16, 64, BF, "generic", 0, NC, serves)
    for s0, ns in ((-1, 2), (0, 0), (3, 3), (5, 1), (2 ** 31 - 1, 2)):
        refused(16, 64, BF, None, s0, ns, r"linear_forward_chunk_split16: the part \[step0, step0 \+ nsteps\) must lie inside \[0, NC\)")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t.float()).all()) for t in touched)          # nothing was launched


@pytest.fixture
def switch():
    from ttt_amd.models.ssm.linear_hip import HipLinear
    old = HipLinear.cs16_scan_split
    yield HipLinear
    HipLinear.cs16_scan_split = old


def test_hiplinear_with_the_switch_on_gives_the_bits_of_the_switch_off(switch):
    """``HipLinear.apply`` in one piece: the output and, through autograd, all eight gradients"""
    e = ext()
    B, NH, NC, G = 2, 3, 9, 4
    d = round_acts(O.make_inputs("linear", B, NH, NC, 16, 64, seed=23), BF)

    def run(v):
        switch.cs16_scan_split = v
        leaves = [d[k].to(DEV, torch.float32).clone().requires_grad_(True) for k in ("ln_w", "ln_b", "W1", "b1")] + \
                 [d[k].to(DEV, BF).clone().requires_grad_(True) for k in ("XQ", "XV", "XK", "eta")]
        st = [p.unsqueeze(0).expand(B, *p.shape) for p in leaves[2:4]]
        before = dict(e.linear_split16_calls)
        out = switch.apply(leaves[0], leaves[1], *st, *leaves[4:], G)
        out.backward(d["dOut"].to(DEV, BF))
        torch.cuda.synchronize()
        ran = e.linear_split16_calls["whole"] - before["whole"]
        return out.detach(), [t.grad for t in leaves], ran

    out0, g0, ran0 = run(0)
    out1, g1, ran1 = run(1)
    assert (ran0, ran1) == (0, 1), "the call counter of the split binding"
    assert torch.equal(out1, out0)
    assert len(g0) == 8 and all(g is not None for g in g0)
    for name, a, b in zip(("ln_w", "ln_b", "W1", "b1", "XQ", "XV", "XK", "eta"), g1, g0):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("grad,G", [(True, 4), (False, 10 ** 6)])
def test_layer_in_parts_with_the_switch_on_gives_the_bits_of_the_switch_off(switch, monkeypatch, grad, G):
    """the TTT-Linear layer with ``linear_pipeline_parts = 3`` at a step quantum of 8 (40 steps: parts of whole checkpoint groups with
    grad, the any-step cut with one group under no_grad): every part of the pre-pass goes through the split chunk entry, and the layer's
    output, input gradient and parameter gradients are the bits of the switch off"""
    from ttt_amd.models.ssm import pipeline
    e = ext()
    monkeypatch.setattr(pipeline, "LIN_QUANTUM", 8)
    m, meta = _layer(16, G, 640, 1)
    gen = torch.Generator().manual_seed(11)
    x0, dy = (torch.randn(1, 640, 128, generator=gen).to(DEV, BF) for _ in range(2))
    m.ttt.linear_pipeline_parts = 3
    res = []
    for v in (0, 1):
        switch.cs16_scan_split = v
        before = dict(e.linear_split16_calls)
        res.append(_run(m, meta, x0, dy, False, grad))
        ran = {k: e.linear_split16_calls[k] - before[k] for k in before}
        assert ran == ({"whole": 0, "chunk": 0} if v == 0 else {"whole": 0, "chunk": 3 if grad else 2}), (v, ran)
    (y0, dx0, p0), (y1, dx1, p1) = res
    assert torch.isfinite(y1.float()).all() and float(y1.float().norm()) > 0
    assert torch.equal(y1, y0)
    if grad:
        assert torch.equal(dx1, dx0) and sorted(p0) == sorted(p1) and p0
        for k in p0:
            assert torch.equal(p1[k], p0[k]), k
