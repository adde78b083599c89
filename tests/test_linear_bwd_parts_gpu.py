"""TTT-Linear backward in parts, on the device: the recompute and the reverse walk over ranges of checkpoint groups
(``ttt_hip_linear_recompute_groups`` / ``ttt_hip_linear_sweep_groups`` of include/ttt_hip_bwd_parts.h; ``recompute_groups`` /
``sweep_groups`` of csrc/ttt_lin16_body.h / ttt_lin64_body.h) and the opt-in autograd schedule that uses them
(``HipLinear.backward_parts``, ttt_amd/models/ssm/linear_hip.py).  Every comparison is ``torch.equal`` against the one-call backward:
the step functions of the parts are its steps."""
import pytest
import torch

from helpers import count_calls
from oracle import ttt_oracle as O
from test_kernels_gpu import DEV, ext, round_acts
from test_linear_parts_gpu import _layer, _run
from test_scan_oracle_gpu import GUARD, assert_written_inside, guarded

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GRADS = ("dln_w", "dln_b", "dW1", "db1", "deta", "dXQ", "dXK", "dXV")
GEOMETRIES = [(16, None, 2, 5, 11, 3), (64, "mfma", 2, 3, 7, 3)]          # CS, impl, B, NH, NC, G: K = 4, last group of 2 ; K = 3, of 1
_CASES = {}


def _case(CS, impl, B, NH, NC, G):
    """device inputs, the checkpoints of the one-call forward, non-zero upstream gradients and the one-call backward's eight results;
    made once per geometry and left unchanged"""
    key = (CS, impl, B, NH, NC, G)
    if key not in _CASES:
        e = ext()
        assert e.get_impl() == "auto"
        assert e.resolved_impl(B, NH, NC, CS, 64, G, BF, mlp=False, backward=True, impl=impl) == "mfma"
        K = -(-NC // G)
        d = round_acts(O.make_inputs("linear", B, NH, NC, CS, 64, seed=700 + CS), BF)
        X = [d[k].to(DEV, BF).contiguous() for k in ("XQ", "XK", "XV")]
        le = d["eta"][:, :, :, -1, :, None].to(DEV, BF).contiguous()
        ln = [d[k].to(DEV, F32).contiguous() for k in ("ln_w", "ln_b")]
        st = [d[k].unsqueeze(0).expand(B, *d[k].shape).to(DEV, F32).contiguous() for k in ("W1", "b1")]
        cks = [torch.empty(B, NH, K, 64, 64, device=DEV), torch.empty(B, NH, K, 1, 64, device=DEV)]
        out = torch.empty(B, NH, NC, CS, 64, device=DEV, dtype=BF)
        e.ttt_linear_forward_impl(impl, *X, le, *ln, *st, *cks, out, G)
        gen = torch.Generator().manual_seed(9)
        up = [(0.05 * torch.randn(B, NH, 64, 64, generator=gen)).to(DEV), (0.05 * torch.randn(B, NH, 1, 64, generator=gen)).to(DEV)]
        dOut = d["dOut"].to(DEV, BF).contiguous()
        inputs = dict(XQ=X[0], XK=X[1], XV=X[2], le=le, ln_w=ln[0], ln_b=ln[1], W1c=cks[0], b1c=cks[1], uW=up[0], ub=up[1], dOut=dOut)
        g = _grad_bufs(B, NH, NC, CS)
        grp = [torch.empty(B, NH, G, 64, 64, device=DEV), torch.empty(B, NH, G, 1, 64, device=DEV)]
        e.ttt_linear_backward_impl(impl, *X, le, *ln, *cks, *up, dOut, *grp, *[g[k][1] for k in GRADS], G)
        torch.cuda.synchronize()
        assert_written_inside(g, "one-call backward")
        _CASES[key] = (inputs, {k: v.clone() for k, v in inputs.items()}, {k: g[k][1] for k in GRADS})
    return _CASES[key]


def _grad_bufs(B, NH, NC, CS):
    return {"dln_w": guarded((B, NH, 1, 64), F32), "dln_b": guarded((B, NH, 1, 64), F32), "dW1": guarded((B, NH, 64, 64), F32),
            "db1": guarded((B, NH, 1, 64), F32), "deta": guarded((B, NH, NC, CS, 1), BF), "dXQ": guarded((B, NH, NC, CS, 64), BF),
            "dXK": guarded((B, NH, NC, CS, 64), BF), "dXV": guarded((B, NH, NC, CS, 64), BF)}


def _ranges(K, cuts):
    """(k0, nk) of the cutting, the LAST range first"""
    assert sum(cuts) == K
    out, k1 = [], K
    for nk in reversed(cuts):
        out.append((k1 - nk, nk))
        k1 -= nk
    return out


def _walk(geometry, cuts, two_streams, stop_after=None):
    """the backward as the ranges the cutting makes, dW1 / db1 carried in place in the (guarded) output buffers from the upstream
    gradients, one ln_carry; on one stream with a workspace per range, or with the schedule of ``linear_hip.backward_in_parts``: the
    recompute of the next range on a side stream into one of two workspaces, events both ways.  -> the guarded buffers"""
    CS, impl, B, NH, NC, G = geometry
    e = ext()
    i, _, _ = _case(*geometry)
    K = -(-NC // G)
    ranges = _ranges(K, cuts)[:stop_after]
    g = _grad_bufs(B, NH, NC, CS)
    g["dW1"][1].copy_(i["uW"]); g["db1"][1].copy_(i["ub"])
    slot_bytes = lambda nk: e.linear_backward_parts_slots(B, NH, NC, CS, 64, G, nk, BF, impl=impl)
    n_ws = 2 if two_streams else len(ranges)
    ws = {f"slots{n}": guarded((slot_bytes(max(nk for _, nk in ranges)) // 4,), F32) for n in range(n_ws)}
    ws["carry"] = guarded((e.linear_backward_parts_carry(B, NH, NC, CS, 64, G, BF, impl=impl) // 4,), F32)
    rec = (None, i["XK"], i["XV"], i["le"], i["ln_w"], i["ln_b"], i["W1c"], i["b1c"]) + (None,) * 13
    swp = (i["XQ"], i["XK"], i["XV"], i["le"], i["ln_w"], i["ln_b"], None, None, g["dW1"][1], g["db1"][1], i["dOut"], None, None,
           *[g[k][1] for k in GRADS])
    slots = lambda n: ws[f"slots{n % n_ws}"][1]
    torch.cuda.synchronize()
    if not two_streams:
        for n, (k0, nk) in enumerate(ranges):
            e.ttt_linear_recompute_groups(impl, *rec, G, k0, nk, slots(n))
            e.ttt_linear_sweep_groups(impl, *swp, G, k0, nk, slots(n), ws["carry"][1])
    else:
        from ttt_amd.models.ssm.pipeline import side_stream
        main, side = torch.cuda.current_stream(), side_stream(DEV)          # the stream the shipped schedule uses
        ready, swept = [torch.cuda.Event() for _ in ranges], [torch.cuda.Event() for _ in ranges]

        def recompute(n):
            with torch.cuda.stream(side):
                if n >= 2:
                    side.wait_event(swept[n - 2])
                e.ttt_linear_recompute_groups(impl, *rec, G, *ranges[n], slots(n))
                ready[n].record(side)

        side.wait_stream(main)
        recompute(0)
        for n, (k0, nk) in enumerate(ranges):
            if n + 1 < len(ranges):
                recompute(n + 1)
            main.wait_event(ready[n])
            e.ttt_linear_sweep_groups(impl, *swp, G, k0, nk, slots(n), ws["carry"][1])
            swept[n].record(main)
        main.wait_stream(side)
    torch.cuda.synchronize()
    for name, (buf, _) in {**g, **ws}.items():
        assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"{cuts}: write outside {name}"
    return g


@pytest.mark.parametrize("two_streams", [False, True])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["cs16", "cs64"])
def test_backward_in_parts_carries_the_one_call_bits(geometry, two_streams):
    """the cuttings (K), (1,) * K and (2, K - 2) of the K checkpoint groups, on one stream and with the two-stream, two-workspace
    schedule: all eight gradients equal the one-call backward's bits, every output is fully written, nothing lands outside the
    guards of the outputs, the slot workspaces and the carry, and the inputs and checkpoints are untouched"""
    CS, impl, B, NH, NC, G = geometry
    inputs, keep, ref = _case(*geometry)
    K = -(-NC // G)
    for cuts in ((K,), (1,) * K, (2, K - 2)):
        g = _walk(geometry, cuts, two_streams)
        assert_written_inside(g, f"parts {cuts}")
        for k in GRADS:
            assert torch.equal(g[k][1], ref[k]), (cuts, k)
    for k, v in inputs.items():
        assert torch.equal(v, keep[k]), f"input {k} was written"


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["cs16", "cs64"])
def test_a_walk_that_stops_leaves_the_rest_nan(geometry):
    """only the last range [2, K) of the cutting (2, K - 2): the gradients of the steps in front of group 2 and dln_w / dln_b stay NaN,
    those of the swept steps are the final bits, dW1 / db1 hold the carried state"""
    CS, impl, B, NH, NC, G = geometry
    _, _, ref = _case(*geometry)
    K = -(-NC // G)
    g = _walk(geometry, (2, K - 2), False, stop_after=1)
    s0 = 2 * G
    assert bool(torch.isnan(g["dln_w"][1]).all()) and bool(torch.isnan(g["dln_b"][1]).all())
    for k in ("deta", "dXQ", "dXK", "dXV"):
        assert bool(torch.isnan(g[k][1][:, :, :s0].float()).all()), k
        assert torch.equal(g[k][1][:, :, s0:], ref[k][:, :, s0:]), k
    assert not torch.isnan(g["dW1"][1]).any() and not torch.isnan(g["db1"][1]).any() and not torch.equal(g["dW1"][1], ref["dW1"])


def test_refusals_launch_nothing():
    """ranges outside [0, K) at both geometries, and mini-batches of 64 under auto: refused with the library's message, and every
    buffer a launch would have written is still NaN"""
    e = ext()
    for geometry in GEOMETRIES:
        CS, impl, B, NH, NC, G = geometry
        i, _, _ = _case(*geometry)
        K = -(-NC // G)
        g = _grad_bufs(B, NH, NC, CS)
        ws = {"slots": guarded((e.linear_backward_parts_slots(B, NH, NC, CS, 64, G, K, BF, impl=impl) // 4,), F32),
              "carry": guarded((e.linear_backward_parts_carry(B, NH, NC, CS, 64, G, BF, impl=impl) // 4,), F32)}
        rec = (None, i["XK"], i["XV"], i["le"], i["ln_w"], i["ln_b"], i["W1c"], i["b1c"]) + (None,) * 13
        swp = (i["XQ"], i["XK"], i["XV"], i["le"], i["ln_w"], i["ln_b"], None, None, i["uW"], i["ub"], i["dOut"], None, None,
               *[g[k][1] for k in GRADS])
        for k0, nk in ((-1, 1), (0, 0), (0, K + 1), (K, 1), (K - 1, 2), (2 ** 31 - 1, 2)):
            with pytest.raises(RuntimeError, match=r"inside \[0, K\)"):
                e.ttt_linear_recompute_groups(impl, *rec, G, k0, nk, ws["slots"][1])
            with pytest.raises(RuntimeError, match=r"inside \[0, K\)"):
                e.ttt_linear_sweep_groups(impl, *swp, G, k0, nk, ws["slots"][1], ws["carry"][1])
        if CS == 64:      # under auto the generic kernels run this geometry: they have no sweep over a range
            with pytest.raises(RuntimeError, match="only the MFMA sweep"):
                e.ttt_linear_recompute_groups(None, *rec, G, 0, 1, ws["slots"][1])
            with pytest.raises(RuntimeError, match="only the MFMA sweep"):
                e.ttt_linear_sweep_groups(None, *swp, G, 0, 1, ws["slots"][1], ws["carry"][1])
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(buf.float()).all()) for buf, _ in {**g, **ws}.values())


# ------------------------------------------------------------------------------------------------------------- autograd level
def _count_calls(monkeypatch, e):
    return count_calls(monkeypatch, e, {"recompute": "ttt_linear_recompute_groups", "sweep": "ttt_linear_sweep_groups",
                                        "one_call": "ttt_linear_backward_impl"})


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["cs16", "cs64"])
def test_autograd_backward_in_parts(monkeypatch, geometry):
    """``HipLinear.apply`` with ``backward_parts`` = 1 and 2 against 0: every returned gradient is equal; with the switch on the
    backward arrives as >= 2 sweep launches and no one-call backward, with it off the other way round"""
    from ttt_amd.models.ssm.linear_hip import HipLinear
    CS, impl, B, NH, NC, G = geometry
    e = ext()
    assert HipLinear.backward_parts == 0, "the switch must be off by default"
    monkeypatch.setattr(HipLinear, "cs64_impl", "mfma" if impl == "mfma" else "auto")
    calls = _count_calls(monkeypatch, e)
    d = round_acts(O.make_inputs("linear", B, NH, NC, CS, 64, seed=40 + CS), BF)
    dOut = d["dOut"].to(DEV, BF)

    def grads(parts):
        monkeypatch.setattr(HipLinear, "backward_parts", parts)
        leaves = [d[k].to(DEV, F32).requires_grad_(True) for k in ("ln_w", "ln_b", "W1", "b1")] + \
                 [d[k].to(DEV, BF).requires_grad_(True) for k in ("XQ", "XV", "XK", "eta")]
        st = [p.unsqueeze(0).expand(B, *p.shape) for p in leaves[2:4]]
        HipLinear.apply(leaves[0], leaves[1], *st, *leaves[4:], G).backward(dOut)
        torch.cuda.synchronize()
        return [t.grad for t in leaves]

    off = grads(0)
    assert calls == {"recompute": 0, "sweep": 0, "one_call": 1}, calls
    K = -(-NC // G)
    for parts in (1, 2):
        before = dict(calls)
        on = grads(parts)
        n = -(-K // parts)
        assert calls == {"recompute": before["recompute"] + n, "sweep": before["sweep"] + n, "one_call": before["one_call"]} and n >= 2, calls
        for name, a, b in zip(("ln_w", "ln_b", "W1", "b1", "XQ", "XV", "XK", "eta"), on, off):
            assert a is not None and torch.equal(a, b), (parts, name)


# ------------------------------------------------------------------------------------------------------------- layer level
@pytest.mark.parametrize("scenes", [1, 3])
@pytest.mark.parametrize("CS,G,L,cs64_impl,forward_parts", [(16, 4, 640, "auto", 0), (64, 2, 704, "mfma", 0), (16, 4, 640, "auto", 3)])
def test_layer_with_backward_in_parts(monkeypatch, CS, G, L, cs64_impl, forward_parts, scenes):
    """the layer of test_linear_parts_gpu.py (model_dim 128, 2 heads), both scan directions: output, dx and every parameter gradient
    are EQUAL with ``HipLinear.backward_parts`` = 2 and 0 - every kernel involved is deterministic and no other node changes.
    ``forward_parts`` = 3: together with the forward in parts (``linear_pipeline_parts``), which shares the side stream."""
    from ttt_amd.models.ssm.linear_hip import HipLinear
    e = ext()
    monkeypatch.setattr(HipLinear, "cs64_impl", cs64_impl)
    m, meta = _layer(CS, G, L, scenes)
    m.ttt.linear_pipeline_parts = forward_parts
    calls = _count_calls(monkeypatch, e)
    gen = torch.Generator().manual_seed(13)
    x0, dy = (torch.randn(1, L, 128, generator=gen).to(DEV, BF) for _ in range(2))
    for reverse in (False, True):
        monkeypatch.setattr(HipLinear, "backward_parts", 0)
        before = dict(calls)
        y0, dx0, g0 = _run(m, meta, x0, dy, reverse, True)
        assert calls["sweep"] == before["sweep"] and calls["one_call"] == before["one_call"] + 1, calls
        monkeypatch.setattr(HipLinear, "backward_parts", 2)
        before = dict(calls)
        y1, dx1, g1 = _run(m, meta, x0, dy, reverse, True)
        assert calls["sweep"] >= before["sweep"] + 2 and calls["one_call"] == before["one_call"], calls
        assert torch.equal(y1, y0) and torch.equal(dx1, dx0), reverse
        assert g0 and sorted(g0) == sorted(g1)
        for k in g0:
            assert torch.equal(g1[k], g0[k]), (reverse, k)
