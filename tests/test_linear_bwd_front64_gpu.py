"""The third stage of the TTT-Linear backward in parts at mini-batches of 64, on the device: the carry-free half of every reverse step of a
range of checkpoint groups, one wave per 16-row token block, and the four-wave walk that consumes its records
(``ttt_hip_linear_front64_groups`` / ``ttt_hip_linear_chain64_groups`` of include/ttt_hip_lin64_bwd_front.h; ``front_groups`` /
``chain_groups`` of csrc/ttt_lin64_body.h), and the opt-in autograd schedule that uses them (``HipLinear.backward_front64``,
ttt_amd/models/ssm/linear_hip.py).  Every comparison is ``torch.equal`` against the one-call backward of
tests/test_linear_bwd_parts_gpu.py's CS = 64 case (made once, shared): front_step + chain_step are the statements of its reverse step."""
import pytest
import torch

from helpers import count_calls
from oracle import ttt_oracle as O
from test_emul_lin_bwd_parts_cpu import _cuttings
from test_kernels_gpu import DEV, ext, round_acts
from test_linear_bwd_parts_gpu import GRADS, _case, _grad_bufs, _ranges
from test_linear_parts_gpu import _layer, _run
from test_scan_oracle_gpu import GUARD, assert_written_inside, guarded

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
GEOMETRY = (64, "mfma", 2, 3, 7, 3)         # CS, impl, B, NH, NC, G: K = 3, last group of one step, B * NH no power of two
CS16 = (16, None, 2, 5, 11, 3)
REC = 77824


def _args(i, g):
    """the tensor lists of the four calls of a range; what a call does not touch is None"""
    rec = (None, i["XK"], i["XV"], i["le"], i["ln_w"], i["ln_b"], i["W1c"], i["b1c"]) + (None,) * 13
    frt = (i["XQ"], i["XK"], i["XV"], None, i["ln_w"], i["ln_b"], None, None, None, None, i["dOut"]) + (None,) * 7 + (g["dXQ"][1], None, None)
    chn = (i["XQ"], i["XK"], None, i["le"], i["ln_w"], i["ln_b"], None, None, g["dW1"][1], g["db1"][1], None, None, None,
           g["dln_w"][1], g["dln_b"][1], g["dW1"][1], g["db1"][1], g["deta"][1], None, g["dXK"][1], g["dXV"][1])
    swp = (i["XQ"], i["XK"], i["XV"], i["le"], i["ln_w"], i["ln_b"], None, None, g["dW1"][1], g["db1"][1], i["dOut"], None, None,
           *[g[k][1] for k in GRADS])
    return rec, frt, chn, swp


def _walk(cuts, two_streams, sweep=()):
    """the backward as the ranges the cutting makes - recompute -> front -> chain each, or recompute -> sweep for the ranges (in walking
    order) named in ``sweep`` -, dW1 / db1 carried in place in the (guarded, NaN-filled) output buffers from the upstream gradients, one
    ln_carry; on one stream with workspaces per range, or with the schedule of ``linear_hip.backward_in_parts``: recompute and front
    of the next range on the side stream into one of two slot / record workspaces, events both ways.  -> the guarded buffers"""
    CS, impl, B, NH, NC, G = GEOMETRY
    e = ext()
    i, _, _ = _case(*GEOMETRY)
    K = -(-NC // G)
    ranges = _ranges(K, cuts)
    g = _grad_bufs(B, NH, NC, CS)
    g["dW1"][1].copy_(i["uW"]); g["db1"][1].copy_(i["ub"])
    nk_max = max(nk for _, nk in ranges)
    n_ws = 2 if two_streams else len(ranges)
    ws = {}
    rbytes = e.linear_backward_front64_records(B, NH, NC, CS, 64, G, nk_max, BF, impl=impl)
    assert rbytes == B * NH * nk_max * G * REC
    for n in range(n_ws):
        ws[f"slots{n}"] = guarded((e.linear_backward_parts_slots(B, NH, NC, CS, 64, G, nk_max, BF, impl=impl) // 4,), F32)
        ws[f"records{n}"] = guarded((rbytes // 4,), F32)
    ws["carry"] = guarded((e.linear_backward_parts_carry(B, NH, NC, CS, 64, G, BF, impl=impl) // 4,), F32)
    rec, frt, chn, swp = _args(i, g)
    slots, records = (lambda n: ws[f"slots{n % n_ws}"][1]), (lambda n: ws[f"records{n % n_ws}"][1])

    def side_work(n):
        e.ttt_linear_recompute_groups(impl, *rec, G, *ranges[n], slots(n))
        if n not in sweep:
            e.ttt_linear_front64_groups(impl, *frt, G, *ranges[n], slots(n), records(n))

    def main_work(n):
        if n in sweep:
            e.ttt_linear_sweep_groups(impl, *swp, G, *ranges[n], slots(n), ws["carry"][1])
        else:
            e.ttt_linear_chain64_groups(impl, *chn, G, *ranges[n], slots(n), records(n), ws["carry"][1])

    torch.cuda.synchronize()
    if not two_streams:
        for n in range(len(ranges)):
            side_work(n)
            main_work(n)
    else:
        from ttt_amd.models.ssm.pipeline import side_stream
        main, side = torch.cuda.current_stream(), side_stream(DEV)          # the stream the shipped schedule uses
        ready, swept = [torch.cuda.Event() for _ in ranges], [torch.cuda.Event() for _ in ranges]

        def prepare(n):
            with torch.cuda.stream(side):
                if n >= 2:
                    side.wait_event(swept[n - 2])
                side_work(n)
                ready[n].record(side)

        side.wait_stream(main)
        prepare(0)
        for n in range(len(ranges)):
            if n + 1 < len(ranges):
                prepare(n + 1)
            main.wait_event(ready[n])
            main_work(n)
            swept[n].record(main)
        main.wait_stream(side)
    torch.cuda.synchronize()
    for name, (buf, _) in {**g, **ws}.items():
        assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"{cuts}: write outside {name}"
    return g


def _assert_one_call_bits(g, ref, what):
    assert_written_inside(g, f"front + chain {what}")
    bad = {k: int((g[k][1] != ref[k]).sum()) for k in GRADS if not torch.equal(g[k][1], ref[k])}
    assert not bad, (what, bad)


@pytest.mark.parametrize("two_streams", [False, True])
def test_front_and_chain_carry_the_one_call_bits(two_streams):
    """every cutting of the K = 3 checkpoint groups - (3), (1, 1, 1), (1, 2), (2, 1) -, on one stream and with the two-stream,
    two-workspace schedule: all eight gradients equal the one-call backward's bits, every output is fully written, nothing lands
    outside the guards of the outputs, the slot and record workspaces and the carry, and the inputs and checkpoints are untouched"""
    CS, impl, B, NH, NC, G = GEOMETRY
    inputs, keep, ref = _case(*GEOMETRY)
    K = -(-NC // G)
    assert K == 3 and len(_cuttings(K)) == 4
    for cuts in _cuttings(K):
        _assert_one_call_bits(_walk(cuts, two_streams), ref, cuts)
    for k, v in inputs.items():
        assert torch.equal(v, keep[k]), f"input {k} was written"


def test_sweep_ranges_and_chain_ranges_give_the_same_bits():
    """one group per range, the ranges alternately by ``ttt_linear_sweep_groups`` and by front + chain, starting with either, on two
    streams: the carries are the same whichever stage wrote them"""
    _, _, ref = _case(*GEOMETRY)
    for sweep in ((0, 2), (1,)):
        _assert_one_call_bits(_walk((1, 1, 1), True, sweep=sweep), ref, f"sweep ranges {sweep}")
    _assert_one_call_bits(_walk((1, 2), False, sweep=(0,)), ref, "sweep [1, 3), chain [0, 1)")


def test_refusals_launch_nothing():
    """a range outside [0, K), a short record workspace, mini-batches of 64 under "auto", and mini-batches of 16: refused with the
    library's message, and every buffer a launch would have written is still NaN"""
    e = ext()
    for geometry in (GEOMETRY, CS16):
        CS, impl, B, NH, NC, G = geometry
        i, _, _ = _case(*geometry)
        K = -(-NC // G)
        g = _grad_bufs(B, NH, NC, CS)
        ws = {"slots": guarded((e.linear_backward_parts_slots(B, NH, NC, CS, 64, G, K, BF, impl=impl) // 4,), F32),
              "records": guarded((B * NH * K * G * REC // 4,), F32),
              "carry": guarded((e.linear_backward_parts_carry(B, NH, NC, CS, 64, G, BF, impl=impl) // 4,), F32)}
        _, frt, chn, _ = _args(i, g)
        chn = chn[:8] + (i["uW"], i["ub"]) + chn[10:15] + (g["dW1"][1], g["db1"][1]) + chn[17:]
        if CS == 16:
            assert e.linear_backward_front64_records(B, NH, NC, CS, 64, G, K, BF, impl=impl) == 0
            with pytest.raises(RuntimeError, match="only mini-batches of 64"):
                e.ttt_linear_front64_groups(impl, *frt, G, 0, 1, ws["slots"][1], ws["records"][1])
            with pytest.raises(RuntimeError, match="only mini-batches of 64"):
                e.ttt_linear_chain64_groups(impl, *chn, G, 0, 1, ws["slots"][1], ws["records"][1], ws["carry"][1])
        else:
            assert e.linear_backward_front64_records(B, NH, NC, CS, 64, G, K, BF, impl=impl) == B * NH * K * G * REC
            assert e.linear_backward_front64_records(B, NH, NC, CS, 64, G, K, BF) == 0
            with pytest.raises(RuntimeError, match="only the MFMA sweep"):
                e.ttt_linear_front64_groups(None, *frt, G, 0, 1, ws["slots"][1], ws["records"][1])
            with pytest.raises(RuntimeError, match="only the MFMA sweep"):
                e.ttt_linear_chain64_groups(None, *chn, G, 0, 1, ws["slots"][1], ws["records"][1], ws["carry"][1])
            for k0, nk in ((-1, 1), (0, 0), (0, K + 1), (K, 1), (K - 1, 2), (2 ** 31 - 1, 2)):
                with pytest.raises(RuntimeError, match=r"inside \[0, K\)"):
                    e.ttt_linear_front64_groups(impl, *frt, G, k0, nk, ws["slots"][1], ws["records"][1])
                with pytest.raises(RuntimeError, match=r"inside \[0, K\)"):
                    e.ttt_linear_chain64_groups(impl, *chn, G, k0, nk, ws["slots"][1], ws["records"][1], ws["carry"][1])
            short = ws["records"][1][:-1]                  # one float less than K groups need
            with pytest.raises(RuntimeError, match="record workspace null or smaller"):
                e.ttt_linear_front64_groups(impl, *frt, G, 0, K, ws["slots"][1], short)
            with pytest.raises(RuntimeError, match="record workspace null or smaller"):
                e.ttt_linear_chain64_groups(impl, *chn, G, 0, K, ws["slots"][1], short, ws["carry"][1])
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(buf.float()).all()) for buf, _ in {**g, **ws}.values())


# ------------------------------------------------------------------------------------------------------------- autograd level
def _count_calls(monkeypatch, e):
    return count_calls(monkeypatch, e, {"recompute": "ttt_linear_recompute_groups", "sweep": "ttt_linear_sweep_groups",
                                        "front": "ttt_linear_front64_groups", "chain": "ttt_linear_chain64_groups",
                                        "front16": "ttt_linear_front_groups", "chain16": "ttt_linear_chain_groups",
                                        "one_call": "ttt_linear_backward_impl"})


def test_autograd_backward_with_the_front(monkeypatch):
    """``HipLinear.apply`` with ``cs64_impl`` = "mfma" and (``backward_parts``, ``backward_front64``) = (1, 1) and (2, 1) against
    (1, 0) and (0, 0): every returned gradient is equal; with the switch on the backward arrives as front and chain launches, no
    sweep and no one-call backward; (0, 1) runs the one call; ``backward_front`` = 1 alone keeps the sweep"""
    from ttt_amd.models.ssm.linear_hip import HipLinear
    CS, impl, B, NH, NC, G = GEOMETRY
    e = ext()
    assert HipLinear.backward_parts == 0 and HipLinear.backward_front == 0 and HipLinear.backward_front64 == 0, \
        "the switches must be off by default"
    monkeypatch.setattr(HipLinear, "cs64_impl", "mfma")
    calls = _count_calls(monkeypatch, e)
    d = round_acts(O.make_inputs("linear", B, NH, NC, CS, 64, seed=40 + CS), BF)
    dOut = d["dOut"].to(DEV, BF)

    def grads(parts, front64, front16=0):
        monkeypatch.setattr(HipLinear, "backward_parts", parts)
        monkeypatch.setattr(HipLinear, "backward_front64", front64)
        monkeypatch.setattr(HipLinear, "backward_front", front16)
        leaves = [d[k].to(DEV, F32).requires_grad_(True) for k in ("ln_w", "ln_b", "W1", "b1")] + \
                 [d[k].to(DEV, BF).requires_grad_(True) for k in ("XQ", "XV", "XK", "eta")]
        st = [p.unsqueeze(0).expand(B, *p.shape) for p in leaves[2:4]]
        HipLinear.apply(leaves[0], leaves[1], *st, *leaves[4:], G).backward(dOut)
        torch.cuda.synchronize()
        return [t.grad for t in leaves]

    names = ("ln_w", "ln_b", "W1", "b1", "XQ", "XV", "XK", "eta")
    K = -(-NC // G)
    zero = {"recompute": 0, "sweep": 0, "front": 0, "chain": 0, "front16": 0, "chain16": 0}
    off = grads(0, 0)
    assert calls == {**zero, "one_call": 1}, calls
    grads(0, 1)
    assert calls == {**zero, "one_call": 2}, calls
    swept = grads(1, 0, front16=1)                       # the CS = 16 switch does not reach mini-batches of 64
    assert calls == {**zero, "recompute": K, "sweep": K, "one_call": 2}, calls
    for name, a, b in zip(names, swept, off):
        assert a is not None and torch.equal(a, b), ("sweep", name)
    for parts in (1, 2):
        before = dict(calls)
        on = grads(parts, 1)
        n = -(-K // parts)
        assert n >= 2 and calls == {**zero, "recompute": before["recompute"] + n, "sweep": K, "front": before["front"] + n,
                                    "chain": before["chain"] + n, "one_call": 2}, calls
        for name, a, b in zip(names, on, off):
            assert a is not None and torch.equal(a, b), (parts, name)


# ------------------------------------------------------------------------------------------------------------- layer level
def test_layer_with_the_front(monkeypatch):
    """the layer of test_linear_parts_gpu.py (model_dim 128, 2 heads) at CS = 64 with ``cs64_impl`` = "mfma", G = 2, L = 704, both scan
    directions, backward in parts of 2 groups: output, dx and every parameter gradient are EQUAL with ``HipLinear.backward_front64`` =
    1 and 0"""
    from ttt_amd.models.ssm.linear_hip import HipLinear
    e = ext()
    monkeypatch.setattr(HipLinear, "cs64_impl", "mfma")
    monkeypatch.setattr(HipLinear, "backward_parts", 2)
    m, meta = _layer(64, 2, 704, 1)
    calls = _count_calls(monkeypatch, e)
    gen = torch.Generator().manual_seed(13)
    x0, dy = (torch.randn(1, 704, 128, generator=gen).to(DEV, BF) for _ in range(2))
    for reverse in (False, True):
        monkeypatch.setattr(HipLinear, "backward_front64", 0)
        before = dict(calls)
        y0, dx0, g0 = _run(m, meta, x0, dy, reverse, True)
        assert calls["sweep"] >= before["sweep"] + 2 and calls["chain"] == before["chain"] and calls["front"] == before["front"], calls
        monkeypatch.setattr(HipLinear, "backward_front64", 1)
        before = dict(calls)
        y1, dx1, g1 = _run(m, meta, x0, dy, reverse, True)
        assert calls["chain"] >= before["chain"] + 2 and calls["front"] == before["front"] + calls["chain"] - before["chain"], calls
        assert calls["sweep"] == before["sweep"] and calls["one_call"] == before["one_call"], calls
        assert calls["front16"] == 0 and calls["chain16"] == 0
        assert torch.equal(y1, y0) and torch.equal(dx1, dx0), reverse
        assert g0 and sorted(g0) == sorted(g1)
        for k in g0:
            assert torch.equal(g1[k], g0[k]), (reverse, k)
