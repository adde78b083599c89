"""The TTT-MLP backward at mini-batches of 16 in parts, on the device: the recompute and the reverse walk over ranges of checkpoint
groups (``ttt_hip_mlp_recompute_groups`` / ``ttt_hip_mlp_sweep_groups`` of include/ttt_hip_mlp_bwd_parts.h; mlp_recompute16_groups_kernel /
mlp_sweep16_groups_kernel of csrc/ttt_mfma16.hip) and the opt-in autograd schedule that uses them (``TkMLP.cs16_backward_parts``,
ttt_amd/models/ssm/mlp_tk.py).  Every comparison is ``torch.equal`` against ``ttt_backward_impl("mfma", ...)`` on the same inputs - the
parts run the one call's ``recompute_group`` / ``sweep_group`` - except the one check against the fp64 oracle.  Cases, seeds and runners:
tests/mlp16_bwd_cases.py, tests/mlp16_bwd_parts_cases.py (every cutting was first run on the wave emulator,
tests/test_emul_mlp16_bwd_parts_cpu.py)."""
import pytest
import torch

import mlp16_bwd_cases as M
import mlp16_bwd_parts_cases as P
from test_mlp_cs16_bwd_mfma_gpu import DEV, device_forward, device_run, ext

pytestmark = pytest.mark.gpu
_CASES = {}


def _case(e, B, NH, NC, G, seed, upstream=True):
    """host inputs, the device forward's checkpoints, an upstream state gradient and the one-call MFMA backward's ten results - made
    once per shape and left unchanged"""
    key = (B, NH, NC, G, seed, upstream)
    if key not in _CASES:
        assert e.resolved_impl(B, NH, NC, M.CS, M.F, G, torch.bfloat16, mlp=True, backward=True, impl="mfma") == "mfma"
        c = M.case(B, NH, NC, seed)
        t = M.host_tensors(c)
        _, cks = device_forward(e, t, G)
        up = M.upstream(c, cks, G, seed) if upstream else tuple(0.01 * torch.randn(B, NH, *s, generator=torch.Generator().manual_seed(seed))
                                                                for s in M.STATE_SHAPES)
        ref, _ = device_run(e, "mfma")(t, cks, up, G)
        assert not any(torch.isnan(ref[k].float()).any() for k in M.GRADS)
        _CASES[key] = (c, t, cks, up, ref)
    return _CASES[key]


def _assert_equal(tag, g, ref):
    for name in M.GRADS:
        assert not torch.isnan(g[name].float()).any(), (tag, name, "not fully written")
        assert torch.equal(g[name], ref[name]), (tag, name)


@pytest.mark.parametrize("two_streams", [False, True], ids=["one_stream", "two_streams"])
@pytest.mark.parametrize("NC,G", M.CHAIN)
def test_backward_in_parts_carries_the_one_call_bits(NC, G, two_streams):
    """the chain shapes (11, 4), (7, 3), (3, 1) at B = 2, NH = 3 (K = 3; ragged last groups of 3 and 1) under the cuttings (K),
    (1,) * K and the uneven (2, 1), on one stream with a workspace per range and with the two-stream, two-workspace schedule: all ten
    gradients equal the one-call MFMA backward's bits from a non-zero upstream; outputs, slot workspaces and the carry start as NaN,
    the guards of the workspaces stay NaN, every output is fully written, the inputs and checkpoints are unchanged"""
    e = ext()
    _, t, cks, up, ref = _case(e, M.CHAIN_B, M.CHAIN_NH, NC, G, 500 + NC)
    K = -(-NC // G)
    for cuts in ((K,), (1,) * K, (2, K - 2)):
        g, _, carry = P.device_walk(e, two_streams)(t, cks, up, G, cuts)
        _assert_equal(f"parts {cuts}", g, ref)
        assert not torch.isnan(carry).any()


def test_slots_hold_the_forward_states():
    """(B, NH, NC, G) = (2, 3, 9, 4), cut (1, 2): slot j of group k holds the bits of checkpoint k G + j of a forward with G = 1; the
    slots the ragged last group (one step) does not use stay NaN"""
    e = ext()
    shape = (2, 3, 9, 4)
    _, t, cks, up, _ = _case(e, *shape, M.seed_of(shape))
    _, cks1 = device_forward(e, t, 1)
    cuts = (1, 2)
    _, spaces, _ = P.device_walk(e, False)(t, cks, up, shape[3], cuts)
    P.check_slots("device parts", spaces, P.ranges(3, cuts), cks1, *shape)


def test_recompute_grid_beyond_the_cu_count():
    """B = 2, NH = 48, NC = 3, G = 1, one range of nk = 3: 288 recompute workgroups on 256 compute units (none waits for another),
    96 walking workgroups; equal to the one-call backward"""
    e = ext()
    B, NH, NC, G = 2, 48, 3, 1
    assert B * NH * NC > torch.cuda.get_device_properties(0).multi_processor_count
    _, t, cks, up, ref = _case(e, B, NH, NC, G, 77, upstream=False)
    g, _, _ = P.device_walk(e, False)(t, cks, up, G, (3,))
    _assert_equal("288 workgroups", g, ref)


def test_parts_against_the_fp64_oracle():
    """the independent check: (2, 3, 9, 4) cut (1, 2), each of the ten gradients within TOL_G = 3e-2 (rel-L2) of the fp64 oracle from
    the same checkpoints and upstream.  (The emulated body holds that bound at this shape - between 6e-4 and 3.1e-3,
    tests/test_emul_mlp16_bwd_cpu.py - so the bound tests the kernels, not the reference.)"""
    e = ext()
    shape = (2, 3, 9, 4)
    c, t, cks, up, _ = _case(e, *shape, M.seed_of(shape))
    g, _, _ = P.device_walk(e, True)(t, cks, up, shape[3], (1, 2))
    errs = M.errors(g, M.oracle_backward(c, cks, shape[3], up))
    print("parts (1, 2) vs fp64 oracle: " + "  ".join(f"{k} {v:.3g}" for k, v in errs.items() if k in M.GRADS))
    bad = {k: v for k, v in errs.items() if k in M.GRADS and not v < M.TOL_G}
    assert not bad, bad


def test_refusals_launch_nothing():
    """a range outside [0, K), mini-batches of 64 and the generic selector are refused with the library's message, and every buffer a
    launch would have written is still NaN"""
    e = ext()
    shape = (2, 3, 9, 4)
    _, t, cks, up, _ = _case(e, *shape, M.seed_of(shape))
    B, NH, NC, G = shape
    d = {k: t[k].to(DEV) for k in ("XQ", "XK", "XV", "eta", "dOut")}
    lw, lb = t["ln_w"].to(DEV).reshape(1, NH, 1, M.F), t["ln_b"].to(DEV).reshape(1, NH, 1, M.F)
    g = M.outputs(B, NH, NC, device=DEV)
    st = [g[n] for n in ("dW1", "db1", "dW2", "db2")]
    slots = torch.full((e.mlp_backward_parts_slots(B, NH, NC, M.CS, M.F, G, 3) // 4,), float("nan"), device=DEV)
    carry = torch.full((e.mlp_backward_parts_carry(B, NH, NC, M.CS, M.F, G) // 4,), float("nan"), device=DEV)
    rec = (None, d["XK"], d["XV"], d["eta"], lw, lb, *[c.to(DEV) for c in cks]) + (None,) * 32
    swp = (d["XQ"], d["XK"], d["XV"], d["eta"], lw, lb) + (None,) * 21 + \
          (*[u.to(DEV) for u in up], d["dOut"], g["dln_w"], g["dln_b"], *st, g["dlast_eta"], g["dXQ"], g["dXK"], g["dXV"])
    for k0, nk in ((-1, 1), (0, 0), (0, 4), (3, 1), (2, 2), (2 ** 31 - 1, 2)):
        with pytest.raises(RuntimeError, match=r"inside \[0, K\)"):
            e.ttt_recompute_groups(*rec, G, k0, nk, slots, impl="mfma")
        with pytest.raises(RuntimeError, match=r"inside \[0, K\)"):
            e.ttt_sweep_groups(*swp, G, k0, nk, slots, carry, impl="mfma")
    with pytest.raises(RuntimeError, match="only the MFMA backward at mini-batches of 16"):
        e.ttt_recompute_groups(*rec, G, 0, 1, slots, impl="generic")
    with pytest.raises(RuntimeError, match="only the MFMA backward at mini-batches of 16"):
        e.ttt_sweep_groups(*swp, G, 0, 1, slots, carry, impl="generic")
    with pytest.raises(RuntimeError, match="slot workspace null or smaller"):
        e.ttt_recompute_groups(*rec, G, 0, 3, slots[:-1], impl="mfma")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v.float()).all()) for v in list(g.values()) + [slots, carry])


# ------------------------------------------------------------------------------------------------------------- autograd level
def _with_switches(impl, parts, fn):
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    old = TkMLP.cs16_bwd_impl, TkMLP.cs16_backward_parts
    TkMLP.cs16_bwd_impl, TkMLP.cs16_backward_parts = impl, parts
    try:
        return fn()
    finally:
        TkMLP.cs16_bwd_impl, TkMLP.cs16_backward_parts = old


def test_autograd_tkmlp_in_parts_equals_one_call():
    """``TkMLP.apply`` at (1, 2, 9, 2) - K = 5 groups, the last of one step - with ``cs16_bwd_impl`` = "mfma": every gradient with
    ``cs16_backward_parts`` = 2 (three ranges) equals the one with 0; the switches are restored; the part entries ran"""
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    e = ext()
    assert TkMLP.cs16_backward_parts == 0, "the switch must be off by default"
    B, NH, NC, G = 1, 2, 9, 2
    assert e.resolved_impl(B, NH, NC, M.CS, M.F, G, torch.bfloat16, mlp=True, backward=True, impl="mfma") == "mfma"
    t = M.host_tensors(M.case(B, NH, NC, 141 + NC))

    def grads():
        leaves = [t[k].to(DEV).requires_grad_(True) for k in ("ln_w", "ln_b", "W1", "b1", "W2", "b2", "XQ", "XV", "XK")]
        eta = t["eta"].to(DEV).transpose(-2, -1).contiguous().requires_grad_(True)
        out = TkMLP.apply(*leaves, eta, G)
        out.backward(t["dOut"].to(DEV))
        torch.cuda.synchronize()
        return out.detach(), [x.grad for x in leaves + [eta]]

    o0, g0 = _with_switches("mfma", 0, grads)
    before = dict(e.mlp_bwd_parts_calls)
    o1, g1 = _with_switches("mfma", 2, grads)
    assert e.mlp_bwd_parts_calls == {"recompute": before["recompute"] + 3, "sweep": before["sweep"] + 3}
    assert (TkMLP.cs16_bwd_impl, TkMLP.cs16_backward_parts) == ("auto", 0)
    assert torch.equal(o0, o1) and len(g0) == len(g1) == 10
    for i, (a, b) in enumerate(zip(g1, g0)):
        assert a is not None and torch.equal(a, b), i


def test_autograd_fused_pre_scan_in_parts_equals_one_call():
    """``FusedPreScanMLP.apply`` at the shape of tests/test_kernels_gpu.py::test_fused_pre_scan_node_equals_two_nodes (B = 2, L = 320,
    NH = 3, G = 2) at mini-batches of 16 (NC = 20, K = 10): every gradient with ``cs16_backward_parts`` = 2 equals the one with 0"""
    from ttt_amd.models.ssm.fused import FusedPreScanMLP
    e = ext()
    gen = torch.Generator().manual_seed(3)
    B, L, NH, CS, G = 2, 320, 3, 16, 2
    NC = L // CS
    assert e.resolved_impl(B, NH, NC, CS, 64, G, torch.bfloat16, mlp=True, backward=True, impl="mfma") == "mfma"
    raws = [torch.randn(B, L, NH * 64, generator=gen).bfloat16().to(DEV) for _ in range(3)]
    lnw, lnb = (1 + 0.1 * torch.randn(NH, 64, generator=gen)).to(DEV), (0.1 * torch.randn(NH, 64, generator=gen)).to(DEV)
    W1, b1 = (0.02 * torch.randn(NH, 64, 256, generator=gen)).to(DEV), torch.zeros(NH, 1, 256, device=DEV)
    W2, b2 = (0.02 * torch.randn(NH, 256, 64, generator=gen)).to(DEV), torch.zeros(NH, 1, 64, device=DEV)
    eta0 = (0.1 * torch.sigmoid(torch.randn(B, NH, NC, 1, CS, generator=gen)) / (64 * CS)).bfloat16().to(DEV)
    rope = torch.randn(L, 32, 2, generator=gen).to(DEV)
    pos = torch.arange(L, dtype=torch.int32, device=DEV)
    pos[:17] = -1
    dOut = torch.randn(B, NH, NC, CS, 64, generator=gen).bfloat16().to(DEV)

    def grads():
        rq, rk, rv = (x.clone().requires_grad_(True) for x in raws)
        ps = [x.clone().requires_grad_(True) for x in (lnw, lnb, W1, b1, W2, b2)]
        eta = eta0.clone().requires_grad_(True)
        st = [p.unsqueeze(0).expand(B, *p.shape) for p in ps[2:]]
        out = FusedPreScanMLP.apply(rq, rk, rv, ps[0], ps[1], rope, None, pos, NH, *st, eta, G)
        out.backward(dOut)
        torch.cuda.synchronize()
        return [out.detach(), rq.grad, rk.grad, rv.grad, eta.grad] + [p.grad for p in ps]

    r0 = _with_switches("mfma", 0, grads)
    before = dict(e.mlp_bwd_parts_calls)
    r1 = _with_switches("mfma", 2, grads)
    assert e.mlp_bwd_parts_calls == {"recompute": before["recompute"] + 5, "sweep": before["sweep"] + 5}
    for i, (a, b) in enumerate(zip(r1, r0)):
        assert a is not None and torch.equal(a, b), i
