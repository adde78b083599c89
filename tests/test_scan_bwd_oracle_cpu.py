"""Fixes the tolerances of ``tests/test_scan_bwd_oracle_gpu.py`` (one call of the TTT-Linear backward sweeps - one step, or one group -
against the fp64 oracle from the same checkpoint and a nonzero upstream state gradient: tests/scan_bwd_cases.py) with a sensitivity
table, as test_scan_oracle_cpu.py does for the forward scans: for every metric the distance of the oracle's ROUNDING MODEL
(``O.lin_step_bwd_rounded``: the fp64 backward step with a bf16 rounding wherever lin16::backward / lin64::backward round) from the
fp64 step, the threshold, and the distance of a set of plausible kernel bugs (the fp64 step with one statement changed).  Then the
two kernel bodies themselves, run on the wave emulators of tests/emul, through the same checks as the device: one step, a horizon,
the chain of one-group calls with equal bits, and every must-catch mutation failing its metric."""
import ctypes
import functools

import pytest
import torch

import scan_bwd_cases as S
import scan_cases as C
from helpers import SCAN_BWD_MEASURED, SCAN_BWD_MEASURED_GENERIC, SCAN_BWD_TOL, SCAN_BWD_TOL_GENERIC
from oracle import cpu_ext
from oracle import ttt_oracle as O

REGIMES = ("base", "high")


# ------------------------------------------------------------------------------------------------ the statements themselves
def test_stand_in_passes_the_upstream_state_gradient():
    """oracle/cpu_ext.py::ttt_linear_backward hands (grad_L_W1_last, grad_L_b1_last) to the oracle: a nonzero upstream changes every
    output that can depend on it (all but dXQ), and the oracle's ``dst_last`` is the state gradient the sweep starts from"""
    c = S.bwd_case(16, 2, 2, 3, 2, 5)
    t, cks, up = S.host_tensors(c, torch.float32)

    def stand_in(u):
        B, NH, NC, CS, F = t["XQ"].shape
        z = lambda *s: torch.zeros(s, dtype=torch.float64)
        g = dict(dln_w=z(B, NH, 1, F), dln_b=z(B, NH, 1, F), dW1=z(B, NH, F, F), db1=z(B, NH, 1, F), dlast_eta=z(B, NH, NC, CS, 1),
                 dXQ=z(B, NH, NC, CS, F), dXK=z(B, NH, NC, CS, F), dXV=z(B, NH, NC, CS, F))
        cpu_ext.ttt_linear_backward(t["XQ"], t["XK"], t["XV"], t["eta"], t["ln_w"], t["ln_b"], cks["W1"], cks["b1"], *u, t["dOut"],
                                    None, None, g["dln_w"], g["dln_b"], g["dW1"], g["db1"], g["dlast_eta"], g["dXQ"], g["dXK"],
                                    g["dXV"], c["G"])
        return g
    zero = stand_in(tuple(torch.zeros_like(u) for u in up))
    full = stand_in(up)
    ref = S.sweep(c, c["cks"], c["up"], c["G"])
    for k in S.GRADS:
        if k != "dXQ":      # dQ = dOut + dZ1b W1n^T reads no state gradient at any step; every other output does
            assert float((full[k] - zero[k]).norm() / zero[k].norm()) > 1e-2, k
        assert float((full[k] - ref[k].reshape(full[k].shape)).norm() / ref[k].norm()) < 1e-12, k
    assert torch.equal(full["dXQ"], zero["dXQ"])


def test_rounded_backward_step_with_every_point_off_is_the_exact_step():
    c = S.bwd_case(16, 2, 2, 2, 1, 3, "high")
    gam, bet = c["ln_w"].reshape(1, 2, 1, 64), c["ln_b"].reshape(1, 2, 1, 64)
    st = (c["cks"]["W1"][:, :, 1], c["cks"]["b1"][:, :, 1])
    a = (c["XQ"][:, :, 1], c["XK"][:, :, 1], c["XV"][:, :, 1], c["eta"][:, :, 1], gam, bet)
    d = c["dOut"][:, :, 1]
    flat = lambda r: list(r[0]) + list(r[1:])
    exact = flat(O._lin_step_bwd(st, *a, O.LN_EPS, d, c["up"]))
    off = flat(O.lin_step_bwd_rounded(st, *a, d, c["up"], on=()))
    assert all(torch.equal(x, y) for x, y in zip(off, exact))
    # the form the roundings are written into (eta carried inside Gs, as the kernels carry it) is the same step, and so is the step
    # the mutations are written into, to the last bits of fp64
    scaled = flat(O._lin_step_bwd_scaled(st, *a, d, c["up"], O.LN_EPS, frozenset()))
    mut = flat(S.step_bwd_mut(st, *a, d, c["up"]))
    for other in (scaled, mut):
        for x, y in zip(other, exact):
            assert float((x - y).abs().max()) < 1e-12 * max(1.0, float(y.abs().max()))
    for pt in O.LIN_BWD_ROUND_POINTS:       # every point moves the result
        one = flat(O.lin_step_bwd_rounded(st, *a, d, c["up"], on={pt}))
        assert not all(torch.equal(x, y) for x, y in zip(one, exact)), pt


# ------------------------------------------------------------------------------------------------ sensitivity table
def gpu_cases():
    """(tag, case) of every call of the GPU file that is compared with the oracle: one step, horizons, the two-step case (high only)"""
    for table in (S.ONE_STEP, S.HORIZON, S.TWO_STEP):
        for name, (CS, B, NH, NC, G, seed) in table.items():
            for regime in REGIMES if table is not S.TWO_STEP else ("high",):
                yield f"{name}/NC={NC}/{regime}", S.bwd_case(CS, B, NH, NC, G, seed, regime)


@functools.lru_cache(maxsize=None)
def model_worst():
    """{metric: (worst value, case)} of the rounding model over every such call, and of the oracle's step in fp32 arithmetic (fp32 and
    bf16 stores) over the one-step cases in the base regime: the generic kernel's"""
    worst, worst32 = {}, {}
    for tag, c in gpu_cases():
        ref = S.sweep(c, c["cks"], c["up"], c["G"])
        m = S.metrics(c, S.sweep(c, c["cks"], c["up"], c["G"], O.LIN_BWD_ROUND), ref, c["up"])
        for k, v in m.items():
            worst[k] = max(worst.get(k, (0.0, "")), (v, tag))
        if c["XQ"].shape[2] == 1 and tag.endswith("base"):
            for how in ("fp32", "fp32_bf16out"):
                m = S.metrics(c, S.sweep(c, c["cks"], c["up"], c["G"], how), ref, c["up"], bf16_rows=how != "fp32")
                for k, v in m.items():
                    worst32[k] = max(worst32.get(k, (0.0, "")), (v, f"{tag}/{how}"))
    return worst, worst32


@functools.lru_cache(maxsize=None)
def sensitivity_table(CS, regime):
    """{metric: (rounding model's worst value over the GPU file's cases, threshold, {must-catch mutation: distance}, {reported
    mutation: distance})}: the mutations on the one-step case of this mini-batch size (the two off-by-one ones on the two-step case)"""
    worst, _ = model_worst()
    table = {k: (worst[k][0], SCAN_BWD_TOL[k], {}, {}) for k in S.METRICS}
    for cases, muts in ((S.ONE_STEP, [m for m in S.MUTATIONS if m not in S.TWO_STEP_MUTATIONS]), (S.TWO_STEP, S.TWO_STEP_MUTATIONS)):
        _, B, NH, NC, G, seed = cases[f"lin{CS}"]
        c = S.bwd_case(CS, B, NH, NC, G, seed, regime)
        ref = S.sweep(c, c["cks"], c["up"], G)
        for mut in muts:
            m = S.metrics(c, S.sweep(c, c["cks"], c["up"], G, mut), ref, c["up"])
            metric = S.MUTATIONS[mut]
            if metric is None:
                for k in ("dstate", "row"):
                    table[k][3][mut] = m[k]
            else:
                table[metric][2][mut] = m[metric]
    return table


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("CS", [16, 64])
def test_sensitivity_table(CS, regime):
    """every threshold >= 2x the rounding model's worst value (and >= 2x the kernels' worst value on an MI355X, recorded after the
    thresholds were fixed) and <= 1/3 of the distance of every mutation its metric must catch; a reported-only mutation is one no
    metric separates by that rule"""
    table = sensitivity_table(CS, regime)
    for metric, (err, tol, must, rep) in table.items():
        print(f"linear CS={CS} {regime}: {metric:12s} model {err:.3g}  MI355X {SCAN_BWD_MEASURED[metric]:.3g}  threshold {tol:.3g}  "
              + ", ".join(f"{k}: {v:.3g}" for k, v in must.items()) + "".join(f", ({k}: {v:.3g}, reported only)" for k, v in rep.items()))
    caught = set()
    for metric, (err, tol, must, rep) in table.items():
        assert 2 * err <= tol, (metric, err, tol)
        assert 2 * SCAN_BWD_MEASURED[metric] <= tol, (metric, SCAN_BWD_MEASURED[metric], tol)
        for name, v in must.items():
            assert v >= 3 * tol, (metric, name, v, tol)
            caught.add(name)
        for name, v in rep.items():
            assert v < 3 * tol, (metric, name, v, "separated: make it must-catch")
    assert {m for m, metric in S.MUTATIONS.items() if metric is not None} <= caught


def test_generic_column_of_the_table():
    """the generic kernel's thresholds: >= 2x the oracle's own step in fp32 arithmetic (and the MI355X values), none above the MFMA
    column"""
    _, worst32 = model_worst()
    for k in S.METRICS:
        print(f"generic: {k:12s} fp32 step {worst32[k][0]:.3g} ({worst32[k][1]})  MI355X {SCAN_BWD_MEASURED_GENERIC[k]:.3g}  "
              f"threshold {SCAN_BWD_TOL_GENERIC[k]:.3g}")
    for k in S.METRICS:
        assert 2 * worst32[k][0] <= SCAN_BWD_TOL_GENERIC[k] <= SCAN_BWD_TOL[k], (k, worst32[k])
        assert 2 * SCAN_BWD_MEASURED_GENERIC[k] <= SCAN_BWD_TOL_GENERIC[k], k


def test_rounding_model_under_half_of_every_threshold():
    """the condition the seeds were picked for: on every call of the GPU file that is compared with the oracle, with no (b, h), step
    or row left out, the rounding model alone is under half of every threshold"""
    worst, _ = model_worst()
    for k in S.METRICS:
        print(f"{k:12s} worst {worst[k][0]:.3g} in {worst[k][1]}")
        assert worst[k][0] < 0.5 * SCAN_BWD_TOL[k], (k, worst[k])


def test_upstream_is_as_large_as_the_call_s_own_contribution():
    """per (b, h) the upstream has the norm of the call's own contribution (the oracle's dW1 / db1 with zero upstream), is drawn per
    (b, h) and holds fp32 values; so are the checkpoints"""
    for CS in (16, 64):
        c = S.bwd_case(*S.ONE_STEP[f"lin{CS}"], "high")
        own = S.sweep(c, c["cks"], tuple(torch.zeros_like(u) for u in c["up"]), 1)
        for name, u in zip(("dW1", "db1"), c["up"]):
            ratio = u.flatten(2).norm(dim=-1) / own[name].flatten(2).norm(dim=-1)
            assert float((ratio - 1).abs().max()) < 1e-6, (CS, name, ratio)
            assert not torch.equal(u[0], u[1]) and torch.equal(u, u.float().double())
        assert not torch.equal(c["cks"]["W1"][0], c["cks"]["W1"][1]) and torch.equal(c["cks"]["W1"], c["cks"]["W1"].float().double())


# ------------------------------------------------------------------------------------------------ the kernel bodies, emulated
@functools.lru_cache(maxsize=None)
def _emul_run(CS):
    so = C.build_emul("lin16_emul" if CS == 16 else "lin64_emul")
    if so is None:
        pytest.skip("host clang of the ROCm toolchain not available")
    return S.emul_run(ctypes.CDLL(so), CS)


# B NH <= 4: the lin64 emulator runs 256 host threads per (b, h) and takes seconds per call
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("CS", [16, 64])
def test_emulated_backward_one_step(CS, regime):
    """lin16::backward / lin64::backward on the wave emulator, NC = G = 1, B = 2 x 2 heads with a state and an upstream per (b, h):
    against the fp64 step at SCAN_BWD_TOL; in the high regime every must-catch mutation written into the oracle side fails its metric"""
    c = S.bwd_case(CS, 2, 2, 1, 1, 81 + CS, regime)
    got, _ = S.check_call(f"emulated lin{CS} one step {regime}", _emul_run(CS), c, SCAN_BWD_TOL)
    if regime == "high":
        S.check_mutations(f"emulated lin{CS}", c, got, SCAN_BWD_TOL, [m for m in S.MUTATIONS if m not in S.TWO_STEP_MUTATIONS])


@pytest.mark.parametrize("CS", [16, 64])
def test_emulated_backward_off_by_one_mutations(CS):
    c = S.bwd_case(CS, 1, 2, 2, 1, 85 + CS, "high")
    got, _ = S.check_call(f"emulated lin{CS} two steps", _emul_run(CS), c, SCAN_BWD_TOL)
    S.check_mutations(f"emulated lin{CS}", c, got, SCAN_BWD_TOL, S.TWO_STEP_MUTATIONS)


@pytest.mark.parametrize("CS,B,NH,G", [(16, 1, 3, 3), (16, 1, 3, 4), (64, 1, 1, 3), (64, 1, 1, 4)])
def test_emulated_backward_horizon(CS, B, NH, G):
    """one group per call, NC = G: the G-step horizon from one checkpoint against the oracle's backward of that group"""
    c = S.bwd_case(CS, B, NH, G, G, 90 + CS + G, "high")
    S.check_call(f"emulated lin{CS} horizon G={G}", _emul_run(CS), c, SCAN_BWD_TOL)


@pytest.mark.parametrize("CS,B,NH,NC,G", [(16, 1, 2, 11, 4), (16, 1, 2, 7, 3), (16, 2, 1, 3, 1), (64, 1, 1, 5, 2), (64, 1, 1, 4, 3)])
def test_emulated_backward_chain_has_equal_bits(CS, B, NH, NC, G):
    """a call over K groups (ragged last group; even and odd G: the park_early / park_late split of the prefetch across group
    boundaries) against K one-group calls chained through dW1 / db1: equal bits of dXQ, dXK, dXV, d eta, dW1, db1; dln_w / dln_b equal
    to the sum of the partials at the fp32 level"""
    c = S.bwd_case(CS, B, NH, NC, G, 100 + CS + NC, "base")
    S.check_chain(f"emulated lin{CS} {(B, NH, NC, G)}", _emul_run(CS), c, SCAN_BWD_TOL, SCAN_BWD_TOL_GENERIC["dln"])
