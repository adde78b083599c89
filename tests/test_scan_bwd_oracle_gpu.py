"""The TTT-Linear backward sweeps on the device (through ``ttt_linear_backward_impl`` of the ``test_time_training`` binding), ONE CALL
AT A TIME against the fp64 oracle: linear_bwd16_kernel (mini-batches of 16, ``auto``), the opt-in linear_bwd_cs64_kernel (mini-batches
of 64, ``impl="mfma"``) and the generic bwd_kernel on its TTT-Linear path.  A call is one step (NC = G = 1) or one group (a G-step
horizon) from the fp64 forward's checkpoint with a NONZERO upstream state gradient drawn per (b, h); a call over K groups must equal
the chain of its K one-group calls - for the MFMA kernels bit for bit (tests/scan_bwd_cases.py).  Tolerances: helpers.SCAN_BWD_TOL /
SCAN_BWD_TOL_GENERIC, fixed by the sensitivity table of tests/test_scan_bwd_oracle_cpu.py.  Every output starts as NaN between NaN
guards, the scratch's bounds are checked, inputs, checkpoints and upstream must come back unchanged, and every test prints its worst
value per metric."""
import pytest
import torch

import scan_bwd_cases as S
from helpers import SCAN_BWD_TOL, SCAN_BWD_TOL_GENERIC
from test_scan_oracle_gpu import assert_written_inside, guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
F = S.F
# mini-batch size -> (impl asked for, what it must resolve to) of the MFMA sweep and of the generic kernel
MFMA = {16: ("auto", "mfma"), 64: ("mfma", "mfma")}
GENERIC = {16: ("generic", "generic"), 64: ("auto", "generic")}


def ext():
    import test_time_training as e
    e.load_library()
    return e


def device_run(e, impl, resolves_to):
    """``run`` of scan_bwd_cases over the binding, the selector given per call"""
    def run(t, cks, up, G):
        B, NH, NC, CS, _ = t["XQ"].shape
        act = t["XQ"].dtype
        assert e.resolved_impl(B, NH, NC, CS, F, G, act, mlp=False, backward=True, impl=impl) == resolves_to
        ins = {k: v.to(DEV).contiguous() for k, v in t.items()}
        ins.update(W1c=cks["W1"].to(DEV), b1c=cks["b1"].to(DEV), dW1_last=up[0].to(DEV), db1_last=up[1].to(DEV))
        keep = {k: v.clone() for k, v in ins.items()}
        gb = {"dln_w": guarded((B, NH, 1, F), F32), "dln_b": guarded((B, NH, 1, F), F32), "dW1": guarded((B, NH, F, F), F32),
              "db1": guarded((B, NH, 1, F), F32), "dlast_eta": guarded((B, NH, NC, CS, 1), act), "dXQ": guarded((B, NH, NC, CS, F), act),
              "dXK": guarded((B, NH, NC, CS, F), act), "dXV": guarded((B, NH, NC, CS, F), act)}
        scr = {"W1_init_group": guarded((B, NH, G, F, F), F32), "b1_init_group": guarded((B, NH, G, 1, F), F32)}
        g = {k: v[1] for k, v in gb.items()}
        e.ttt_linear_backward_impl(impl, ins["XQ"], ins["XK"], ins["XV"], ins["eta"], ins["ln_w"], ins["ln_b"], ins["W1c"], ins["b1c"],
                                   ins["dW1_last"], ins["db1_last"], ins["dOut"], scr["W1_init_group"][1], scr["b1_init_group"][1],
                                   g["dln_w"], g["dln_b"], g["dW1"], g["db1"], g["dlast_eta"], g["dXQ"], g["dXK"], g["dXV"], G)
        torch.cuda.synchronize()
        what = f"linear backward CS={CS} {impl} {(B, NH, NC, G)}"
        assert_written_inside(gb, what)
        for name, (buf, _) in scr.items():       # opaque scratch: only its bounds are checked
            assert bool(torch.isnan(buf[:256]).all()) and bool(torch.isnan(buf[-256:]).all()), f"{what}: write outside {name}"
        for k, v in ins.items():
            assert torch.equal(v, keep[k]), f"{what}: {k} was written"
        assert e.get_impl() == "auto"
        return {k: v.cpu() for k, v in g.items()}
    return run


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("CS", [16, 64])
def test_mfma_backward_one_step(CS, regime):
    """NC = G = 1, B = 2 x 5 heads, a checkpoint and an upstream per (b, h): the MFMA sweeps against O._lin_step_bwd"""
    c = S.bwd_case(*S.ONE_STEP[f"lin{CS}"], regime)
    S.check_call(f"lin{CS} mfma one step {regime}", device_run(ext(), *MFMA[CS]), c, SCAN_BWD_TOL)


@pytest.mark.parametrize("act", [BF, F32])
@pytest.mark.parametrize("CS", [16, 64])
def test_generic_backward_one_step(CS, act):
    """the generic kernel (fp32 arithmetic; only bf16 stores round) on the same one-step cases, bf16 and fp32 activations, at the
    table's generic column"""
    c = S.bwd_case(*S.ONE_STEP[f"lin{CS}"], "base")
    impl = GENERIC[CS] if act == BF else ("generic", "generic")
    S.check_call(f"lin{CS} generic one step {act}", device_run(ext(), *impl), c, SCAN_BWD_TOL_GENERIC, act=act)


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("name", list(S.HORIZON))
def test_mfma_backward_horizon(name, regime):
    """one group per call, NC = G in {3, 4}: the G-step horizon from one checkpoint against the oracle's backward of that group"""
    c = S.bwd_case(*S.HORIZON[name], regime)
    CS = S.HORIZON[name][0]
    S.check_call(f"{name} mfma horizon {regime}", device_run(ext(), *MFMA[CS]), c, SCAN_BWD_TOL)


CHAINS = [(CS, NC, G) for CS in S.CHAIN for NC, G in S.CHAIN[CS]]


@pytest.mark.parametrize("CS,NC,G", CHAINS)
def test_mfma_backward_chain_has_equal_bits(CS, NC, G):
    """a call over K groups (ragged last group, G in {1, 2, 3, 4}: both parities of the prefetch across group boundaries) against K
    one-group calls chained through dW1 / db1 from the same checkpoints: equal bits of dXQ, dXK, dXV, d eta, dW1, db1; dln_w / dln_b
    equal to the sum of the calls' partials at the fp32 level"""
    c = S.bwd_case(CS, S.CHAIN_B, S.CHAIN_NH, NC, G, 100 + CS + NC, "base")
    S.check_chain(f"lin{CS} mfma {(NC, G)}", device_run(ext(), *MFMA[CS]), c, SCAN_BWD_TOL, SCAN_BWD_TOL_GENERIC["dln"])


@pytest.mark.parametrize("CS,NC,G", CHAINS)
def test_generic_backward_chain(CS, NC, G):
    """the same chain on the generic kernel, every metric of the whole call against the chain at the generic column; whether the bits
    are equal is printed"""
    c = S.bwd_case(CS, S.CHAIN_B, S.CHAIN_NH, NC, G, 100 + CS + NC, "base")
    S.check_chain(f"lin{CS} generic {(NC, G)}", device_run(ext(), *GENERIC[CS]), c, SCAN_BWD_TOL_GENERIC, SCAN_BWD_TOL_GENERIC["dln"],
                  exact=False)


@pytest.mark.parametrize("CS", [16, 64])
def test_comparison_fails_for_every_must_catch_mutation(CS):
    """each must-catch mutation of the sensitivity table written into the ORACLE side of the comparison with the device's own results
    (the one-step case in the high regime; the two-step case for the two off-by-one mutations): the metric named for it fails"""
    run = device_run(ext(), *MFMA[CS])
    c = S.bwd_case(*S.ONE_STEP[f"lin{CS}"], "high")
    got, _ = S.check_call(f"lin{CS} mfma one step high", run, c, SCAN_BWD_TOL)
    S.check_mutations(f"lin{CS} mfma", c, got, SCAN_BWD_TOL, [m for m in S.MUTATIONS if m not in S.TWO_STEP_MUTATIONS])
    c = S.bwd_case(*S.TWO_STEP[f"lin{CS}"], "high")
    got, _ = S.check_call(f"lin{CS} mfma two steps high", run, c, SCAN_BWD_TOL)
    S.check_mutations(f"lin{CS} mfma", c, got, SCAN_BWD_TOL, S.TWO_STEP_MUTATIONS)
