"""The forward TTT scans on the device (through the ``test_time_training`` binding), ONE STEP AT A TIME against the fp64 oracle:
the state delta between consecutive fp32 checkpoints and the step's output, the oracle stepped from the kernel's own checkpoint
(tests/scan_cases.py), at the tolerances the sensitivity table of tests/test_scan_oracle_cpu.py fixes (helpers.SCAN_TOL; the
generic kernels SCAN_TOL_GENERIC).  Initial states differ per batch element, outputs and checkpoints start as NaN between NaN
guards, and every test prints its worst value per metric."""
import pytest
import torch

import scan_cases as C
from helpers import SCAN_TOL, SCAN_TOL_GENERIC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 256     # elements of NaN in front of and behind every output buffer


def ext():
    import test_time_training as e
    e.load_library()
    return e


def guarded(shape, dtype):
    """(buffer, view): a NaN buffer with GUARD elements around the contiguous view of ``shape`` a kernel writes"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def assert_written_inside(bufs, what):
    for name, (buf, view) in bufs.items():
        assert bool(torch.isnan(buf[:GUARD].float()).all()) and bool(torch.isnan(buf[-GUARD:].float()).all()), f"{what}: write outside {name}"
        assert not bool(torch.isnan(view.float()).any()), f"{what}: {name} not fully written"


def run_scan(e, c, G, act=torch.bfloat16, impl="mfma", cuts=None, pair=None):
    """the forward scan of the case: one call (``cuts`` None), or - TTT-MLP on the MFMA scan - ``ttt_forward_chunk`` over the
    parts the cuts make, the state carried in place -> out, {name: checkpoints}, state after the last step or None"""
    kind = c["kind"]
    B, NH, NC, CS, F = c["XQ"].shape
    K = -(-NC // G)
    X = [c[k].to(DEV, act).contiguous() for k in ("XQ", "XK", "XV", "eta")]
    lshape = (1, NH, 1, F) if kind == "mlp" else (NH, F)
    ln = [c[k].reshape(lshape).to(DEV, torch.float32).contiguous() for k in ("ln_w", "ln_b")]
    st = [c[k].to(DEV, torch.float32).contiguous() for k in C.STATE[kind]]
    bufs = {"out": guarded((B, NH, NC, CS, F), act)}
    for k, s in zip(C.STATE[kind], st):
        bufs[k] = guarded((B, NH, K) + tuple(s.shape[2:]), torch.float32)
    out, cks = bufs["out"][1], [bufs[k][1] for k in C.STATE[kind]]
    final = None
    e.set_impl(impl)
    if pair is not None:
        e.debug_option("scan_pair", pair)
    try:
        if cuts is not None:
            assert kind == "mlp"
            final = [s.clone() for s in st]
            for s0, s1 in zip((0,) + tuple(cuts), tuple(cuts) + (NC,)):
                e.ttt_forward_chunk(*X, *ln, *final, *cks, out, G, s0, s1 - s0)
        elif kind == "mlp":
            e.ttt_forward(*X, *ln, *st, *cks, out, G)
        else:
            e.ttt_linear_forward(*X, *ln, *st, *cks, out, G)
        torch.cuda.synchronize()
    finally:
        e.set_impl("auto")
        if pair is not None:
            e.debug_option("scan_pair", 1)
    assert_written_inside(bufs, f"{kind} CS={CS} {(B, NH, NC, G)} cuts={cuts}")
    if kind == "mlp":
        assert e.sweep_error() == 0
    for s, k in zip(st, C.STATE[kind]):
        assert torch.equal(s.cpu().double(), c[k]), f"the initial state {k} was written"
    return out.cpu(), {k: v.cpu() for k, v in zip(C.STATE[kind], cks)}, None if final is None else [f.cpu() for f in final]


def check(tag, c, out, cks, G, final, tol=SCAN_TOL):
    C.assert_initial_state(c, cks)
    m = C.compare(c, out, cks, G, final, round_ref=out.dtype == torch.bfloat16)
    print(f"{tag}: {C.fmt(m)}")
    bad = {k: (v, tol[k]) for k, v in m.items() if not v < tol[k]}
    assert not bad, (tag, bad)
    return m


def case(name, regime, table=C.MFMA_CASES):
    kind, CS, B, NH, NC, G, seed = table[name]
    return C.scan_case(kind, B, NH, C.run_steps(kind, NC, G), CS, seed, regime), kind, CS, B, NH, G


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("name", ["mlp64_b2", "mlp64_ragged", "mlp64_9heads"])
def test_mlp_cs64_mfma_scan_one_step_at_a_time(name, pair, regime):
    """TTT-MLP at mini-batches of 64, forced ``mfma``, as the pair of workgroups (``scan_pair`` 1) and as one workgroup (0):
    B = 2 x 5 heads; G = 3 with a ragged last group (3-step horizons from each checkpoint); 9 heads, where the pair form's
    role-B workgroups start past block 8"""
    e = ext()
    c, kind, CS, B, NH, G = case(name, regime)
    assert e.resolved_impl(B, NH, c["XQ"].shape[2], CS, 64, G, torch.bfloat16, mlp=True, backward=False) == "mfma"
    out, cks, _ = run_scan(e, c, G, pair=pair)
    check(f"{name} pair={pair} {regime}", c, out, cks, G, None)


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("pair", [1, 0])
def test_mlp_cs64_mfma_scan_in_parts_with_the_last_state(pair, regime):
    """the first case through ``ttt_forward_chunk`` cut at steps 1, 2, 7 (a part of one step): every step, and the delta of the
    last one from the state the last part hands back"""
    e = ext()
    c, kind, CS, B, NH, G = case("mlp64_b2", regime)
    out, cks, final = run_scan(e, c, G, cuts=C.PART_CUTS, pair=pair)
    check(f"mlp64_b2 in parts pair={pair} {regime}", c, out, cks, G, final)


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("cuts", [None, C.PART_CUTS])
@pytest.mark.parametrize("name", ["mlp16_b2", "mlp16_ragged"])
def test_mlp_cs16_mfma_scan_one_step_at_a_time(name, cuts, regime):
    """TTT-MLP at mini-batches of 16: one call, and parts cut at 1, 2, 7 (off the boundaries of the groups of 4) with the state
    after the last step"""
    e = ext()
    c, kind, CS, B, NH, G = case(name, regime)
    assert e.resolved_impl(B, NH, c["XQ"].shape[2], CS, 64, G, torch.bfloat16, mlp=True, backward=False) == "mfma"
    out, cks, final = run_scan(e, c, G, cuts=cuts)
    check(f"{name} cuts={cuts} {regime}", c, out, cks, G, final)


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("name", ["lin16_b2", "lin16_ragged", "lin64_b2"])
def test_linear_scan_one_step_at_a_time(name, regime):
    """TTT-Linear with bf16 activations as ``auto`` resolves it: the MFMA scan at mini-batches of 16; at mini-batches of 64 this
    library has no MFMA TTT-Linear kernel (``ttt::mfma::supports``) and ``resolved_impl`` says ``generic``, whose fp32 arithmetic
    is held to the tighter generic column.  With G = 1 the scan runs one step more than have a delta."""
    e = ext()
    c, kind, CS, B, NH, G = case(name, regime)
    impl = e.resolved_impl(B, NH, c["XQ"].shape[2], CS, 64, G, torch.bfloat16, mlp=False, backward=False)
    assert impl == ("mfma" if CS == 16 else "generic")
    out, cks, _ = run_scan(e, c, G, impl="auto")
    check(f"{name} {regime} ({impl})", c, out, cks, G, None, SCAN_TOL if impl == "mfma" else SCAN_TOL_GENERIC)


@pytest.mark.parametrize("act", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("name", list(C.GENERIC_CASES))
def test_generic_scans_one_step_at_a_time(name, act):
    """the ``generic`` kernels (fp32 arithmetic; only a bf16 output store rounds), TTT-MLP and TTT-Linear at both mini-batch
    sizes, bf16 and fp32 activations, at the table's second column"""
    e = ext()
    c, kind, CS, B, NH, G = case(name, "base", C.GENERIC_CASES)
    out, cks, _ = run_scan(e, c, G, act=act, impl="generic")
    check(f"generic {name} {act}", c, out, cks, G, None, SCAN_TOL_GENERIC)


@pytest.mark.parametrize("name", ["mlp64_b2", "mlp16_b2", "lin16_b2"])
def test_comparison_fails_for_every_must_catch_mutation(name):
    """each must-catch mutation of the sensitivity table written into the ORACLE side of the comparison with the kernel: the
    metric named for it fails (the comparison can fail, on the device's own results)"""
    e = ext()
    c, kind, CS, B, NH, G = case(name, "high")
    out, cks, _ = run_scan(e, c, G)
    for mut, metric in C.MUTATIONS.items():
        if metric is None or (mut == "no_b2" and kind != "mlp"):
            continue
        m = C.compare(c, out, cks, G, None, how=mut)
        print(f"{name} {mut:20s} {metric}: {m[metric]:.3g} (threshold {SCAN_TOL[metric]:.3g})")
        assert m[metric] > SCAN_TOL[metric], (name, mut, m)
