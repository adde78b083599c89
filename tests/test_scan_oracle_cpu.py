"""Fixes the tolerances of ``tests/test_scan_oracle_gpu.py`` (one step of the forward TTT scans against the fp64 oracle, stepped
from the scan's own checkpoints: tests/scan_cases.py) with a sensitivity table, as test_glue_oracle_cpu.py does for the glue
kernels: for every metric the distance of the oracle's ROUNDING MODEL (``O.mlp_step_rounded`` / ``O.lin_step_rounded``: the fp64
step with a bf16 rounding wherever the MFMA kernels round) from the fp64 step, the threshold, and the distance of a set of
plausible kernel bugs (the fp64 step with one statement changed).  Then the two mini-batch-16 kernel bodies themselves, run on
the wave emulator of tests/emul, through the same comparison: their arithmetic is checked here, without a GPU."""
import ctypes
import functools

import pytest
import torch

import scan_cases as C
from helpers import SCAN_MEASURED, SCAN_MEASURED_GENERIC, SCAN_TOL, SCAN_TOL_GENERIC
from oracle import ttt_oracle as O


def round_points(kind, CS):
    return O.LIN_ROUND if kind == "linear" else O.MLP_ROUND_CS64 if CS == 64 else O.MLP_ROUND_CS16


def _case(kind, B, NH, NC, CS, G, seed, regime):
    c = C.scan_case(kind, B, NH, NC, CS, seed, regime)
    return c, {k: v.double() for k, v in C.oracle_checkpoints(c, G).items()}


def _distance(c, cks, G, how, ref):
    """metrics of ``how`` (see scan_cases.make_step) stepped from the checkpoints against the fp64 step from the same ones; the
    outputs of a mutated step are rounded to bf16 as a kernel would store them"""
    out, ends = C.horizons(c, cks, G, how)
    if isinstance(how, str) and not how.startswith("fp32"):
        out = out.bfloat16().double()
    return C.metrics(c, out, C.deltas(c["kind"], cks, ends), ref[0], ref[1], round_ref=how != "fp32")


def _ref(c, cks, G):
    out, ends = C.horizons(c, cks, G)
    return out, C.deltas(c["kind"], cks, ends)


# ------------------------------------------------------------------------------------------------ the statements themselves
@pytest.mark.parametrize("kind", ["mlp", "linear"])
def test_rounded_step_with_every_point_off_is_the_primal_step(kind):
    c, cks = _case(kind, 2, 2, 3, 16, 1, 3, "high")
    NH = 2
    gam, bet = c["ln_w"].reshape(1, NH, 1, 64), c["ln_b"].reshape(1, NH, 1, 64)
    st = tuple(cks[k][:, :, 1] for k in C.STATE[kind])
    a = (c["XQ"][:, :, 1], c["XK"][:, :, 1], c["XV"][:, :, 1], c["eta"][:, :, 1], gam, bet, O.LN_EPS)
    prim = (O._mlp_step_primal if kind == "mlp" else O._lin_step_primal)(*st, *a)
    rounded = (O.mlp_step_rounded if kind == "mlp" else O.lin_step_rounded)(*st, *a, on=())
    assert all(torch.equal(x, y) for x, y in zip(rounded[0], prim[0])) and torch.equal(rounded[1], prim[1])
    # ... and the form the roundings are written into (eta carried inside Gs, as the kernels carry it) is the same step, and so
    # is the step the mutations are written into, to the last bits of fp64
    scaled = (O._mlp_step_scaled if kind == "mlp" else O._lin_step_scaled)(*st, *a, frozenset())
    mut = C.step_mut(kind, st, *a[:6])
    for new, out in (scaled, mut):
        assert all(float((x - y).abs().max()) < 1e-15 for x, y in zip(new, prim[0]))
        assert float((out - prim[1]).abs().max()) < 1e-11
    # every point moves the result
    pts = O.MLP_ROUND_POINTS if kind == "mlp" else O.LIN_ROUND_POINTS
    for pt in pts:
        one = (O.mlp_step_rounded if kind == "mlp" else O.lin_step_rounded)(*st, *a, on={pt} | ({"gZ1s"} if pt == "b1_sum" else set()))
        assert not (torch.equal(one[1], prim[1]) and all(torch.equal(x, y) for x, y in zip(one[0], prim[0]))), pt


# ------------------------------------------------------------------------------------------------ sensitivity table
@functools.lru_cache(maxsize=None)
def model_worst():
    """{metric: (worst value, case)} of the rounding model over every MFMA case of the GPU file in both regimes, and the same of
    the oracle's fp32 step over the generic cases (fp32 and bf16 output)"""
    worst, worst32 = {}, {}
    for name, (kind, CS, B, NH, NC, G, seed) in C.MFMA_CASES.items():
        for regime in ("base", "high"):
            c, cks = _case(kind, B, NH, C.run_steps(kind, NC, G), CS, G, seed, regime)
            m = _distance(c, cks, G, round_points(kind, CS), _ref(c, cks, G))
            for k, v in m.items():
                worst[k] = max(worst.get(k, (0.0, "")), (v, f"{name}/{regime}"))
    for name, (kind, CS, B, NH, NC, G, seed) in C.GENERIC_CASES.items():
        c, cks = _case(kind, B, NH, C.run_steps(kind, NC, G), CS, G, seed, "base")
        for how in ("fp32", "fp32_bf16out"):
            m = _distance(c, cks, G, how, _ref(c, cks, G))
            for k, v in m.items():
                worst32[k] = max(worst32.get(k, (0.0, "")), (v, f"{name}/{how}"))
    return worst, worst32


def sensitivity_table(kind, CS, regime):
    """{metric: (rounding model's worst value over the GPU file's cases, threshold, {must-catch mutation: distance},
    {reported mutation: distance})} with the mutations on a B = 2, NH = 3, 5-step scan of this kind"""
    c, cks = _case(kind, 2, 3, 5, CS, 1, 7, regime)
    ref = _ref(c, cks, 1)
    worst, _ = model_worst()
    table = {k: (worst[k][0], SCAN_TOL[k], {}, {}) for k in C.METRICS}
    for mut, metric in C.MUTATIONS.items():
        if mut == "no_b2" and kind != "mlp":
            continue
        m = _distance(c, cks, 1, mut, ref)
        if metric is None:        # reported; must-catch where a metric separates it: 3 thresholds away
            sep = [k for k in ("delta", "row", "gain") if m[k] >= 3 * SCAN_TOL[k]]
            for k in sep[:1] or ["delta"]:
                table[k][2 if sep else 3][mut] = m[k]
        else:
            table[metric][2][mut] = m[metric]
    return table


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("kind,CS", [("mlp", 64), ("mlp", 16), ("linear", 16), ("linear", 64)])
def test_sensitivity_table(kind, CS, regime):
    """every threshold >= 2x the rounding model's worst value and >= 2x the kernels' worst value measured on an MI355X, and
    <= 1/3 of the distance of every mutation its metric must catch"""
    table = sensitivity_table(kind, CS, regime)
    for metric, (err, tol, must, rep) in table.items():
        print(f"{kind} CS={CS} {regime}: {metric:11s} model {err:.3g}  MI355X {SCAN_MEASURED[metric]:.3g}  threshold {tol:.3g}  "
              + ", ".join(f"{k}: {v:.3g}" for k, v in must.items()) + "".join(f", ({k}: {v:.3g}, not separated)" for k, v in rep.items()))
    caught = set()
    for metric, (err, tol, must, rep) in table.items():
        assert 2 * err <= tol, (metric, err, tol)
        assert 2 * SCAN_MEASURED[metric] <= tol, (metric, SCAN_MEASURED[metric], tol)
        for name, v in must.items():
            assert v >= 3 * tol, (metric, name, v, tol)
            caught.add(name)
    want = {m for m, metric in C.MUTATIONS.items() if metric is not None and not (m == "no_b2" and kind != "mlp")}
    assert want <= caught, want - caught
    if kind == "mlp":
        assert "eps_1e-6" in caught          # separated by delta for TTT-MLP; not for TTT-Linear (4e-3), nor erf GELU (1e-7: |Z1| << 1)


def test_generic_column_of_the_table():
    """the generic kernels' thresholds: >= 2x the oracle's own fp32 step and the MI355X values, none above the MFMA column"""
    _, worst32 = model_worst()
    for k in C.METRICS:
        print(f"generic: {k:11s} fp32 step {worst32[k][0]:.3g} ({worst32[k][1]})  MI355X {SCAN_MEASURED_GENERIC[k]:.3g}  threshold {SCAN_TOL_GENERIC[k]:.3g}")
    for k in C.METRICS:
        assert 2 * worst32[k][0] <= SCAN_TOL_GENERIC[k] <= SCAN_TOL[k], (k, worst32[k])
        assert 2 * SCAN_MEASURED_GENERIC[k] <= SCAN_TOL_GENERIC[k], k


def test_rounding_model_under_half_of_every_threshold():
    """the condition the cases (seeds, base_lr of the "high" regime) were picked for: on every case of the GPU file, with no step,
    head or row left out, the rounding model alone is under half of every threshold"""
    worst, _ = model_worst()
    for k in C.METRICS:
        print(f"{k:11s} worst {worst[k][0]:.3g} in {worst[k][1]}")
        assert worst[k][0] < 0.5 * SCAN_TOL[k], (k, worst[k])


def test_high_regime_moves_the_state_by_percents():
    for kind, name in (("mlp", "W2"), ("linear", "W1")):
        for regime, lo, hi in (("base", 0.0, 1.0), ("high", 0.01, 10.0)):
            c, cks = _case(kind, 1, 2, 4, 64, 1, 5, regime)
            _, d = _ref(c, cks, 1)
            rel = d[name].flatten(3).norm(dim=-1) / cks[name].flatten(3).norm(dim=-1)
            print(f"{kind} {regime}: a step moves {name} by {float(rel.min()):.3g} .. {float(rel.max()):.3g} of its norm")
            assert lo <= float(rel.min()) and float(rel.max()) <= hi, (kind, regime, rel)


# ------------------------------------------------------------------------------------------------ the CS = 16 bodies, emulated
class MlpParams(ctypes.Structure):            # wv::Mlp16Params (csrc/ttt_wave_types.h)
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("XQ", "XK", "XV", "eta", "ln_w", "ln_b", "W1", "b1", "W2", "b2", "W1c", "b1c", "W2c", "b2c", "out")] + \
               [(n, ctypes.c_int) for n in ("NH", "NC", "G", "K")] + [("eps", ctypes.c_float)]


class ChunkParams(ctypes.Structure):          # wv::Mlp16ChunkParams
    _fields_ = [("p", MlpParams), ("step0", ctypes.c_int), ("NCs", ctypes.c_int)] + \
               [(n, ctypes.c_void_p) for n in ("W1f", "b1f", "W2f", "b2f")]


def _lin_params():
    from test_emul_cpu import Params
    return Params


def _emul(name):
    so = C.build_emul(name)
    if so is None:
        pytest.skip("host clang of the ROCm toolchain not available")
    return ctypes.CDLL(so)


def _host_buffers(c):
    kind = c["kind"]
    B, NH, NC, CS, _ = c["XQ"].shape
    bf = lambda t: t.to(torch.bfloat16).contiguous()
    t = {k: bf(c[k]) for k in ("XQ", "XK", "XV", "eta")}
    t.update(ln_w=c["ln_w"].float().contiguous(), ln_b=c["ln_b"].float().contiguous())
    t.update({k: c[k].float().contiguous() for k in C.STATE[kind]})
    return t


def _check(tag, c, out, cks, G, final, tol=SCAN_TOL):
    assert not torch.isnan(out.float()).any() and not any(torch.isnan(v).any() for v in cks.values()), tag
    C.assert_initial_state(c, cks)
    m = C.compare(c, out, cks, G, final)
    print(f"{tag}: {C.fmt(m)}")
    bad = {k: (v, tol[k]) for k, v in m.items() if not v < tol[k]}
    assert not bad, (tag, bad)
    return m


def _run_mlp16(lib, c, G, cuts):
    t = _host_buffers(c)
    B, NH, NC = c["XQ"].shape[:3]
    K = -(-NC // G)
    nan = lambda *s: torch.full(s, float("nan"))
    cks = dict(W1=nan(B, NH, K, 64, 256), b1=nan(B, NH, K, 1, 256), W2=nan(B, NH, K, 256, 64), b2=nan(B, NH, K, 1, 64))
    out = torch.full((B, NH, NC, 16, 64), float("nan"), dtype=torch.bfloat16)
    state = [t[k].clone() for k in C.STATE["mlp"]]
    msg = ctypes.create_string_buffer(256)
    for s0, s1 in zip((0,) + cuts, cuts + (NC,)):
        p = ChunkParams()
        for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=state[0], b1=state[1],
                         W2=state[2], b2=state[3], W1c=cks["W1"], b1c=cks["b1"], W2c=cks["W2"], b2c=cks["b2"], out=out).items():
            setattr(p.p, n, v.data_ptr())
        p.p.NH, p.p.NC, p.p.G, p.p.K, p.p.eps = NH, s1 - s0, G, K, 1e-8
        p.step0, p.NCs = s0, NC
        p.W1f, p.b1f, p.W2f, p.b2f = (s.data_ptr() for s in state)
        assert lib.emul_mlp16_forward_part(ctypes.byref(p), B * NH, msg, 256) == 0, msg.value.decode()
    return out, cks, state


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("B,NH,NC,G,cuts", [(2, 2, 4, 1, ()), (1, 2, 7, 3, (1, 2))])
def test_emulated_mlp16_scan_one_step_at_a_time(B, NH, NC, G, cuts, regime):
    """csrc/ttt_mlp16_body.h on the wave emulator: every step (G = 1), every 3-step horizon (G = 3, ragged, the scan cut at steps
    1 and 2, off the group boundaries) and the state after the last step against the fp64 step at SCAN_TOL; the initial state
    differs per batch element"""
    lib = _emul("mlp16_chunk_emul")
    assert lib.emul_mlp16_chunk_params_size() == ctypes.sizeof(ChunkParams)
    c = C.scan_case("mlp", B, NH, NC, 16, 31 + NC, regime)
    out, cks, final = _run_mlp16(lib, c, G, cuts)
    _check(f"emulated mlp16 {(B, NH, NC, G)} {regime}", c, out, cks, G, final)


def _run_lin16(lib, c, G):
    Params = _lin_params()
    assert lib.emul_lin16_params_size() == ctypes.sizeof(Params)
    t = _host_buffers(c)
    B, NH, NC = c["XQ"].shape[:3]
    K = -(-NC // G)
    cks = dict(W1=torch.full((B, NH, K, 64, 64), float("nan")), b1=torch.full((B, NH, K, 1, 64), float("nan")))
    out = torch.full((B, NH, NC, 16, 64), float("nan"), dtype=torch.bfloat16)
    p = Params()
    for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=t["W1"], b1=t["b1"],
                     W1c=cks["W1"], b1c=cks["b1"], out=out).items():
        setattr(p, n, v.data_ptr())
    p.NH, p.NC, p.G, p.K, p.eps = NH, NC, G, K, 1e-8
    lib.emul_lin16_forward(ctypes.byref(p), B * NH)
    return out, cks


@pytest.mark.parametrize("regime", ["base", "high"])
@pytest.mark.parametrize("B,NH,NC,G", [(2, 3, 6, 1), (1, 2, 7, 3)])
def test_emulated_lin16_forward_one_step_at_a_time(B, NH, NC, G, regime):
    """csrc/ttt_lin16_body.h ``forward`` on the wave emulator (nothing hands back the last state: with G = 1 the scan runs one
    step more than have a delta)"""
    lib = _emul("lin16_emul")
    c = C.scan_case("linear", B, NH, NC, 16, 41 + NC, regime)
    out, cks = _run_lin16(lib, c, G)
    _check(f"emulated lin16 {(B, NH, NC, G)} {regime}", c, out, cks, G, None)


def test_comparison_fails_for_every_must_catch_mutation_on_the_emulated_kernels():
    """each must-catch mutation written into the ORACLE side of the comparison with the (correct) emulated kernels: the metric
    named for it fails - the comparison can fail"""
    for kind, lib_name in (("mlp", "mlp16_chunk_emul"), ("linear", "lin16_emul")):
        lib = _emul(lib_name)
        c = C.scan_case(kind, 2, 2, 4, 16, 77, "high")
        if kind == "mlp":
            out, cks, final = _run_mlp16(lib, c, 1, ())
        else:
            (out, cks), final = _run_lin16(lib, c, 1), None
        for mut, metric in C.MUTATIONS.items():
            if metric is None or (mut == "no_b2" and kind != "mlp"):
                continue
            m = C.compare(c, out, cks, 1, final, how=mut)
            print(f"{kind} {mut:20s} {metric}: {m[metric]:.3g} (threshold {SCAN_TOL[metric]:.3g})")
            assert m[metric] > SCAN_TOL[metric], (kind, mut, m)
