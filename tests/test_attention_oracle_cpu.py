"""Pins the rounding-aware statements of the segment-attention kernels (``oracle/attn_oracle.py``: ``fwd``, ``bwd``, ``pre``) to the
exact attention and to the module's unfused bf16 path, and fixes the tolerances of ``tests/test_attention_oracle_gpu.py`` with a
sensitivity table, as ``test_glue_oracle_cpu.py`` does for the glue kernels: for every metric the GPU file asserts, the distance a
correct fp32 kernel can have (the statement in fp32 against fp64; for dK / dV the accumulator-initialised form of the shipped
kernel) and the distance of seeded kernel bugs (the statement with one line changed).  Then the workgroup bodies of
``csrc/attn_body.h`` run on the CPU wave emulator under the same tolerances."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import attn_cases as C
from helpers import ATTN_TOL, ATTN_TOL_LARGE, rel_l2, ulp_stats
from oracle import attn_oracle as AO
from test_emul_attention_cpu import _bwd_params, _forward, emul  # noqa: F401  (emul: the wave emulator fixture)

SHAPES = [(1, 2, 40), (2, 3, 300), (1, 1, 577)]


@pytest.mark.parametrize("B,NH,S", SHAPES)
def test_statements_without_rounding_are_exact_attention(B, NH, S):
    """rnd=False: fwd == AO.attention == fp64 SDPA, bwd (plain and accumulator-initialised) == autograd of AO.attention"""
    q, k, v, do = C.model_case(B, NH, S, S, torch.float64)
    o, lse = AO.fwd(q, k, v, rnd=False)
    q64, k64, v64 = (t.clone().requires_grad_(True) for t in (q, k, v))
    ro, rl = AO.attention(q64, k64, v64)
    ro.backward(do)
    sdpa = F.scaled_dot_product_attention(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False)
    assert rel_l2(o, ro) < 1e-12 and rel_l2(o, sdpa) < 1e-12
    assert float((lse - rl.detach()).abs().max()) < 1e-12
    for acc_init in (False, True):
        g = AO.bwd(q, k, v, do, ro.detach(), rl.detach(), rnd=False, acc_init=acc_init)
        for n, want in (("dq", q64.grad), ("dk", k64.grad), ("dv", v64.grad)):
            assert rel_l2(g[n], want) < 1e-12, (acc_init, n, rel_l2(g[n], want))
        assert rel_l2(g["delta"], (ro * do).sum(-1)) < 1e-12


@pytest.mark.parametrize("B,S,NH,n_text", [(2, 200, 3, 37), (1, 96, 2, 0), (1, 50, 2, 50)])
def test_pre_statement_matches_module(B, S, NH, n_text):
    """rnd=False in fp64: pre == AO.qk_pre, forward and gradients.  rnd=True in fp64 on bf16 inputs == the module's unfused bf16 path
    (dit.py ``_segment``, else branch: q_norm / k_norm, then Rotary3DPositionEmbedding on the video tokens, bf16 CPU tensors).
    That path forms LN(x) w + b in fp32 before its one rounding, the statement in fp64: where the two straddle a rounding boundary
    they differ by 1 ulp, and the rotation carries it on - at most 1 ulp, on well under 1 % of the elements (printed)."""
    from ttt_amd.models.cogvideo.utils import Rotary3DPositionEmbedding
    d = C.pre_case(B, S, NH, n_text, 9, torch.float64)
    x = {n: d[n].clone().requires_grad_(True) for n in ("q_raw", "k_raw") + C.PRE_PARAMS}
    q, k = AO.pre(x["q_raw"], x["k_raw"], x["wq"], x["bq"], x["wk"], x["bk"], d["cos"], d["sin"], NH, n_text, rnd=False)
    y = {n: d[n].clone().requires_grad_(True) for n in ("q_raw", "k_raw") + C.PRE_PARAMS}
    rq, rk = AO.qk_pre(y["q_raw"], y["k_raw"], y["wq"], y["bq"], y["wk"], y["bk"], d["cos"], d["sin"], NH, n_text)
    assert rel_l2(q.transpose(1, 2), rq) < 1e-12 and rel_l2(k.transpose(1, 2), rk) < 1e-12
    ga = torch.autograd.grad((q, k), list(x.values()), (d["dq"], d["dk"]))
    gb = torch.autograd.grad((rq, rk), list(y.values()), (d["dq"].transpose(1, 2), d["dk"].transpose(1, 2)))
    assert all(rel_l2(a, b) < 1e-12 for a, b in zip(ga, gb))

    want = AO.pre(*(d[n] for n in ("q_raw", "k_raw", "wq", "bq", "wk", "bk", "cos", "sin")), NH, n_text)
    rot = Rotary3DPositionEmbedding(4, 4, (S - n_text + 16) // 16, 64)
    for raw, w, b, ref in ((d["q_raw"], d["wq"], d["bq"], want[0]), (d["k_raw"], d["wk"], d["bk"], want[1])):
        ln = torch.nn.LayerNorm(64, eps=1e-6).bfloat16()
        with torch.no_grad():
            ln.weight.copy_(w)
            ln.bias.copy_(b)
            t = ln(raw.bfloat16().view(B, S, NH, 64).transpose(1, 2))
            t = torch.cat((t[:, :, :n_text], rot(t[:, :, n_text:])), dim=2).transpose(1, 2)
        frac_flips = float((t.double() != ref).double().mean())
        frac, mx = ulp_stats(t, ref, floor=float(ref.square().mean().sqrt()))
        print(f"pre vs module (B={B} S={S} NH={NH} n_text={n_text}): {frac_flips:.2e} of the elements differ, max {mx:.2f} ulp")
        assert mx <= 1.0 and frac_flips < 1e-2


# ------------------------------------------------------------------------------------------------ sensitivity table
def _metrics(got, want):
    """the GPU file's metrics of one result set: {metric: distance}, the worst over the tensors it is asserted on"""
    r = {}
    for n in ("O", "dq", "dk", "dv", "q", "k", "dq_raw", "dk_raw"):
        if n in want:
            frac, mx, row = C.out_metrics(got[n], want[n], C.PRE_FLOOR if n in C.PRE_OUTS else 0.125)
            r["ulp_frac"] = max(r.get("ulp_frac", 0.0), frac)
            r["ulp_max"] = max(r.get("ulp_max", 0.0), mx)
            r["row"] = max(r.get("row", 0.0), row)
    if "LSE" in want:
        r["lse"] = float((got["LSE"].double() - want["LSE"]).abs().max())
    if "dq_mag" in want:
        r["cancel"] = max(C.cancel_err(got[n], want[n], want[n + "_mag"]) for n in ("dq", "dk"))
    if "delta" in want:
        r["delta"] = C.delta_err(got["delta"], want["delta"], want["_o"], want["_do"])
    ps = [rel_l2(got[n], want[n]) for n in C.PRE_PARAMS if n in want]
    if ps:
        r["psum"] = max(ps)
    return r


def _attn_runs(q, k, v, do, dtype, **mut):
    """forward and backward statements on one set of inputs: the backward takes the fp64 forward's O and LSE (fp32, as stored)"""
    fmut = {n: x for n, x in mut.items() if n in ("mask", "rescale_o", "drop_tile_last", "lse_units", "half_rowsum", "l_rounded")}
    bmut = {n: x for n, x in mut.items() if n not in fmut}
    cast = lambda *ts: [t.to(dtype) for t in ts]
    o64, lse64 = AO.fwd(q, k, v)
    o, lse = AO.fwd(*cast(q, k, v), **fmut)
    lse_in = lse64.float().double()
    g = AO.bwd(*cast(q, k, v, do, o64, lse_in), mags=dtype == torch.float64, **bmut)
    if dtype == torch.float32 and not bmut:     # dK / dV: the kernel's accumulator-initialised form in fp32; dQ the plain form
        gi = AO.bwd(*cast(q, k, v, do, o64, lse_in), acc_init=True)
        g["dk"], g["dv"] = gi["dk"], gi["dv"]
    r = {"O": o, "LSE": lse, "_o": o64, "_do": do}
    r.update(g)
    return r


def sensitivity_table():
    """{metric: (fp32 error, threshold, {mutation: distance})}, the large-|LSE| regime {metric: (fp32 error, threshold)} and the
    in-band mutations {name: (metric, distance)}, on model-range inputs at 3 heads x 300 tokens (ragged: 4 full tiles + 44) and
    the pre kernel's inputs at 2 x 200 tokens, 3 heads, 37 text tokens"""
    q, k, v, do = C.model_case(1, 3, 300, 1, torch.float64)
    ref = _attn_runs(q, k, v, do, torch.float64)
    fp32 = _metrics(_attn_runs(q, k, v, do, torch.float32), ref)
    ql, kl, vl, dol = C.large_lse_case(1, 4, 300, 2, dtype=torch.float64)
    large = _metrics(_attn_runs(ql, kl, vl, dol, torch.float32), _attn_runs(ql, kl, vl, dol, torch.float64))
    B, S, NH, nt = 2, 200, 3, 37
    d = C.pre_case(B, S, NH, nt, 5)
    pref = C.pre_oracle(d, NH, nt)
    for m, x in _metrics(C.pre_oracle(d, NH, nt, torch.float32), pref).items():
        fp32[m] = max(fp32.get(m, 0.0), x)

    attn = lambda **kw: _metrics(_attn_runs(q, k, v, do, torch.float64, **kw), ref)
    prem = lambda **kw: _metrics(C.pre_oracle(d, NH, nt, **kw), pref)
    must = {    # name: (metric it must trip, its distances)
        "fwd: ragged mask off": ("ulp_frac", attn(mask=False)),
        "fwd: ragged mask off (LSE)": ("lse", attn(mask=False)),
        "fwd: O not rescaled when the max grows": ("row", attn(rescale_o=False)),
        "fwd: last key of every tile dropped": ("row", attn(drop_tile_last=True)),
        "fwd: LSE in log2 units": ("lse", attn(lse_units="log2")),
        "fwd: LSE without m*scale": ("lse", attn(lse_units="no_m")),
        "fwd: row sum of one half-wave": ("row", attn(half_rowsum=True)),
        "bwd: Delta from dO*dO": ("delta", attn(delta_from_do=True)),
        "bwd: dK without scale": ("row", attn(dk_scale=False)),
        "bwd: dK without scale (cancel)": ("cancel", attn(dk_scale=False)),
        "bwd: LSE of the neighbouring head": ("row", attn(lse_head_shift=1)),
        "bwd: LSE of the neighbouring head (cancel)": ("cancel", attn(lse_head_shift=1)),
        "bwd: last partial query tile left out of dK/dV": ("row", attn(drop_last_qtile=True)),
        "pre: sign of sin": ("row", prem(sin_sign=-1.0)),
        "pre: RoPE from n_text - 1": ("row", prem(rope_start=nt - 1)),
        "pre: unbiased variance": ("ulp_frac", prem(unbiased=True)),
        "pre: cos/sin not rounded (dw)": ("psum", prem(round_tables=False)),
        "pre: unbiased variance (dw)": ("psum", prem(unbiased=True)),
    }
    in_band = {"fwd: l summed from bf16 P": ("lse", attn(l_rounded=True)["lse"]),
               "pre: cos/sin not rounded": ("ulp_frac", prem(round_tables=False)["ulp_frac"])}
    table = {m: (fp32[m], tol, {}) for m, tol in ATTN_TOL.items()}
    for name, (m, dist) in must.items():
        table[m][2][name] = dist[m]
    return table, {m: (large[m], ATTN_TOL_LARGE[m]) for m in large}, in_band


def test_sensitivity_table():
    """every threshold >= 10x the fp32 arithmetic's distance from fp64 (also in the large-|LSE| regime under its own thresholds),
    every mutation marked "must catch" >= 10x its threshold; the in-band mutations are printed with their numbers (ulp_max has no
    mutation of its own: the fraction and row metrics catch the mutations that move elements by more than a few ulps)"""
    table, large, in_band = sensitivity_table()
    for m, (err, tol, muts) in table.items():
        print(f"{m:9s} fp32 {err:.3g}  threshold {tol:.3g}  large |LSE|: fp32 {large[m][0] if m in large else float('nan'):.3g} "
              f"threshold {large[m][1] if m in large else float('nan'):.3g}  " + ", ".join(f"{n}: {v:.3g}" for n, v in muts.items()))
    for n, (m, v) in in_band.items():
        print(f"in band ({m}): {n}: {v:.3g} = {v / ATTN_TOL[m]:.3g}x the threshold")
    for m, (err, tol, muts) in table.items():
        assert 10 * err <= tol, (m, err, tol)
        for name, v in muts.items():
            assert v >= 10 * tol, (m, name, v, tol)
    for m, (err, tol) in large.items():
        assert 10 * err <= tol, ("large |LSE|", m, err, tol)


# ------------------------------------------------------------------------------------------------ emulated bodies
@pytest.mark.parametrize("B,NH,S", [(1, 2, 40), (1, 1, 300), (1, 1, 577)])
def test_emulated_bodies_under_attn_tol(emul, B, NH, S):
    """the revision-2 forward, dq_wide<1> and the shipped dkdv_staged<12, true, 2> (variant 4, two tiles per stage) on the wave
    emulator, [B, NH, S, 64] views of [B, S, NH, 64] memory, against the statements under ATTN_TOL; the backward takes the emulated
    forward's O and LSE"""
    q, k, v, do = (t.bfloat16().transpose(1, 2).contiguous().transpose(1, 2) for t in C.model_case(B, NH, S, 31 + S))
    c64 = lambda t: t.double()
    out, lse = _forward(emul, q, k, v)
    wo, wl = AO.fwd(c64(q), c64(k), c64(v))
    p, (dq, dk, dv), (o, lse32, delta) = _bwd_params(q, k, v, do, out, lse)
    msg = ctypes.create_string_buffer(256)
    assert emul.emul_attn_dq_wide(ctypes.byref(p), 1, msg, 256) == 0, msg.value.decode()
    assert emul.emul_attn_dkdv_n(ctypes.byref(p), 4, 2, msg, 256) == 0, msg.value.decode()
    want = AO.bwd(c64(q), c64(k), c64(v), c64(do), c64(o), c64(lse32))
    want.update({"O": wo, "LSE": wl, "_o": c64(o), "_do": c64(do)})
    got = {"O": out, "LSE": lse, "dq": dq, "dk": dk, "dv": dv, "delta": delta}
    assert not any(torch.isnan(t.float()).any() for t in got.values())
    res = _metrics(got, want)
    print((B, NH, S), {m: f"{x:.3g}" for m, x in res.items()})
    for m, x in res.items():
        assert x <= ATTN_TOL[m], (m, x)
