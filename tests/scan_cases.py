"""Inputs, the one-step comparison and its metrics for the forward TTT scans (tests/test_scan_oracle_cpu.py,
tests/test_scan_oracle_gpu.py), in the pattern of attn_cases.py / glue_cases.py.

A scan is a dynamical system, so a tolerance on a whole trajectory is a drift allowance and says little about one step.  Here
every comparison starts from the KERNEL'S OWN state: with G = 1 the fp32 checkpoints hold the state entering every step, the
fp64 oracle makes ONE step from each of them (a G-step horizon from each stored checkpoint for G > 1), and what is compared is
the state DELTA ck[k + 1] - ck[k] and the step's output.  No error is carried from step to step."""
import math
import os
import subprocess

import torch

from helpers import bf16_ulp
from oracle import ttt_oracle as O

F, H = 64, 256
STATE = {"mlp": ("W1", "b1", "W2", "b2"), "linear": ("W1", "b1")}
# regimes of the learning rate (make_inputs' base_lr): "base" = the op-level inputs every other scan test uses, a step moves
# W1 / W2 of the TTT-MLP by 2e-3 .. 5e-3 of their norm; "high" = a step moves W2 (TTT-Linear: W1) by 2 .. 4 percent and the first
# step, from the near-constant rows of the initial Z2, by a quarter and more, so that the update matters to the step's output
BASE_LR = {("mlp", "base"): 0.1, ("mlp", "high"): 4.0, ("linear", "base"): 1.0, ("linear", "high"): 8.0}
WAVE = 32    # the slice of the hidden units / the features one wave of ttt_mfma2.hip owns (wave (w, p): Hp, Fp)


def scan_case(kind, B, NH, NC, CS, seed, regime="base"):
    """bf16-valued XQ / XK / XV [B, NH, NC, CS, F] and eta [B, NH, NC, CS, 1] (the last row of make_inputs' tile), ln_w / ln_b
    [NH, F] drawn per head, and an initial state drawn independently for every batch element ([B, NH, ...]): a kernel that
    indexes the state by head only cannot pass.  Everything fp64 holding the values the kernels are given."""
    d = O.make_inputs(kind, B, NH, NC, CS, F, seed=seed, dtype=torch.float64, base_lr=BASE_LR[kind, regime])
    bf = lambda t: t.to(torch.bfloat16).double()
    c = {"XQ": bf(d["XQ"]), "XK": bf(d["XK"]), "XV": bf(d["XV"]), "eta": bf(d["eta"][:, :, :, -1, :, None]).contiguous(),
         "ln_w": d["ln_w"].float().double(), "ln_b": d["ln_b"].float().double(), "kind": kind}
    g = torch.Generator().manual_seed(seed + 100003)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    hid = H if kind == "mlp" else F
    st = {"W1": 0.02 * rn(B, NH, F, hid), "b1": 0.01 * rn(B, NH, 1, hid)}
    if kind == "mlp":
        st.update(W2=0.02 * rn(B, NH, hid, F), b2=0.01 * rn(B, NH, 1, F))
    c.update({k: v.float().double() for k, v in st.items()})
    return c


# The cases of tests/test_scan_oracle_gpu.py: name -> (kind, CS, B, NH, NC, G, seed).  For TTT-Linear nothing hands back the state
# after the last step, so with G = 1 the scan runs one step more than NC (``run_steps``) and NC steps have their delta.  The seeds were picked on the CPU (test_scan_oracle_cpu.py::test_rounding_model_under_half_of_every
# _threshold): a draw with a near-constant inner-LayerNorm row has an ill-conditioned step and is replaced, not masked.
MFMA_CASES = {
    "mlp64_b2": ("mlp", 64, 2, 5, 9, 1, 7),          # the batched pair of the sampler, 10 workgroups
    "mlp64_ragged": ("mlp", 64, 1, 3, 7, 3, 8),      # G = 3: horizons of 3, 3, 1 steps, ragged last group
    "mlp64_9heads": ("mlp", 64, 1, 9, 5, 1, 9),      # pair form: the role-B workgroups start past block 8
    "mlp16_b2": ("mlp", 16, 2, 5, 20, 1, 10),
    "mlp16_ragged": ("mlp", 16, 1, 3, 11, 4, 11),
    "lin16_b2": ("linear", 16, 2, 5, 20, 1, 12),
    "lin16_ragged": ("linear", 16, 1, 3, 11, 4, 13),
    "lin64_b2": ("linear", 64, 2, 3, 7, 1, 14),
}
GENERIC_CASES = {f"{kind}{CS}": (kind, CS, 2, 3, 5, 1, 20 + CS + (kind == "mlp")) for kind in ("mlp", "linear") for CS in (64, 16)}
PART_CUTS = (1, 2, 7)       # cuts of the runs in parts: a part of one step, none at a multiple of a group size used with them


def run_steps(kind, NC, G):
    """steps the scan runs so that NC of them have an observed delta"""
    return NC + 1 if G == 1 and kind == "linear" else NC


def oracle_checkpoints(c, G):
    """{name: fp32 [B, NH, K, ...]} checkpoints of the fp64 oracle's scan of the case: states on a trajectory, for the comparisons
    that need no kernel (the rounding model and the mutations, each stepped from them)"""
    kind = c["kind"]
    f = O.mlp_forward if kind == "mlp" else O.linear_forward
    _, cks, _ = f(c["XQ"], c["XK"], c["XV"], c["eta"], c["ln_w"], c["ln_b"], *[c[k] for k in STATE[kind]], G)
    return {k: v.float() for k, v in zip(STATE[kind], cks)}


# ------------------------------------------------------------------------------------------------ one step, exact / mutated
def _erf_gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _erf_gelu_bwd(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _ln(x, eps, unbiased=False):
    mu = x.mean(-1, keepdim=True)
    std = torch.sqrt(x.var(-1, keepdim=True, unbiased=unbiased) + eps)
    return (x - mu) / std, std


# the kernel bugs of the sensitivity table: name -> the metric that must catch it (None: reported only)
MUTATIONS = {
    "out_var_unbiased": "gain",       # unbiased variance in the output LayerNorm
    "inner_var_unbiased": "delta",    # ... in the inner (fused L2-backward) LayerNorm
    "no_b1": "delta",                 # the b1 update dropped
    "no_b2": "delta",                 # the b2 update dropped (TTT-MLP only)
    "eta_neighbour": "delta",         # eta taken from the neighbouring token
    "eta_next_step": "delta",         # eta taken from step i + 1: the prefetch off by one
    "batch0_state": "delta",          # the state of batch 0 used for every b
    "block_1.05": "delta_block",      # the update scaled by 1.05 in one 32-wide block of the hidden units
    "skip_last_token": "delta",       # the last token of the mini-batch left out of the update
    "q_next_step": "row",             # Q of step i + 1 in the output path
    "erf_gelu": None,                 # erf GELU in place of tanh GELU
    "eps_1e-6": None,                 # LayerNorm epsilon 1e-6 in place of 1e-8
}


def step_mut(kind, st, Q, K, V, eta, gam, bet, eps=O.LN_EPS, mut=None, nxt=None):
    """One primal step in fp64 with one statement changed (``mut``, a key of MUTATIONS; None: the step itself, the arithmetic
    of O._mlp_step_primal / O._lin_step_primal).  ``nxt``: {"Q", "eta"} of the following step for the two off-by-one mutations."""
    mlp = kind == "mlp"
    T = lambda x: x.transpose(-1, -2)
    if mut == "eta_neighbour":
        eta = eta.roll(1, -2)
    elif mut == "eta_next_step":
        eta = nxt["eta"]
    elif mut == "skip_last_token":
        eta = eta.clone()
        eta[..., -1, :] = 0
    elif mut == "eps_1e-6":
        eps = 1e-6
    elif mut == "batch0_state":
        st = tuple(s[:1].expand_as(s) for s in st)
    gelu, dgelu = (_erf_gelu, _erf_gelu_bwd) if mut == "erf_gelu" else (O.gelu_tanh, O.gelu_bwd)
    W1, b1 = st[:2]
    Z1 = K @ W1 + b1
    if mlp:
        W2, b2 = st[2:]
        X2 = gelu(Z1)
        Z = X2 @ W2 + b2
    else:
        Z = Z1
    xh, std = _ln(Z, eps, mut == "inner_var_unbiased")
    gxh = (gam * xh + bet - (V - K)) * gam
    gZ = (F * gxh - gxh.sum(-1, keepdim=True) - xh * (gxh * xh).sum(-1, keepdim=True)) / (F * std)
    gZ1 = (gZ @ T(W2)) * dgelu(Z1) if mlp else gZ
    d = [-T(eta * K) @ gZ1, -(eta * gZ1).sum(-2, keepdim=True)]
    if mlp:
        d += [-T(eta * X2) @ gZ, -(eta * gZ).sum(-2, keepdim=True)]
    if mut == "no_b1":
        d[1] = torch.zeros_like(d[1])
    elif mut == "no_b2" and mlp:
        d[3] = torch.zeros_like(d[3])
    elif mut == "block_1.05":       # hidden units [32, 64) (TTT-Linear: the output features [32, 64) of W1 / b1)
        d = [x.clone() for x in d]
        d[0][..., WAVE:2 * WAVE] *= 1.05
        d[1][..., WAVE:2 * WAVE] *= 1.05
        if mlp:
            d[2][..., WAVE:2 * WAVE, :] *= 1.05
    new = tuple(s + x for s, x in zip(st, d))
    Qo = nxt["Q"] if mut == "q_next_step" else Q
    Zb = Qo @ new[0] + new[1]
    if mlp:
        Zb = gelu(Zb) @ new[2] + new[3]
    xhl, _ = _ln(Zb, eps, mut == "out_var_unbiased")
    return new, Qo + gam * xhl + bet


def make_step(kind, how=None):
    """step(st, Q, K, V, eta, gam, bet, nxt) -> (state, out): how = None the fp64 primal step of the oracle, a frozenset the
    oracle's rounding model with those points on, "fp32" / "fp32_bf16out" the primal step in fp32 arithmetic (with the output
    rounded to bf16) - the reference-alone level of the generic kernels -, another string the mutation of that name"""
    if how in ("fp32", "fp32_bf16out"):
        f = O._mlp_step_primal if kind == "mlp" else O._lin_step_primal

        def step32(st, Q, K, V, eta, gam, bet, nxt):
            new, out = f(*[t.float() for t in st + (Q, K, V, eta, gam, bet)], O.LN_EPS)[:2]
            return tuple(t.double() for t in new), (out.bfloat16() if how == "fp32_bf16out" else out).double()
        return step32
    if how is None or isinstance(how, (set, frozenset)):
        f = O.mlp_step_rounded if kind == "mlp" else O.lin_step_rounded
        on = frozenset() if how is None else how
        return lambda st, Q, K, V, eta, gam, bet, nxt: f(*st, Q, K, V, eta, gam, bet, O.LN_EPS, on=on)
    return lambda st, Q, K, V, eta, gam, bet, nxt: step_mut(kind, st, Q, K, V, eta, gam, bet, mut=how, nxt=nxt)


# ------------------------------------------------------------------------------------------------ the comparison
def horizons(c, cks, G, how=None, nsteps=None):
    """From every stored checkpoint cks[name][:, :, k] (fp64 values of the scan's own fp32 checkpoints: the state entering step
    k G) the steps of group k with ``make_step(kind, how)``: -> (out [B, NH, n, CS, F], {name: [B, NH, K, ...] state after the
    last step of each group}).  ``nsteps`` (default: all) limits the steps that are looked at."""
    kind = c["kind"]
    step = make_step(kind, how)
    B, NH, NC = c["XQ"].shape[:3]
    n = NC if nsteps is None else nsteps
    gam, bet = c["ln_w"].reshape(1, NH, 1, F), c["ln_b"].reshape(1, NH, 1, F)
    outs, ends = [], {k: [] for k in STATE[kind]}
    for k in range(-(-n // G)):
        st = tuple(cks[name][:, :, k] for name in STATE[kind])
        for i in range(k * G, min((k + 1) * G, n)):
            j = i + 1 if i + 1 < NC else max(i - 1, 0)      # "the following step" of the last one: the one before it
            nxt = {"Q": c["XQ"][:, :, j], "eta": c["eta"][:, :, j]}
            st, o = step(st, c["XQ"][:, :, i], c["XK"][:, :, i], c["XV"][:, :, i], c["eta"][:, :, i], gam, bet, nxt)
            outs.append(o)
        for name, s in zip(STATE[kind], st):
            ends[name].append(s)
    return torch.stack(outs, 2), {k: torch.stack(v, 2) for k, v in ends.items()}


def deltas(kind, cks, ends, final=None):
    """{name: [B, NH, M, ...]} state deltas over the groups whose end is observed: ``ends[name][:, :, k] - cks[name][:, :, k]``
    for an oracle's group ends (every group), or - ``ends`` None - the scan's own ``cks[k + 1] - cks[k]`` plus, with the state
    after the last step given (``final``), that of the last group.  Formed in fp64 from the fp32 values: fp32 spacing at 0.02 is
    2e-9 against delta elements of ~1e-4."""
    out = {}
    for i, name in enumerate(STATE[kind]):
        ck = cks[name].double()
        if ends is not None:
            out[name] = ends[name].double() - ck[:, :, :ends[name].shape[2]]
        else:
            nxt = ck[:, :, 1:] if final is None else torch.cat((ck[:, :, 1:], final[i].double().unsqueeze(2)), 2)
            out[name] = nxt - ck[:, :, :nxt.shape[2]]
    return out


def _blocks(x):
    """[B, NH, M, R, C] -> [B, NH, M, blocks, elements]: the last dim in blocks of WAVE, the rows too where they are the hidden
    units (R = 256)"""
    B, NH, M, R, C = x.shape
    rb = R // WAVE if R == H else 1
    x = x.reshape(B, NH, M, rb, R // rb, C // WAVE, WAVE).permute(0, 1, 2, 3, 5, 4, 6)
    return x.reshape(B, NH, M, rb * (C // WAVE), -1)


def _rel(diff, ref):
    r = ref.norm(dim=-1)
    return float((diff.norm(dim=-1) / r.clamp_min(1e-300)).max())


METRICS = ("delta", "delta_block", "row", "ulp_frac", "ulp_max", "gain")


def metrics(c, got_out, got_delta, ref_out, ref_delta, round_ref=True):
    """The one-step metrics of SCAN_TOL, each the worst over everything compared (no step, head or row is left out):
    delta        rel-L2 of one (b, h, group) state delta, the worst of W1, b1, W2, b2
    delta_block  the same of one WAVE-wide block of it (W1 columns, b1, W2 rows x W2 columns, b2): a fault confined to one wave
                 of the kernel is not averaged over the other seven
    row          rel-L2 of one (b, h, step, token) row of the output against the oracle's (bf16-rounded where the scan's is bf16)
    ulp_frac, ulp_max   helpers.ulp_stats of the output (bf16 ulps, floor 1/8 of the RMS)
    gain         per (b, h, step): <A, A_ref> / <A_ref, A_ref> - 1 of the LayerNorm part A = out - Q - ln_b; rounding noise
                 averages out of it, a wrong variance convention, epsilon or gamma is a pure scale
    ``got_delta`` may cover fewer groups than ``ref_delta`` (the last one unobserved)."""
    m = {"delta": 0.0, "delta_block": 0.0}
    for name, gd in got_delta.items():
        M = min(gd.shape[2], ref_delta[name].shape[2])
        if M == 0:
            continue
        gd, rd = gd[:, :, :M], ref_delta[name][:, :, :M]
        m["delta"] = max(m["delta"], _rel((gd - rd).flatten(3), rd.flatten(3)))
        m["delta_block"] = max(m["delta_block"], _rel(_blocks(gd - rd), _blocks(rd)))
    n = got_out.shape[2]
    a, b = got_out.double(), ref_out.double()[:, :, :n]
    br = b.bfloat16().double() if round_ref else b
    m["row"] = _rel(a - br, br)
    u = bf16_ulp(b.abs().clamp_min(0.125 * float(b.square().mean().sqrt())))
    dist = (a - b).abs() / u
    m["ulp_frac"], m["ulp_max"] = float((dist > 1.0).double().mean()), float(dist.max())
    NH = a.shape[1]
    base = c["XQ"][:, :, :n] + c["ln_b"].reshape(1, NH, 1, 1, F)
    A, Ar = (a - base).flatten(3), (b - base).flatten(3)
    m["gain"] = float(((A * Ar).sum(-1) / (Ar * Ar).sum(-1) - 1.0).abs().max())
    return m


def compare(c, out, cks, G, final=None, how=None, round_ref=True):
    """metrics of a scan's results (out [B, NH, n, CS, F]; cks {name: [B, NH, K, ...]} fp32; final: the state after step n - 1 or
    None) against ``how`` (see make_step) stepped from the scan's own checkpoints"""
    n = out.shape[2]
    cks64 = {k: v.double() for k, v in cks.items()}
    ref_out, ends = horizons(c, cks64, G, how, n)
    return metrics(c, out, deltas(c["kind"], cks64, None, final), ref_out, deltas(c["kind"], cks64, ends), round_ref)


def assert_initial_state(c, cks):
    """checkpoint 0 is the initial state of ITS batch element and head, bit for bit (the one-step comparison starts from the
    scan's own checkpoints, so a scan that loaded the state of another (b, h) would otherwise be consistent with itself)"""
    for name in STATE[c["kind"]]:
        assert torch.equal(cks[name][:, :, 0].double().cpu(), c[name]), f"checkpoint 0 of {name} is not the initial state"


def fmt(m):
    return "  ".join(f"{k} {m[k]:.3g}" for k in METRICS)


# ------------------------------------------------------------------------------------------------ the wave emulator
CLANG = "/opt/rocm/lib/llvm/bin/amdclang++"


def build_emul(name):
    """tests/emul/<name>.cpp as a shared library on the host compiler of the ROCm toolchain (as tests/test_emul_cpu.py builds
    it; rebuilt when a source is newer) -> path, or None without that compiler"""
    here = os.path.dirname(os.path.abspath(__file__))
    csrc = os.path.join(os.path.dirname(here), "ttt-video-dit_amd", "csrc")
    if not os.path.exists(CLANG):
        return None
    build = os.path.join(here, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, f"lib{name}.so")
    srcs = [os.path.join(here, "emul", f) for f in (name + ".cpp", "wave_emul.h")] + \
           [os.path.join(csrc, f) for f in ("ttt_lin16_body.h", "ttt_lin64_body.h", "ttt_mlp16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", csrc, "-I", os.path.join(here, "emul"), srcs[0], "-o", so])
    return so
