"""Inputs, comparisons and metrics for the TTT-Linear BACKWARD sweeps (tests/test_scan_bwd_oracle_cpu.py,
tests/test_scan_bwd_oracle_gpu.py), in the pattern of scan_cases.py.

The backward of a scan is a pure function of one call: the checkpoints (the state entering every group), the upstream state
gradient (dW1_last, db1_last) and Q, K, V, eta, dOut map to (dW1, db1, dXQ, dXK, dXV, d eta, dln_w, dln_b), every (b, h) on its
own.  So nothing here follows a trajectory: the checkpoints are the fp64 forward's (held as fp32, what a kernel is given), a call
covers ONE step (NC = G = 1) or one group (a G-step horizon), and the fp64 oracle makes the same step(s) from the same checkpoint
and the same upstream.  A call over K groups is compared with K one-group calls chained through dW1 / db1 (``chain``): for the MFMA
kernels that hand-over is exact, bit for bit.

A ``run`` below is any callable (t, cks, up, G) -> {dW1, db1, dXQ, dXK, dXV, dlast_eta, dln_w, dln_b} over host tensors: t = XQ XK XV
eta dOut (activations) and ln_w ln_b [NH, F] fp32, cks = {W1 [B, NH, K, F, F], b1 [B, NH, K, 1, F]} fp32, up = (dW1_last, db1_last) fp32.
The device's (test_scan_bwd_oracle_gpu.py) and the wave emulators' (``emul_run``) go through the same ``check_*`` functions."""
import ctypes

import torch

import scan_cases as C
from oracle import ttt_oracle as O

F = C.F
FB = 16      # columns of one ``fb`` tile of the lane map (csrc/ttt_lin16_body.h: dWt[fa][fb]; lin64: the slice of one wave)
GRADS = ("dW1", "db1", "dXQ", "dXK", "dXV", "dlast_eta", "dln_w", "dln_b")
EXACT = ("dXQ", "dXK", "dXV", "dlast_eta", "dW1", "db1")      # equal bits between a whole call and the chain of its groups


# ------------------------------------------------------------------------------------------------ cases
# name -> (CS, B, NH, NC, G, seed).  The seeds were picked on the CPU (test_scan_bwd_oracle_cpu.py::test_rounding_model_under_half_of
# _every_threshold): a draw with a near-constant LayerNorm row has an ill-conditioned step and is replaced by another seed, not
# masked - as in scan_cases.py.
ONE_STEP = {"lin16": (16, 2, 5, 1, 1, 51), "lin64": (64, 2, 5, 1, 1, 52)}
HORIZON = {f"lin{CS}_g{G}": (CS, 1, 3, G, G, 60 + CS + G) for CS in (16, 64) for G in (3, 4)}
TWO_STEP = {"lin16": (16, 2, 3, 2, 1, 71), "lin64": (64, 2, 3, 2, 1, 72)}       # the two off-by-one mutations
CHAIN = {16: ((11, 4), (7, 3), (3, 1)), 64: ((7, 3), (4, 2))}                   # (NC, G) at B = 2, NH = 3: ragged, even and odd G
CHAIN_B, CHAIN_NH = 2, 3


def bwd_case(CS, B, NH, NC, G, seed, regime="base", up_scale=1.0):
    """scan_cases.scan_case (bf16-valued activations, a state per (b, h)) plus: dOut bf16-valued randn; ``cks`` the fp64 forward's
    checkpoints held as fp32; ``up`` = (dW1_last, db1_last) drawn independently per (b, h), each (b, h) scaled to ``up_scale`` times
    the norm of the call's own contribution (the oracle's dW1 / db1 with zero upstream), held as fp32 values.  Everything fp64."""
    c = C.scan_case("linear", B, NH, NC, CS, seed, regime)
    g = torch.Generator().manual_seed(seed + 200003)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c["dOut"] = rn(B, NH, NC, CS, F).bfloat16().double()
    c["G"] = G
    c["cks"] = {k: v.double() for k, v in C.oracle_checkpoints(c, G).items()}
    zero = (torch.zeros(B, NH, F, F, dtype=torch.float64), torch.zeros(B, NH, 1, F, dtype=torch.float64))
    own = sweep(c, c["cks"], zero, G)
    up = []
    for x, o in zip((rn(B, NH, F, F), rn(B, NH, 1, F)), (own["dW1"], own["db1"])):
        n = lambda t: t.flatten(2).norm(dim=-1)[:, :, None, None]
        up.append((x * (up_scale * n(o) / n(x))).float().double())
    c["up"] = tuple(up)
    return c


# ------------------------------------------------------------------------------------------------ one step, mutated
# the kernel bugs of the sensitivity table: name -> the metric that must catch it (None: reported only, see helpers.SCAN_BWD_TOL)
MUTATIONS = {
    "no_upstream_W": "row",            # dW1_last left out of the operand copy of dW1n (dgZ1, A1); the accumulator keeps it
    "no_upstream_b": "dstate",         # db1_last left out of db1n where dgZ1 and d eta read it
    "batch0_upstream": "dstate",       # the upstream of batch 0 used for every b
    "batch0_state": "dstate",          # the checkpoint of batch 0 used for every b
    "eta_neighbour": "row",            # eta taken from the neighbouring token
    "dQ_old_W": "row",                 # W1 in place of W1n in dQ
    "dgZ1_no_b": "dstate",             # the eta db1n term of dgZ1 dropped
    "deta_no_b": "deta",               # the gZ1 . db1n term of d eta dropped
    "dln_no_inner": "dln",             # the inner LayerNorm's share of dln_w / dln_b dropped
    "dK_no_dt": "row",                 # the -dt term of dK dropped
    "dK_no_etaA1": "row",              # the -eta A1 term of dK dropped
    "skip_last_token": "dstate",       # the last token left out of the dW1 / db1 update
    "no_inner_dW": "dstate",           # K^T dZ1 dropped from dW1
    "block_1.05": "dstate_block",      # the increment scaled by 1.05 in one 16-column block
    "outer_var_unbiased": "gain",      # unbiased variance in the output LayerNorm
    "dout_next_step": "row",           # dOut of step i + 1: the prefetch off by one (two-step case)
    "q_next_step": "row",              # Q of step i + 1 (two-step case)
    "eps_1e-6": None,                  # LayerNorm epsilon 1e-6 in place of 1e-8
}
TWO_STEP_MUTATIONS = ("dout_next_step", "q_next_step")


def step_bwd_mut(st, Q, K, V, eta, gam, bet, dOut, dst, eps=O.LN_EPS, mut=None, nxt=None):
    """The fp64 backward step with one statement changed (``mut``, a key of MUTATIONS; None: the arithmetic of O._lin_step_bwd).
    ``nxt``: {"Q", "dOut"} of the following step for the two off-by-one mutations."""
    T = lambda x: x.transpose(-1, -2)
    if mut == "batch0_state":
        st = tuple(s[:1].expand_as(s) for s in st)
    elif mut == "batch0_upstream":
        dst = tuple(s[:1].expand_as(s) for s in dst)
    elif mut == "eta_neighbour":
        eta = eta.roll(1, -2)
    elif mut == "eps_1e-6":
        eps = 1e-6
    elif mut == "dout_next_step":
        dOut = nxt["dOut"]
    elif mut == "q_next_step":
        Q = nxt["Q"]
    W1, b1 = st
    (W1n, b1n), _, s = O._lin_step_primal(W1, b1, Q, K, V, eta, gam, bet, eps)
    xhl, stdl = C._ln(Q @ W1n + b1n, eps, mut == "outer_var_unbiased")
    dW1l, db1l = dst
    dgam = (dOut * xhl).sum(-2, keepdim=True)
    dbet = dOut.sum(-2, keepdim=True)
    dZ1b = O._ln_bwd(dOut, xhl, stdl, gam, F)
    incW, incb = T(Q) @ dZ1b, dZ1b.sum(-2, keepdim=True)
    dW1n = incW if mut == "no_upstream_W" else dW1l + incW              # what dgZ1 / A1 / d eta read
    db1n = incb if mut == "no_upstream_b" else db1l + incb
    dQ = dOut + dZ1b @ T(W1 if mut == "dQ_old_W" else W1n)
    A1 = s["gZ1"] @ T(dW1n)
    dgZ1 = -(eta * K) @ dW1n - (0.0 if mut == "dgZ1_no_b" else eta * db1n)
    deta = -(K * A1).sum(-1, keepdim=True) - (0.0 if mut == "deta_no_b" else (s["gZ1"] * db1n).sum(-1, keepdim=True))
    dZ1, dgam2, dbet2, dt = O._ln_l2_bwd_bwd(dgZ1, s["xh"], s["std"], s["go"], s["gxh"], s["gZ1"], gam, F)
    if mut != "dln_no_inner":
        dgam = dgam + dgam2.sum(-2, keepdim=True)
        dbet = dbet + dbet2.sum(-2, keepdim=True)
    dK = dZ1 @ T(W1)
    if mut != "dK_no_dt":
        dK = dK - dt
    if mut != "dK_no_etaA1":
        dK = dK - eta * A1
    dZ1u = dZ1
    if mut == "skip_last_token":
        dZ1u = dZ1.clone()
        dZ1u[..., -1, :] = 0
    if mut != "no_inner_dW":
        incW = incW + T(K) @ dZ1u
    incb = incb + dZ1u.sum(-2, keepdim=True)
    if mut == "block_1.05":           # the columns [16, 32): one fb tile of lin16, the slice of wave 1 of lin64
        incW, incb = incW.clone(), incb.clone()
        incW[..., FB:2 * FB] *= 1.05
        incb[..., FB:2 * FB] *= 1.05
    return (dW1l + incW, db1l + incb), dQ, dK, dt, deta, dgam, dbet


# ------------------------------------------------------------------------------------------------ the oracle's side of a call
def sweep(c, cks, up, G, how=None):
    """The backward of the call (c's steps, checkpoints ``cks``, upstream ``up``, groups of G) -> {GRADS} fp64.  how: None the
    fp64 oracle (O._lin_step_bwd from O._lin_step_primal's states); a frozenset the oracle's rounding model with those points on
    (O.lin_step_bwd_rounded, the group re-run by O.lin_step_rounded as the kernels re-run it); "fp32" / "fp32_bf16out" the oracle's
    step in fp32 arithmetic (dXQ, dXK, dXV, d eta rounded to bf16) - the reference-alone level of the generic kernel -; another
    string the mutation of that name (calls of one step per group only)."""
    B, NH, NC = c["XQ"].shape[:3]
    f32 = how in ("fp32", "fp32_bf16out")
    cast = (lambda t: t.float()) if f32 else (lambda t: t)
    gam, bet = cast(c["ln_w"].reshape(1, NH, 1, F)), cast(c["ln_b"].reshape(1, NH, 1, F))
    X = {k: cast(c[k]) for k in ("XQ", "XK", "XV", "eta", "dOut")}
    model = isinstance(how, (set, frozenset))
    mutation = isinstance(how, str) and not f32
    assert not mutation or G == 1 or NC == 1
    dst = tuple(cast(u) for u in up)
    res = {k: [None] * NC for k in ("dXQ", "dXK", "dXV", "dlast_eta")}
    dgam = dbet = 0.0
    for k in reversed(range(cks["W1"].shape[2])):
        lo, hi = k * G, min((k + 1) * G, NC)
        st = (cast(cks["W1"][:, :, k]), cast(cks["b1"][:, :, k]))
        states = []
        for i in range(lo, hi):
            states.append(st)
            a = (X["XQ"][:, :, i], X["XK"][:, :, i], X["XV"][:, :, i], X["eta"][:, :, i], gam, bet)
            st = O.lin_step_rounded(*st, *a, on=frozenset(how) & {"W", "Gs"})[0] if model else O._lin_step_primal(*st, *a, O.LN_EPS)[0]
        for i in reversed(range(lo, hi)):
            a = (X["XQ"][:, :, i], X["XK"][:, :, i], X["XV"][:, :, i], X["eta"][:, :, i], gam, bet)
            d = X["dOut"][:, :, i]
            if model:
                r = O.lin_step_bwd_rounded(states[i - lo], *a, d, dst, on=frozenset(how))
            elif mutation:
                j = i + 1 if i + 1 < NC else max(i - 1, 0)      # "the following step" of the last one: the one before it
                r = step_bwd_mut(states[i - lo], *a, d, dst, mut=how, nxt={"Q": X["XQ"][:, :, j], "dOut": X["dOut"][:, :, j]})
            else:
                r = O._lin_step_bwd(states[i - lo], *a, O.LN_EPS, d, dst)
            dst = r[0]
            res["dXQ"][i], res["dXK"][i], res["dXV"][i], res["dlast_eta"][i] = r[1:5]
            dgam, dbet = dgam + r[5], dbet + r[6]
    out = {k: torch.stack(v, 2) for k, v in res.items()}
    if how == "fp32_bf16out" or mutation:         # as a kernel with bf16 activations would store them
        out = {k: v.bfloat16() for k, v in out.items()}
    out.update(dW1=dst[0], db1=dst[1], dln_w=dgam, dln_b=dbet)
    return {k: v.double() for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ metrics
METRICS = ("dstate", "dstate_block", "row", "deta", "dln", "gain")


def _rel(diff, ref):
    return float((diff.norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)).max())


def _col_blocks(x):
    """[B, NH, R, 64] -> [B, NH, 4, R * 16]: the 16-column blocks"""
    B, NH, R, _ = x.shape
    return x.reshape(B, NH, R, F // FB, FB).permute(0, 1, 3, 2, 4).reshape(B, NH, F // FB, R * FB)


def metrics(c, got, ref, up, bf16_rows=True):
    """The metrics of SCAN_BWD_TOL, each the worst over everything compared (no (b, h), step or row is left out):
    dstate        rel-L2 per (b, h) of the increments dW1 - dW1_last and db1 - db1_last (formed in fp64), the worse of the two
    dstate_block  the same of one 16-column block of the increment: one fb tile of the lane map
    row           rel-L2 of one (b, h, step, token) row of dXQ, dXK, dXV against the oracle's (bf16-rounded where the kernel's is bf16)
    deta          rel-L2 per (b, h, step) over the CS values of d eta
    dln           rel-L2 per (b, h) of dln_w and of dln_b
    gain          per (b, h, step): <A, A_ref> / <A_ref, A_ref> - 1 with A = dXQ - dOut, the part that went through the output
                  LayerNorm's backward: a wrong variance convention or epsilon there is a pure scale, rounding averages out"""
    g = {k: got[k].detach().double().cpu() for k in GRADS}
    m = {"dstate": 0.0, "dstate_block": 0.0, "row": 0.0, "dln": 0.0}
    for name, u in zip(("dW1", "db1"), up):
        a, b = g[name].reshape(u.shape) - u, ref[name] - u
        m["dstate"] = max(m["dstate"], _rel((a - b).flatten(2), b.flatten(2)))
        m["dstate_block"] = max(m["dstate_block"], _rel(_col_blocks(a - b), _col_blocks(b)))
    for name in ("dXQ", "dXK", "dXV"):
        b = ref[name].bfloat16().double() if bf16_rows else ref[name]
        m["row"] = max(m["row"], _rel(g[name] - b, b))
    m["deta"] = _rel((g["dlast_eta"] - ref["dlast_eta"]).flatten(3), ref["dlast_eta"].flatten(3))
    for name in ("dln_w", "dln_b"):
        b = ref[name]
        m["dln"] = max(m["dln"], _rel(g[name].reshape(b.shape) - b, b))
    A, Ar = (g["dXQ"] - c["dOut"]).flatten(3), (ref["dXQ"] - c["dOut"]).flatten(3)
    m["gain"] = float(((A * Ar).sum(-1) / (Ar * Ar).sum(-1) - 1.0).abs().max())
    return m


def fmt(m):
    return "  ".join(f"{k} {m[k]:.3g}" for k in METRICS)


def compare(c, got, how=None):
    """metrics of a call's results against ``how`` (see sweep) from the call's own checkpoints and upstream"""
    return metrics(c, got, sweep(c, c["cks"], c["up"], c["G"], how), c["up"], bf16_rows=got["dXQ"].dtype == torch.bfloat16)


# ------------------------------------------------------------------------------------------------ running a case
def host_tensors(c, act=torch.bfloat16):
    """what a kernel is given: (t, cks, up) of host tensors"""
    t = {k: c[k].to(act).contiguous() for k in ("XQ", "XK", "XV", "eta", "dOut")}
    t.update({k: c[k].float().contiguous() for k in ("ln_w", "ln_b")})
    return t, {k: v.float().contiguous() for k, v in c["cks"].items()}, tuple(u.float().contiguous() for u in c["up"])


def check_call(tag, run, c, tol, act=torch.bfloat16):
    """one call of the case (one step, or one group: a G-step horizon) against the fp64 oracle at ``tol`` -> (results, metrics)"""
    t, cks, up = host_tensors(c, act)
    got = run(t, cks, up, c["G"])
    assert not any(torch.isnan(got[k].float()).any() for k in GRADS), tag
    m = compare(c, got)
    print(f"{tag}: {fmt(m)}")
    bad = {k: (v, tol[k]) for k, v in m.items() if not v < tol[k]}
    assert not bad, (tag, bad)
    return got, m


def check_mutations(tag, c, got, tol, names):
    """each must-catch mutation written into the ORACLE side of the comparison with the results ``got``: the metric named for it
    fails (the comparison can fail, on the kernel's own results)"""
    for mut in names:
        metric = MUTATIONS[mut]
        if metric is None:
            continue
        m = compare(c, got, how=mut)
        print(f"{tag} {mut:20s} {metric}: {m[metric]:.3g} (threshold {tol[metric]:.3g})")
        assert m[metric] > tol[metric], (tag, mut, m)


def chain(run, t, cks, up, NC, G):
    """K one-group calls in place of the call over K groups, from the last group to the first: each is given its group's steps and
    checkpoint slice and the dW1 / db1 of the call before it as its upstream -> the results of the whole in the whole's shapes, dln_w /
    dln_b the sum (fp32, in call order) of the calls' partials"""
    K = -(-NC // G)
    parts, dln = {k: [None] * K for k in ("dXQ", "dXK", "dXV", "dlast_eta")}, None
    for k in reversed(range(K)):
        lo, hi = k * G, min((k + 1) * G, NC)
        tk = {n: (v[:, :, lo:hi].contiguous() if n in ("XQ", "XK", "XV", "eta", "dOut") else v) for n, v in t.items()}
        g = run(tk, {n: v[:, :, k:k + 1].contiguous() for n, v in cks.items()}, up, G)
        up = (g["dW1"].clone(), g["db1"].clone())
        for n in parts:
            parts[n][k] = g[n]
        dln = (g["dln_w"].clone(), g["dln_b"].clone()) if dln is None else (dln[0] + g["dln_w"], dln[1] + g["dln_b"])
    out = {n: torch.cat(v, 2) for n, v in parts.items()}
    out.update(dW1=up[0], db1=up[1], dln_w=dln[0], dln_b=dln[1])
    return out


def check_chain(tag, run, c, tol, dln_tol, exact=True, act=torch.bfloat16):
    """the whole call of the case against the chain of its one-group calls: with ``exact`` (the MFMA kernels) dXQ, dXK, dXV, d eta,
    dW1, db1 have equal bits and dln_w / dln_b agree with the sum of the partials within ``dln_tol`` (an fp32 add order); without,
    every metric of the whole against the chain is under ``tol`` and whether the bits are equal is printed"""
    t, cks, up = host_tensors(c, act)
    NC, G = c["XQ"].shape[2], c["G"]
    whole = run(t, cks, up, G)
    parts = chain(run, t, cks, up, NC, G)
    assert not any(torch.isnan(whole[k].float()).any() for k in GRADS), tag
    same = {k: torch.equal(whole[k], parts[k]) for k in EXACT}
    m = metrics(c, whole, {k: parts[k].double().reshape(whole[k].shape) for k in GRADS}, c["up"], bf16_rows=False)
    print(f"{tag}: whole call vs chain of {-(-NC // G)} one-group calls: {fmt(m)}  equal bits: {same}")
    if exact:
        assert all(same.values()), (tag, same)
        assert m["dln"] < dln_tol, (tag, m["dln"], dln_tol)
    else:
        bad = {k: (v, tol[k]) for k, v in m.items() if not v < tol[k]}
        assert not bad, (tag, bad)
    return m


# ------------------------------------------------------------------------------------------------ the wave emulators
def emul_run(lib, CS):
    """``run`` over tests/emul/lin16_emul.cpp (CS 16) / lin64_emul.cpp (CS 64): the kernel bodies themselves on the CPU; outputs
    start as NaN, the scratch of the tensor contract lies between NaN guards"""
    from test_emul_cpu import Params
    name = "lin16" if CS == 16 else "lin64"
    assert getattr(lib, f"emul_{name}_params_size")() == ctypes.sizeof(Params)

    def run(t, cks, up, G):
        B, NH, NC = t["XQ"].shape[:3]
        K = cks["W1"].shape[2]
        assert K == -(-NC // G) and t["XQ"].dtype == torch.bfloat16
        nan = lambda *s, dt=torch.float32: torch.full(s, float("nan"), dtype=dt)
        bf = torch.bfloat16
        g = dict(dln_w=nan(B, NH, 1, F), dln_b=nan(B, NH, 1, F), dW1=nan(B, NH, F, F), db1=nan(B, NH, 1, F),
                 dlast_eta=nan(B, NH, NC, CS, 1, dt=bf), dXQ=nan(B, NH, NC, CS, F, dt=bf), dXK=nan(B, NH, NC, CS, F, dt=bf),
                 dXV=nan(B, NH, NC, CS, F, dt=bf))
        guard = 64
        scr_w, scr_b = nan(B * NH * G * F * F + 2 * guard), nan(B * NH * G * F + 2 * guard)
        ins = dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1c=cks["W1"], b1c=cks["b1"],
                   dOut=t["dOut"], dW1_last=up[0], db1_last=up[1])
        keep = {k: v.clone() for k, v in ins.items()}
        p = Params()
        for n, v in dict(ins, scratch_w=scr_w[guard:], scratch_b=scr_b[guard:], dln_w=g["dln_w"], dln_b=g["dln_b"], dW1=g["dW1"],
                         db1=g["db1"], deta=g["dlast_eta"], dXQ=g["dXQ"], dXK=g["dXK"], dXV=g["dXV"]).items():
            assert v.is_contiguous()
            setattr(p, n, v.data_ptr())
        p.NH, p.NC, p.G, p.K, p.eps = NH, NC, G, K, 1e-8
        if CS == 16:
            lib.emul_lin16_backward(ctypes.byref(p), B * NH)
        else:
            msg = ctypes.create_string_buffer(256)
            assert lib.emul_lin64_backward(ctypes.byref(p), B * NH, msg, 256) == 0, f"LDS race: {msg.value.decode()}"
        for s in (scr_w, scr_b):
            assert torch.isnan(s[:guard]).all() and torch.isnan(s[-guard:]).all(), "write outside the documented scratch"
        for k, v in ins.items():
            assert torch.equal(v, keep[k]), f"input {k} was written"
        return g
    return run
