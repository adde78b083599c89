"""Glue kernels of csrc/ttt_prepost.hip (pre / post / gate / AdaLN / residual gate), called through the C ABI (-m gpu), against the
fp64 oracle (oracle/glue_oracle.py) on the same bf16 inputs, at the geometries the training run uses: 48 heads, the 18 048-token
3 s segment (the pre kernel's grid-stride second pass), every P = pre_backward_partials(NH) of the head counts in use, every token
team width of the LayerNorm-over-D backward kernels.  Metrics (tests/helpers.py): fraction of bf16 outputs more than 1 ulp off and
the largest ulp distance, the worst row, and the parameter-gradient sums from the kernels' partials.  Every tolerance is
GLUE_TOL, fixed by the sensitivity table of tests/test_glue_oracle_cpu.py: >= 10x the oracle's own fp32 error, >= 10x below the
nearest mutation (biased std, sign of sin, pos off by one text token, no RoPE on the last video token, src and inverse swapped,
eps outside the sqrt, the text gate on token n_text)."""
import pytest
import torch

import glue_cases as C
from helpers import GLUE_TOL as T, glue_maps, rel_l2, row_rel_err, scene_meta, ulp_stats

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
# 3 s at 5B: 498 text tokens + 13 latent frames of 30 x 45 = 18 048 tokens
META_3S = (498, 1, 13, 30, 45)
# three scenes, 4 434 tokens (scene 0 owns the remainder frame)
META_3SC = (48, 3, 13, 15, 22)


def ext():
    import test_time_training as e
    e.load_library()
    return e


def dev(t):
    return None if t is None else t.to(DEV)


def nanbuf(*shape, dtype=BF):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def check(tag, got, want, rows, psum=()):
    """assert the glue metrics of ``got`` (kernel, bf16 / fp32 sums) against ``want`` (fp64 oracle); prints the measured values"""
    res = {}
    for k, rd in rows.items():
        a = got[k].detach().cpu()
        assert not torch.isnan(a.float()).any(), (tag, k)
        frac, mx = ulp_stats(a, want[k])
        row = row_rel_err(a, want[k].bfloat16(), rd)
        res[k] = (frac, mx, row)
        assert frac <= T["ulp_frac"] and mx <= T["ulp_max"], (tag, k, frac, mx)   # 1e-3 / 64: fp32 4.7e-6 / 4, biased std 0.44
        assert row <= T["row"], (tag, k, row)                                      # 2e-2: fp32 1.5e-3, nearest mutation 0.41
    for k in psum:
        e = rel_l2(got[k], want[k])
        res[k] = e
        assert e <= T["psum"], (tag, k, e)                                         # 1e-4: fp32 2.6e-6, nearest mutation 7.9e-3
    print("GLUE", tag, {k: (tuple(f"{x:.3g}" for x in v) if isinstance(v, tuple) else f"{v:.3g}") for k, v in res.items()})


# ------------------------------------------------------------------------------------------------ pre
def run_pre(e, d, rope, src, pos, NH, ld3=False):
    """pre_forward + pre_backward on NaN-filled outputs; parameter gradients summed (fp64) from the partials"""
    B, L, D = d["q"].shape
    q, k, v = (dev(d[n]) for n in ("q", "k", "v"))
    w, b = dev(d["ln_w"]), dev(d["ln_b"])
    rope, src, pos = dev(rope), dev(src), dev(pos)
    outs = [nanbuf(B, NH, L, 64) for _ in range(3)]
    e.pre_forward(q, k, v, rope, src, pos, w, b, *outs, NH)
    P = e.pre_backward_partials(NH)
    pw, pb = nanbuf(P, D, dtype=torch.float32), nanbuf(P, D, dtype=torch.float32)
    if ld3:
        buf = nanbuf(B, L, 3 * D)
        raw = [buf[..., i * D:(i + 1) * D] for i in range(3)]
    else:
        raw = [nanbuf(B, L, D) for _ in range(3)]
    e.pre_backward(q, k, v, rope, src, pos, w, *(dev(d[n]) for n in ("dXQ", "dXK", "dXV")), *raw, pw, pb, NH,
                   ld_out=3 * D if ld3 else None)
    torch.cuda.synchronize()
    r = dict(zip(("XQ", "XK", "XV"), (o.cpu() for o in outs)))
    r.update(zip(("dq", "dk", "dv"), (t.cpu() for t in raw)))
    r["dln_w"], r["dln_b"] = (p.double().sum(0).view(NH, 64).cpu() for p in (pw, pb))
    if ld3:
        r["buf"] = buf.cpu()
    return r


def heads_of(r, hs, NH):
    """the kernel results restricted to heads hs (outputs [B, NH, L, 64], raw gradients [B, L, NH*64], sums [NH, 64])"""
    cols = torch.cat([torch.arange(h * 64, (h + 1) * 64) for h in hs])
    out = {k: r[k][:, hs] for k in ("XQ", "XK", "XV")}
    out.update({k: r[k].index_select(2, cols) for k in ("dq", "dk", "dv")})
    out.update({k: r[k][hs] for k in ("dln_w", "dln_b")})
    return out


PRE_ROWS = {"XQ": (0, 1, 2), "XK": (0, 1, 2), "XV": (0, 1, 2), "dq": (0, 1), "dk": (0, 1), "dv": (0, 1)}


def _head_subset(NH):
    return sorted({0, NH // 2, NH - 1})


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("NH", [1, 3, 8, 24, 48])
def test_pre_vs_oracle_heads_and_partials(NH, B):
    """P = pre_backward_partials(NH) for the debug model (8), a tp = 2 shard of 5B (24) and 5B (48), one head, and an odd head count
    (3: its thread period of 24 does not divide 2 048 x 256 threads, the persistent grid steps down); 3 scenes, B = 2 time-reversed"""
    e = ext()
    L, src, pos, rope = glue_maps(scene_meta(*META_3SC), reverse=B == 2)
    d = C.pre_case(B, L, NH, seed=NH + B)
    got = run_pre(e, d, rope, src, pos, NH)
    hs = _head_subset(NH)
    want = C.pre_oracle(d, rope, src, pos, NH, heads=hs)
    check(f"pre NH={NH} B={B} P={e.pre_backward_partials(NH)}", heads_of(got, hs, NH), want, PRE_ROWS, psum=("dln_w", "dln_b"))


@pytest.mark.parametrize("maps", ["3scene", "no_src", "no_pos", "1scene_text_rev"])
def test_pre_vs_oracle_token_maps(maps):
    e = ext()
    NH, B = 8, 2
    meta = scene_meta(*((32, 1, 10, 4, 8) if maps == "1scene_text_rev" else (32, 3, 10, 4, 8)))
    L, src, pos, rope = glue_maps(meta, reverse=maps.endswith("_rev"))
    if maps == "no_src":
        src = None
    if maps == "no_pos":
        pos = rope = None
    d = C.pre_case(B, L, NH, seed=3)
    check(f"pre maps={maps}", run_pre(e, d, rope, src, pos, NH), C.pre_oracle(d, rope, src, pos, NH), PRE_ROWS, psum=("dln_w", "dln_b"))


def test_pre_full_3s_segment():
    """B = 1, NH = 48, L = 18 048: the forward's grid (8 192 blocks x 256 threads = 5 461.3 tokens of 384 threads) takes four
    grid-stride passes, the backward's persistent threads 13 - 14 tokens each.  Heads {0, 23, 47} over every token in fp64; every
    head on sampled positions (the first and last token of every grid-stride pass among them)."""
    e = ext()
    NH, B = 48, 1
    L, src, pos, rope = glue_maps(scene_meta(*META_3S))
    assert L == 18048
    d = C.pre_case(B, L, NH, seed=48)
    got = run_pre(e, d, rope, src, pos, NH)
    hs = [0, 23, 47]
    want = C.pre_oracle(d, rope, src, pos, NH, heads=hs)
    check("pre 3s heads 0,23,47", heads_of(got, hs, NH), want, PRE_ROWS, psum=("dln_w", "dln_b"))
    per_pass = 8192 * 256 / (NH * 8)
    edges = set()
    for k in range(4):
        edges |= {int(k * per_pass), int(k * per_pass) - 1, int((k + 1) * per_pass) - 1, int((k + 1) * per_pass)}
    g = torch.Generator().manual_seed(0)
    ts = sorted({t for t in edges if 0 <= t < L} | set(torch.randint(0, L, (256,), generator=g).tolist()))
    ts = torch.tensor(ts)
    s = src[ts].long()
    sub = {n: d[n][:, s] for n in ("q", "k", "v")}
    sub.update({n: d[n][:, :, ts] for n in ("dXQ", "dXK", "dXV")})
    sub.update({n: d[n] for n in ("ln_w", "ln_b")})
    want = C.pre_oracle(sub, rope, None, pos[ts], NH)
    mine = {k: got[k][:, :, ts] for k in ("XQ", "XK", "XV")}
    mine.update({k: got[k][:, s] for k in ("dq", "dk", "dv")})
    check(f"pre 3s sampled positions ({len(ts)}) all heads", mine, want, PRE_ROWS)


def test_pre_zero_row_and_v_equals_k():
    """A zero raw q / k row: the norm clamp (1e-12), forward and backward (the gradient is g / 1e-12).  A row with V = K (text token,
    k = 1 -> 0.125 exactly): zero variance, the target is beta + K; forward only (the reference gradient is 0 / 0 there)."""
    e = ext()
    NH, B = 8, 1
    L, src, pos, rope = glue_maps(scene_meta(32, 3, 10, 4, 8))
    d = C.pre_case(B, L, NH, seed=9)
    h, tz = 3, int(src[200])                                         # a video token
    cz = slice(h * 64, (h + 1) * 64)
    d["q"][0, tz, cz] = 0
    d["k"][0, tz, cz] = 0
    got, want = run_pre(e, d, rope, src, pos, NH), C.pre_oracle(d, rope, src, pos, NH)
    zr = {k: (got[k][0, tz, cz].clone(), want[k][0, tz, cz].clone()) for k in ("dq", "dk")}
    for k in ("dq", "dk"):                                          # rows of size 1e12: checked on their own
        assert rel_l2(*zr[k]) <= T["row"], (k, rel_l2(*zr[k]))
        got[k][0, tz, cz] = 0
        want[k][0, tz, cz] = 0
    assert float(zr["dq"][1].abs().max()) > 1e11
    check("pre zero q/k row", got, want, PRE_ROWS, psum=("dln_w", "dln_b"))

    tv = int(src[5])                                                 # a text token of scene 0
    assert int(pos[5]) < 0
    d["k"][0, tv, cz] = 1.0
    d["v"][0, tv, cz] = 0.125
    got, want = run_pre(e, d, rope, src, pos, NH), C.pre_oracle(d, rope, src, pos, NH)
    want_xv = d["ln_b"][h].double() + 0.125
    assert torch.equal(got["XV"][0, h, 5].double(), want_xv.bfloat16().double())
    check("pre V = K row (forward)", got, want, {k: PRE_ROWS[k] for k in ("XQ", "XK", "XV")})


def test_pre_backward_qkv_grad_blocks_layout():
    """ld_out = 3 D (the column blocks of one [B, L, 3 D] buffer, fused.qkv_grad_blocks): NaN-filled buffer, none left, bits equal
    to the contiguous call"""
    e = ext()
    NH, B = 8, 2
    L, src, pos, rope = glue_maps(scene_meta(32, 3, 10, 4, 8))
    d = C.pre_case(B, L, NH, seed=4)
    a, b = run_pre(e, d, rope, src, pos, NH), run_pre(e, d, rope, src, pos, NH, ld3=True)
    assert not torch.isnan(b["buf"].float()).any()
    for k in ("XQ", "XK", "XV", "dq", "dk", "dv", "dln_w", "dln_b"):
        assert torch.equal(a[k], b[k]), k


def test_pre_and_post_ranges():
    """t0 / tn parts (cuts at multiples of CS = 64): each part writes exactly its own scan positions (pre) / tokens (post) into
    NaN-filled outputs; the union is bit-equal to the one-call result and matches the oracle"""
    e = ext()
    NH, B = 8, 2
    L, src, pos, rope = glue_maps(scene_meta(*META_3SC), reverse=True)
    cuts = [0, 64, 192, 1024, 4416, L]
    d = C.pre_case(B, L, NH, seed=12)
    q, k, v, w, b = (dev(d[n]) for n in ("q", "k", "v", "ln_w", "ln_b"))
    rs, ss, ps = dev(rope), dev(src), dev(pos)
    one = [torch.empty(B, NH, L, 64, dtype=BF, device=DEV) for _ in range(3)]
    e.pre_forward(q, k, v, rs, ss, ps, w, b, *one, NH)
    parts = [nanbuf(B, NH, L, 64) for _ in range(3)]
    for i in range(len(cuts) - 1):
        e.pre_forward(q, k, v, rs, ss, ps, w, b, *parts, NH, t0=cuts[i], tn=cuts[i + 1] - cuts[i])
        written = ~torch.isnan(parts[0].float()).all(dim=(0, 1, 3)).cpu()
        assert torch.equal(written, torch.arange(L) < cuts[i + 1]), i
    torch.cuda.synchronize()
    for a, o in zip(parts, one):
        assert torch.equal(a, o)
    want = C.pre_oracle(d, rope, src, pos, NH)
    check("pre ranges", dict(zip(("XQ", "XK", "XV"), (p.cpu() for p in parts))), want, {k: PRE_ROWS[k] for k in ("XQ", "XK", "XV")})

    pc = C.post_case(B, L, NH, seed=13)
    Y, pw, pb = dev(pc["Y"]), dev(pc["w"]), dev(pc["b"])
    one = torch.empty(B, L, NH * 64, dtype=BF, device=DEV)
    e.post_forward(Y, ss, pw, pb, one, 1e-6)
    part = nanbuf(B, L, NH * 64)
    for i in range(len(cuts) - 1):
        e.post_forward(Y, ss, pw, pb, part, 1e-6, t0=cuts[i], tn=cuts[i + 1] - cuts[i])
        written = ~torch.isnan(part.float()).all(dim=(0, 2)).cpu()
        want_tok = torch.zeros(L, dtype=torch.bool)
        want_tok[src[:cuts[i + 1]].long()] = True
        assert torch.equal(written, want_tok), i
    torch.cuda.synchronize()
    assert torch.equal(part, one)
    check("post ranges", {"out": part.cpu()}, C.post_oracle(pc, src, 1e-6), {"out": (0, 1)})


def test_pre_forward_parts_odd_head_count():
    """NH = 3 (24 threads per token: a block of 256 holds 10 2/3 tokens) in three t0 / tn parts cut at odd positions: bit-equal to
    one call"""
    e = ext()
    NH, B = 3, 2
    L, src, pos, rope = glue_maps(scene_meta(*META_3SC), reverse=True)
    d = C.pre_case(B, L, NH, seed=33)
    q, k, v, w, b = (dev(d[n]) for n in ("q", "k", "v", "ln_w", "ln_b"))
    rs, ss, ps = dev(rope), dev(src), dev(pos)
    one, parts = ([nanbuf(B, NH, L, 64) for _ in range(3)] for _ in range(2))
    e.pre_forward(q, k, v, rs, ss, ps, w, b, *one, NH)
    cuts = [0, 1477, 2950, L]
    for i in range(3):
        e.pre_forward(q, k, v, rs, ss, ps, w, b, *parts, NH, t0=cuts[i], tn=cuts[i + 1] - cuts[i])
    torch.cuda.synchronize()
    for a, o in zip(parts, one):
        assert not torch.isnan(o.float()).any() and torch.equal(a, o)


# ------------------------------------------------------------------------------------------------ post
def _post_vs_oracle(NH, B, L, src, seed):
    e = ext()
    eps = 1e-6
    pc = C.post_case(B, L, NH, seed=seed)
    D = NH * 64
    Y, w, b, sd = dev(pc["Y"]), dev(pc["w"]), dev(pc["b"]), dev(src)
    if src is None:
        src = torch.arange(L)
    out = nanbuf(B, L, D)
    e.post_forward(Y, sd, w, b, out, eps)
    P = e.post_partials(B, L)
    dY, pw, pb = nanbuf(B, NH, L, 64), nanbuf(P, D, dtype=torch.float32), nanbuf(P, D, dtype=torch.float32)
    e.post_backward(Y, dev(pc["dOut"]), sd, w, dY, pw, pb, eps)
    torch.cuda.synchronize()
    out, dY = out.cpu(), dY.cpu()
    got = {"out": out, "dY": dY, "dw": pw.double().sum(0).cpu(), "db": pb.double().sum(0).cpu()}
    want = {"dw": 0, "db": 0}
    mine = {"out": [], "dY": []}
    theirs = {"out": [], "dY": []}
    step = max(1, (1 << 22) // D)
    for t0 in range(0, L, step):
        ts = slice(t0, min(L, t0 + step))
        s = src[ts].long()
        r = C.post_oracle({"Y": pc["Y"][:, :, ts], "w": pc["w"], "b": pc["b"], "dOut": pc["dOut"][:, s]}, None, eps)
        want["dw"] = want["dw"] + r["dw"]
        want["db"] = want["db"] + r["db"]
        mine["out"].append(out[:, s]); theirs["out"].append(r["out"])
        mine["dY"].append(dY[:, :, ts]); theirs["dY"].append(r["dY"])
    got.update(out=torch.cat(mine["out"], 1), dY=torch.cat(mine["dY"], 2))
    want.update(out=torch.cat(theirs["out"], 1), dY=torch.cat(theirs["dY"], 2))
    check(f"post NH={NH} B={B} L={L} P={P}", got, want, {"out": (0, 1), "dY": (0, 1, 2)}, psum=("dw", "db"))


@pytest.mark.parametrize("NH", [2, 8, 20, 48, 64])
def test_post_vs_oracle(NH):
    """NH = 2 / 8 / 20 / 48 / 64: ln_team_waves 1 / 1 / 1 (a partial lane group) / 2 / 4; B = 2, L = 18 048, scene permutation;
    rows of RMS 1e-3 .. 1 (eps matters).  Per-token operation: the oracle runs on chunks of scan positions."""
    L, src, pos, rope = glue_maps(scene_meta(166, 3, 13, 30, 45))
    assert L == 18048
    _post_vs_oracle(NH, 2, L, src, seed=NH)


@pytest.mark.parametrize("NH,B,L,mapped", [(8, 1, 8256, True), (64, 2, 1100, True), (24, 2, 1100, False)])
def test_post_vs_oracle_small(NH, B, L, mapped):
    """Few tokens, where the token teams of the backward run ragged.  NH = 8, 8 256 tokens: one wave per team, eight teams, chunk
    slot 0 alone active, 1 024 blocks x 8 tokens and a ragged second iteration.  NH = 64, 2 x 1 100: four waves per team, two teams,
    chunk slot 2 wholly inactive, a ragged second iteration.  NH = 24 without a token map: all three chunk slots active."""
    src = torch.randperm(L, generator=torch.Generator().manual_seed(L)).to(torch.int32) if mapped else None
    _post_vs_oracle(NH, B, L, src, seed=NH + L)


# ------------------------------------------------------------------------------------------------ gate
def _gate_vs_oracle(D, n_text, B, L):
    e = ext()
    gc = C.gate_case(B, L, D, seed=D + n_text)
    tt, tv = (torch.tanh(gc[n]).to(DEV) for n in ("at", "av"))
    res, y, g = (dev(gc[n]) for n in ("res", "y", "g"))
    out, dy = nanbuf(B, L, D), nanbuf(B, L, D)
    e.gate_forward(res, y, tt, tv, out, n_text)
    P = e.gate_backward_partials(D)
    part = nanbuf(P, 2, D, dtype=torch.float32)
    e.gate_backward(g, y, tt, tv, dy, part, n_text)
    torch.cuda.synchronize()
    assert not torch.isnan(out).any() and not torch.isnan(dy).any()
    sums = part.double().sum(0).cpu()
    cols = torch.cat((torch.arange(64), torch.arange(D - 64, D), torch.randperm(D - 128, generator=torch.Generator().manual_seed(D))[:128] + 64))
    sub = {"res": gc["res"][..., cols], "y": gc["y"][..., cols], "g": gc["g"][..., cols], "at": gc["at"][cols], "av": gc["av"][cols]}
    want = C.gate_oracle(sub, n_text)
    got = {"out": out.cpu()[..., cols], "dy": dy.cpu()[..., cols], "dtanh_t": sums[0, cols], "dtanh_v": sums[1, cols]}
    if n_text == 0:
        assert not got["dtanh_t"].any()
        want["dtanh_t"] = got["dtanh_t"] = torch.ones(len(cols))
    if n_text >= L:
        assert not got["dtanh_v"].any()
        want["dtanh_v"] = got["dtanh_v"] = torch.ones(len(cols))
    check(f"gate D={D} L={L} n_text={n_text} P={P}", got, want, {"out": (0, 1), "dy": (0, 1)}, psum=("dtanh_t", "dtanh_v"))


@pytest.mark.parametrize("n_text", [0, 1, 498, 1506, 18048])
@pytest.mark.parametrize("D", [512, 3072])
def test_gate_vs_oracle(D, n_text):
    """B = 2, L = 18 048; n_text = one scene's text at 3 s (498), three scenes at 9 s (1 506), none, one, all.  Per-feature
    operation: the oracle runs on 256 features (the first and last octets among them) over every token."""
    _gate_vs_oracle(D, n_text, 2, 18048)


@pytest.mark.parametrize("n_text", [0, 498, 2100])
def test_gate_vs_oracle_period_not_dividing_the_block(n_text):
    """D = 520: the backward's thread period D / 8 = 65 does not divide 256, the persistent grid steps down to a multiple of 65 blocks
    and a block's threads straddle rows of partials; B = 2, L = 2 100, no text / some / all"""
    _gate_vs_oracle(520, n_text, 2, 2100)


# ------------------------------------------------------------------------------------------------ AdaLN, residual gates
def _adaln_and_resgate_vs_oracle(D, Lt, Lv):
    e = ext()
    B, eps = 2, 1e-6
    ac = C.adaln_case(B, Lt, Lv, D, seed=D + Lt + Lv)
    vid, text = dev(ac["vid"]), dev(ac["text"])
    w, b = dev(ac["w"]), dev(ac["b"])
    shift = torch.stack((ac["sh_t"], ac["sh_v"]), 1).to(DEV)
    scale1p = torch.stack((1 + ac["sc_t"], 1 + ac["sc_v"]), 1).bfloat16().float().to(DEV)   # formed in bf16, as FusedAdaLN does
    out = nanbuf(B, Lt + Lv, D)
    e.adaln_forward(vid, text, w, b, shift, scale1p, out, eps)
    P = e.adaln_backward_partials()
    dvid, dtext = nanbuf(B, Lv, D), nanbuf(B, Lt, D)
    part = nanbuf(B * 2 * P, 4, D, dtype=torch.float32)
    e.adaln_backward(vid, text, dev(ac["dout"]), w, b, scale1p, dvid, dtext, part, eps)
    torch.cuda.synchronize()
    s = part.double().view(B, 2, P, 4, D).sum(2).cpu()                  # [B, group, 4, D]
    got = {"out": out.cpu(), "dvid": dvid.cpu(), "dtext": dtext.cpu(), "dw": s[:, :, 0].sum((0, 1)), "db": s[:, :, 1].sum((0, 1)),
           "dsc_t": s[:, 0, 2], "dsc_v": s[:, 1, 2], "dsh_t": s[:, 0, 3], "dsh_v": s[:, 1, 3]}
    want = C.adaln_oracle(ac, eps)
    rows = {k: (0, 1) for k, n in (("out", 1), ("dvid", Lv), ("dtext", Lt)) if n}
    psum = [k for k, n in (("dw", 1), ("db", 1), ("dsc_t", Lt), ("dsc_v", Lv), ("dsh_t", Lt), ("dsh_v", Lv)) if n]
    for k, n in (("dsc_t", Lt), ("dsc_v", Lv), ("dsh_t", Lt), ("dsh_v", Lv)):
        if not n:
            assert not got[k].any(), k
    check(f"adaln D={D} Lt={Lt} Lv={Lv}", got, want, rows, psum=psum)

    gate = torch.stack((ac["g_t"], ac["g_v"]), 1).to(DEV)
    y = dev(ac["y"])
    ovid, otext = nanbuf(B, Lv, D), nanbuf(B, Lt, D)
    e.resgate_forward(vid, text, y, gate, ovid, otext)
    P = e.resgate_backward_partials(D)
    dy, part = nanbuf(B, Lt + Lv, D), nanbuf(P, B, 2, D, dtype=torch.float32)
    e.resgate_backward(dev(ac["dvid"]), dev(ac["dtext"]), y, gate, dy, part)
    torch.cuda.synchronize()
    s = part.double().sum(0).cpu()                                       # [B, group, D]
    got = {"ovid": ovid.cpu(), "otext": otext.cpu(), "dy": dy.cpu(), "dg_t": s[:, 0], "dg_v": s[:, 1]}
    want = C.resgate_oracle(ac)
    rows = {k: (0, 1) for k, n in (("ovid", Lv), ("otext", Lt), ("dy", 1)) if n}
    for k, n in (("dg_t", Lt), ("dg_v", Lv)):
        if not n:
            assert not got[k].any(), k
    check(f"resgate D={D} Lt={Lt} Lv={Lv} P={P}", got, want, rows, psum=[k for k, n in (("dg_t", Lt), ("dg_v", Lv)) if n])


@pytest.mark.parametrize("Lt,Lv", [(0, 3001), (1, 3001), (498, 3001), (498, 0)])
@pytest.mark.parametrize("D", [512, 1280, 3072, 4096])
def test_adaln_and_resgate_vs_oracle(D, Lt, Lv):
    """D = 512 / 1280 / 3072 / 4096: ln_team_waves 1 (lanes e = 1, 2 idle) / 1 (a partial lane group) / 2 / 4; distinct
    modulation per batch (B = 2); 3 001 video tokens: a ragged number of tokens per block of the backward (P = 256 per group)"""
    _adaln_and_resgate_vs_oracle(D, Lt, Lv)


@pytest.mark.parametrize("D,Lt,Lv", [(512, 5, 2100), (4096, 3, 600), (520, 0, 2100), (520, 5, 2100), (520, 498, 0)])
def test_adaln_and_resgate_vs_oracle_small(D, Lt, Lv):
    """D = 512, 5 text tokens: fewer than the 256 blocks of their group, most of which never hold a valid token; 2 100 video tokens:
    a ragged second iteration.  D = 4 096, 3 + 600 tokens: four waves per team, the team reduction [2, D] and the constants [3, D]
    share the LDS area sized for 3 rows.  D = 520: the residual gate backward's thread period of 65 does not divide 256 (the
    persistent grid steps down), with an empty text / video group."""
    _adaln_and_resgate_vs_oracle(D, Lt, Lv)
