"""Segment-attention kernels (csrc/attn_fwd.hip, attn_bwd.hip, attn_v2.hip with the bodies of attn_body.h, attn_pre.hip) called
through the C ABI (-m gpu) against the rounding-aware fp64 statements of oracle/attn_oracle.py (``fwd``, ``bwd``, ``pre``), every
row of every head: the whole 48-head, 18 048-token 3 s segment at 5B size with the model's strides, the Delta kernel's second
grid-stride pass (3 x 48 x 18 048 rows), the ragged tails and both workgroup -> head mappings, the value regimes of the online
softmax, the pre kernel with both grid caps active.  Every output buffer is NaN-filled first; every element the kernel should
write must come back finite and every other one (guard rows, the columns of a shared buffer that belong to another tensor) NaN.
Metrics (tests/attn_cases.py): fraction of bf16 outputs more than 1 ulp off and the largest ulp distance, the worst
(batch, head, token) row, LSE max abs error, Delta max relative error, the rel-L2 of the LayerNorm parameter gradients summed from
the pre kernel's partials.  Tolerances ATTN_TOL / ATTN_TOL_LARGE, fixed by the sensitivity table of
tests/test_attention_oracle_cpu.py (>= 10x the statement's own fp32 error, >= 10x below every mutation it must catch)."""
import pytest
import torch

import attn_cases as C
from helpers import ATTN_TOL, ATTN_TOL_LARGE, rel_l2
from oracle import attn_oracle as AO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
S5B, NH5B, NTEXT5B = 18048, 48, 498          # 3 s at 5B: 498 text tokens + 13 latent frames of 30 x 45


def ext():
    import test_time_training as e
    e.load_library()
    return e


def nanbuf(*shape, dtype=BF):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def all_nan(t):
    return bool(torch.isnan(t.float()).all())


def finite(t):
    return bool(torch.isfinite(t.float()).all())


def bshd(t):
    """[B, NH, S, 64] values -> a bf16 [B, NH, S, 64] view of [B, S, NH, 64] device memory (the block's layout)"""
    return t.to(DEV).transpose(1, 2).to(BF).contiguous().transpose(1, 2)


def out_view(B, NH, S):
    """NaN [B, S + 1, NH, 64] buffer and its [B, NH, S, 64] view: token S is a guard row no kernel may write"""
    buf = nanbuf(B, S + 1, NH, 64)
    return buf, buf[:, :S].transpose(1, 2)


def row_vec(B, NH, S):
    """NaN fp32 buffer of B*NH*S + 64 and its contiguous [B, NH, S] head (the tail: guard)"""
    buf = nanbuf(B * NH * S + 64, dtype=torch.float32)
    return buf, buf[:B * NH * S].view(B, NH, S)


def run_fwd(e, q, k, v):
    B, NH, S, _ = q.shape
    obuf, o = out_view(B, NH, S)
    lbuf, lse = row_vec(B, NH, S)
    e.attn_forward(q, k, v, o, lse, C.SCALE)
    torch.cuda.synchronize()
    assert finite(o) and finite(lse), "forward left an output element unwritten"
    assert all_nan(obuf[:, S]) and all_nan(lbuf[B * NH * S:]), "forward wrote past its outputs"
    return o, lse


def run_bwd(e, q, k, v, o, do, lse, dv=None):
    """dQ, dK (and dV unless a view is given) into NaN [B, S + 1, NH, 64] buffers; Delta into a guarded fp32 vector"""
    B, NH, S, _ = q.shape
    bufs = [out_view(B, NH, S) for _ in range(2 if dv is not None else 3)]
    dbuf, delta = row_vec(B, NH, S)
    dq, dk = bufs[0][1], bufs[1][1]
    dv = bufs[2][1] if dv is None else dv
    e.attn_backward(q, k, v, o, do, lse, delta, dq, dk, dv, C.SCALE)
    torch.cuda.synchronize()
    assert all(finite(t) for t in (dq, dk, dv, delta)), "backward left an output element unwritten"
    assert all(all_nan(b[:, S]) for b, _ in bufs) and all_nan(dbuf[B * NH * S:]), "backward wrote past its outputs"
    return {"dq": dq, "dk": dk, "dv": dv, "delta": delta}


def oracle(q, k, v, do, o, lse, heads_per_call=None):
    """fp64 statements on the device, a group of heads at a time (the scores of one 18 048-token head are 2.6 GB in fp64); the
    backward takes the kernel's O and LSE"""
    B, NH, S, _ = q.shape
    f = lambda t: t.double()
    want = {n: torch.empty(B, NH, S, 64, dtype=torch.float64, device=DEV) for n in ("O", "dq", "dk", "dv", "dq_mag", "dk_mag")}
    want["LSE"], want["delta"] = (torch.empty(B, NH, S, dtype=torch.float64, device=DEV) for _ in range(2))
    step = heads_per_call or 8
    for b in range(B):
        for h0 in range(0, NH, step):
            sl = (slice(b, b + 1), slice(h0, h0 + step))
            wo, wl = AO.fwd(f(q[sl]), f(k[sl]), f(v[sl]))
            g = AO.bwd(f(q[sl]), f(k[sl]), f(v[sl]), f(do[sl]), f(o[sl]), f(lse[sl]), mags=True)
            want["O"][sl], want["LSE"][sl] = wo, wl
            for n in ("dq", "dk", "dv", "delta", "dq_mag", "dk_mag"):
                want[n][sl] = g[n]
    return want


def check(tag, got, want, o, do, tol=ATTN_TOL, cancel=False):
    """assert the metrics of every result in ``got`` (kernel) against ``want`` (fp64 statement); prints the measured values.
    ``cancel``: dQ / dK are sums of terms that cancel to (near) 0 - held to the cancellation metric only (ATTN_TOL["cancel"])"""
    res = {}
    for n in ("dq", "dk"):
        if n in got:
            res[n + " cancel"] = C.cancel_err(got[n], want[n], want[n + "_mag"])
            assert res[n + " cancel"] <= tol["cancel"], (tag, n, res[n + " cancel"])
    for n in ("O", "dv") if cancel else ("O", "dq", "dk", "dv"):
        if n in got:
            frac, mx, row = C.out_metrics(got[n], want[n])
            res[n] = (frac, mx, row)
            assert frac <= tol["ulp_frac"] and mx <= tol["ulp_max"], (tag, n, frac, mx)
            assert row <= tol["row"], (tag, n, row)
    if "LSE" in got:
        res["LSE"] = float((got["LSE"].double() - want["LSE"]).abs().max())
        assert res["LSE"] <= tol["lse"], (tag, res["LSE"])
    if "delta" in got:
        res["delta"] = C.delta_err(got["delta"], want["delta"], o, do)
        assert res["delta"] <= tol["delta"], (tag, res["delta"])
    print("ATTN", tag, {n: (tuple(f"{x:.3g}" for x in v) if isinstance(v, tuple) else f"{v:.3g}") for n, v in res.items()})


def fwd_bwd_check(e, tag, q, k, v, do, tol=ATTN_TOL, heads_per_call=None, cancel=False):
    o, lse = run_fwd(e, q, k, v)
    g = run_bwd(e, q, k, v, o, do, lse)
    want = oracle(q, k, v, do, o, lse, heads_per_call)
    got = dict(g, O=o, LSE=lse)
    check(tag, got, want, o, do, tol, cancel)
    return got


# ------------------------------------------------------------------------------------------------ the 5B segment
def test_5b_segment_every_row_model_strides():
    """B = 1, 48 heads, S = 18 048, every row of every head, forward and backward.  Strides as FusedSegmentAttention passes them: q, k
    views of [B, S, NH*64] buffers, v a view of the [B, S, 3 D] projection output, dV written through a token stride of 3 D into
    the third column block of a NaN-filled [B, S, 3 D] gradient buffer (its q / k blocks must stay NaN), O / dQ / dK as
    [B, S, NH, 64] buffers.  Then: attn_prio 0 against 1 and a repeated call give the same bits."""
    e = ext()
    B, NH, S = 1, NH5B, S5B
    D = NH * 64
    q, k, v, do = C.model_case(B, NH, S, 5, device=DEV)
    heads = lambda t: t.view(B, S, NH, 64).transpose(1, 2)
    qv, kv = (heads(t.transpose(1, 2).reshape(B, S, D).to(BF).contiguous()) for t in (q, k))
    act = torch.randn(B, S, 3 * D, device=DEV).to(BF)                      # the q / k blocks hold other data
    act[..., 2 * D:] = v.transpose(1, 2).reshape(B, S, D).to(BF)
    vv = heads(act[..., 2 * D:])
    dov = bshd(do)
    o, lse = run_fwd(e, qv, kv, vv)
    gbuf = nanbuf(B, S, 3 * D)
    dvv = heads(gbuf[..., 2 * D:])
    g = run_bwd(e, qv, kv, vv, o, dov, lse, dv=dvv)
    assert all_nan(gbuf[..., :2 * D]), "dV wrote into the q / k columns of the shared gradient buffer"
    want = oracle(qv, kv, vv, dov, o, lse, heads_per_call=1)
    check("5B 48x18048", dict(g, O=o, LSE=lse), want, o, dov)

    # same bits: a second identical call, and the backward without the s_setprio pair
    o2, lse2 = run_fwd(e, qv, kv, vv)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    g2 = run_bwd(e, qv, kv, vv, o, dov, lse)
    try:
        e.debug_option("attn_prio", 0)
        g0 = run_bwd(e, qv, kv, vv, o, dov, lse)
    finally:
        e.debug_option("attn_prio", 1)
    for n in ("dq", "dk", "dv", "delta"):
        assert torch.equal(g2[n], g[n]), ("repeat", n)
        assert torch.equal(g0[n], g[n]), ("attn_prio 0", n)


def test_delta_second_grid_stride_pass():
    """B = 3, 48 heads, S = 18 048: 2.6 M rows x 8 threads > the Delta kernel's 65 536 x 256-thread grid, so its grid-stride loop
    runs a second pass.  Delta of every row against fp64; dQ, dK, dV on sampled heads of every batch (the last head included)."""
    e = ext()
    B, NH, S = 3, NH5B, S5B
    assert B * NH * S * 8 > 65536 * 256
    q, k, v, do = (bshd(t) for t in C.model_case(B, NH, S, 6, device=DEV))
    o, lse = run_fwd(e, q, k, v)
    g = run_bwd(e, q, k, v, o, do, lse)
    want = (o.double() * do.double()).sum(-1)
    err = C.delta_err(g["delta"], want, o, do)
    print("ATTN delta 3x48x18048", f"{err:.3g}")
    assert err <= ATTN_TOL["delta"], err
    for b, h in ((0, 0), (1, 23), (2, NH - 1)):
        sl = (slice(b, b + 1), slice(h, h + 1))
        w = oracle(q[sl], k[sl], v[sl], do[sl], o[sl], lse[sl])
        check(f"3x48x18048 b={b} h={h}", {n: g[n][sl] for n in ("dq", "dk", "dv", "delta")} | {"O": o[sl], "LSE": lse[sl]}, w,
              o[sl], do[sl])


# ------------------------------------------------------------------------------------------------ ragged and mapping edges
S_EDGES = [1, 31, 63, 64, 65, 255, 256, 257, 383, 384, 385, 511, 513, 4097]
EDGE_CASES = [(1, 3, s) for s in S_EDGES] + [(2, 4, s) for s in S_EDGES] + \
    [(b, nh, s) for b, nh in ((1, 1), (2, 8), (2, 25)) for s in (65, 385, 513, 4097)]


@pytest.mark.parametrize("B,NH,S", EDGE_CASES)
def test_ragged_and_mapping_edges(B, NH, S):
    """the 64-key tile, the 256-row forward block, the 384-key dK / dV block and the 512-row dQ block, each at, one below and one
    above its edge; B * NH in {1, 3, 8, 16, 50}: both branches of head_of_block (B * NH % 8 == 0 or not)"""
    e = ext()
    q, k, v, do = (bshd(t) for t in C.model_case(B, NH, S, 1000 + S + 7 * NH, device=DEV))
    fwd_bwd_check(e, f"edge B={B} NH={NH} S={S}", q, k, v, do, cancel=S == 1)      # one key: dS = P (dP - Delta) = 0


def test_ragged_same_bits_prio_and_repeat():
    e = ext()
    q, k, v, do = (bshd(t) for t in C.model_case(2, 3, 577, 12, device=DEV))
    o, lse = run_fwd(e, q, k, v)
    o2, lse2 = run_fwd(e, q, k, v)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    g1, g2 = run_bwd(e, q, k, v, o, do, lse), run_bwd(e, q, k, v, o, do, lse)
    try:
        e.debug_option("attn_prio", 0)
        g0 = run_bwd(e, q, k, v, o, do, lse)
    finally:
        e.debug_option("attn_prio", 1)
    for n in ("dq", "dk", "dv", "delta"):
        assert torch.equal(g1[n], g2[n]) and torch.equal(g1[n], g0[n]), n


# ------------------------------------------------------------------------------------------------ value regimes
def _regime(name, B=1, NH=2, S=577, seed=40):
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(B, NH, S, 64, generator=g).bfloat16().float()
    q, k, v, do = r(), r(), r(), r()
    u = torch.randn(64, generator=g).sign()                                  # +-1: bf16-exact
    if name == "saturated":            # one key wins every row by ~120 scaled units: every other probability underflows to 0
        q = (u + 0.5 * r()).bfloat16().float()
        k[:, :, 300] = 15 * u
    elif name == "equal_keys":         # every score of a row equal: after tile 0 the running max never grows
        k[:] = k[:, :, :1].clone()
    elif name == "max_in_last_tile":   # the winning key is the only key of the ragged last tile (577 = 9 x 64 + 1)
        q = (u + 0.5 * r()).bfloat16().float()
        k[:, :, S - 1] = 4 * u
    elif name == "one_lane":           # equal keys, except key 300 raises the score of query row 37 alone: one lane of one wave
        k0 = k[:, :, :1].clone()       # takes the rescale branch in tile 4, every other row's maximum stays put
        k0[..., 0] = 0
        k[:] = k0
        q[..., 0] = -(q[..., 0].abs() + 0.5)
        q[:, :, 37, 0] = 2.0
        k[:, :, 300, 0] = 4.0
    return q, k, v, do


@pytest.mark.parametrize("name", ["saturated", "equal_keys", "max_in_last_tile", "one_lane"])
def test_softmax_value_regimes(name):
    e = ext()
    q, k, v, do = (bshd(t) for t in _regime(name))
    fwd_bwd_check(e, f"regime {name}", q, k, v, do, cancel=True)


@pytest.mark.parametrize("S", [300, 4097])
def test_large_lse_regime(S):
    """|LSE| ~ 1e3 (heads alternate the sign): the dK / dV kernel's accumulator starts from -LSE / scale in fp32; ATTN_TOL_LARGE"""
    e = ext()
    q, k, v, do = (bshd(t) for t in C.large_lse_case(1, 4, S, 3))
    got = fwd_bwd_check(e, f"large |LSE| S={S}", q, k, v, do, tol=ATTN_TOL_LARGE, cancel=True)
    assert float(got["LSE"].abs().max()) > 900


# ------------------------------------------------------------------------------------------------ pre kernel
def run_pre(e, d, NH, n_text, ld3=False, exact_table=False):
    """attn_pre_forward + attn_pre_backward on NaN-filled outputs (guarded); the parameter gradients summed (fp64) from the partials"""
    B, S, D = d["q_raw"].shape
    dv = {n: t.to(DEV) for n, t in d.items()}
    qr, kr = dv["q_raw"].to(BF), dv["k_raw"].to(BF)
    cos, sin = dv["cos"], dv["sin"]
    if exact_table:                    # exactly S - n_text rows, followed by NaN rows: a read past the table shows as NaN
        n = S - n_text
        tabs = []
        for t in (cos, sin):
            buf = nanbuf(n + 64, 64, dtype=torch.float32)
            buf[:n] = t[:n]
            tabs.append(buf[:n])
        cos, sin = tabs
    n_el = B * S * D
    qb, kb = nanbuf(n_el + 64), nanbuf(n_el + 64)
    q, k = qb[:n_el].view(B, S, D), kb[:n_el].view(B, S, D)
    e.attn_pre_forward(qr, kr, dv["wq"], dv["bq"], dv["wk"], dv["bk"], cos, sin, q, k, NH, n_text, 1e-6)
    dq, dk = (dv[n].to(BF).transpose(1, 2) for n in ("dq", "dk"))
    if ld3:
        buf = nanbuf(B, S, 3 * D)
        dq_raw, dk_raw = buf[..., :D], buf[..., D:2 * D]
    else:
        rb_q, rb_k = nanbuf(n_el + 64), nanbuf(n_el + 64)
        dq_raw, dk_raw = rb_q[:n_el].view(B, S, D), rb_k[:n_el].view(B, S, D)
    P = e.attn_pre_partials(B, S, NH)
    part = nanbuf(P, 4, 64, dtype=torch.float32)
    e.attn_pre_backward(qr, kr, dq, dk, dv["wq"], dv["wk"], cos, sin, dq_raw, dk_raw, part, NH, n_text, 1e-6,
                        ld_out=3 * D if ld3 else None)
    torch.cuda.synchronize()
    assert all(finite(t) for t in (q, k, dq_raw, dk_raw, part)), "pre left an output element unwritten"
    assert all_nan(qb[n_el:]) and all_nan(kb[n_el:]), "pre forward wrote past its outputs"
    if ld3:
        assert all_nan(buf[..., 2 * D:]), "pre backward wrote into the dV columns of the shared buffer"
    else:
        assert all_nan(rb_q[n_el:]) and all_nan(rb_k[n_el:]), "pre backward wrote past its outputs"
    sums = part.double().sum(0)
    r = {"q": q.view(B, S, NH, 64), "k": k.view(B, S, NH, 64), "dq_raw": dq_raw.reshape(B, S, NH, 64),
         "dk_raw": dk_raw.reshape(B, S, NH, 64)}
    r.update(zip(C.PRE_PARAMS, sums))
    return r, P


def pre_check(tag, got, d, NH, n_text, P):
    want = C.pre_oracle({n: t.to(DEV) for n, t in d.items()}, NH, n_text)
    res = {}
    for n in ("q", "k", "dq_raw", "dk_raw"):
        frac, mx, row = C.out_metrics(got[n], want[n], C.PRE_FLOOR)
        res[n] = (frac, mx, row)
        assert frac <= ATTN_TOL["ulp_frac"] and mx <= ATTN_TOL["ulp_max"], (tag, n, frac, mx)
        assert row <= ATTN_TOL["row"], (tag, n, row)
    for n in C.PRE_PARAMS:
        res[n] = rel_l2(got[n], want[n])
        assert res[n] <= ATTN_TOL["psum"], (tag, n, res[n])
    print("ATTN", tag, f"P={P}", {n: (tuple(f"{x:.3g}" for x in v) if isinstance(v, tuple) else f"{v:.3g}") for n, v in res.items()})


@pytest.mark.parametrize("n_text", [0, NTEXT5B, S5B])
def test_pre_5b_segment(n_text):
    """48 heads x 18 048 tokens = 866 k rows: the forward's 8 192-block and the backward's 2 048-partial grid caps are both active,
    so the grid-stride loops and the partial-sum reduction run as in the model; all text, 498 text tokens, no video"""
    e = ext()
    B, S, NH = 1, S5B, NH5B
    assert B * S * NH * 8 > 8192 * 256
    d = C.pre_case(B, S, NH, n_text, 20 + n_text)
    got, P = run_pre(e, d, NH, n_text, ld3=n_text == NTEXT5B)
    assert P == 2048
    pre_check(f"pre 5B n_text={n_text}", got, d, NH, n_text, P)


@pytest.mark.parametrize("NH", [1, 2, 3])
def test_pre_heads_ld3_degenerate_rows_exact_table(NH):
    """B = 2, NH 1 / 2 / 3; dq_raw / dk_raw as column blocks of a [B, S, 3 D] buffer (ld_out = 3 D; the dV block stays NaN); a zero
    row and a constant row (variance 0) in q and k; a RoPE table of exactly S - n_text rows followed by NaN"""
    e = ext()
    B, S, n_text = 2, 333, 37
    d = C.pre_case(B, S, NH, n_text, 30 + NH)
    h = NH - 1
    for n in ("q_raw", "k_raw"):
        d[n][0, 5, 64 * h:64 * (h + 1)] = 0.0
        d[n][1, 200, :64] = 0.375
    got, P = run_pre(e, d, NH, n_text, ld3=True, exact_table=True)
    pre_check(f"pre NH={NH} B=2", got, d, NH, n_text, P)
