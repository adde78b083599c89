#!/usr/bin/env python
"""Round 5: the TTT-MLP layer (projections -> pre -> scan -> post-norm -> output projection, both scan directions) at the 5B / 9 s
geometry as one piece and as a pipeline over parts of the sequence (ttt_amd/models/ssm/pipeline.py); interleaved rounds in one
process, medians, forward alone and forward + backward; outputs / gradients compared.

    python tools/ttt_layer_bench.py [--parts 0,2,3,4] [--video-length 9sec] [--rounds 5]

The sampling geometry (mini-batches of 16, one checkpoint group, the guidance pair as a batch of two, forward only):

    python tools/ttt_layer_bench.py --mini-batch 16 --batch 2 --no-grad --video-length 63sec --parts 0,default,4,8,16

("default" = the library's plan; at mini-batches of 16 a number means exactly that many parts).  --scan-only times the scans
alone: the one-call forward against the same scan as the chunk launches of each plan, back to back on one stream.

The TTT-Linear layer (--ssm ttt_linear; --parts sets TTTBase.linear_pipeline_parts, "default" = off; mini-batches of 64 run in parts
on the opt-in MFMA scan only, --cs64-impl mfma; mini-batches of 16 have an MFMA backward, so --no-grad is optional there):

    python tools/ttt_layer_bench.py --ssm ttt_linear --cs64-impl mfma --no-grad --parts 0,2,4,8
    python tools/ttt_layer_bench.py --ssm ttt_linear --mini-batch 16 --batch 2 --no-grad --video-length 63sec --parts 0,4,8 [--scan-only]

A variant with "+split" behind it runs with HipLinear.cs16_scan_split on (the two-wave CS = 16 scan), interleaved with the others:

    python tools/ttt_layer_bench.py --ssm ttt_linear --mini-batch 16 --batch 2 --no-grad --parts 0,0+split,4,4+split
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ttt-video-dit_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402


def timeit(fn, iters=3):
    fn(); torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for s, e in ev:
        s.record(); fn(); e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    return ms[len(ms) // 2]


def scan_only(a, ext, layer, meta, x, L, parts, set_parts, res):
    """the scan kernels alone at this geometry (random inputs): ttt_forward against the chunk launches of each plan"""
    dev = x.device
    mlp = a.ssm == "ttt_mlp"
    B, NH, CS, Fh = x.shape[0], layer.ttt.num_heads, a.mini_batch, 64
    NC = L // CS
    G = layer.ttt._group_size(NC)
    K = -(-NC // G)
    g = torch.Generator(device=dev).manual_seed(3)
    mk = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=g) * scale
    l2 = lambda t: torch.nn.functional.normalize(t, dim=-1)
    XQ, XK, XV = l2(mk(B, NH, NC, CS, Fh)).bfloat16(), l2(mk(B, NH, NC, CS, Fh)).bfloat16(), mk(B, NH, NC, CS, Fh, scale=0.5).bfloat16()
    eta = (torch.rand(B, NH, NC, CS, 1, device=dev, generator=g) * 0.02 + 0.005).bfloat16()
    ln_shape = (1, NH, 1, Fh) if mlp else (NH, Fh)
    lw, lb = (1 + 0.1 * mk(*ln_shape)).float(), (0.1 * mk(*ln_shape)).float()
    shapes = ((Fh, 4 * Fh), (1, 4 * Fh), (4 * Fh, Fh), (1, Fh)) if mlp else ((Fh, Fh), (1, Fh))
    st = [mk(B, NH, *sh, scale=0.02) for sh in shapes]
    cks = tuple(torch.empty(B, NH, K, *sh, device=dev, dtype=torch.float32) for sh in shapes)
    out0, out1 = torch.empty_like(XQ), torch.empty_like(XQ)
    if mlp:
        scan, scan_chunk = ext.ttt_forward, ext.ttt_forward_chunk
    else:
        from ttt_amd.models.ssm.linear_hip import HipLinear
        impl = HipLinear._impl(CS, Fh, torch.bfloat16)
        res["scan_impl"] = ext.resolved_impl(B, NH, NC, CS, Fh, G, torch.bfloat16, mlp=False, backward=False, impl=impl)
        scan = lambda *t: ext.ttt_linear_forward_impl(impl, *t)
        scan_chunk = lambda *t: ext.ttt_linear_forward_chunk(impl, *t)

    def one_call():
        scan(XQ, XK, XV, eta, lw, lb, *st, *cks, out0, G)

    def in_parts(plan):
        carry = [t.clone() for t in st]
        for s0, ns, _ in plan:
            scan_chunk(XQ, XK, XV, eta, lw, lb, *carry, *cks, out1, G, s0, ns)

    plans = {}
    for n in parts:
        set_parts(n)
        with torch.no_grad():
            plans[n] = layer.ttt._pipeline_plan(x, meta, L, False, False)
    t = {n: [] for n in parts}
    for _ in range(a.rounds):
        for n in parts:
            t[n].append(timeit(one_call if plans[n] is None else (lambda: in_parts(plans[n]))))
    for n in parts:
        ent = {"scan_ms_median": sorted(t[n])[len(t[n]) // 2], "scan_ms_runs": [round(v, 3) for v in t[n]],
               "launches": 1 if plans[n] is None else len(plans[n])}
        if plans[n] is not None:
            one_call(); in_parts(plans[n]); torch.cuda.synchronize()
            ent["bits_of_one_call"] = bool(torch.equal(out0, out1))
        res["by_parts"][str(n)] = ent
    res["scan"] = {"B": B, "NH": NH, "NC": NC, "G": G}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="0,2,3,4", help='variants: N parts, "default", each optionally with "+pair" (the TTT-MLP CS = 16 pair scan on) or "+split" (the TTT-Linear CS = 16 two-wave scan on)')
    ap.add_argument("--video-length", default="9sec")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mini-batch", type=int, default=64, choices=[64, 16], help="16: the evaluation settings (no scan checkpoints)")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--no-grad", action="store_true", help="forward only (required at mini-batches of 16: no MFMA backward there)")
    ap.add_argument("--scan-only", action="store_true", help="time the scan kernels alone: one call against the parts of each plan")
    ap.add_argument("--ssm", default="ttt_mlp", choices=["ttt_mlp", "ttt_linear"], help="ttt_linear: --parts sets linear_pipeline_parts")
    ap.add_argument("--cs64-impl", default=None, choices=["auto", "mfma"], help="HipLinear.cs64_impl for the whole run (TTT-Linear at mini-batches of 64)")
    ap.add_argument("--tuning-file", default=None, help="GEMM solution selections to load instead of the committed ttt_amd/infra/gemm_tuning_gfx950.csv")
    ap.add_argument("--debug-option", action="append", default=[], metavar="NAME=VALUE", help="library debug option(s) for the whole run (e.g. scan_pair=0)")
    a = ap.parse_args()
    import test_time_training as ext
    from bench import TEXT_LEN, TOKENS_PER_FRAME
    from ttt_amd.infra.parallelisms import enable_tuned_gemms
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm.ttt_layer import TTTWrapper
    ext.load_library()
    for kv in a.debug_option:
        ext.debug_option(kv.split("=")[0], int(kv.split("=")[1]))
    dev = torch.device("cuda:0")
    tuned = enable_tuned_gemms(a.tuning_file)
    linear = a.ssm == "ttt_linear"
    if a.mini_batch == 16 and not a.no_grad and not linear:
        ap.error("--mini-batch 16 needs --no-grad")
    from ttt_amd.models.ssm.linear_hip import HipLinear
    if a.cs64_impl is not None:
        HipLinear.cs64_impl = a.cs64_impl
    over = {"mini_batch_size": 16} if a.mini_batch == 16 else {}
    if a.mini_batch == 16 and a.no_grad:
        over["scan_checkpoint_group_size"] = 10 ** 6          # the evaluation settings: no scan checkpoints
    cfg = ModelConfig.get_preset("5B", a.video_length, ssm_layer=a.ssm, adapter_method="qkvo", **over)
    frames, tl = cfg.compressed_num_frames, TEXT_LEN[a.video_length]
    scenes = max((frames - 1) // 12, 1)
    n_vid = frames * TOKENS_PER_FRAME
    L = n_vid + scenes * tl
    torch.manual_seed(0)
    layer = TTTWrapper(cfg).to(dev).to(torch.bfloat16)
    layer.ttt.init_weights()
    layer.init_freqs()
    meta = SequenceMetadata(text_length=tl, seq_text_length=tl * scenes, num_frames=frames, num_chunks=scenes, tokens_per_frame=TOKENS_PER_FRAME,
                            latent_height=60, latent_width=90, t_emb=None)
    if meta.is_multiscene:
        meta.init_multiscene_offsets()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(a.batch, L, cfg.model_dim, device=dev, generator=g).bfloat16().requires_grad_(not a.no_grad)
    dy = torch.randn(a.batch, L, cfg.model_dim, device=dev, generator=g).bfloat16() * 0.1
    params = [p for p in layer.parameters() if p.requires_grad]
    # a variant: a number of parts or "default", with "+pair" behind it = TTTBase.cs16_scan_pair on for that variant (CS = 16)
    # ... or "+split" = HipLinear.cs16_scan_split on for that variant (TTT-Linear, CS = 16)
    parts = [v if (v == "default" or v.endswith("+pair") or v.endswith("+split")) else int(v) for v in a.parts.split(",")]
    res = {"L": L, "batch": a.batch, "mini_batch": a.mini_batch, "ssm": a.ssm, "tuned_gemms": bool(tuned), "by_parts": {}}
    if linear:
        res["cs64_impl"] = HipLinear.cs64_impl
    default_plan = (layer.ttt.pipeline_parts, layer.ttt.pipeline_parts_auto)
    default_linear = layer.ttt.linear_pipeline_parts

    def set_parts(n):
        from ttt_amd.models.ssm.ttt_layer import TTTBase
        pair = isinstance(n, str) and n.endswith("+pair")
        TTTBase.cs16_scan_pair = int(pair)
        if pair:
            n = n[:-5] if n[:-5] == "default" else int(n[:-5])
        split = isinstance(n, str) and n.endswith("+split")
        HipLinear.cs16_scan_split = int(split)
        if split:
            n = n[:-6] if n[:-6] == "default" else int(n[:-6])
        if linear:
            layer.ttt.linear_pipeline_parts = default_linear if n == "default" else n
        elif n == "default":
            layer.ttt.pipeline_parts, layer.ttt.pipeline_parts_auto = default_plan
        else:
            layer.ttt.pipeline_parts = n
            layer.ttt.pipeline_parts_auto = default_plan[1] and a.mini_batch == 64      # (CS = 64: "at least n", as always)

    def fwd(n, reverse):
        set_parts(n)
        with torch.no_grad():
            return layer(x, meta, reverse)

    def fwd_bwd(n, reverse):
        set_parts(n)
        y = layer(x, meta, reverse)
        return y, torch.autograd.grad(y, [x] + params, dy)

    if a.scan_only:
        return scan_only(a, ext, layer, meta, x, L, parts, set_parts, res)
    if a.no_grad:
        t = {n: {"fwd": [], "fwd_rev": []} for n in parts}
        for _ in range(a.rounds):
            for n in parts:
                t[n]["fwd"].append(timeit(lambda: fwd(n, False)))
                t[n]["fwd_rev"].append(timeit(lambda: fwd(n, True)))
        rl2 = lambda p, q: float((p.double() - q.double()).norm() / q.double().norm().clamp_min(1e-30))
        ref = {rev: fwd(parts[0], rev) for rev in (False, True)}
        for n in parts:
            ent = {"median_ms": {k: sorted(v)[len(v) // 2] for k, v in t[n].items()}, "runs_ms": {k: [round(u, 3) for u in v] for k, v in t[n].items()}}
            set_parts(n)
            with torch.no_grad():
                plan = layer.ttt._pipeline_plan(x, meta, L, False, False)
            ent["part_steps"] = None if plan is None else [p[1] for p in plan]
            if n != parts[0]:
                for rev in (False, True):
                    y = fwd(n, rev)
                    ent["reverse" if rev else "forward"] = {"out_equal": bool(torch.equal(y, ref[rev])), "out_rel_l2": rl2(y, ref[rev])}
            res["by_parts"][str(n)] = ent
        print(json.dumps(res))
        return

    t = {n: {"fwd": [], "fwd_rev": [], "fwd_bwd": []} for n in parts}
    for _ in range(a.rounds):
        for n in parts:
            t[n]["fwd"].append(timeit(lambda: fwd(n, False)))
            t[n]["fwd_rev"].append(timeit(lambda: fwd(n, True)))
            t[n]["fwd_bwd"].append(timeit(lambda: fwd_bwd(n, False)))
    ref = {rev: fwd_bwd(parts[0], rev) for rev in (False, True)}
    rl2 = lambda p, q: float((p.double() - q.double()).norm() / q.double().norm().clamp_min(1e-30))
    for n in parts:
        med = {k: sorted(v)[len(v) // 2] for k, v in t[n].items()}
        ent = {"median_ms": med}
        set_parts(n)
        plan = layer.ttt._pipeline_plan(x, meta, L, False, False)
        ent["part_steps"] = None if plan is None else [p[1] for p in plan]
        if n != parts[0]:
            for rev in (False, True):
                y, gr = fwd_bwd(n, rev)
                y0, gr0 = ref[rev]
                ent["reverse" if rev else "forward"] = {"out_equal": bool(torch.equal(y, y0)), "out_rel_l2": rl2(y, y0),
                                                        "grads_equal": bool(all(torch.equal(p, q) for p, q in zip(gr, gr0))),
                                                        "grads_worst_rel_l2": max(rl2(p, q) for p, q in zip(gr, gr0))}
        res["by_parts"][str(n)] = ent
    print(json.dumps(res))


if __name__ == "__main__":
    main()
