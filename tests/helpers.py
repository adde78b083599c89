"""Shared test helpers (golden loading, error metrics)."""
import os

import torch

from oracle import ttt_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return torch.load(os.path.join(GOLDEN, name), weights_only=False)


def op_inputs(g):
    """Regenerate the seeded inputs of an op-level golden and verify their checksums."""
    dtype = getattr(torch, g["dtype"])
    d = O.make_inputs(dtype=dtype, **g["gen"])
    for k, ref in g["input_checksums"].items():
        got = float(d[k].double().abs().sum())
        assert abs(got - ref) <= 1e-9 * max(1.0, abs(ref)), f"input RNG drift in {k}: {got} vs {ref}"
    return d


def rel_l2(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def max_abs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def row_rel_err(a, b, row_dims):
    """Worst rel-L2 over rows: ``row_dims`` are the dims that index a row (e.g. (0, 1, 2) of [B, L, NH, F]: one (batch, token,
    head)); the rest make up the row.  A tensor-wide rel-L2 hides one wrong token: at 18 048 tokens an entirely wrong token adds
    about 7e-3.  Rows whose reference is zero count their absolute error."""
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    rest = [d for d in range(b.dim()) if d not in row_dims]
    perm = list(row_dims) + rest
    n = 1
    for d in row_dims:
        n *= b.shape[d]
    diff = (a - b).permute(perm).reshape(n, -1).norm(dim=1)
    ref = b.permute(perm).reshape(n, -1).norm(dim=1)
    return float((diff / ref.clamp_min(1e-30)).where(ref > 0, diff).max())


def bf16_ulp(x):
    """spacing of bf16 numbers at |x| (x fp64): 2^(e - 7) for |x| in [2^e, 2^(e+1))"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-38))) - 7)


def ulp_stats(a, b64, floor=None):
    """(fraction of elements more than 1 bf16 ulp from the fp64 reference, largest distance in bf16 ulps).  The ulp is taken at
    max(|b|, floor): ``floor`` (default 1/8 of the reference's RMS) keeps results of cancellation near zero from counting
    thousands of ulps for an absolute error at the level of the row's own rounding."""
    a = a.detach().double().cpu(); b = b64.detach().double().cpu()
    if floor is None:
        floor = 0.125 * float(b.square().mean().sqrt())
    u = bf16_ulp(b.abs().clamp_min(floor))
    d = (a - b).abs() / u
    return float((d > 1.0).double().mean()), float(d.max())


# Tolerances of the glue kernels against oracle/glue_oracle.py (tests/test_prepost_oracle_gpu.py), fixed by the sensitivity table
# of tests/test_glue_oracle_cpu.py: each sits >= 10x above the oracle's own fp32-vs-fp64 distance and >= 10x below the nearest
# mutation it must catch.
GLUE_TOL = {
    "ulp_frac": 1e-3,     # fraction of bf16 outputs more than 1 ulp from fp64
    "ulp_max": 64.0,      # largest distance in ulps (floor: 1/8 of the reference's RMS): one wild element
    "row": 2e-2,          # worst rel-L2 of one (batch, token, head) / (batch, token) row against the bf16-rounded reference
    "psum": 1e-4,         # rel-L2 of an fp32 parameter gradient summed from the kernels' partials (AdaLN's d scale sums the
}                         # bf16-rounded LN output: its rounding flips put the kernel at 2e-5)

# Tolerances of the segment-attention kernels against oracle/attn_oracle.py (tests/test_attention_oracle_gpu.py), fixed by the
# sensitivity table of tests/test_attention_oracle_cpu.py in the same way: >= 10x the oracle's own fp32-vs-fp64 distance, >= 10x
# below every mutation the table marks as one the metric must catch.
ATTN_TOL = {
    "ulp_frac": 2e-3,     # fraction of bf16 outputs (O, dQ, dK, dV, q, k, dq_raw, dk_raw) more than 1 ulp from the statement
    "ulp_max": 64.0,      # largest distance in ulps (floor: 1/8 of the reference's RMS)
    "row": 3e-2,          # worst rel-L2 of one (batch, head, token) row against the bf16-rounded statement
    "lse": 5e-5,          # largest |LSE - LSE_ref| (natural-log units)
    "delta": 1e-6,        # largest |Delta - Delta_ref| / sum |O dO| of the row
    "psum": 2e-5,         # rel-L2 of a LayerNorm parameter gradient summed (fp64) from the pre kernel's [P, 4, 64] partials
    "cancel": 1e-3,       # rel-L2 of the dQ / dK error against the size of the terms they sum (attn_cases.cancel_err): the regimes
}                         # where those terms cancel (a saturated softmax, equal keys, |LSE| ~ 1e3, S = 1)
# Scores offset by |LSE| ~ 1e3 (attn_cases.large_lse_case): fp32 keeps ~1e-4 raw-score units of such a score, and the dK / dV
# kernel starts its accumulator from -LSE / scale; dQ = sum dS K cancels the shared key direction.  The table's fp32 row for that
# regime sets these (the other metrics as ATTN_TOL).
ATTN_TOL_LARGE = dict(ATTN_TOL, ulp_frac=5e-3, row=5e-2, lse=5e-4)

# Tolerances of ONE STEP of the forward TTT scans against oracle/ttt_oracle.py, stepped from the scan's own checkpoints
# (tests/scan_cases.py: the metrics; tests/test_scan_oracle_gpu.py), fixed by the sensitivity table of
# tests/test_scan_oracle_cpu.py: each >= 2x the larger of the oracle's rounding model (mlp_step_rounded / lin_step_rounded, worst
# over the cases of the GPU file) and the kernels' worst value measured on an MI355X (SCAN_MEASURED), each <= 1/3 of the nearest
# mutation its metric must catch.
#   metric       rounding model   MI355X    threshold   nearest must-catch mutation (its distance)
#   delta        3.6e-3           3.5e-3    1e-2        LayerNorm epsilon 1e-6, TTT-MLP only (3.7e-2); unbiased inner variance (5.0e-2)
#   delta_block  6.2e-3           6.2e-3    1.5e-2      update x 1.05 in one 32-wide block (5.0e-2)
#   row          5.5e-3           5.1e-3    2e-2        Q of step i + 1 in the output path (2.1e-1)
#   ulp_frac     0.094            0.093     0.25        none of its own (unbiased output variance: 0.75)
#   ulp_max      13.3             13.3      32          none of its own
#   gain         7.9e-4           5.5e-4    2.5e-3      unbiased output variance (7.9e-3)
# Not separated by any metric, reported by the table: erf GELU in place of tanh GELU (delta 5e-7: |Z1| << 1 on these inputs) and,
# for TTT-Linear, epsilon 1e-6 (delta 4e-3 .. 6e-3).
SCAN_TOL = {
    "delta": 1e-2,          # worst rel-L2 of one (b, h, step) state delta, each of W1, b1, W2, b2
    "delta_block": 1.5e-2,  # the same of one 32-wide block of the hidden units / the features: the slice of one wave
    "row": 2e-2,            # worst rel-L2 of one (b, h, step, token) output row against the bf16-rounded oracle
    "ulp_frac": 0.25,       # fraction of outputs more than 1 bf16 ulp from the fp64 step (floor: 1/8 of the RMS)
    "ulp_max": 32.0,        # largest distance in ulps
    "gain": 2.5e-3,         # worst |least-squares gain - 1| of the output's LayerNorm part of one (b, h, step)
}
# The generic kernels: fp32 arithmetic, only the output store rounds (to bf16; nothing with fp32 activations).  The table's second
# column; its reference-alone level is the oracle's step in fp32 (delta 1.7e-5: the fp32 spacing of the state against its delta;
# row 1.0e-3, gain 2.5e-4: the bf16 store), the MI355X values are SCAN_MEASURED_GENERIC (row 1.1e-3, gain 3.4e-4).
SCAN_TOL_GENERIC = dict(SCAN_TOL, delta=1e-4, delta_block=1e-4, row=5e-3, ulp_frac=1e-2, ulp_max=2.0, gain=1e-3)
# the kernels' worst values on an MI355X over the cases of test_scan_oracle_gpu.py (profiles/r9_scan_oracle_gpu.log)
SCAN_MEASURED = {"delta": 0.00353, "delta_block": 0.00616, "row": 0.00508, "ulp_frac": 0.0928, "ulp_max": 13.3, "gain": 0.000548}
SCAN_MEASURED_GENERIC = {"delta": 1.36e-05, "delta_block": 1.45e-05, "row": 0.00111, "ulp_frac": 0.0, "ulp_max": 0.5, "gain": 0.000339}

# Tolerances of ONE CALL of the TTT-Linear backward sweeps (one step, or one group: a G-step horizon) against oracle/ttt_oracle.py
# from the same checkpoint and the same nonzero upstream state gradient (tests/scan_bwd_cases.py: the metrics;
# tests/test_scan_bwd_oracle_gpu.py), fixed by the sensitivity table of tests/test_scan_bwd_oracle_cpu.py BEFORE the device ran (the
# device column was filled in afterwards: the kernels round where the model rounds and land on its values to three digits):
# each >= 2x the oracle's rounding model (O.lin_step_bwd_rounded, worst over the cases of the GPU file), each <= 1/3 of the nearest
# mutation its metric must catch (the minimum over mini-batches of 16 and 64, base and high learning rate).
#   metric        rounding model   MI355X    threshold   nearest must-catch mutation (its distance)
#   dstate        2.6e-3           2.6e-3    1e-2        last token left out of the dW1 / db1 update (1.5e-1)
#   dstate_block  3.0e-3           3.0e-3    1.2e-2      increment x 1.05 in one 16-column block (5.0e-2)
#   row           5.4e-3           5.4e-3    2e-2        Q of step i + 1 (1.2e-1); dK without -eta A1 (2.0e-1); dW1_last left out (2.0e-1)
#   deta          2.7e-3           2.7e-3    1e-2        the gZ1 . db1n term dropped (1.0)
#   dln           1.7e-3           1.7e-3    5e-3        the inner LayerNorm's share dropped (1.0)
#   gain          7.6e-4           7.6e-4    2.5e-3      unbiased variance in the output LayerNorm (8.0e-3)
# Reported only: LayerNorm epsilon 1e-6 (dstate 1.5e-2 .. 1.7e-2, row 1.7e-2 .. 2.0e-2): separating it would take a threshold under
# 5e-3, which is under 2x the rounding model.  The unbiased output variance is caught by gain alone (row 1.0e-2 .. 1.4e-2).
SCAN_BWD_TOL = {
    "dstate": 1e-2,         # worst rel-L2 per (b, h) of the increments dW1 - dW1_last, db1 - db1_last
    "dstate_block": 1.2e-2, # the same of one 16-column block of the increment
    "row": 2e-2,            # worst rel-L2 of one (b, h, step, token) row of dXQ, dXK, dXV against the bf16-rounded oracle
    "deta": 1e-2,           # worst rel-L2 per (b, h, step) of d eta
    "dln": 5e-3,            # worst rel-L2 per (b, h) of dln_w, dln_b
    "gain": 2.5e-3,         # worst |least-squares gain - 1| of dXQ - dOut of one (b, h, step)
}
# The generic kernel: fp32 arithmetic, only the stores of dXQ, dXK, dXV, d eta round (to bf16; nothing with fp32 activations).  Its
# reference-alone level is the oracle's step in fp32 arithmetic (dstate 7.2e-7, dstate_block 7.9e-7, dln 1.7e-7: fp32 sums of 16 .. 64
# terms; with the bf16 stores row 1.6e-3, d eta 2.1e-3 - one bf16 rounding per element bounds both by 2^-8 = 3.9e-3 -, gain 1.5e-4).
# dln is also the bound on the fp32 add order when dln_w / dln_b of a call are summed from the partials of its one-group calls.
SCAN_BWD_TOL_GENERIC = dict(SCAN_BWD_TOL, dstate=2e-5, dstate_block=2e-5, row=5e-3, deta=5e-3, dln=1e-5, gain=1e-3)
# the kernels' worst values on an MI355X over the cases of test_scan_bwd_oracle_gpu.py (profiles/r14_scan_bwd_oracle_gpu.log)
# (a call over K groups against the chain of its one-group calls: equal bits on all three kernels; dln_w / dln_b within 1.2e-7 of the
# sum of the partials)
SCAN_BWD_MEASURED = {"dstate": 0.00255, "dstate_block": 0.00297, "row": 0.00541, "deta": 0.00265, "dln": 0.00168, "gain": 0.000759}
SCAN_BWD_MEASURED_GENERIC = {"dstate": 7.51e-07, "dstate_block": 8.2e-07, "row": 0.000911, "deta": 0.00213, "dln": 1.81e-07, "gain": 0.000153}


def scene_meta(text_length, num_chunks, num_frames, H, W):
    """SequenceMetadata of ``num_chunks`` scenes of ``text_length`` text tokens over ``num_frames`` H x W latent frames"""
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    meta = SequenceMetadata(text_length=text_length, seq_text_length=num_chunks * text_length, num_frames=num_frames,
                            num_chunks=num_chunks, tokens_per_frame=H * W, latent_height=H, latent_width=W, t_emb=torch.zeros(1))
    if meta.is_multiscene:
        meta.init_multiscene_offsets()
    return meta


def glue_maps(meta, reverse=False):
    """(L, src, pos, rope) of the fused pre / post kernels for ``meta``, from the module's own ``TTTBase._token_maps`` and RoPE
    table (head_dim 64, the video fills every row of the table: its last row is used)"""
    import types
    from ttt_amd.models.ssm.ttt_layer import TTTBase
    from ttt_amd.models.ssm.utils import precompute_freqs_cis_3d
    L = meta.seq_text_length + meta.num_frames * meta.tokens_per_frame
    src, pos, _ = TTTBase._token_maps(types.SimpleNamespace(_perm_cache={}), meta, L, "cpu", reverse)
    rope = precompute_freqs_cis_3d(64, meta.latent_height, meta.latent_width, meta.num_frames, as_real=True)
    return L, src, pos, rope


def tile_states(d, B):
    t = lambda w: torch.tile(w.unsqueeze(0), dims=(B, 1, 1, 1)).contiguous()
    return {k: t(d[k]) for k in ("W1", "b1", "W2", "b2") if k in d}


# ---- the schedule tests without a device: stand-ins for the two streams and their events ----------------------------------------
class FakeStream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append(("wait_stream", self.name, other.name))

    def wait_event(self, ev):
        self.log.append(("wait_event", self.name, ev.n))


def fake_streams(monkeypatch):
    """``torch.cuda.current_stream`` / ``Event`` / ``stream`` and ``pipeline.side_stream`` replaced by stand-ins that write every wait
    and record to a log -> (log, current): the log, and a one-element list with the name of the stream work is being issued on
    ("main" / "side"), for a recording extension to read.  Events are numbered in the order they are made."""
    import contextlib
    from ttt_amd.models.ssm import pipeline
    log, current, n_events = [], ["main"], [0]
    main, side = FakeStream("main", log), FakeStream("side", log)

    class FakeEvent:
        def __init__(self):
            self.n = n_events[0]
            n_events[0] += 1

        def record(self, stream):
            assert stream.name == current[0], "an event is recorded on the stream its work was issued on"
            log.append(("record", stream.name, self.n))

    @contextlib.contextmanager
    def on(stream):
        old, current[0] = current[0], stream.name
        try:
            yield
        finally:
            current[0] = old

    monkeypatch.setattr(pipeline, "side_stream", lambda device: side)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: main)
    monkeypatch.setattr(torch.cuda, "Event", FakeEvent)
    monkeypatch.setattr(torch.cuda, "stream", on)
    return log, current


def count_calls(monkeypatch, e, names):
    """{label: 0} that counts the calls of the extension's entries ``names`` = {label: attribute} (the TTT-Linear backward's: the
    plain ``ttt_linear_backward`` is sent through ``ttt_linear_backward_impl``, so that one label counts every one-call backward)"""
    calls = dict.fromkeys(names, 0)

    def count(label, fn):
        def wrapped(*a):
            calls[label] += 1
            return fn(*a)
        return wrapped

    for label, attr in names.items():
        monkeypatch.setattr(e, attr, count(label, getattr(e, attr)))
    monkeypatch.setattr(e, "ttt_linear_backward", lambda *a: e.ttt_linear_backward_impl(None, *a))
    return calls


class ToyNet(torch.nn.Module):
    """Stand-in for the DiT in sampler tests: nonlinear in x, depends on text and timestep, independent per sample."""

    def forward(self, x, text, t):
        g = torch.tanh(text.float().mean(dim=(1, 2, 3))).view(-1, 1, 1, 1, 1)
        tt = torch.sin(t.float() / 100).view(-1, 1, 1, 1, 1)
        xf = x.float()
        return (0.6 * torch.tanh(xf.roll(1, -1)) + 0.3 * g * xf.roll(1, 1) + 0.1 * tt).to(x.dtype)
