"""Inputs and metrics shared by the attention oracle tests (tests/test_attention_oracle_cpu.py, tests/test_attention_oracle_gpu.py):
q / k in the model's value range (the per-head LayerNorm with weight ~ 1 + 0.3 randn in front of the attention), the value
regimes of the online softmax, and the metrics of ATTN_TOL on [B, NH, S, 64] results."""
import math

import torch

from helpers import bf16_ulp

SCALE = 1.0 / math.sqrt(64)


def model_qk(B, NH, S, g, dtype=torch.float32):
    """bf16-valued q, k [B, NH, S, 64] as the pre kernel leaves them: LayerNorm(64) rows times w ~ 1 + 0.3 randn plus b ~ 0.1 randn
    per head (peaked scores: a few keys of a row stand out); ``g`` a generator on the device the tensors are made on"""
    dev = g.device
    def one():
        x = torch.randn(B, NH, S, 64, generator=g, dtype=torch.float64, device=dev)
        x = (x - x.mean(-1, keepdim=True)) / x.std(-1, unbiased=False, keepdim=True)
        w = 1 + 0.3 * torch.randn(NH, 1, 64, generator=g, dtype=torch.float64, device=dev)
        b = 0.1 * torch.randn(NH, 1, 64, generator=g, dtype=torch.float64, device=dev)
        return (x * w + b).bfloat16().to(dtype)
    return one(), one()


def model_case(B, NH, S, seed, dtype=torch.float32, device="cpu"):
    """q, k (model_qk), v, dO [B, NH, S, 64], bf16 values"""
    g = torch.Generator(device=device).manual_seed(seed)
    q, k = model_qk(B, NH, S, g, dtype)
    v, do = (torch.randn(B, NH, S, 64, generator=g, device=device).bfloat16().to(dtype) for _ in range(2))
    return q, k, v, do


def large_lse_case(B, NH, S, seed, lse=1000.0, dtype=torch.float32):
    """scores offset by ~ +-lse / scale: q = a u + n_q, k = +-a u + n_k with the noise orthogonal to a shared direction u, so
    every score is a^2 |u|^2 plus a spread of a few units and |LSE| ~ lse (heads alternate the sign) - the regime where the
    dK / dV kernel's accumulator, started from -LSE / scale in fp32, carries the fewest fraction bits"""
    g = torch.Generator().manual_seed(seed)
    u = torch.ones(64, dtype=torch.float64)                                     # |u|^2 = 64
    a = math.sqrt(lse / SCALE / 64)
    sign = torch.tensor([1.0 if h % 2 == 0 else -1.0 for h in range(NH)], dtype=torch.float64).view(1, NH, 1, 1)
    noise = lambda: (lambda n: n - n.mean(-1, keepdim=True))(1.2 * torch.randn(B, NH, S, 64, generator=g, dtype=torch.float64))
    q = (a * u + noise()).bfloat16().to(dtype)
    k = (sign * a * u + noise()).bfloat16().to(dtype)
    v, do = (torch.randn(B, NH, S, 64, generator=g).bfloat16().to(dtype) for _ in range(2))
    return q, k, v, do


def delta_err(a, b, o, do):
    """largest |Delta - Delta_ref| over a row's sum of |O dO| (the scale of its rounding; a row's Delta can cancel to 0)"""
    den = (o.double() * do.double()).abs().sum(-1).clamp_min(1e-30)
    return float(((a.double() - b.double()).abs() / den).max())


def out_metrics(a, b64, floor=0.125):
    """(ulp fraction, max ulp, worst row) of a bf16 [..., 64] result against the fp64 statement, on the statement's device: the
    metrics of helpers.ulp_stats (ulps at no less than ``floor`` times the reference's RMS) and helpers.row_rel_err with every
    leading index a row, against the bf16-rounded statement"""
    b = b64.double()
    a = a.to(b.device).double()
    u = bf16_ulp(b.abs().clamp_min(floor * float(b.square().mean().sqrt())))
    d = (a - b).abs() / u
    ar, br = a.bfloat16().double(), b.bfloat16().double()
    diff, ref = (ar - br).norm(dim=-1), br.norm(dim=-1)
    return float((d > 1.0).double().mean()), float(d.max()), float((diff / ref.clamp_min(1e-30)).where(ref > 0, diff).max())


def pre_case(B, S, NH, n_text, seed, dtype=torch.float32):
    """raw q / k projections [B, S, NH*64] (bf16 values, q with an offset), LayerNorm parameters [64] (fp32, as AttnPre passes
    them), the module's RoPE tables with one row more than the video needs (cos, sin [S - n_text + 1, 64] fp32) and bf16 output
    gradients dq, dk [B, S, NH, 64]"""
    from ttt_amd.models.cogvideo.utils import Rotary3DPositionEmbedding
    g = torch.Generator().manual_seed(seed)
    d = {"q_raw": (torch.randn(B, S, NH * 64, generator=g) * 2 + 0.3).bfloat16().to(dtype),
         "k_raw": (torch.randn(B, S, NH * 64, generator=g) * 0.5).bfloat16().to(dtype)}
    for n, s in (("wq", 1.0), ("bq", 0.0), ("wk", 1.0), ("bk", 0.0)):
        d[n] = (s + 0.3 * torch.randn(64, generator=g)).bfloat16().to(dtype)
    n = S - n_text + 1
    frames = (n + 15) // 16
    rot = Rotary3DPositionEmbedding(4, 4, frames, 64)
    d["cos"], d["sin"] = (t[:n].to(dtype).contiguous() for t in (rot.freqs_cos, rot.freqs_sin))
    d["dq"], d["dk"] = (torch.randn(B, S, NH, 64, generator=g).bfloat16().to(dtype) for _ in range(2))
    return d


PRE_PARAMS = ("wq", "bq", "wk", "bk")
# ulps of the pre kernel's outputs are taken at no less than the RMS (as test_glue_oracle_cpu.py does for rotated rows): the two
# products of the rotation are rounded at the magnitude of y, so where they cancel the output carries their rounding flips, and a
# 1-ulp flip of y from the fp32 LayerNorm becomes several ulps of a small output
PRE_FLOOR = 1.0
PRE_OUTS = ("q", "k", "dq_raw", "dk_raw")


def cancel_err(a, b64, mag):
    """rel-L2 of the error of dQ / dK against the size of the terms they sum (bwd(..., mags=True)): the metric of the regimes where
    those terms cancel and the result is (near) 0"""
    b = b64.double()
    return float((a.to(b.device).double() - b).norm() / mag.double().norm().clamp_min(1e-30))


def pre_oracle(d, NH, n_text, dtype=torch.float64, **kw):
    """forward and gradients of oracle.attn_oracle.pre on the inputs of pre_case, in ``dtype``:
    {"q", "k" [B, S, NH, 64], "dq_raw", "dk_raw" [B, S, NH, 64], "wq", "bq", "wk", "bk" [64]}"""
    from oracle import attn_oracle as AO
    x = {n: d[n].to(dtype).detach().requires_grad_(n in ("q_raw", "k_raw") + PRE_PARAMS) for n in d}
    q, k = AO.pre(x["q_raw"], x["k_raw"], x["wq"], x["bq"], x["wk"], x["bk"], x["cos"], x["sin"], NH, n_text, **kw)
    grads = torch.autograd.grad((q, k), [x[n] for n in ("q_raw", "k_raw") + PRE_PARAMS], (x["dq"], x["dk"]))
    B, S, _ = d["q_raw"].shape
    r = {"q": q.detach(), "k": k.detach(), "dq_raw": grads[0].view(B, S, NH, 64), "dk_raw": grads[1].view(B, S, NH, 64)}
    r.update(zip(PRE_PARAMS, grads[2:]))
    return r
