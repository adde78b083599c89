"""Optional (None) arguments of the glue and attention wrappers reach the C ABI as null pointers through the prototypes that
``test_time_training.load_library()`` applies (-m gpu): each call with None is bit-identical to the call that spells the default
out.  B = 1, NH = 2, L = 128, F = 64, bf16, seeded inputs, every output buffer NaN-filled before its call; no tolerance."""
import pytest
import torch

import glue_cases as C
from helpers import glue_maps, scene_meta

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
B, NH, L, F = 1, 2, 128, 64
D = NH * F


def nanbuf(*shape, dtype=BF):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def test_none_arguments_are_the_spelled_out_defaults():
    import test_time_training as e
    e.load_library()
    _, _, pos, rope = glue_maps(scene_meta(32, 1, 6, 4, 4))            # 32 text tokens + 6 frames of 4 x 4 = 128
    assert pos.numel() == L
    rope, pos = rope.to(DEV), pos.to(DEV)
    ident = torch.arange(L, dtype=torch.int32, device=DEV)
    d = {k: v.to(DEV) for k, v in C.pre_case(B, L, NH, seed=21).items()}

    # pre_forward: no table, no maps = identity permutation, every token a text token (position -1: not rotated)
    none, full = [nanbuf(B, NH, L, F) for _ in range(3)], [nanbuf(B, NH, L, F) for _ in range(3)]
    e.pre_forward(d["q"], d["k"], d["v"], None, None, None, d["ln_w"], d["ln_b"], *none, NH)
    e.pre_forward(d["q"], d["k"], d["v"], rope, ident, torch.full_like(ident, -1), d["ln_w"], d["ln_b"], *full, NH)
    for a, b in zip(none, full):
        assert not torch.isnan(a.float()).any() and torch.equal(a, b)

    # post_forward: no map = identity permutation
    pc = {k: v.to(DEV) for k, v in C.post_case(B, L, NH, seed=22).items()}
    none, full = nanbuf(B, L, D), nanbuf(B, L, D)
    e.post_forward(pc["Y"], None, pc["w"], pc["b"], none, 1e-6)
    e.post_forward(pc["Y"], ident, pc["w"], pc["b"], full, 1e-6)
    assert not torch.isnan(none.float()).any() and torch.equal(none, full)

    # attn_forward: the log-sum-exp output is optional
    g = torch.Generator().manual_seed(23)
    q, k, v = (torch.randn(B, NH, L, F, generator=g).bfloat16().to(DEV) for _ in range(3))
    none, full, lse = nanbuf(B, NH, L, F), nanbuf(B, NH, L, F), nanbuf(B, NH, L, dtype=torch.float32)
    e.attn_forward(q, k, v, none, None, F ** -0.5)
    e.attn_forward(q, k, v, full, lse, F ** -0.5)
    assert not torch.isnan(none.float()).any() and not torch.isnan(lse).any() and torch.equal(none, full)

    # pre_backward: ld_out None = contiguous raw gradients (row stride D); 3 D = the column blocks of one [B, L, 3 D] buffer
    P = e.pre_backward_partials(NH)
    res = []
    for ld in (None, 3 * D):
        buf = nanbuf(B, L, 3 * D)
        raw = [nanbuf(B, L, D) for _ in range(3)] if ld is None else [buf[..., i * D:(i + 1) * D] for i in range(3)]
        part = [nanbuf(P, D, dtype=torch.float32) for _ in range(2)]
        e.pre_backward(d["q"], d["k"], d["v"], rope, ident, pos, d["ln_w"], d["dXQ"], d["dXK"], d["dXV"], *raw, *part, NH, ld_out=ld)
        res.append([t.clone() for t in raw + part])
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert not torch.isnan(a.float()).any() and torch.equal(a, b)
