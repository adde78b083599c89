"""The TTT-MLP backward at mini-batches of 16 (csrc/ttt_mlp16_bwd_body.h: eight waves per (b, h), group recompute into the caller's
*_init_group buffers, reverse walk) executed on the CPU by the multi-wave emulator of tests/emul, its LDS race detector on: against the
fp64 oracle with a nonzero upstream state gradient, whole tensors and per 32-hidden-unit slice; a call over K groups against K chained
one-group calls (equal bits); the recomputed slots against the forward's own checkpoints (equal bits); the reference-executed golden.
The same template body is instantiated with the device backend in csrc/ttt_mfma16.hip (mlp_bwd16_kernel).  Cases, bounds and seeds:
tests/mlp16_bwd_cases.py."""
import os

import pytest
import torch

import mlp16_bwd_cases as M
import scan_cases as C
from helpers import SCAN_BWD_TOL_GENERIC, load_golden, op_inputs, rel_l2, tile_states
from test_kernels_gpu import check_vs_golden


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(C.CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    return M.build_emul()


_CASES = {}


def _case(lib, B, NH, NC, G, seed):
    """the case, the emulated forward's output and checkpoints, the upstream state gradient - computed once per shape"""
    key = (B, NH, NC, G, seed)
    if key not in _CASES:
        c = M.case(B, NH, NC, seed)
        out, cks = M.emul_forward(lib, M.host_tensors(c), G)
        _CASES[key] = (c, out, cks, M.upstream(c, cks, G, seed))
    return _CASES[key]


@pytest.mark.parametrize("shape", M.SHAPES)
def test_emulated_mlp_cs16_backward_vs_oracle(emul, shape):
    """forward output and checkpoints at 1e-2, the ten gradients at 3e-2 - whole tensors, and dW1 / db1 / dW2 per 32-hidden-unit
    slice - against the fp64 oracle from the kernel's checkpoints with a nonzero upstream (dW1, db1, dW2, db2)_last; outputs start as
    NaN, the scratch lies between NaN guards, inputs and checkpoints come back unchanged, no LDS race.  Measured on the emulator:
    every gradient and every slice between 6e-4 and 3.1e-3 at all five shapes."""
    B, NH, NC, G = shape
    c, out, cks, up = _case(emul, B, NH, NC, G, M.seed_of(shape))
    ro, rc = M.oracle_forward(c, G)
    errs = {"XQW": rel_l2(out, ro), **{f"ck{i}": rel_l2(a, b) for i, (a, b) in enumerate(zip(cks, rc))}}
    print("emulated mlp CS=16 forward", shape, {k: round(v, 5) for k, v in errs.items()})
    assert all(v < M.TOL_OUT for v in errs.values()), errs
    M.check_call(f"emulated mlp CS=16 backward {shape}", M.emul_run(emul), c, cks, up, G)


@pytest.mark.parametrize("NC,G", M.CHAIN)
def test_emulated_whole_call_is_the_chain_of_its_groups(emul, NC, G):
    """a call over K groups and K one-group calls chained through dW1, db1, dW2, db2 from the same checkpoints: equal bits in dXQ, dXK,
    dXV, d eta and the four state gradients (the call parks the state gradient in its outputs between groups, which is what a chain
    does); dln_w / dln_b are the sum of the calls' partials up to an fp32 add order"""
    c, _, cks, up = _case(emul, M.CHAIN_B, M.CHAIN_NH, NC, G, 500 + NC)
    M.check_chain(f"emulated mlp CS=16 chain NC={NC} G={G}", M.emul_run(emul), c, cks, up, G, SCAN_BWD_TOL_GENERIC["dln"])


def test_emulated_recompute_leaves_the_forward_states_in_the_scratch(emul):
    """after a backward with G = 3 over 7 steps the slots of group 0 in the four *_init_group buffers hold the bits a forward of the
    same inputs with G = 1 stored as checkpoints 0, 1, 2: the recompute is the forward's arithmetic, the scratch has the documented
    layout ([B, NH, G, F, H], [B, NH, G, 1, H], [B, NH, G, H, F], [B, NH, G, 1, F])"""
    B, NH, NC, G = 1, 2, 7, 3
    c, _, cks, up = _case(emul, B, NH, NC, G, M.seed_of((B, NH, NC, G)))
    t = M.host_tensors(c)
    _, scr = M.emul_run(emul)(t, cks, up, G)
    _, cks1 = M.emul_forward(emul, t, 1)
    for name, s, k1 in zip(("W1", "b1", "W2", "b2"), scr, cks1):
        assert torch.equal(s[:, :, :G], k1[:, :, :G]), name


def test_emulated_mlp_cs16_vs_reference_golden(emul):
    """against the results of the executed reference (tests/golden/op_mlp_f64_cs16.pt) on its inputs rounded to bf16, at the bounds of
    its CS = 64 sibling (tests/test_kernels_gpu.py::test_mfma_mlp_vs_reference_golden)"""
    gold = load_golden("op_mlp_f64_cs16.pt")
    d = op_inputs(gold)
    B, NH, NC = d["XQ"].shape[:3]
    G = gold["G"]
    bf = lambda x: x.to(torch.bfloat16).contiguous()
    t = dict(XQ=bf(d["XQ"]), XK=bf(d["XK"]), XV=bf(d["XV"]), eta=bf(d["eta"][:, :, :, -1, :, None]), dOut=bf(d["dOut"]),
             ln_w=d["ln_w"].float().contiguous(), ln_b=d["ln_b"].float().contiguous())
    t.update({k: v.float().contiguous() for k, v in tile_states(d, B).items()})
    out, cks = M.emul_forward(emul, t, G)
    up = tuple(torch.zeros(B, NH, *s) for s in M.STATE_SHAPES)
    g, _ = M.emul_run(emul)(t, cks, up, G)
    check_vs_golden(gold, out, g, 1.5e-2, 4e-2)
