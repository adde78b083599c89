"""The TTT-MLP backward at mini-batches of 16 over RANGES of checkpoint groups (csrc/ttt_mlp16_bwd_body.h: ``recompute_groups`` re-runs
the groups [k0, k0 + nk) from their checkpoints into a slot workspace, one eight-wave workgroup per (b, h, group); ``sweep_groups``
walks them in reverse from a carried gradient state, one workgroup per (b, h)) on the wave emulator of tests/emul, its LDS race
detector on.  However the K groups are cut into ranges, the ten gradients are the BITS of the emulated one-call ``backward()``: both
run ``recompute_group`` / ``sweep_group``, and the slots hold what the one call keeps in the *_init_group buffers.  The same bodies are
instantiated with the device backend in csrc/ttt_mfma16.hip (mlp_recompute16_groups_kernel, mlp_sweep16_groups_kernel).  The one-call
body is held to the fp64 oracle by tests/test_emul_mlp16_bwd_cpu.py; bit equality gives the parts that bound."""
import os

import pytest
import torch

import mlp16_bwd_cases as M
import mlp16_bwd_parts_cases as P
import scan_cases as C


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(C.CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    return M.build_emul(), P.build_emul()


_CASES = {}


def _case(one, NC, G):
    """the chain case, the emulated forward's checkpoints at G and at 1, a non-zero upstream state gradient and the emulated one-call
    backward - made once per shape and left unchanged"""
    if (NC, G) not in _CASES:
        seed = 500 + NC
        c = M.case(M.CHAIN_B, M.CHAIN_NH, NC, seed)
        t = M.host_tensors(c)
        _, cks = M.emul_forward(one, t, G)
        _, cks1 = M.emul_forward(one, t, 1) if G > 1 else (None, cks)
        up = M.upstream(c, cks, G, seed)
        assert all(float(u.abs().max()) > 0 for u in up)
        ref, scr = M.emul_run(one)(t, cks, up, G)
        assert not any(torch.isnan(ref[k].float()).any() for k in M.GRADS)
        _CASES[NC, G] = (t, cks, cks1, up, ref, scr)
    return _CASES[NC, G]


@pytest.mark.parametrize("NC,G", M.CHAIN)
def test_every_cutting_gives_the_one_call_bits(emul, NC, G):
    """(NC, G) = (11, 4): a ragged last group of 3; (7, 3): of 1; (3, 1): one step per group - at B = 2, NH = 3, K = 3 each.  Every
    cutting of the K groups into ranges - (3), (1, 2), (2, 1), (1, 1, 1): one range, all ones, the ragged last group alone - gives
    ``torch.equal`` with the emulated one-call backward in all ten gradients, from a non-zero upstream; slot workspaces and carry start
    as NaN between NaN guards that stay NaN; the slots hold the bits of the checkpoints of a forward with G = 1 (and so the bits the
    one call leaves in *_init_group), slots a ragged group does not use stay NaN; inputs and checkpoints come back unchanged; no LDS
    race in either body."""
    one, parts = emul
    t, cks, cks1, up, ref, scr = _case(one, NC, G)
    K = -(-NC // G)
    cuts_all = P.cuttings(K)
    assert len(cuts_all) == 2 ** (K - 1) and (K,) in cuts_all and (1,) * K in cuts_all and (K - 1, 1) in cuts_all
    for cuts in cuts_all:
        g, spaces, carry = P.emul_walk(parts)(t, cks, up, G, cuts)
        for name in M.GRADS:
            assert torch.equal(g[name], ref[name]), (cuts, name)
        assert not torch.isnan(carry).any(), cuts
        P.check_slots(f"emulated parts {cuts}", spaces, P.ranges(K, cuts), cks1, M.CHAIN_B, M.CHAIN_NH, NC, G)
    # what the one call left in the *_init_group buffers: the slots of group 0, which it recomputed last
    n0 = P.group_steps(NC, G, 0)
    f = P.slot_fields(spaces[-1], M.CHAIN_B, M.CHAIN_NH, P.ranges(K, cuts)[-1][1], G)
    for name, a, b in zip(("W1", "b1", "W2", "b2"), f, scr):
        assert torch.equal(a[:, :, 0, :n0], b[:, :, :n0]), name

