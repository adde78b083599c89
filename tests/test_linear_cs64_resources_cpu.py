"""Register / scratch budget of the TTT-Linear kernels at mini-batches of 64 (csrc/ttt_lin64_body.h in csrc/ttt_mfma16.hip;
cross-compiled for gfx950, no GPU needed).  Four waves per workgroup, one per SIMD, so a lane may use up to 512 registers; both
kernels are written to stay out of scratch memory (opaque per-step lane indices, the whole-state operand fragments taken from LDS /
the caller's scratch instead of being carried), and the compiler gives both no spill at all - pinned here."""
from test_kernel_resources_cpu import kernel_resources


def _kernel(res, name):
    ks = [v for k, v in res.items() if name in k]
    assert len(ks) == 1, list(res)
    return ks[0]


def test_forward_kernel_does_not_spill():
    v = _kernel(kernel_resources("ttt_mfma16.hip"), "linear_fwd_cs64_kernel")
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 512, v


def test_backward_kernel_does_not_spill():
    """measured on the shipped code: 484 registers, 0 spilled dwords, no private segment"""
    v = _kernel(kernel_resources("ttt_mfma16.hip"), "linear_bwd_cs64_kernel")
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 512, v

