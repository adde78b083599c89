"""Register / scratch budget of the four kernels of the TTT-Linear backward in parts (csrc/ttt_mfma16.hip: the recompute and the
reverse walk over a range of checkpoint groups, at mini-batches of 16 - one wave per workgroup - and of 64 - four waves, one per SIMD;
cross-compiled for gfx950, no GPU needed).  A lane may use up to 512 registers in all four; none may touch scratch memory."""
import pytest

from test_kernel_resources_cpu import kernel_resources

KERNELS = ("linear_recompute16_groups_kernel", "linear_sweep16_groups_kernel",
           "linear_recompute_cs64_groups_kernel", "linear_sweep_cs64_groups_kernel")


@pytest.fixture(scope="module")
def res():
    return kernel_resources("ttt_mfma16.hip")


@pytest.mark.parametrize("name", KERNELS)
def test_part_kernel_does_not_spill(res, name):
    """measured on the shipped code: 316 / 506 / 212 / 423 registers, 0 spilled dwords, no private segment"""
    ks = [v for k, v in res.items() if name in k]
    assert len(ks) == 1, list(res)
    v = ks[0]
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 512, v


def test_new_names_leave_the_one_call_kernels_selectable(res):
    """the resource tests of the one-call kernels select by name substring and want exactly one match"""
    for old in ("linear_bwd_cs64_kernel", "linear_fwd_cs64_kernel", "linear_bwd16_kernel", "linear_scan16_kernel"):
        assert sum(old in k for k in res) == 1, (old, list(res))
