"""Register / scratch budget of the two kernels of the third stage of the TTT-Linear backward in parts (csrc/ttt_mfma16.hip: the
carry-free half of every reverse step of a range, one wave per step, and the walk that consumes its records, one wave per (b, h);
cross-compiled for gfx950, no GPU needed).  A lane may use up to 512 registers; neither may touch scratch memory."""
import pytest

from test_kernel_resources_cpu import kernel_resources

KERNELS = ("linear_front16_groups_kernel", "linear_chain16_groups_kernel")
OLDER = ("linear_bwd_cs64_kernel", "linear_fwd_cs64_kernel", "linear_bwd16_kernel", "linear_scan16_kernel",
         "linear_recompute16_groups_kernel", "linear_sweep16_groups_kernel", "linear_recompute_cs64_groups_kernel",
         "linear_sweep_cs64_groups_kernel")


@pytest.fixture(scope="module")
def res():
    return kernel_resources("ttt_mfma16.hip")


@pytest.mark.parametrize("name", KERNELS)
def test_front_kernel_does_not_spill(res, name):
    ks = [v for k, v in res.items() if name in k]
    assert len(ks) == 1, list(res)
    v = ks[0]
    print(name, v)
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 512, v


def test_new_names_leave_the_older_kernels_selectable(res):
    """the resource tests of the older TTT-Linear kernels select by name substring and want exactly one match"""
    for old in OLDER:
        assert sum(old in k for k in res) == 1, (old, list(res))
