"""Register / scratch budget of the two kernels of the TTT-MLP backward in parts at mini-batches of 16 (csrc/ttt_mfma16.hip:
mlp_recompute16_groups_kernel, mlp_sweep16_groups_kernel; eight waves per workgroup = two per SIMD = 256 registers per lane;
cross-compiled for gfx950, no GPU needed), and the names the older resource tests select by substring."""
import pytest

from test_kernel_resources_cpu import kernel_resources

NEW = ("mlp_recompute16_groups_kernel", "mlp_sweep16_groups_kernel")
OLDER = ("linear_bwd_cs64_kernel", "linear_fwd_cs64_kernel", "linear_bwd16_kernel", "linear_scan16_kernel", "mlp_scan16_body_kernel",
         "linear_recompute16_groups_kernel", "linear_sweep16_groups_kernel", "linear_recompute_cs64_groups_kernel",
         "linear_sweep_cs64_groups_kernel", "mlp_bwd16_kernel")


@pytest.fixture(scope="module")
def res():
    return kernel_resources("ttt_mfma16.hip")


@pytest.mark.parametrize("name", NEW)
def test_part_kernels_fit_the_register_file_without_scratch(res, name):
    """measured on the shipped code: the recompute 170 registers, the walk 255 (as the one-call kernel, whose walk it is); neither
    spills, neither has a private segment"""
    ks = [v for k, v in res.items() if name in k]
    assert len(ks) == 1, list(res)
    v = ks[0]
    print(name, v)
    assert v["vgpr_count"] <= 256, v
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v


def test_new_names_leave_the_older_kernels_selectable(res):
    """the resource tests select by name substring and want exactly one match"""
    for old in OLDER:
        assert sum(old in k for k in res) == 1, (old, list(res))
    assert sum("mlp_scan16" in k for k in res) == 1 and sum("mlp_bwd16_kernel" in k for k in res) == 1
