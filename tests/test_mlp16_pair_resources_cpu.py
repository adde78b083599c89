"""Register / scratch budget of the TTT-MLP forward scan at mini-batches of 16 in pair form (csrc/ttt_mfma16.hip: mlp_pair16_kernel,
eight waves per workgroup = two per SIMD = 256 registers per lane; cross-compiled for gfx950, no GPU needed), and the names the older
resource tests select by substring.  (Its LDS maps: tests/test_emul_mlp16_pair_cpu.py::test_lds_maps_fit.)"""
import pytest

from test_kernel_resources_cpu import kernel_resources


@pytest.fixture(scope="module")
def res():
    return kernel_resources("ttt_mfma16.hip")


def test_mlp_pair16_kernel_budget(res):
    """no spill, no private segment, at most 256 registers per lane - both roles are branches of the one kernel, so the figure is the
    larger role's"""
    ks = [v for k, v in res.items() if "mlp_pair16_kernel" in k]
    assert len(ks) == 1, list(res)
    v = ks[0]
    print("mlp_pair16_kernel", v)
    assert v["vgpr_count"] <= 256, v
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v


def test_new_name_leaves_the_older_kernels_selectable(res):
    """the resource tests select by name substring and want exactly one match"""
    for old in ("linear_bwd_cs64_kernel", "linear_fwd_cs64_kernel", "linear_bwd16_kernel", "linear_scan16_kernel", "mlp_scan16_body_kernel",
                "linear_recompute16_groups_kernel", "linear_sweep16_groups_kernel", "linear_recompute_cs64_groups_kernel",
                "linear_sweep_cs64_groups_kernel", "mlp_bwd16_kernel", "mlp_scan16", "mlp_pair16"):
        assert sum(old in k for k in res) == 1, (old, list(res))
