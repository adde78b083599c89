"""Register / scratch budget of the two-wave TTT-Linear forward scan at mini-batches of 16 (csrc/ttt_mfma16.hip:
linear_split16_kernel, two waves per workgroup on two SIMDs = up to 512 registers per lane; cross-compiled for gfx950, no GPU needed),
and the names the older resource tests select by substring.  Both roles are branches of the one kernel, so the figures are the larger
role's.  (Its LDS map: tests/test_emul_lin16_split_cpu.py::test_lds_map.)"""
import pytest

from test_kernel_resources_cpu import kernel_resources

OLDER = ("linear_bwd_cs64_kernel", "linear_fwd_cs64_kernel", "linear_bwd16_kernel", "linear_scan16_kernel", "mlp_scan16_body_kernel",
         "linear_recompute16_groups_kernel", "linear_sweep16_groups_kernel", "linear_recompute_cs64_groups_kernel",
         "linear_sweep_cs64_groups_kernel", "linear_front16_groups_kernel", "linear_chain16_groups_kernel", "mlp_bwd16_kernel",
         "mlp_recompute16_groups_kernel", "mlp_sweep16_groups_kernel", "mlp_scan16", "mlp_pair16")


@pytest.fixture(scope="module")
def res():
    return kernel_resources("ttt_mfma16.hip")


def test_linear_split16_kernel_budget(res):
    ks = [v for k, v in res.items() if "linear_split16_kernel" in k]
    assert len(ks) == 1, list(res)
    v = ks[0]
    print("linear_split16_kernel", v)
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 512, v


def test_new_names_leave_the_older_kernels_selectable(res):
    """the resource tests select by name substring and want exactly one match"""
    for old in OLDER:
        assert sum(old in k for k in res) == 1, (old, list(res))
