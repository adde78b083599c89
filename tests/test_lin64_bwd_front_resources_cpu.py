"""Register / scratch budget of the two kernels of the third stage of the TTT-Linear backward in parts at mini-batches of 64
(csrc/ttt_mfma16.hip: the carry-free half of every reverse step of a range, one wave per 16-row token block, and the walk that
consumes its records, one four-wave workgroup per (b, h), each wave holding two block records in registers; cross-compiled for gfx950,
no GPU needed).  A lane may use up to 512 registers; neither kernel may touch scratch memory."""
import pytest

import test_lin16_split_resources_cpu
import test_linear_bwd_front_resources_cpu
import test_mlp16_bwd_parts_resources_cpu
from test_kernel_resources_cpu import kernel_resources

KERNELS = ("linear_front_cs64_groups_kernel", "linear_chain_cs64_groups_kernel")
OLDER = sorted(set(test_lin16_split_resources_cpu.OLDER) | set(test_linear_bwd_front_resources_cpu.OLDER) |
               set(test_mlp16_bwd_parts_resources_cpu.OLDER) | set(test_linear_bwd_front_resources_cpu.KERNELS))


@pytest.fixture(scope="module")
def res():
    return kernel_resources("ttt_mfma16.hip")


@pytest.mark.parametrize("name", KERNELS)
def test_front64_kernel_does_not_spill(res, name):
    ks = [v for k, v in res.items() if name in k]
    assert len(ks) == 1, list(res)
    v = ks[0]
    print(name, v)
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 512, v


def test_new_names_leave_the_older_kernels_selectable(res):
    """the resource tests of the older kernels select by name substring and want exactly one match"""
    assert "linear_front16_groups_kernel" in OLDER and "linear_chain16_groups_kernel" in OLDER
    for old in OLDER:
        assert sum(old in k for k in res) == 1, (old, list(res))
