"""Register / scratch / LDS budget of the TTT-MLP backward at mini-batches of 16 (csrc/ttt_mfma16.hip: mlp_bwd16_kernel, eight waves
per workgroup = two per SIMD = 256 registers per lane; cross-compiled for gfx950, no GPU needed), and the names the older resource
tests select by substring."""
import os
import re

import pytest

from test_kernel_resources_cpu import CSRC, kernel_resources


@pytest.fixture(scope="module")
def res():
    return kernel_resources("ttt_mfma16.hip")


def _body_constants():
    text = open(os.path.join(CSRC, "ttt_mlp16_bwd_body.h")).read()
    m = re.search(r"constexpr int WAVES = (\d+), NS = (\d+);", text)
    return int(m.group(1)), int(m.group(2))


def test_mlp_bwd16_kernel_budget(res):
    """budget: 512 / (waves per SIMD) registers per lane, 0 spilled dwords, no private segment.  Measured on the shipped code (eight
    waves, two per SIMD: a budget of 256): 255 registers, 0 spilled dwords, no private segment; the recompute half alone needs 172."""
    ks = [v for k, v in res.items() if "mlp_bwd16_kernel" in k]
    assert len(ks) == 1, list(res)
    v = ks[0]
    waves, ns = _body_constants()
    assert waves * ns == 8 and waves in (4, 8)
    print("mlp_bwd16_kernel", v)
    assert v["vgpr_count"] <= 512 // (waves // 4), v
    assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v


def test_mlp_bwd16_lds_fits():
    import mlp16_bwd_cases as M
    import scan_cases as C
    if not os.path.exists(C.CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    assert 0 < M.build_emul().emul_mlp16_bwd_lds_bytes() <= 160 * 1024


def test_new_name_leaves_the_older_kernels_selectable(res):
    """the resource tests select by name substring and want exactly one match"""
    for old in ("linear_bwd_cs64_kernel", "linear_fwd_cs64_kernel", "linear_bwd16_kernel", "linear_scan16_kernel", "mlp_scan16_body_kernel",
                "linear_recompute16_groups_kernel", "linear_sweep16_groups_kernel", "linear_recompute_cs64_groups_kernel",
                "linear_sweep_cs64_groups_kernel", "mlp_bwd16_kernel"):
        assert sum(old in k for k in res) == 1, (old, list(res))
    assert sum("mlp_scan16" in k for k in res) == 1 and not any("mlp_bwd_cluster4_kernel" in k for k in res)
