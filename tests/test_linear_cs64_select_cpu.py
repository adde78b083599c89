"""Which kernels a TTT-Linear call at mini-batches of 64 runs (no device needed: ``ttt_hip_resolve_impl`` only looks at the dims).
The MFMA scan and sweep of csrc/ttt_lin64_body.h are opt-in: an explicit TTT_IMPL_MFMA is accepted for bf16 activations at F = 64,
TTT_IMPL_AUTO keeps resolving the geometry to the generic kernels, and the per-call ``impl=`` keyword of the binding reaches the dims
without touching the global selector."""
import ctypes

import pytest
import torch

import test_time_training as ext

AUTO, GENERIC, MFMA = ext.IMPL_AUTO, ext.IMPL_GENERIC, ext.IMPL_MFMA
BF16, F32 = 0, 1


def _d(CS=64, F=64, act=BF16, impl=MFMA, B=1, NH=2, NC=4, G=2):
    return ext._Dims(B, NH, NC, CS, F, G, act, impl, 1e-8)


def _resolve(d, bwd):
    return ext.load_library().ttt_hip_resolve_impl(ctypes.byref(d), 0, bwd)


@pytest.mark.parametrize("bwd", [0, 1])
def test_explicit_mfma_is_accepted_at_cs64(bwd):
    assert _resolve(_d(), bwd) == MFMA


@pytest.mark.parametrize("bwd", [0, 1])
def test_auto_stays_on_the_generic_kernels_at_cs64(bwd):
    assert _resolve(_d(impl=AUTO), bwd) == GENERIC
    assert _resolve(_d(impl=GENERIC), bwd) == GENERIC
    assert _resolve(_d(CS=16, impl=AUTO), bwd) == MFMA          # mini-batches of 16: as before


@pytest.mark.parametrize("bwd", [0, 1])
def test_explicit_mfma_is_still_refused_off_the_geometry(bwd):
    assert _resolve(_d(act=F32), bwd) == -1
    assert _resolve(_d(F=32), bwd) == -1
    assert _resolve(_d(CS=32), bwd) == -1


def test_no_workspace_is_asked_for():
    """the sweep's per-step state fits the documented W1_init_group / b1_init_group scratch (G x 16 KiB, G x 64 floats per (b, h))"""
    lib = ext.load_library()
    assert lib.ttt_hip_linear_forward_workspace(ctypes.byref(_d())) == 0
    assert lib.ttt_hip_linear_backward_workspace(ctypes.byref(_d())) == 0


def test_impl_keyword_reaches_the_dims_and_leaves_the_global_selector():
    assert ext.get_impl() == "auto"
    assert ext._dims(1, 2, 4, 64, 64, 2, torch.bfloat16).impl == AUTO
    assert ext._dims(1, 2, 4, 64, 64, 2, torch.bfloat16, "mfma").impl == MFMA
    assert ext._dims(1, 2, 4, 64, 64, 2, torch.bfloat16, impl="generic").impl == GENERIC
    assert ext.resolved_impl(1, 2, 4, 64, 64, 2, mlp=False, impl="mfma") == "mfma"
    assert ext.resolved_impl(1, 2, 4, 64, 64, 2, mlp=False, backward=True, impl="mfma") == "mfma"
    assert ext.resolved_impl(1, 2, 4, 64, 64, 2, mlp=False) == "generic"
    assert ext.resolved_impl(1, 2, 4, 64, 64, 2, torch.float32, mlp=False, impl="mfma") == "unsupported"
    assert ext.get_impl() == "auto"
    with pytest.raises(ValueError):
        ext._dims(1, 2, 4, 64, 64, 2, torch.bfloat16, "fast")
    ext.set_impl("generic")
    try:                                                   # None = the global selector
        assert ext._dims(1, 2, 4, 64, 64, 2, torch.bfloat16).impl == GENERIC
        assert ext._dims(1, 2, 4, 64, 64, 2, torch.bfloat16, "auto").impl == AUTO
    finally:
        ext.set_impl("auto")


def test_per_call_selector_leaves_the_reference_signatures_alone():
    """``resolved_impl`` takes ``impl`` as a keyword only; the two scan wrappers keep the reference's parameter lists (12 / 22) and
    the per-call selector goes through ``ttt_linear_forward_impl`` / ``ttt_linear_backward_impl``, which take the same tensors by name after ``impl``"""
    import inspect
    p = inspect.signature(ext.resolved_impl).parameters["impl"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert len(inspect.signature(ext.ttt_linear_forward).parameters) == 12
    assert len(inspect.signature(ext.ttt_linear_backward).parameters) == 22
    x = torch.zeros(1)
    with pytest.raises(TypeError):
        ext.ttt_linear_forward_impl("mfma", *[x] * 10, 1)
    with pytest.raises(TypeError):
        ext.ttt_linear_backward_impl("mfma", *[x] * 20, 1)
    with pytest.raises(RuntimeError):              # the usual checks run: a CPU tensor, no CPU path
        ext.ttt_linear_forward_impl("mfma", *[torch.zeros(1, 1, 1, 64, 64)] * 11, 1)


def test_hiplinear_switch_selects_only_the_cs64_bf16_geometry():
    from ttt_amd.models.ssm.linear_hip import HipLinear
    assert HipLinear.cs64_impl in ("auto", "mfma")
    old = HipLinear.cs64_impl
    try:
        HipLinear.cs64_impl = "auto"
        assert HipLinear._impl(64, 64, torch.bfloat16) is None
        HipLinear.cs64_impl = "mfma"
        assert HipLinear._impl(64, 64, torch.bfloat16) == "mfma"
        assert HipLinear._impl(16, 64, torch.bfloat16) is None
        assert HipLinear._impl(64, 32, torch.bfloat16) is None
        assert HipLinear._impl(64, 64, torch.float32) is None
        HipLinear.cs64_impl = "fast"
        with pytest.raises(ValueError):
            HipLinear._impl(64, 64, torch.bfloat16)
    finally:
        HipLinear.cs64_impl = old
