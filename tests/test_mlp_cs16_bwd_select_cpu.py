"""Which kernels a TTT-MLP backward at mini-batches of 16 runs (no device needed: ``ttt_hip_resolve_impl`` only looks at the dims).
The MFMA backward of csrc/ttt_mlp16_bwd_body.h is opt-in: an explicit TTT_IMPL_MFMA is accepted for bf16 activations at F = 64,
TTT_IMPL_AUTO keeps resolving the call to the generic kernels, the per-call ``impl`` of ``ttt_backward_impl`` reaches the dims without
touching the global selector, and the layer switch ``TkMLP.cs16_bwd_impl`` selects only this geometry."""
import ctypes
import inspect

import pytest
import torch

import test_time_training as ext

AUTO, GENERIC, MFMA = ext.IMPL_AUTO, ext.IMPL_GENERIC, ext.IMPL_MFMA
BF16, F32 = 0, 1


def _d(CS=16, F=64, act=BF16, impl=MFMA, B=1, NH=2, NC=5, G=2):
    return ext._Dims(B, NH, NC, CS, F, G, act, impl, 1e-8)


def _resolve(d, mlp=1, bwd=1):
    return ext.load_library().ttt_hip_resolve_impl(ctypes.byref(d), mlp, bwd)


def test_explicit_mfma_is_accepted_for_the_mlp_backward_at_cs16():
    assert ext.resolved_impl(1, 2, 5, 16, 64, 2, torch.bfloat16, mlp=True, backward=True, impl="mfma") == "mfma"
    assert _resolve(_d()) == MFMA


def test_auto_and_generic_stay_on_the_generic_kernels():
    assert _resolve(_d(impl=AUTO)) == GENERIC
    assert _resolve(_d(impl=GENERIC)) == GENERIC
    assert ext.resolved_impl(1, 2, 5, 16, 64, 2, torch.bfloat16, mlp=True, backward=True) == "generic"
    # ... and nothing else moved: the forward at 16, the CS = 64 kernels, TTT-Linear at 16 and 64
    assert _resolve(_d(impl=AUTO), bwd=0) == MFMA
    assert _resolve(_d(impl=AUTO), mlp=0, bwd=1) == MFMA and _resolve(_d(impl=AUTO), mlp=0, bwd=0) == MFMA
    assert _resolve(_d(CS=64, impl=AUTO), mlp=0, bwd=1) == GENERIC and _resolve(_d(CS=64, impl=AUTO), mlp=0, bwd=0) == GENERIC
    assert _resolve(_d(CS=64, impl=AUTO), bwd=0) == MFMA


def test_explicit_mfma_is_still_refused_off_the_geometry():
    assert _resolve(_d(act=F32)) == -1
    assert _resolve(_d(F=32)) == -1
    assert _resolve(_d(CS=32)) == -1


def test_no_workspace_is_asked_for():
    """the per-step state fits the four documented *_init_group buffers"""
    assert ext.load_library().ttt_hip_mlp_backward_workspace(ctypes.byref(_d())) == 0


def test_state_buffers_are_required_on_the_mfma_path():
    """the four *_init_group pointers are checked before any launch (fake pointers: the call is refused on the null one)"""
    lib = ext.load_library()
    fake = 0x1000
    vals = [fake] * len(ext._MlpBwd._fields_)
    names = [n for n, _ in ext._MlpBwd._fields_]
    vals[names.index("W2_init_group")] = None
    args = ext._MlpBwd(*vals)
    d = _d()
    lib.ttt_hip_mlp_backward.restype = ctypes.c_int
    rc = lib.ttt_hip_mlp_backward(ctypes.byref(d), ctypes.byref(args), ctypes.c_void_p(None), ctypes.c_size_t(0), ctypes.c_void_p(None))
    assert rc == -1 and b"W2_init_group" in lib.ttt_hip_last_error()


def test_per_call_selector_leaves_the_reference_signature_alone():
    assert len(inspect.signature(ext.ttt_backward).parameters) == 43
    assert len(inspect.signature(ext.ttt_backward_impl).parameters) == 44
    assert list(inspect.signature(ext.ttt_backward_impl).parameters)[1:] == list(inspect.signature(ext.ttt_backward).parameters)
    assert ext.get_impl() == "auto"
    with pytest.raises(TypeError):
        ext.ttt_backward_impl("mfma", *[torch.zeros(1)] * 41, 1)
    with pytest.raises(RuntimeError):              # the usual checks run: a CPU tensor, no CPU path
        ext.ttt_backward_impl("mfma", *[torch.zeros(1, 1, 1, 16, 64)] * 42, 1)
    with pytest.raises(ValueError):
        ext.resolved_impl(1, 2, 5, 16, 64, 2, torch.bfloat16, mlp=True, backward=True, impl="fast")
    assert ext.get_impl() == "auto"


def test_layer_switch_selects_only_the_cs16_bf16_geometry(monkeypatch):
    from ttt_amd.models.ssm import mlp_tk
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    assert TkMLP.cs16_bwd_impl in ("auto", "mfma")
    old = TkMLP.cs16_bwd_impl
    try:
        TkMLP.cs16_bwd_impl = "auto"
        assert TkMLP.bwd_impl(16, 64, torch.bfloat16) is None
        TkMLP.cs16_bwd_impl = "mfma"
        assert TkMLP.bwd_impl(16, 64, torch.bfloat16) == "mfma"
        assert TkMLP.bwd_impl(64, 64, torch.bfloat16) is None
        assert TkMLP.bwd_impl(16, 32, torch.bfloat16) is None
        assert TkMLP.bwd_impl(16, 64, torch.float32) is None
        TkMLP.cs16_bwd_impl = "fast"
        with pytest.raises(ValueError):
            TkMLP.bwd_impl(16, 64, torch.bfloat16)
    finally:
        TkMLP.cs16_bwd_impl = old
    with pytest.raises(ValueError):                # the environment variable's value goes through the same check
        mlp_tk._check_cs16_bwd_impl("generic")
    assert ext.get_impl() == "auto"


def test_pipeline_plan_still_leaves_a_cs16_layer_under_grad_in_one_piece(monkeypatch):
    from test_mlp16_chunk_emul_cpu import _layer_and_meta
    from ttt_amd.models.ssm.mlp_tk import TkMLP
    monkeypatch.setattr(ext, "resolved_impl", lambda *a, **k: "mfma")
    monkeypatch.setattr(TkMLP, "cs16_bwd_impl", "mfma")
    layer, meta, x, L = _layer_and_meta(4096)
    with torch.enable_grad():
        assert layer._pipeline_plan(x, meta, L, False, False) is None
