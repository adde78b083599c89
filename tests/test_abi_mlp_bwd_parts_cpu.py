"""include/ttt_hip_mlp_bwd_parts.h, the fifth header of libttt_hip.so (the TTT-MLP backward at mini-batches of 16 over ranges of
checkpoint groups): its declarations against the binding's prototype table ``_PROTOTYPES_MLP_BWD_PARTS``, the exports, the two size
queries, and the argument checks of ``ttt_hip_mlp_recompute_groups`` / ``ttt_hip_mlp_sweep_groups`` that are reached before any launch
(fake pointers, no GPU)."""
import ctypes
import os
import re

import pytest

import test_abi_cpu as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ttt_hip_mlp_bwd_parts.h")
NAMES = ("ttt_hip_mlp_backward_parts_slots", "ttt_hip_mlp_backward_parts_carry", "ttt_hip_mlp_recompute_groups",
         "ttt_hip_mlp_sweep_groups")
SLOT = (64 * 256 + 256 + 256 * 64 + 64) * 4
RECOMPUTE_NEEDS = ("XK", "XV", "last_eta", "ttt_norm_weight", "ttt_norm_bias", "W1_checkpoints", "b1_checkpoints", "W2_checkpoints",
                   "b2_checkpoints")
REFUSED = b"only the MFMA backward at mini-batches of 16"


def _sweep_unused(ext):
    return ("W1_checkpoints", "b1_checkpoints", "W2_checkpoints", "b2_checkpoints", "XQW") + tuple(ext.MLP_BWD_FIELDS[11:27])


def test_fifth_prototype_table_matches_the_fifth_header():
    import test_time_training as ext
    declared = A._declared_prototypes(HEADER)
    assert sorted(declared) == sorted(ext._PROTOTYPES_MLP_BWD_PARTS) == sorted(NAMES)
    for other in (ext._PROTOTYPES, ext._PROTOTYPES_PARTS, ext._PROTOTYPES_BWD_PARTS, ext._PROTOTYPES_PAIR16):
        assert not set(ext._PROTOTYPES_MLP_BWD_PARTS) & set(other), "a symbol belongs to one header"
    assert len(ext._PROTOTYPES) == 46 and len(ext.EXPORTED_SYMBOLS) == 46
    for name, (ret, params) in declared.items():
        restype, argtypes = ext._PROTOTYPES_MLP_BWD_PARTS[name]
        assert A._ctypes_kind(restype) == ret, (name, restype, ret)
        assert [A._ctypes_kind(a) for a in argtypes] == params, (name, argtypes, params)
    p, i, z = "pointer", ctypes.c_int, ctypes.c_size_t
    assert declared["ttt_hip_mlp_backward_parts_slots"] == (z, [p, i])
    assert declared["ttt_hip_mlp_backward_parts_carry"] == (z, [p])
    assert declared["ttt_hip_mlp_recompute_groups"] == (i, [p, p, i, i, p, z, p])
    assert declared["ttt_hip_mlp_sweep_groups"] == (i, [p, p, i, i, p, z, p, z, p])
    src = open(HEADER).read()
    assert '#include "ttt_hip.h"' in src and "#define TTT_HIP_ABI_VERSION" not in src
    assert not set(NAMES) & set(A._declared_symbols())


def test_library_exports_the_symbols_and_the_abi_version_is_unchanged():
    import test_time_training as ext
    lib = ext.load_library()
    raw = ctypes.CDLL(ext.library_path())
    for name in NAMES:
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (ext._PROTOTYPES_MLP_BWD_PARTS[name][0], ext._PROTOTYPES_MLP_BWD_PARTS[name][1])
    assert lib.ttt_hip_abi_version() == 5 == ext.ABI_VERSION
    assert re.search(r"#define\s+TTT_HIP_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "ttt_hip.h")).read())


def _dims(ext, impl=2, act=0, CS=16, NC=11, G=4):
    return ext._Dims(2, 3, NC, CS, 64, G, act, impl, 1e-8)               # K = 3


def test_size_queries_return_the_documented_formulas():
    import test_time_training as ext
    lib = ext.load_library()
    for impl in (0, 2):
        d = _dims(ext, impl)
        assert lib.ttt_hip_mlp_backward_parts_slots(ctypes.byref(d), 2) == 2 * 3 * 2 * 4 * 132352 == 2 * 3 * 2 * 4 * SLOT
        assert lib.ttt_hip_mlp_backward_parts_slots(ctypes.byref(d), 3) == 2 * 3 * 3 * 4 * 132352
        assert lib.ttt_hip_mlp_backward_parts_carry(ctypes.byref(d)) == 2 * 3 * 8192
    d = _dims(ext)
    bad = ext._Dims(2, 0, 11, 16, 64, 4, 0, 2, 1e-8)
    assert lib.ttt_hip_mlp_backward_parts_slots(ctypes.byref(d), 0) == 0 and lib.ttt_hip_mlp_backward_parts_slots(ctypes.byref(d), -1) == 0
    assert lib.ttt_hip_mlp_backward_parts_slots(None, 1) == 0 and lib.ttt_hip_mlp_backward_parts_slots(ctypes.byref(bad), 1) == 0
    assert lib.ttt_hip_mlp_backward_parts_carry(None) == 0 and lib.ttt_hip_mlp_backward_parts_carry(ctypes.byref(bad)) == 0
    assert ext.mlp_backward_parts_slots(2, 3, 11, 16, 64, 4, 2) == 2 * 3 * 2 * 4 * SLOT
    assert ext.mlp_backward_parts_carry(1, 48, 1128, 16, 64, 16, impl="mfma") == 48 * 8192


FAKE = 0x1000                                      # never dereferenced: every case below is refused before the launch
BIG = 1 << 40


def _recompute(lib, ext, d, k0, nk, a=True, slots=FAKE, nbytes=BIG, null=None):
    args = ext._MlpBwd(*[FAKE if f in RECOMPUTE_NEEDS and f != null else None for f in ext.MLP_BWD_FIELDS])
    rc = lib.ttt_hip_mlp_recompute_groups(ctypes.byref(d) if d is not None else None, ctypes.byref(args) if a else None, k0, nk,
                                          slots, nbytes, None)
    return rc, lib.ttt_hip_last_error()


def _sweep(lib, ext, d, k0, nk, a=True, slots=FAKE, nbytes=BIG, carry=FAKE, cbytes=BIG, null=None):
    args = ext._MlpBwd(*[None if f in _sweep_unused(ext) or f == null else FAKE for f in ext.MLP_BWD_FIELDS])
    rc = lib.ttt_hip_mlp_sweep_groups(ctypes.byref(d) if d is not None else None, ctypes.byref(args) if a else None, k0, nk,
                                      slots, nbytes, ctypes.cast(carry, ctypes.c_void_p) if carry else None, cbytes, None)
    return rc, lib.ttt_hip_last_error()


@pytest.mark.parametrize("call", [_recompute, _sweep])
def test_argument_checks_without_gpu(call):
    """null dims / args / a needed field; mini-batches of 64, fp32 activations, the generic kernels; a range outside [0, K) in the
    overflow-safe form; a slot workspace that is null or too small - each a negative code with a message.  What a call may leave NULL
    is NULL in every case here (the sweep: the checkpoints, XQW and all sixteen *_group buffers), under TTT_IMPL_MFMA and under
    TTT_IMPL_AUTO alike."""
    import test_time_training as ext
    lib = ext.load_library()
    rc, err = call(lib, ext, None, 0, 1)
    assert rc == -1 and b"null dims" in err
    rc, err = call(lib, ext, _dims(ext), 0, 1, a=False)
    assert rc == -1 and b"null args" in err
    needs = RECOMPUTE_NEEDS if call is _recompute else [f for f in ext.MLP_BWD_FIELDS if f not in _sweep_unused(ext)]
    assert len(needs) == (9 if call is _recompute else 21)
    for f in needs:
        rc, err = call(lib, ext, _dims(ext), 0, 1, null=f)
        assert rc == -1 and f"null pointer argument {f}".encode() in err, (f, err)
    refused = {"CS = 64": _dims(ext, CS=64, NC=7, G=3), "CS = 64 under auto": _dims(ext, impl=0, CS=64, NC=7, G=3),
               "fp32 activations": _dims(ext, act=1), "fp32 activations under auto": _dims(ext, impl=0, act=1),
               "the generic kernels": _dims(ext, impl=1)}
    for what, d in refused.items():
        rc, err = call(lib, ext, d, 0, 1)
        assert rc < 0 and REFUSED in err, (what, err)
    for impl in (2, 0):                               # K = 3
        d = _dims(ext, impl)
        for k0, nk in ((-1, 1), (0, 0), (1, -1), (0, 4), (3, 1), (2, 2), (2 ** 31 - 1, 2), (1, 2 ** 31 - 1)):
            rc, err = call(lib, ext, d, k0, nk)
            assert rc < 0 and b"inside [0, K)" in err, (k0, nk, err)
        need = lib.ttt_hip_mlp_backward_parts_slots(ctypes.byref(d), 2)
        for kw in (dict(slots=None), dict(nbytes=need - 1)):
            rc, err = call(lib, ext, d, 1, 2, **kw)
            assert rc < 0 and b"slot workspace null or smaller" in err, (kw, err)


def test_sweep_refuses_a_missing_or_small_carry():
    import test_time_training as ext
    lib = ext.load_library()
    d = _dims(ext)
    need = lib.ttt_hip_mlp_backward_parts_carry(ctypes.byref(d))
    for kw in (dict(carry=None), dict(cbytes=need - 1)):
        rc, err = _sweep(lib, ext, d, 0, 3, **kw)
        assert rc < 0 and b"ln_carry null" in err and b"smaller than ttt_hip_mlp_backward_parts_carry" in err, (kw, err)


def test_binding_checks_tensors_before_the_call():
    """both wrappers check what they are given against the contract of ``ttt_backward``, field by field (no CPU path); what a call
    does not touch may be None"""
    import torch
    import test_time_training as ext
    good = A._scan_tensors(ext.MLP_BWD_FIELDS, True, on_device=False)
    slots = carry = torch.zeros(8)
    swp = {f: (None if f in _sweep_unused(ext) else t) for f, t in good.items()}
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_sweep_groups(*swp.values(), A._G, 0, 1, slots, carry)
    rec = {f: (t if f in RECOMPUTE_NEEDS else None) for f, t in good.items()}
    with pytest.raises(RuntimeError, match=r"^XK: tensor must live on a HIP device"):
        ext.ttt_recompute_groups(*rec.values(), A._G, 0, 1, slots)
    good = A._scan_tensors(ext.MLP_BWD_FIELDS, True, on_device=True)
    rec = {f: (t if f in RECOMPUTE_NEEDS else None) for f, t in good.items()}
    swp = {f: (None if f in _sweep_unused(ext) else t) for f, t in good.items()}
    for f in ("XV", "b2_checkpoints", "ttt_norm_bias"):
        with pytest.raises(RuntimeError, match=re.escape(f"{f}: expected shape {A._contract_of(f, True)[0]}, got ")):
            ext.ttt_recompute_groups(*{**rec, f: A._wrong_shape(good[f])}.values(), A._G, 0, 1, slots, impl="mfma")
    with pytest.raises(TypeError, match="W2_checkpoints: expected a torch.Tensor"):
        ext.ttt_recompute_groups(*{**rec, "W2_checkpoints": None}.values(), A._G, 0, 1, slots, impl="mfma")
    for f in ("XK", "grad_L_W2_last", "grad_L_last_eta", "grad_L_ttt_norm_weight"):
        with pytest.raises(RuntimeError, match=re.escape(f"{f}: expected shape {A._contract_of(f, True)[0]}, got ")):
            ext.ttt_sweep_groups(*{**swp, f: A._wrong_shape(good[f])}.values(), A._G, 0, 1, slots, carry, impl="mfma")
    with pytest.raises(TypeError, match="grad_L_XQW: expected a torch.Tensor"):
        ext.ttt_sweep_groups(*{**swp, "grad_L_XQW": None}.values(), A._G, 0, 1, slots, carry, impl="mfma")
    with pytest.raises(ValueError, match="impl: expected"):
        ext.ttt_sweep_groups(*swp.values(), A._G, 0, 1, slots, carry, impl="fast")
    # every tensor fits: the next check is the slot workspace's
    with pytest.raises(RuntimeError, match="slots: expected a contiguous tensor on a HIP device"):
        ext.ttt_sweep_groups(*swp.values(), A._G, 0, 1, slots, carry, impl="mfma")
