"""include/ttt_hip_bwd_parts.h, the third header of libttt_hip.so (the TTT-Linear backward over ranges of checkpoint groups): its
declarations against the binding's third prototype table, the exports, the two size queries, and the argument checks of
``ttt_hip_linear_recompute_groups`` / ``ttt_hip_linear_sweep_groups`` that are reached before any launch (fake pointers, no GPU)."""
import ctypes
import os
import re

import pytest

import test_abi_cpu as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ttt_hip_bwd_parts.h")
NAMES = ("ttt_hip_linear_backward_parts_slots", "ttt_hip_linear_backward_parts_carry", "ttt_hip_linear_recompute_groups",
         "ttt_hip_linear_sweep_groups")
SLOT = 16 * 1024 + 256
RECOMPUTE_NEEDS = ("XK", "XV", "last_eta", "ttt_norm_weight", "ttt_norm_bias", "W1_checkpoints", "b1_checkpoints")
SWEEP_UNUSED = ("W1_checkpoints", "b1_checkpoints", "W1_init_group", "b1_init_group")


def test_third_prototype_table_matches_the_third_header():
    import test_time_training as ext
    declared = A._declared_prototypes(HEADER)
    assert sorted(declared) == sorted(ext._PROTOTYPES_BWD_PARTS)
    assert set(NAMES) <= set(declared)
    for other in (ext._PROTOTYPES, ext._PROTOTYPES_PARTS):
        assert not set(ext._PROTOTYPES_BWD_PARTS) & set(other), "a symbol belongs to one header"
    assert len(ext.EXPORTED_SYMBOLS) == 46 and sorted(ext._PROTOTYPES_PARTS) == ["ttt_hip_linear_forward_chunk"]
    for name, (ret, params) in declared.items():
        restype, argtypes = ext._PROTOTYPES_BWD_PARTS[name]
        assert A._ctypes_kind(restype) == ret, (name, restype, ret)
        assert [A._ctypes_kind(a) for a in argtypes] == params, (name, argtypes, params)
    p, i, z = "pointer", ctypes.c_int, ctypes.c_size_t
    assert declared["ttt_hip_linear_backward_parts_slots"] == (z, [p, i])
    assert declared["ttt_hip_linear_backward_parts_carry"] == (z, [p])
    assert declared["ttt_hip_linear_recompute_groups"] == (i, [p, p, i, i, p, z, p])
    assert declared["ttt_hip_linear_sweep_groups"] == (i, [p, p, i, i, p, z, p, z, p])
    src = open(HEADER).read()
    assert '#include "ttt_hip.h"' in src and "#define TTT_HIP_ABI_VERSION" not in src
    assert not set(NAMES) & set(A._declared_symbols())


def test_library_exports_the_symbols_with_their_prototypes():
    import test_time_training as ext
    lib = ext.load_library()
    raw = ctypes.CDLL(ext.library_path())
    for name in NAMES:
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (ext._PROTOTYPES_BWD_PARTS[name][0], ext._PROTOTYPES_BWD_PARTS[name][1])
    assert lib.ttt_hip_abi_version() == 5


def _dims16(ext, impl=0, act=0):
    return ext._Dims(2, 3, 11, 16, 64, 4, act, impl, 1e-8)               # K = 3


def _dims64(ext, impl=2):
    return ext._Dims(2, 3, 7, 64, 64, 3, 0, impl, 1e-8)                  # K = 3, on an explicit MFMA


def test_size_queries_return_the_documented_formulas():
    import test_time_training as ext
    lib = ext.load_library()
    d16, d64 = _dims16(ext), _dims64(ext)
    assert lib.ttt_hip_linear_backward_parts_slots(ctypes.byref(d16), 2) == 2 * 3 * 2 * (4 + 1) * SLOT
    assert lib.ttt_hip_linear_backward_parts_slots(ctypes.byref(d64), 3) == 2 * 3 * 3 * (3 + 1) * SLOT
    assert lib.ttt_hip_linear_backward_parts_carry(ctypes.byref(d16)) == 2 * 3 * 8 * 64 * 4
    assert lib.ttt_hip_linear_backward_parts_carry(ctypes.byref(d64)) == 2 * 3 * 8 * 256 * 4
    assert lib.ttt_hip_linear_backward_parts_slots(ctypes.byref(d16), 0) == 0 and lib.ttt_hip_linear_backward_parts_slots(None, 1) == 0
    assert ext.linear_backward_parts_slots(2, 3, 11, 16, 64, 4, 2) == 2 * 3 * 2 * 5 * SLOT
    assert ext.linear_backward_parts_carry(2, 3, 7, 64, 64, 3, impl="mfma") == 2 * 3 * 8 * 256 * 4


FAKE = 0x1000                                      # never dereferenced: every case below is refused before the launch
BIG = 1 << 40


def _recompute(lib, ext, d, k0, nk, a=True, slots=FAKE, nbytes=BIG, null=None):
    args = ext._LinBwd(*[FAKE if f in RECOMPUTE_NEEDS and f != null else None for f in ext.LIN_BWD_FIELDS])
    rc = lib.ttt_hip_linear_recompute_groups(ctypes.byref(d) if d is not None else None, ctypes.byref(args) if a else None, k0, nk,
                                             slots, nbytes, None)
    return rc, lib.ttt_hip_last_error()


def _sweep(lib, ext, d, k0, nk, a=True, slots=FAKE, nbytes=BIG, carry=FAKE, cbytes=BIG, null=None):
    args = ext._LinBwd(*[None if f in SWEEP_UNUSED or f == null else FAKE for f in ext.LIN_BWD_FIELDS])
    rc = lib.ttt_hip_linear_sweep_groups(ctypes.byref(d) if d is not None else None, ctypes.byref(args) if a else None, k0, nk,
                                         slots, nbytes, ctypes.cast(carry, ctypes.c_void_p) if carry else None, cbytes, None)
    return rc, lib.ttt_hip_last_error()


@pytest.mark.parametrize("call", [_recompute, _sweep])
def test_argument_checks_without_gpu(call):
    """null dims / args / a needed field; a geometry that does not resolve to the MFMA family; a range outside [0, K) in the
    overflow-safe form; a slot workspace that is null or too small.  What a call may leave NULL is NULL in every case here."""
    import test_time_training as ext
    lib = ext.load_library()
    d16, d64 = _dims16(ext), _dims64(ext)
    rc, err = call(lib, ext, None, 0, 1)
    assert rc == -1 and b"null dims" in err
    rc, err = call(lib, ext, d16, 0, 1, a=False)
    assert rc == -1 and b"null args" in err
    needs = RECOMPUTE_NEEDS if call is _recompute else [f for f in ext.LIN_BWD_FIELDS if f not in SWEEP_UNUSED]
    for f in needs:
        rc, err = call(lib, ext, d16, 0, 1, null=f)
        assert rc == -1 and f"null pointer argument {f}".encode() in err, (f, err)
    refused = {"CS = 64 under auto": _dims64(ext, impl=0), "fp32 activations": _dims16(ext, act=1),
               "fp32 activations, MFMA requested": _dims16(ext, impl=2, act=1), "the generic kernels": _dims16(ext, impl=1)}
    for what, d in refused.items():
        rc, err = call(lib, ext, d, 0, 1)
        assert rc == -1 and b"only the MFMA sweep" in err, (what, err)
    for d in (d16, d64):                            # K = 3 in both
        for k0, nk in ((-1, 1), (0, 0), (1, -1), (0, 4), (3, 1), (2, 2), (2 ** 31 - 1, 2), (1, 2 ** 31 - 1)):
            rc, err = call(lib, ext, d, k0, nk)
            assert rc == -1 and b"inside [0, K)" in err, (k0, nk, err)
        need = lib.ttt_hip_linear_backward_parts_slots(ctypes.byref(d), 2)
        for kw in (dict(slots=None), dict(nbytes=need - 1)):
            rc, err = call(lib, ext, d, 1, 2, **kw)
            assert rc == -1 and b"slot workspace null or smaller" in err, (kw, err)


def test_sweep_refuses_a_missing_or_small_carry():
    import test_time_training as ext
    lib = ext.load_library()
    for d in (_dims16(ext), _dims64(ext)):
        need = lib.ttt_hip_linear_backward_parts_carry(ctypes.byref(d))
        for kw in (dict(carry=None), dict(cbytes=need - 1)):
            rc, err = _sweep(lib, ext, d, 0, 3, **kw)
            assert rc == -1 and b"ln_carry null or smaller" in err, (kw, err)


def test_binding_checks_tensors_before_the_call():
    """both wrappers check what they are given against the contract of ``ttt_linear_backward``, field by field (no CPU path); what a
    call does not touch may be None"""
    import torch
    import test_time_training as ext
    good = A._scan_tensors(ext.LIN_BWD_FIELDS, False, on_device=False)
    slots = carry = torch.zeros(8)
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_linear_sweep_groups(None, *good.values(), A._G, 0, 1, slots, carry)
    rec = {f: (t if f in RECOMPUTE_NEEDS else None) for f, t in good.items()}
    with pytest.raises(RuntimeError, match=r"^XK: tensor must live on a HIP device"):
        ext.ttt_linear_recompute_groups(None, *rec.values(), A._G, 0, 1, slots)
    good = A._scan_tensors(ext.LIN_BWD_FIELDS, False, on_device=True)
    rec = {f: (t if f in RECOMPUTE_NEEDS else None) for f, t in good.items()}
    swp = {f: (None if f in SWEEP_UNUSED else t) for f, t in good.items()}
    for f in ("XV", "b1_checkpoints", "ttt_norm_bias"):
        with pytest.raises(RuntimeError, match=re.escape(f"{f}: expected shape {A._contract_of(f, False)[0]}, got ")):
            ext.ttt_linear_recompute_groups("mfma", *{**rec, f: A._wrong_shape(good[f])}.values(), A._G, 0, 1, slots)
    with pytest.raises(TypeError, match="W1_checkpoints: expected a torch.Tensor"):
        ext.ttt_linear_recompute_groups("mfma", *{**rec, "W1_checkpoints": None}.values(), A._G, 0, 1, slots)
    for f in ("XK", "grad_L_W1_last", "grad_L_last_eta", "grad_L_ttt_norm_weight"):
        with pytest.raises(RuntimeError, match=re.escape(f"{f}: expected shape {A._contract_of(f, False)[0]}, got ")):
            ext.ttt_linear_sweep_groups("mfma", *{**swp, f: A._wrong_shape(good[f])}.values(), A._G, 0, 1, slots, carry)
    with pytest.raises(TypeError, match="grad_L_XQW: expected a torch.Tensor"):
        ext.ttt_linear_sweep_groups("mfma", *{**swp, "grad_L_XQW": None}.values(), A._G, 0, 1, slots, carry)
    with pytest.raises(ValueError, match="impl: expected"):
        ext.ttt_linear_sweep_groups("fast", *swp.values(), A._G, 0, 1, slots, carry)
    # every tensor fits: the next check is the slot workspace's
    with pytest.raises(RuntimeError, match="slots: expected a contiguous tensor on a HIP device"):
        ext.ttt_linear_sweep_groups("mfma", *swp.values(), A._G, 0, 1, slots, carry)
