"""include/ttt_hip_lin64_bwd_front.h, the eighth header of libttt_hip.so (the front / chain stage of the TTT-Linear backward in parts at
mini-batches of 64): its declarations against the binding's eighth prototype table, the exports, the size query, and the argument
checks of ``ttt_hip_linear_front64_groups`` / ``ttt_hip_linear_chain64_groups`` that are reached before any launch (fake pointers, no
GPU) - in the order of the shared entry checks.  The entries of the sixth header keep refusing mini-batches of 64."""
import ctypes
import os
import re

import pytest

import test_abi_cpu as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ttt_hip_lin64_bwd_front.h")
NAMES = ("ttt_hip_linear_backward_front64_records", "ttt_hip_linear_front64_groups", "ttt_hip_linear_chain64_groups")
SLOT = 16 * 1024 + 256
RECORD = 77824
FRONT_NEEDS = ("XQ", "XK", "XV", "ttt_norm_weight", "ttt_norm_bias", "grad_L_XQW", "grad_L_XQ")
CHAIN_UNUSED = ("W1_checkpoints", "b1_checkpoints", "W1_init_group", "b1_init_group", "XV", "grad_L_XQW", "grad_L_XQ")


def test_eighth_prototype_table_matches_the_eighth_header():
    import test_time_training as ext
    declared = A._declared_prototypes(HEADER)
    assert sorted(declared) == sorted(ext._PROTOTYPES_LIN64_BWD_FRONT) == sorted(NAMES)
    for other in (ext._PROTOTYPES, ext._PROTOTYPES_PARTS, ext._PROTOTYPES_BWD_PARTS, ext._PROTOTYPES_PAIR16, ext._PROTOTYPES_MLP_BWD_PARTS,
                  ext._PROTOTYPES_LIN_BWD_FRONT, ext._PROTOTYPES_LIN_SPLIT16):
        assert not set(ext._PROTOTYPES_LIN64_BWD_FRONT) & set(other), "a symbol belongs to one header"
    assert len(ext.EXPORTED_SYMBOLS) == 46
    for name, (ret, params) in declared.items():
        restype, argtypes = ext._PROTOTYPES_LIN64_BWD_FRONT[name]
        assert A._ctypes_kind(restype) == ret, (name, restype, ret)
        assert [A._ctypes_kind(a) for a in argtypes] == params, (name, argtypes, params)
    p, i, z = "pointer", ctypes.c_int, ctypes.c_size_t
    assert declared["ttt_hip_linear_backward_front64_records"] == (z, [p, i])
    assert declared["ttt_hip_linear_front64_groups"] == (i, [p, p, i, i, p, z, p, z, p])
    assert declared["ttt_hip_linear_chain64_groups"] == (i, [p, p, i, i, p, z, p, z, p, z, p])
    src = open(HEADER).read()
    assert '#include "ttt_hip.h"' in src and "#define TTT_HIP_ABI_VERSION" not in src
    assert not set(NAMES) & set(A._declared_symbols())
    for other in ("ttt_hip_parts.h", "ttt_hip_bwd_parts.h", "ttt_hip_pair16.h", "ttt_hip_mlp_bwd_parts.h", "ttt_hip_lin_bwd_front.h",
                  "ttt_hip_lin_split16.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert not any(n in text for n in NAMES), other


def test_library_exports_the_symbols_with_their_prototypes():
    import test_time_training as ext
    lib = ext.load_library()
    raw = ctypes.CDLL(ext.library_path())
    for name in NAMES:
        assert hasattr(raw, name), name
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (ext._PROTOTYPES_LIN64_BWD_FRONT[name][0], ext._PROTOTYPES_LIN64_BWD_FRONT[name][1])
    assert lib.ttt_hip_abi_version() == 5 and len(ext.EXPORTED_SYMBOLS) == 46


def _dims64(ext, impl=2, act=0):
    return ext._Dims(2, 3, 7, 64, 64, 3, act, impl, 1e-8)                # K = 3, on an explicit MFMA


def _dims16(ext, impl=0):
    return ext._Dims(2, 3, 11, 16, 64, 4, 0, impl, 1e-8)                 # K = 3


def test_size_query_returns_the_documented_formula():
    import test_time_training as ext
    lib = ext.load_library()
    q = lib.ttt_hip_linear_backward_front64_records
    d64 = _dims64(ext)
    for nk in (1, 2, 3):
        assert q(ctypes.byref(d64), nk) == 2 * 3 * nk * 3 * RECORD
    assert RECORD == 4 * 19456
    assert q(ctypes.byref(d64), 0) == 0
    assert q(ctypes.byref(d64), -1) == 0
    assert q(None, 1) == 0
    assert q(ctypes.byref(_dims16(ext)), 1) == 0                          # CS = 16
    assert q(ctypes.byref(_dims16(ext, impl=2)), 1) == 0
    assert q(ctypes.byref(_dims64(ext, impl=0)), 1) == 0                  # auto
    assert q(ctypes.byref(_dims64(ext, impl=1)), 1) == 0                  # the generic kernels
    assert q(ctypes.byref(_dims64(ext, act=1)), 1) == 0                   # fp32 activations
    assert q(ctypes.byref(ext._Dims(2, 3, 7, 64, 32, 3, 0, 2, 1e-8)), 1) == 0       # F != 64
    assert ext.linear_backward_front64_records(2, 3, 7, 64, 64, 3, 2, impl="mfma") == 2 * 3 * 2 * 3 * RECORD
    assert ext.linear_backward_front64_records(2, 3, 7, 64, 64, 3, 2) == 0
    assert ext.linear_backward_front64_records(2, 3, 11, 16, 64, 4, 2) == 0
    # the sixth header's query is what it was
    assert lib.ttt_hip_linear_backward_front_records(ctypes.byref(d64), 1) == 0
    assert lib.ttt_hip_linear_backward_front_records(ctypes.byref(_dims16(ext)), 1) == 2 * 3 * 4 * 19456


FAKE = 0x1000                                      # never dereferenced: every case below is refused before the launch
BIG = 1 << 40


def _front(lib, ext, d, k0, nk, a=True, slots=FAKE, nbytes=BIG, records=FAKE, rbytes=BIG, null=None, entry="ttt_hip_linear_front64_groups", **_):
    args = ext._LinBwd(*[FAKE if f in FRONT_NEEDS and f != null else None for f in ext.LIN_BWD_FIELDS])
    rc = getattr(lib, entry)(ctypes.byref(d) if d is not None else None, ctypes.byref(args) if a else None, k0, nk,
                             slots, nbytes, records, rbytes, None)
    return rc, lib.ttt_hip_last_error()


def _chain(lib, ext, d, k0, nk, a=True, slots=FAKE, nbytes=BIG, records=FAKE, rbytes=BIG, carry=FAKE, cbytes=BIG, null=None,
           entry="ttt_hip_linear_chain64_groups"):
    args = ext._LinBwd(*[None if f in CHAIN_UNUSED or f == null else FAKE for f in ext.LIN_BWD_FIELDS])
    rc = getattr(lib, entry)(ctypes.byref(d) if d is not None else None, ctypes.byref(args) if a else None, k0, nk,
                             slots, nbytes, records, rbytes, ctypes.cast(carry, ctypes.c_void_p) if carry else None, cbytes, None)
    return rc, lib.ttt_hip_last_error()


@pytest.mark.parametrize("call", [_front, _chain])
def test_argument_checks_without_gpu(call):
    """In the order of the shared entry checks: null dims / args / a needed field; a geometry that does not resolve to the MFMA family
    (mini-batches of 64 under auto, fp32 activations, the generic kernels); mini-batches of 16; a range outside [0, K) in the
    overflow-safe form; a slot workspace, then a record workspace, that is null or too small.  Every earlier check wins over every
    later one.  What a call may leave NULL is NULL in every case here."""
    import test_time_training as ext
    lib = ext.load_library()
    d64 = _dims64(ext)
    rc, err = call(lib, ext, None, 0, 1)
    assert rc == -1 and b"null dims" in err
    rc, err = call(lib, ext, d64, 0, 1, a=False)
    assert rc == -1 and b"null args" in err
    needs = FRONT_NEEDS if call is _front else [f for f in ext.LIN_BWD_FIELDS if f not in CHAIN_UNUSED]
    assert len(needs) == (7 if call is _front else 14)
    for f in needs:
        rc, err = call(lib, ext, d64, 0, 1, null=f)
        assert rc == -1 and f"null pointer argument {f}".encode() in err, (f, err)
        rc, err = call(lib, ext, _dims16(ext), 9, 9, null=f, slots=None, records=None)       # the pointers come first
        assert rc == -1 and f"null pointer argument {f}".encode() in err, (f, err)
    refused = {"CS = 64 under auto": _dims64(ext, impl=0), "fp32 activations": _dims64(ext, impl=0, act=1),
               "fp32 activations, MFMA requested": _dims64(ext, act=1), "the generic kernels": _dims64(ext, impl=1),
               "CS = 16 on the generic kernels": _dims16(ext, impl=1)}
    for what, d in refused.items():
        rc, err = call(lib, ext, d, 9, 9, slots=None, records=None)                          # ... the family before the range
        assert rc == -1 and b"only the MFMA sweep" in err, (what, err)
    for d in (_dims16(ext), _dims16(ext, impl=2)):
        rc, err = call(lib, ext, d, 0, 1)
        assert rc == -1 and b"only mini-batches of 64" in err, err
    for k0, nk in ((-1, 1), (0, 0), (1, -1), (0, 4), (3, 1), (2, 2), (2 ** 31 - 1, 2), (1, 2 ** 31 - 1)):      # K = 3
        rc, err = call(lib, ext, d64, k0, nk, slots=None, records=None)                      # ... the range before the workspaces
        assert rc == -1 and b"inside [0, K)" in err, (k0, nk, err)
    need = lib.ttt_hip_linear_backward_parts_slots(ctypes.byref(d64), 2)
    for kw in (dict(slots=None), dict(nbytes=need - 1)):
        rc, err = call(lib, ext, d64, 1, 2, records=None, **kw)                              # ... the slots before the records
        assert rc == -1 and b"slot workspace null or smaller" in err, (kw, err)
    need = lib.ttt_hip_linear_backward_front64_records(ctypes.byref(d64), 2)
    assert need == 2 * 3 * 2 * 3 * RECORD
    for kw in (dict(records=None), dict(rbytes=need - 1)):
        rc, err = call(lib, ext, d64, 1, 2, **kw)
        assert rc == -1 and b"record workspace null or smaller than ttt_hip_linear_backward_front64_records" in err, (kw, err)


def test_chain_refuses_a_missing_or_small_carry():
    import test_time_training as ext
    lib = ext.load_library()
    d = _dims64(ext)
    need = lib.ttt_hip_linear_backward_parts_carry(ctypes.byref(d))
    assert need == 2 * 3 * 8 * 256 * 4
    for kw in (dict(carry=None), dict(cbytes=need - 1)):
        rc, err = _chain(lib, ext, d, 0, 3, **kw)
        assert rc == -1 and b"ln_carry null or smaller" in err, (kw, err)
    rc, err = _chain(lib, ext, d, 0, 3, records=None, carry=None)                            # the records before the carry
    assert rc == -1 and b"record workspace null or smaller" in err, err


def test_the_entries_of_the_sixth_header_still_refuse_mini_batches_of_64():
    import test_time_training as ext
    lib = ext.load_library()
    d64 = _dims64(ext)
    for call, entry in ((_front, "ttt_hip_linear_front_groups"), (_chain, "ttt_hip_linear_chain_groups")):
        rc, err = call(lib, ext, d64, 0, 1, entry=entry)
        assert rc == -1 and b"only mini-batches of 16" in err, err


def test_binding_checks_tensors_before_the_call():
    """both wrappers check what they are given against the contract of ``ttt_linear_backward``, field by field (no CPU path); what a
    call does not touch may be None"""
    import torch
    import test_time_training as ext
    good = A._scan_tensors(ext.LIN_BWD_FIELDS, False, on_device=False)
    slots = records = carry = torch.zeros(8)
    chn = {f: (None if f in CHAIN_UNUSED else t) for f, t in good.items()}
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_linear_chain64_groups("mfma", *chn.values(), A._G, 0, 1, slots, records, carry)
    frt = {f: (t if f in FRONT_NEEDS else None) for f, t in good.items()}
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_linear_front64_groups("mfma", *frt.values(), A._G, 0, 1, slots, records)
    good = A._scan_tensors(ext.LIN_BWD_FIELDS, False, on_device=True)
    frt = {f: (t if f in FRONT_NEEDS else None) for f, t in good.items()}
    chn = {f: (None if f in CHAIN_UNUSED else t) for f, t in good.items()}
    for f in ("XV", "grad_L_XQ", "ttt_norm_bias"):
        with pytest.raises(RuntimeError, match=re.escape(f"{f}: expected shape {A._contract_of(f, False)[0]}, got ")):
            ext.ttt_linear_front64_groups("mfma", *{**frt, f: A._wrong_shape(good[f])}.values(), A._G, 0, 1, slots, records)
    with pytest.raises(TypeError, match="grad_L_XQW: expected a torch.Tensor"):
        ext.ttt_linear_front64_groups("mfma", *{**frt, "grad_L_XQW": None}.values(), A._G, 0, 1, slots, records)
    for f in ("XK", "grad_L_W1_last", "grad_L_last_eta", "grad_L_ttt_norm_weight"):
        with pytest.raises(RuntimeError, match=re.escape(f"{f}: expected shape {A._contract_of(f, False)[0]}, got ")):
            ext.ttt_linear_chain64_groups("mfma", *{**chn, f: A._wrong_shape(good[f])}.values(), A._G, 0, 1, slots, records, carry)
    with pytest.raises(TypeError, match="grad_L_XK: expected a torch.Tensor"):
        ext.ttt_linear_chain64_groups("mfma", *{**chn, "grad_L_XK": None}.values(), A._G, 0, 1, slots, records, carry)
    with pytest.raises(ValueError, match="impl: expected"):
        ext.ttt_linear_chain64_groups("fast", *chn.values(), A._G, 0, 1, slots, records, carry)
    # every tensor fits: the next checks are the workspaces'
    with pytest.raises(RuntimeError, match="slots: expected a contiguous tensor on a HIP device"):
        ext.ttt_linear_chain64_groups("mfma", *chn.values(), A._G, 0, 1, slots, records, carry)
    with pytest.raises(RuntimeError, match="slots: expected a contiguous tensor on a HIP device"):
        ext.ttt_linear_front64_groups("mfma", *frt.values(), A._G, 0, 1, slots, records)
