"""include/ttt_hip_parts.h, the second header of libttt_hip.so (extensions beside the reference's operator boundary): its
declarations against the binding's second prototype table, the export, and the argument checks of ``ttt_hip_linear_forward_chunk``
that are reached before any launch (fake pointers, no GPU)."""
import ctypes
import os
import re

import test_abi_cpu as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ttt_hip_parts.h")


def test_second_prototype_table_matches_the_second_header():
    import test_time_training as ext
    declared = A._declared_prototypes(HEADER)
    assert sorted(declared) == sorted(ext._PROTOTYPES_PARTS) == ["ttt_hip_linear_forward_chunk"]
    assert not set(ext._PROTOTYPES_PARTS) & set(ext._PROTOTYPES), "a symbol belongs to one header"
    assert not set(ext._PROTOTYPES_PARTS) & set(ext.EXPORTED_SYMBOLS) and len(ext.EXPORTED_SYMBOLS) == 46
    for name, (ret, params) in declared.items():
        restype, argtypes = ext._PROTOTYPES_PARTS[name]
        assert A._ctypes_kind(restype) == ret, (name, restype, ret)
        assert [A._ctypes_kind(a) for a in argtypes] == params, (name, argtypes, params)
    p = "pointer"
    assert declared["ttt_hip_linear_forward_chunk"] == (ctypes.c_int, [p, p, ctypes.c_int, ctypes.c_int, p, p, p, ctypes.c_size_t, p])
    # the second header builds on the first and keeps its ABI version; the first mentions it in a comment only
    src = open(HEADER).read()
    assert '#include "ttt_hip.h"' in src and "#define TTT_HIP_ABI_VERSION" not in src
    assert "ttt_hip_parts.h" in open(os.path.join(ROOT, "include", "ttt_hip.h")).read()
    assert "ttt_hip_linear_forward_chunk" not in A._declared_symbols()


def test_library_exports_the_symbol_with_its_prototype():
    import test_time_training as ext
    lib = ext.load_library()
    assert hasattr(ctypes.CDLL(ext.library_path()), "ttt_hip_linear_forward_chunk")
    fn = lib.ttt_hip_linear_forward_chunk
    assert (fn.restype, list(fn.argtypes)) == (ext._PROTOTYPES_PARTS["ttt_hip_linear_forward_chunk"][0],
                                               ext._PROTOTYPES_PARTS["ttt_hip_linear_forward_chunk"][1])
    assert lib.ttt_hip_abi_version() == 5


def _chunk_call(lib, ext, dims, step0, nsteps, finals, args=True):
    fake = 0x1000                                  # never dereferenced: every case below is refused before the launch
    a = ext._LinFwd(*[fake] * len(ext.LIN_FWD_FIELDS))
    vp = lambda ok: fake if ok else None
    rc = lib.ttt_hip_linear_forward_chunk(ctypes.byref(dims) if dims is not None else None, ctypes.byref(a) if args else None,
                                          step0, nsteps, *[vp(f) for f in finals], None, 0, None)
    return rc, lib.ttt_hip_last_error()


def test_linear_forward_chunk_argument_checks_without_gpu():
    """null arguments; a geometry the MFMA family does not take under this selector (mini-batches of 64 under auto, fp32 activations,
    the generic kernels on request); a part outside [0, NC), in the overflow-safe form; one final-state buffer only.  Parts off the
    checkpoint-group boundaries pass the range check at both mini-batch sizes: there is no group rule."""
    import test_time_training as ext
    lib = ext.load_library()
    both = (True, True)
    d16 = ext._Dims(1, 2, 12, 16, 64, 4, 0, 0, 1e-8)                   # bf16, impl = AUTO, G = 4
    d64 = ext._Dims(1, 2, 12, 64, 64, 4, 0, 2, 1e-8)                   # mini-batches of 64: on an explicit MFMA
    for d in (d16, d64):
        assert lib.ttt_hip_resolve_impl(ctypes.byref(d), 0, 0) == 2
        assert lib.ttt_hip_linear_forward_workspace(ctypes.byref(d)) == 0
        for step0, nsteps in ((-1, 2), (0, 0), (3, -1), (5, 8), (12, 1), (0, 13), (2 ** 31 - 1, 2)):
            rc, err = _chunk_call(lib, ext, d, step0, nsteps, both)
            assert rc == -1 and b"inside [0, NC)" in err, (step0, nsteps, err)
        # off-group parts pass the range check: the next check ("both or neither") is what refuses these calls
        for step0, nsteps in ((1, 2), (5, 6), (0, 12), (11, 1)):
            for finals in ((True, False), (False, True)):
                rc, err = _chunk_call(lib, ext, d, step0, nsteps, finals)
                assert rc == -1 and b"both final-state buffers or neither" in err, (step0, nsteps, err)
    rc, err = _chunk_call(lib, ext, None, 0, 4, both)
    assert rc == -1 and b"null dims" in err
    rc, err = _chunk_call(lib, ext, d16, 0, 4, both, args=False)
    assert rc == -1 and b"null args" in err
    a = ext._LinFwd(*[0x1000] * len(ext.LIN_FWD_FIELDS))
    a.W1_init = None
    assert lib.ttt_hip_linear_forward_chunk(ctypes.byref(d16), ctypes.byref(a), 0, 4, None, None, None, 0, None) == -1
    assert b"null pointer argument W1_init" in lib.ttt_hip_last_error()
    refused = {"CS = 64 under auto": ext._Dims(1, 2, 12, 64, 64, 4, 0, 0, 1e-8),
               "fp32 activations": ext._Dims(1, 2, 12, 16, 64, 4, 1, 0, 1e-8),
               "fp32 activations, MFMA requested": ext._Dims(1, 2, 12, 16, 64, 4, 1, 2, 1e-8),
               "the generic kernels": ext._Dims(1, 2, 12, 16, 64, 4, 0, 1, 1e-8)}
    for what, d in refused.items():
        rc, err = _chunk_call(lib, ext, d, 0, 4, both)
        assert rc == -1 and b"only the MFMA scan" in err and b"continues from a state" in err, (what, err)


def test_binding_checks_tensors_before_the_call():
    """``ttt_linear_forward_chunk`` checks its tensors against the contract of ``ttt_linear_forward``, field by field (no CPU path)"""
    import pytest
    import test_time_training as ext
    good = A._scan_tensors(ext.LIN_FWD_FIELDS, False, on_device=False)
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_linear_forward_chunk(None, *good.values(), A._G, 0, 1)
    good = A._scan_tensors(ext.LIN_FWD_FIELDS, False, on_device=True)
    for f in ("W1_init", "b1_checkpoints", "ttt_norm_bias"):
        ts = {**good, f: A._wrong_shape(good[f])}
        with pytest.raises(RuntimeError, match=re.escape(f"{f}: expected shape {A._contract_of(f, False)[0]}, got ")):
            ext.ttt_linear_forward_chunk("mfma", *ts.values(), A._G, 0, 1)
    with pytest.raises(ValueError, match="impl: expected"):
        ext.ttt_linear_forward_chunk("fast", *good.values(), A._G, 0, 1)
