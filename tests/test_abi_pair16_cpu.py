"""include/ttt_hip_pair16.h, the fourth header of libttt_hip.so (the TTT-MLP forward scan at mini-batches of 16 as a pair of workgroups
per (b, h)): its declarations against the binding's fourth prototype table, the workspace formula, and every argument check of
``ttt_hip_mlp_forward_chunk_pair16`` that is reached before a launch (fake pointers, no GPU)."""
import ctypes
import os
import re

import test_abi_cpu as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ttt_hip_pair16.h")
REC_BYTES = 64 * 1024 + 1024 + 256
FLAG_BYTES = 2 * 128


def _ring():
    return int(re.search(r"^#define TTT_HIP_PAIR16_RING (\d+)\s*$", open(HEADER).read(), flags=re.M).group(1))


def test_fourth_prototype_table_matches_the_fourth_header():
    import test_time_training as ext
    declared = A._declared_prototypes(HEADER)
    assert sorted(declared) == sorted(ext._PROTOTYPES_PAIR16) == ["ttt_hip_mlp_forward_chunk_pair16", "ttt_hip_mlp_forward_pair16_workspace"]
    others = {**ext._PROTOTYPES, **ext._PROTOTYPES_PARTS, **ext._PROTOTYPES_BWD_PARTS}
    assert not set(ext._PROTOTYPES_PAIR16) & set(others), "a symbol belongs to one header"
    assert not set(ext._PROTOTYPES_PAIR16) & set(ext.EXPORTED_SYMBOLS) and len(ext.EXPORTED_SYMBOLS) == 46
    for name, (ret, params) in declared.items():
        restype, argtypes = ext._PROTOTYPES_PAIR16[name]
        assert A._ctypes_kind(restype) == ret, (name, restype, ret)
        assert [A._ctypes_kind(a) for a in argtypes] == params, (name, argtypes, params)
    p = "pointer"
    assert declared["ttt_hip_mlp_forward_pair16_workspace"] == (ctypes.c_size_t, [p])
    assert declared["ttt_hip_mlp_forward_chunk_pair16"] == (ctypes.c_int, [p, p, ctypes.c_int, ctypes.c_int, p, p, p, p, p, ctypes.c_size_t, p])
    # the chunk entry has the parameter list of ttt_hip_mlp_forward_chunk
    assert ext._PROTOTYPES_PAIR16["ttt_hip_mlp_forward_chunk_pair16"] == ext._PROTOTYPES["ttt_hip_mlp_forward_chunk"]
    src = open(HEADER).read()
    assert '#include "ttt_hip.h"' in src and "#define TTT_HIP_ABI_VERSION" not in src
    assert not set(declared) & set(A._declared_symbols())


def test_library_exports_the_symbols_with_their_prototypes_and_keeps_abi_5():
    import test_time_training as ext
    lib = ext.load_library()
    raw = ctypes.CDLL(ext.library_path())
    for name, (restype, argtypes) in ext._PROTOTYPES_PAIR16.items():
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (restype, argtypes)
    assert lib.ttt_hip_abi_version() == 5 == ext.ABI_VERSION
    assert callable(ext.ttt_forward_pair16) and callable(ext.ttt_forward_chunk_pair16)


def test_workspace_formula_follows_the_ring_depth():
    """flags block (two 128-byte lines per (b, h), in front) + B * NH * RING records; 0 where the pair form does not serve the
    geometry; the main header's query still answers 0 at mini-batches of 16"""
    import test_time_training as ext
    lib = ext.load_library()
    ring = _ring()
    assert ring >= 2
    for B, NH, impl in ((2, 48, 0), (1, 5, 2), (3, 7, 0)):
        d = ext._Dims(B, NH, 21, 16, 64, 4, 0, impl, 1e-8)
        assert lib.ttt_hip_mlp_forward_pair16_workspace(ctypes.byref(d)) == B * NH * FLAG_BYTES + B * NH * ring * REC_BYTES
        assert lib.ttt_hip_mlp_forward_workspace(ctypes.byref(d)) == 0
    for what, d in {"CS = 64": ext._Dims(1, 2, 12, 64, 64, 4, 0, 0, 1e-8), "fp32": ext._Dims(1, 2, 12, 16, 64, 4, 1, 0, 1e-8),
                    "F = 32": ext._Dims(1, 2, 12, 16, 32, 4, 0, 0, 1e-8), "generic": ext._Dims(1, 2, 12, 16, 64, 4, 0, 1, 1e-8),
                    "B = 0": ext._Dims(0, 2, 12, 16, 64, 4, 0, 0, 1e-8)}.items():
        assert lib.ttt_hip_mlp_forward_pair16_workspace(ctypes.byref(d)) == 0, what
    assert lib.ttt_hip_mlp_forward_pair16_workspace(None) == 0


def _call(lib, ext, dims, step0, nsteps, finals, ws=0x2000, wsb=None, args=True):
    fake = 0x1000                                  # never dereferenced: every case below is refused before the launch
    a = ext._MlpFwd(*[fake] * len(ext.MLP_FWD_FIELDS))
    if wsb is None:
        wsb = lib.ttt_hip_mlp_forward_pair16_workspace(ctypes.byref(dims)) if dims is not None else 0
    rc = lib.ttt_hip_mlp_forward_chunk_pair16(ctypes.byref(dims) if dims is not None else None, ctypes.byref(a) if args else None,
                                              step0, nsteps, *[fake if f else None for f in finals], ws, wsb, None)
    return rc, lib.ttt_hip_last_error()


def test_chunk_pair16_refusals_without_gpu():
    import test_time_training as ext
    lib = ext.load_library()
    all4, none4 = (True,) * 4, (False,) * 4
    d16 = ext._Dims(1, 2, 12, 16, 64, 4, 0, 0, 1e-8)                   # bf16, impl = AUTO, G = 4
    assert lib.ttt_hip_resolve_impl(ctypes.byref(d16), 1, 0) == 2
    need = lib.ttt_hip_mlp_forward_pair16_workspace(ctypes.byref(d16))
    assert need > 0
    # anything but bf16 activations, F = 64, CS = 16 (on the MFMA scan)
    for what, d in {"CS = 64": ext._Dims(1, 2, 12, 64, 64, 4, 0, 0, 1e-8), "CS = 64, MFMA requested": ext._Dims(1, 2, 12, 64, 64, 4, 0, 2, 1e-8),
                    "fp32 activations": ext._Dims(1, 2, 12, 16, 64, 4, 1, 0, 1e-8), "F = 32": ext._Dims(1, 2, 12, 16, 32, 4, 0, 0, 1e-8),
                    "the generic kernels": ext._Dims(1, 2, 12, 16, 64, 4, 0, 1, 1e-8)}.items():
        rc, err = _call(lib, ext, d, 0, 4, all4, wsb=1 << 30)
        assert rc == -1 and b"mlp_forward_chunk_pair16" in err and b"mini-batches of 16" in err, (what, err)
    # a part outside [0, NC), in the overflow-safe form
    for step0, nsteps in ((-1, 2), (0, 0), (3, -1), (5, 8), (12, 1), (0, 13), (2 ** 31 - 1, 2)):
        rc, err = _call(lib, ext, d16, step0, nsteps, all4)
        assert rc == -1 and b"inside [0, NC)" in err, (step0, nsteps, err)
    # one to three of the four final-state pointers NULL (off-group parts pass the range check)
    for finals in ((True, True, False, True), (False, True, True, True), (True, False, False, False), (False, False, True, False),
                   (True, True, True, False)):
        for step0, nsteps in ((1, 2), (0, 12), (11, 1)):
            rc, err = _call(lib, ext, d16, step0, nsteps, finals)
            assert rc == -1 and b"all four final-state buffers or none" in err, (finals, err)
    # a NULL or too-small workspace - with all four finals and with none
    for finals in (all4, none4):
        for ws, wsb in ((None, need), (0x2000, need - 1), (0x2000, 0), (None, 0)):
            rc, err = _call(lib, ext, d16, 0, 12, finals, ws=ws, wsb=wsb)
            assert rc == -1 and b"workspace null or smaller" in err, (ws, wsb, err)
    rc, err = _call(lib, ext, None, 0, 4, all4)
    assert rc == -1 and b"null dims" in err
    rc, err = _call(lib, ext, d16, 0, 4, all4, args=False)
    assert rc == -1 and b"null args" in err
    a = ext._MlpFwd(*[0x1000] * len(ext.MLP_FWD_FIELDS))
    a.W2_init = None
    assert lib.ttt_hip_mlp_forward_chunk_pair16(ctypes.byref(d16), ctypes.byref(a), 0, 4, None, None, None, None, 0x2000, need, None) == -1
    assert b"null pointer argument W2_init" in lib.ttt_hip_last_error()


def test_binding_checks_tensors_before_the_call():
    """the pair entries check their tensors against the contract of ``ttt_forward``, field by field (no CPU path)"""
    import pytest
    import test_time_training as ext
    good = A._scan_tensors(ext.MLP_FWD_FIELDS, True, on_device=False)
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_forward_pair16(*good.values(), A._G)
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_forward_chunk_pair16(*good.values(), A._G, 0, 1)
