"""include/ttt_hip_lin_split16.h, the seventh header of libttt_hip.so (the TTT-Linear forward scan at mini-batches of 16 with its
output path on a second wave): its declaration against the binding's seventh prototype table, the export, the other six tables as they
were, and every refusal of ``ttt_hip_linear_forward_chunk_split16`` that is reached before a launch (fake pointers, no GPU)."""
import ctypes
import os

import pytest

import test_abi_cpu as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ttt_hip_lin_split16.h")
ENTRY = "ttt_hip_linear_forward_chunk_split16"

# the six older tables: symbol -> parameter list in the binding's notation (restype int unless given)
Z = ctypes.c_size_t
OLDER = {
    "_PROTOTYPES_PARTS": {"ttt_hip_linear_forward_chunk": ("2p 2i 3p z p",)},
    "_PROTOTYPES_BWD_PARTS": {"ttt_hip_linear_backward_parts_slots": ("p i", Z), "ttt_hip_linear_backward_parts_carry": ("p", Z),
                              "ttt_hip_linear_recompute_groups": ("2p 2i p z p",), "ttt_hip_linear_sweep_groups": ("2p 2i p z p z p",)},
    "_PROTOTYPES_PAIR16": {"ttt_hip_mlp_forward_pair16_workspace": ("p", Z), "ttt_hip_mlp_forward_chunk_pair16": ("2p 2i 5p z p",)},
    "_PROTOTYPES_MLP_BWD_PARTS": {"ttt_hip_mlp_backward_parts_slots": ("p i", Z), "ttt_hip_mlp_backward_parts_carry": ("p", Z),
                                  "ttt_hip_mlp_recompute_groups": ("2p 2i p z p",), "ttt_hip_mlp_sweep_groups": ("2p 2i p z p z p",)},
    "_PROTOTYPES_LIN_BWD_FRONT": {"ttt_hip_linear_backward_front_records": ("p i", Z), "ttt_hip_linear_front_groups": ("2p 2i p z p z p",),
                                  "ttt_hip_linear_chain_groups": ("2p 2i p z p z p z p",)},
}


def test_seventh_prototype_table_matches_the_seventh_header():
    import test_time_training as ext
    declared = A._declared_prototypes(HEADER)
    assert sorted(declared) == sorted(ext._PROTOTYPES_LIN_SPLIT16) == [ENTRY]
    for name, (ret, params) in declared.items():
        restype, argtypes = ext._PROTOTYPES_LIN_SPLIT16[name]
        assert A._ctypes_kind(restype) == ret, (name, restype, ret)
        assert [A._ctypes_kind(a) for a in argtypes] == params, (name, argtypes, params)
    p = "pointer"
    assert declared[ENTRY] == (ctypes.c_int, [p, p, ctypes.c_int, ctypes.c_int, p, p, p, ctypes.c_size_t, p])
    # the signature of ttt_hip_linear_forward_chunk
    assert ext._PROTOTYPES_LIN_SPLIT16[ENTRY] == ext._PROTOTYPES_PARTS["ttt_hip_linear_forward_chunk"]
    src = open(HEADER).read()
    assert '#include "ttt_hip.h"' in src and "#define TTT_HIP_ABI_VERSION" not in src
    assert not set(declared) & set(A._declared_symbols())


def test_the_other_six_tables_are_unchanged():
    import test_time_training as ext
    assert len(ext.EXPORTED_SYMBOLS) == 46 and ext.EXPORTED_SYMBOLS == tuple(ext._PROTOTYPES)
    assert sorted(A._declared_symbols()) == sorted(ext._PROTOTYPES), "ttt_hip.h keeps its 46 exports"
    seen = set(ext._PROTOTYPES)
    for table, want in OLDER.items():
        have = getattr(ext, table)
        assert {k: ext._sig(*v) for k, v in want.items()} == have, table
        assert not seen & set(have), "a symbol belongs to one header"
        seen |= set(have)
    assert ENTRY not in seen


def test_library_exports_the_symbol_with_its_prototype_and_keeps_abi_5():
    import test_time_training as ext
    lib = ext.load_library()
    assert hasattr(ctypes.CDLL(ext.library_path()), ENTRY)
    fn = getattr(lib, ENTRY)
    assert (fn.restype, list(fn.argtypes)) == ext._PROTOTYPES_LIN_SPLIT16[ENTRY]
    assert lib.ttt_hip_abi_version() == 5 == ext.ABI_VERSION
    assert callable(ext.ttt_linear_forward_split16) and callable(ext.ttt_linear_forward_chunk_split16)


def _call(lib, ext, dims, step0, nsteps, finals, args=True):
    fake = 0x1000                                  # never dereferenced: every case below is refused before the launch
    a = ext._LinFwd(*[fake] * len(ext.LIN_FWD_FIELDS))
    rc = getattr(lib, ENTRY)(ctypes.byref(dims) if dims is not None else None, ctypes.byref(a) if args else None,
                             step0, nsteps, *[fake if f else None for f in finals], None, 0, None)
    return rc, lib.ttt_hip_last_error()


def test_split16_refusals_without_gpu():
    """CS = 64 (under auto and on an explicit MFMA), fp32, F != 64, the generic kernels ; a part not inside [0, NC) ; exactly one final ;
    the null arguments the existing chunk entry refuses - each negative, each message names the entry"""
    import test_time_training as ext
    lib = ext.load_library()
    both = (True, True)
    for impl in (0, 2):
        assert lib.ttt_hip_resolve_impl(ctypes.byref(ext._Dims(1, 2, 12, 16, 64, 4, 0, impl, 1e-8)), 0, 0) == 2
    d16 = ext._Dims(1, 2, 12, 16, 64, 4, 0, 0, 1e-8)                   # bf16, impl = AUTO, G = 4
    refused = {"CS = 64 under auto": ext._Dims(1, 2, 12, 64, 64, 4, 0, 0, 1e-8),
               "CS = 64, MFMA requested": ext._Dims(1, 2, 12, 64, 64, 4, 0, 2, 1e-8),
               "fp32 activations": ext._Dims(1, 2, 12, 16, 64, 4, 1, 0, 1e-8),
               "fp32 activations, MFMA requested": ext._Dims(1, 2, 12, 16, 64, 4, 1, 2, 1e-8),
               "F = 32": ext._Dims(1, 2, 12, 16, 32, 4, 0, 0, 1e-8),
               "F = 128, MFMA requested": ext._Dims(1, 2, 12, 16, 128, 4, 0, 2, 1e-8),
               "the generic kernels": ext._Dims(1, 2, 12, 16, 64, 4, 0, 1, 1e-8)}
    for what, d in refused.items():
        for finals in (both, (False, False)):
            rc, err = _call(lib, ext, d, 0, 4, finals)
            assert rc < 0 and b"linear_forward_chunk_split16" in err and b"mini-batches of 16" in err, (what, err)
    for d in (d16, ext._Dims(1, 2, 12, 16, 64, 4, 0, 2, 1e-8)):
        for step0, nsteps in ((-1, 2), (0, 0), (3, -1), (5, 8), (12, 1), (0, 13), (2 ** 31 - 1, 2)):
            rc, err = _call(lib, ext, d, step0, nsteps, both)
            assert rc < 0 and b"linear_forward_chunk_split16" in err and b"inside [0, NC)" in err, (step0, nsteps, err)
        for step0, nsteps in ((1, 2), (5, 6), (0, 12), (11, 1)):
            for finals in ((True, False), (False, True)):
                rc, err = _call(lib, ext, d, step0, nsteps, finals)
                assert rc < 0 and b"linear_forward_chunk_split16: give both final-state buffers or neither" in err, (step0, nsteps, err)
    rc, err = _call(lib, ext, None, 0, 4, both)
    assert rc < 0 and b"null dims" in err
    rc, err = _call(lib, ext, d16, 0, 4, both, args=False)
    assert rc < 0 and b"null args" in err
    for f in ext.LIN_FWD_FIELDS:
        a = ext._LinFwd(*[0x1000] * len(ext.LIN_FWD_FIELDS))
        setattr(a, f, None)
        assert getattr(lib, ENTRY)(ctypes.byref(d16), ctypes.byref(a), 0, 4, None, None, None, 0, None) < 0
        assert f"null pointer argument {f}".encode() in lib.ttt_hip_last_error()


def test_split16_check_order_is_the_chunk_entry_s():
    """two faults per call: dims, then args, then the fields, then the geometry, then the steps, then the finals"""
    import test_time_training as ext
    lib = ext.load_library()
    fp32 = ext._Dims(1, 2, 12, 16, 64, 4, 1, 0, 1e-8)
    a = ext._LinFwd(*[0x1000] * len(ext.LIN_FWD_FIELDS))
    a.W1_init = None
    assert getattr(lib, ENTRY)(ctypes.byref(fp32), ctypes.byref(a), 0, 13, None, None, None, 0, None) == -1
    assert b"null pointer argument W1_init" in lib.ttt_hip_last_error()
    rc, err = _call(lib, ext, fp32, 0, 13, (True, False))
    assert rc == -1 and b"mini-batches of 16" in err, err
    rc, err = _call(lib, ext, ext._Dims(1, 2, 12, 16, 64, 4, 0, 0, 1e-8), 0, 13, (True, False))
    assert rc == -1 and b"inside [0, NC)" in err, err


def test_binding_checks_tensors_before_the_call():
    """the split entries check their tensors against the contract of ``ttt_linear_forward``, field by field (no CPU path)"""
    import test_time_training as ext
    good = A._scan_tensors(ext.LIN_FWD_FIELDS, False, on_device=False)
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_linear_forward_split16(None, *good.values(), A._G)
    with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
        ext.ttt_linear_forward_chunk_split16(None, *good.values(), A._G, 0, 1)
