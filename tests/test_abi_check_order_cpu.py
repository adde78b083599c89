"""The ORDER of the argument checks of the scan entries of libttt_hip.so (csrc/capi.hip).  The ABI tests of the six headers null one
thing at a time: they pin every message, not which of two faults is reported.  Each case here gives a call two faults and asserts the
one that the entry meets first (fake pointers, no GPU: every call is refused before a launch)."""
import ctypes

import pytest

import test_abi_bwd_parts_cpu as L
import test_abi_lin_bwd_front_cpu as FR
import test_abi_mlp_bwd_parts_cpu as M
import test_abi_pair16_cpu as P
import test_abi_parts_cpu as C

FAKE, BIG = L.FAKE, L.BIG
RANGE = b"inside [0, K)"
STEPS = b"inside [0, NC)"
# (recompute, sweep, a geometry the entry serves, the same with fp32 activations, the words of its refusal)
LINEAR = (L._recompute, L._sweep, lambda ext: L._dims16(ext), lambda ext: L._dims16(ext, act=1), b"only the MFMA sweep")
MLP = (M._recompute, M._sweep, lambda ext: M._dims(ext), lambda ext: M._dims(ext, act=1), M.REFUSED)


def _lib():
    import test_time_training as ext
    return ext.load_library(), ext


@pytest.mark.parametrize("family", [LINEAR, MLP], ids=["linear", "mlp"])
@pytest.mark.parametrize("which", [0, 1], ids=["recompute", "sweep"])
def test_group_entries_check_dims_args_fields_geometry_range_slots(family, which):
    lib, ext = _lib()
    call, good, fp32, refused = family[which], family[2](ext), family[3](ext), family[4]
    rc, err = call(lib, ext, None, 0, 1, a=False)
    assert rc == -1 and b"null dims" in err, err
    rc, err = call(lib, ext, fp32, 0, 1, null="XK")
    assert rc == -1 and b"null pointer argument XK" in err, err
    rc, err = call(lib, ext, fp32, 0, 4)                       # K = 3
    assert rc == -1 and refused in err, err
    rc, err = call(lib, ext, good, 0, 4, slots=None)
    assert rc == -1 and RANGE in err, err


@pytest.mark.parametrize("family", [LINEAR, MLP], ids=["linear", "mlp"])
def test_sweeps_check_the_slots_before_the_carry(family):
    lib, ext = _lib()
    rc, err = family[1](lib, ext, family[2](ext), 0, 3, slots=None, carry=None)
    assert rc == -1 and b"slot workspace null or smaller" in err, err


def test_mlp_sweep_checks_slot_size_then_alignment_then_the_carry():
    lib, ext = _lib()
    d = M._dims(ext)
    need = lib.ttt_hip_mlp_backward_parts_slots(ctypes.byref(d), 3)
    rc, err = M._sweep(lib, ext, d, 0, 3, slots=0x1008, nbytes=need - 1)
    assert rc == -1 and b"slot workspace null or smaller" in err, err
    rc, err = M._sweep(lib, ext, d, 0, 3, slots=0x1008, carry=None)
    assert rc == -1 and b"the slot workspace must be 16-byte aligned" in err, err


@pytest.mark.parametrize("call", [FR._front, FR._chain])
def test_front_and_chain_check_cs64_range_records_carry(call):
    lib, ext = _lib()
    rc, err = call(lib, ext, FR._dims64(ext), 0, 4)            # explicit TTT_IMPL_MFMA, K = 3
    assert rc == -1 and b"only mini-batches of 16" in err, err
    rc, err = call(lib, ext, FR._dims16(ext), 0, 4, records=None)
    assert rc == -1 and RANGE in err, err
    if call is FR._chain:
        rc, err = call(lib, ext, FR._dims16(ext), 0, 3, records=None, carry=None)
        assert rc == -1 and b"record workspace null or smaller" in err, err


def _d(ext, CS=16, F=64, act=0, impl=0):
    return ext._Dims(1, 2, 12, CS, F, 4, act, impl, 1e-8)                # NC = 12, G = 4


def test_linear_forward_chunk_checks_fields_geometry_steps_finals():
    lib, ext = _lib()
    fp32 = _d(ext, act=1)
    a = ext._LinFwd(*[FAKE] * len(ext.LIN_FWD_FIELDS))
    a.W1_init = None
    assert lib.ttt_hip_linear_forward_chunk(ctypes.byref(fp32), ctypes.byref(a), 0, 4, None, None, None, 0, None) == -1
    assert b"null pointer argument W1_init" in lib.ttt_hip_last_error()
    rc, err = C._chunk_call(lib, ext, fp32, 0, 13, (True, True))
    assert rc == -1 and b"only the MFMA scan" in err, err
    rc, err = C._chunk_call(lib, ext, _d(ext), 0, 13, (True, False))
    assert rc == -1 and STEPS in err, err


def _mlp_chunk(lib, ext, d, step0, nsteps, finals):
    a = ext._MlpFwd(*[FAKE] * len(ext.MLP_FWD_FIELDS))
    rc = lib.ttt_hip_mlp_forward_chunk(ctypes.byref(d), ctypes.byref(a), step0, nsteps, *[FAKE if f else None for f in finals], None, 0, None)
    return rc, lib.ttt_hip_last_error()


def test_mlp_forward_chunk_checks_geometry_steps_groups_finals():
    lib, ext = _lib()
    all4 = (True,) * 4
    rc, err = _mlp_chunk(lib, ext, _d(ext, act=1), 0, 13, all4)
    assert rc == -1 and b"only the MFMA scan" in err, err
    d64 = _d(ext, CS=64)
    assert lib.ttt_hip_resolve_impl(ctypes.byref(d64), 1, 0) == 2
    rc, err = _mlp_chunk(lib, ext, d64, 5, 8, all4)            # outside [0, 12) and off the groups of 4
    assert rc == -1 and STEPS in err, err
    rc, err = _mlp_chunk(lib, ext, d64, 1, 2, (True, True, True, False))
    assert rc == -1 and b"checkpoint-group boundaries" in err, err


def test_mlp_forward_chunk_pair16_checks_geometry_steps_finals_workspace():
    lib, ext = _lib()
    rc, err = P._call(lib, ext, _d(ext, CS=64), 0, 13, (True,) * 4, wsb=1 << 30)
    assert rc == -1 and b"mlp_forward_chunk_pair16" in err and b"mini-batches of 16" in err, err
    rc, err = P._call(lib, ext, _d(ext), 0, 13, (True, True, False, True))
    assert rc == -1 and STEPS in err, err
    rc, err = P._call(lib, ext, _d(ext), 0, 12, (True, True, False, True), ws=None)
    assert rc == -1 and b"all four final-state buffers or none" in err, err


def _backward(lib, ext, mlp, d, null=(), ws=None, wsb=0):
    struct, fields = (ext._MlpBwd, ext.MLP_BWD_FIELDS) if mlp else (ext._LinBwd, ext.LIN_BWD_FIELDS)
    a = struct(*[None if f in null else FAKE for f in fields])
    fn = lib.ttt_hip_mlp_backward if mlp else lib.ttt_hip_linear_backward
    rc = fn(ctypes.byref(d), ctypes.byref(a), ws, wsb, None)
    return rc, lib.ttt_hip_last_error()


@pytest.mark.parametrize("mlp", [False, True], ids=["linear", "mlp"])
def test_backward_checks_fields_then_geometry_then_workspace(mlp):
    lib, ext = _lib()
    what = b"mlp_backward" if mlp else b"linear_backward"
    f32 = _d(ext, F=32, impl=2)                                # TTT_IMPL_MFMA serves F = 64 only
    rc, err = _backward(lib, ext, mlp, f32, null=("grad_L_XV",))
    assert rc == -1 and b"null pointer argument grad_L_XV" in err, err
    rc, err = _backward(lib, ext, mlp, f32)
    assert rc == -1 and what + b": unsupported geometry" in err, err
    if mlp:
        # the one geometry with a workspace: mini-batches of 64 on the MFMA backward (0 where no device answers for it)
        d64 = _d(ext, CS=64, impl=2)
        if lib.ttt_hip_mlp_backward_workspace(ctypes.byref(d64)):
            rc, err = _backward(lib, ext, True, d64)
            assert rc == -1 and b"mlp_backward: workspace too small" in err, err
            rc, err = _backward(lib, ext, True, _d(ext, CS=64, F=32, impl=2))
            assert rc == -1 and b"mlp_backward: unsupported geometry" in err, err


def test_generic_mlp_backward_asks_for_the_state_buffers_last():
    """the four *_init_group buffers are checked behind the geometry, the workspace and the sticky error word: a null W1_init_group is
    reported only when every other field is there"""
    lib, ext = _lib()
    d = _d(ext, impl=1)
    scratch = ext.MLP_BWD_FIELDS[11:27]
    for f in ext.MLP_BWD_FIELDS:
        if f in scratch or f == "XQW":
            continue
        rc, err = _backward(lib, ext, True, d, null=("W1_init_group", f), ws=FAKE, wsb=BIG)
        assert rc == -1 and f"null pointer argument {f}".encode() in err and b"W1_init_group" not in err, (f, err)
    rc, err = _backward(lib, ext, True, d, null=("W1_init_group",))
    assert rc == -1 and b"mlp_backward: workspace too small" in err, err
    rc, err = _backward(lib, ext, True, _d(ext, F=32, act=0, impl=2), null=("W1_init_group",), ws=FAKE, wsb=BIG)
    assert rc == -1 and b"mlp_backward: unsupported geometry" in err, err
    rc, err = _backward(lib, ext, True, d, null=("W1_init_group",), ws=FAKE, wsb=BIG)
    assert rc == -1 and b"null pointer argument W1_init_group" in err, err
