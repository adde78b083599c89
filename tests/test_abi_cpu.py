"""The C-ABI library builds for gfx950 without a GPU, loads, and exports every symbol that
include/ttt_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "ttt_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ttt_hip_\w+)\s*\(", src)))


_C_KINDS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "unsigned": ctypes.c_uint, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "void": None}


def _c_kind(decl, is_param):
    """ctypes kind of a C return type / parameter declaration: ``const char*`` -> c_char_p, any other pointer -> "pointer",
    a value type -> its ctypes type (the parameter's name dropped)"""
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl:
        return ctypes.c_char_p if decl.startswith("const char *") and decl.count("*") == 1 else "pointer"
    words = [w for w in decl.split() if w != "const"]
    return _C_KINDS[" ".join(words[:-1] if is_param else words)]


def _declared_prototypes(header_path=os.path.join(ROOT, "include", "ttt_hip.h")):
    """{symbol: (return kind, [parameter kinds])} of every ttt_hip_* function declared in a header of the library (default:
    include/ttt_hip.h; the tests of the other headers call this on theirs); every ``ttt_hip_*(`` of the header must parse"""
    src = re.sub(r"/\*.*?\*/", "", open(header_path).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(ttt_hip_\w+)\s*\(", src)))
    protos = {}
    for ret, name, params in re.findall(r"(?:^|[;}{])\s*((?:const\s+)?\w+[\s*]+)(ttt_hip_\w+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        assert name not in protos, name
        params = [] if params.strip() == "void" else params.split(",")
        protos[name] = (_c_kind(ret, False), [_c_kind(p, True) for p in params])
    assert sorted(protos) == names
    return protos


def _ctypes_kind(t):
    if t is ctypes.c_char_p or t is None:
        return t
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return "pointer"
    return t


def test_prototype_table_matches_the_header():
    """Every function of include/ttt_hip.h has an entry in the binding's prototype table with the declared number of parameters,
    the declared kind in each position and the declared return kind (a parameter of another width or a missing one would be
    truncated or misread silently at the call)."""
    import test_time_training as ext
    declared = _declared_prototypes()
    assert sorted(declared) == _declared_symbols() == sorted(ext._PROTOTYPES) and len(declared) == 46
    for name, (ret, params) in declared.items():
        restype, argtypes = ext._PROTOTYPES[name]
        assert _ctypes_kind(restype) == ret, (name, restype, ret)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for i, (a, c) in enumerate(zip(argtypes, params)):
            assert _ctypes_kind(a) == c, (name, i, a, c)
            if c == "pointer":
                assert ctypes.sizeof(a) == ctypes.sizeof(ctypes.c_void_p), (name, i, a)
    # the parser tells the kinds apart (a table that passed by accident would pass here too)
    assert declared["ttt_hip_pre_backward_ld"][1][17] is ctypes.c_int64 and declared["ttt_hip_mlp_forward"][1][3] is ctypes.c_size_t
    assert declared["ttt_hip_post_forward"][1][4] is ctypes.c_float and declared["ttt_hip_debug_option"][1] == [ctypes.c_char_p, ctypes.c_int]
    assert declared["ttt_hip_last_error"] == (ctypes.c_char_p, []) and declared["ttt_hip_debug_sweep_error"] == (ctypes.c_uint, [])
    assert declared["ttt_hip_mlp_forward_workspace"] == (ctypes.c_size_t, ["pointer"]) and declared["ttt_hip_debug_timing"] == (None, ["pointer"])
    assert declared["ttt_hip_stream_create_masked"][1] == ["pointer", ctypes.c_int, "pointer"]


def test_prototypes_are_applied_at_load():
    import test_time_training as ext
    lib = ext.load_library()
    for name in ext.EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
        assert (fn.restype, list(fn.argtypes)) == (ext._PROTOTYPES[name][0], ext._PROTOTYPES[name][1]), name


def test_library_exports_every_declared_symbol():
    import test_time_training as ext
    if not os.path.exists(ext.library_path()):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(ext.library_path())
    names = _declared_symbols()
    assert len(names) >= 11
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/ttt_hip.h but not exported"
    assert sorted(ext.EXPORTED_SYMBOLS) == names
    lib.ttt_hip_abi_version.restype = ctypes.c_int
    assert lib.ttt_hip_abi_version() == 5


def test_argument_validation_without_gpu():
    """Dimension / impl validation happens before any launch, so it can be exercised on CPU."""
    import test_time_training as ext
    lib = ext.load_library()
    d = ext._Dims(1, 2, 4, 64, 64, 2, 0, 0, 1e-8)
    assert lib.ttt_hip_resolve_impl(ctypes.byref(d), 1, 0) in (1, 2)
    bad = ext._Dims(1, 2, 4, 24, 64, 2, 0, 0, 1e-8)        # CS=24 unsupported by every kernel family
    assert lib.ttt_hip_resolve_impl(ctypes.byref(bad), 1, 0) == -1
    neg = ext._Dims(0, 2, 4, 64, 64, 2, 0, 0, 1e-8)
    assert lib.ttt_hip_resolve_impl(ctypes.byref(neg), 1, 0) == -1
    assert b"dimension" in lib.ttt_hip_last_error()
    assert lib.ttt_hip_mlp_forward_workspace(ctypes.byref(d)) > 0 or lib.ttt_hip_resolve_impl(ctypes.byref(d), 1, 0) == 2


def test_cpu_tensors_are_rejected():
    import torch
    import test_time_training as ext
    x = torch.zeros(1, 1, 2, 16, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="HIP device"):
        ext.ttt_forward(x, x, x, x, *[x] * 11, 1)


# ------------------------------------------------------------------------------------------------ tensor contracts of the scan ops
_B, _NH, _NC, _CS, _F, _G, _K = 1, 2, 3, 16, 64, 2, 2
_TILE_FIELDS = ("XQ", "XK", "XV", "XQW", "grad_L_XQW", "grad_L_XQ", "grad_L_XK", "grad_L_XV")


def _contract_of(field, mlp):
    """(shape, dtype) of a field of the scan ops' argument structs at the geometry above with bf16 activations, written from the
    comments of include/ttt_hip.h (not from the binding's tables)"""
    import torch
    bf, f32 = torch.bfloat16, torch.float32
    H = 4 * _F if mlp else _F
    if field in _TILE_FIELDS:
        return (_B, _NH, _NC, _CS, _F), bf
    if field in ("last_eta", "grad_L_last_eta"):
        return (_B, _NH, _NC, _CS, 1), bf
    if field in ("ttt_norm_weight", "ttt_norm_bias"):
        return ((1, _NH, 1, _F) if mlp else (_NH, _F)), f32
    if field in ("grad_L_ttt_norm_weight", "grad_L_ttt_norm_bias"):
        return (_B, _NH, 1, _F), f32
    m = re.fullmatch(r"(?:grad_L_)?(W1|b1|W2|b2)_(init|last|checkpoints|init_group)", field)
    if m:
        lead = {"checkpoints": (_B, _NH, _K), "init_group": (_B, _NH, _G)}.get(m.group(2), (_B, _NH))
        return lead + {"W1": (_F, H), "b1": (1, H), "W2": (H, _F), "b2": (1, _F)}[m.group(1)], f32
    assert mlp and field.endswith("_group"), field                  # the twelve re-materialisation buffers of the TTT-MLP backward
    if field.startswith("std_"):
        return (_B, _NH, _G, _CS, 1), f32
    wide = field in ("X2_group", "Z1_group", "Z1_bar_group", "X2_bar_group", "grad_l_wrt_Z1_group")
    return (_B, _NH, _G, _CS, H if wide else _F), bf


def _scan_ops(ext):
    """(name, wrapper, field names, is TTT-MLP, trailing arguments) of the five scan wrappers"""
    return (("ttt_forward", ext.ttt_forward, ext.MLP_FWD_FIELDS, True, (_G,)),
            ("ttt_forward_chunk", ext.ttt_forward_chunk, ext.MLP_FWD_FIELDS, True, (_G, 0, 2)),
            ("ttt_backward", ext.ttt_backward, ext.MLP_BWD_FIELDS, True, (_G,)),
            ("ttt_linear_forward", ext.ttt_linear_forward, ext.LIN_FWD_FIELDS, False, (_G,)),
            ("ttt_linear_backward", ext.ttt_linear_backward, ext.LIN_BWD_FIELDS, False, (_G,)))


def _scan_tensors(fields, mlp, on_device):
    """correct CPU tensors for ``fields``; ``on_device``: of a Tensor subclass that claims to live on a HIP device, so that the
    binding's checks behind the device check can run without one (nothing is launched: the tests make a later check fail)"""
    import torch

    class OnDevice(torch.Tensor):
        is_cuda = property(lambda self: True)

    ts = {}
    for f in fields:
        shape, dtype = _contract_of(f, mlp)
        t = torch.zeros(shape, dtype=dtype)
        ts[f] = t.as_subclass(OnDevice) if on_device else t
    return ts


def _wrong_shape(t):
    return t.new_zeros(tuple(t.shape[:-1]) + (t.shape[-1] + 1,)).as_subclass(type(t))


def test_scan_wrappers_report_the_device_first():
    """CPU tensors of the right shape and dtype: every scan wrapper stops at its first field's device check - also when a later
    field has a wrong shape (checks run field by field, in the struct's order)."""
    import test_time_training as ext
    for name, fn, fields, mlp, tail in _scan_ops(ext):
        ts = _scan_tensors(fields, mlp, on_device=False)
        with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
            fn(*ts.values(), *tail)
        ts[fields[1]] = _wrong_shape(ts[fields[1]])
        with pytest.raises(RuntimeError, match=r"^XQ: tensor must live on a HIP device"):
            fn(*ts.values(), *tail)
    with pytest.raises(RuntimeError, match=r"XQ: expected a 5-D tensor"):
        import torch
        ext.ttt_forward(*[torch.zeros(2, 3, 16, 64)] * 15, 1)


def test_scan_wrappers_name_the_field_and_the_expected_shape():
    """Tensors that pass the device check: a wrong shape on any one field is reported with that field's name and the shape the
    contract asks for at B = 1, NH = 2, NC = 3, CS = 16, F = 64, G = 2 (K = 2), before anything is launched."""
    import test_time_training as ext
    for name, fn, fields, mlp, tail in _scan_ops(ext):
        good = _scan_tensors(fields, mlp, on_device=True)
        for f in fields:
            ts = dict(good)
            ts[f] = _wrong_shape(good[f])
            want = _contract_of(f, mlp)[0]
            if f == "XQ":                           # the sizes are XQ's: the next field no longer fits them
                f, want = "XK", tuple(ts["XQ"].shape)
            with pytest.raises(RuntimeError, match=re.escape(f"{f}: expected shape {want}, got ")):
                fn(*ts.values(), *tail)


def test_scan_check_order_and_optional_fields():
    """Per field: type, device, dtype, shape, contiguity.  Only the sixteen re-materialisation buffers of ttt_backward may be None."""
    import torch
    import test_time_training as ext
    good = _scan_tensors(ext.MLP_BWD_FIELDS, True, on_device=True)
    call = lambda ts: ext.ttt_backward(*ts.values(), _G)
    bad = _wrong_shape(good["XV"])
    with pytest.raises(RuntimeError, match="XV: expected dtype torch.bfloat16, got torch.float32"):
        call({**good, "XV": bad.float().as_subclass(type(bad))})
    with pytest.raises(RuntimeError, match=r"XV: expected shape \(1, 2, 3, 16, 64\), got \(1, 2, 3, 64, 16\)"):
        call({**good, "XV": good["XV"].transpose(3, 4)})
    with pytest.raises(RuntimeError, match="XV: tensor must be contiguous"):
        call({**good, "XV": torch.zeros(1, 2, 3, 16, 128, dtype=torch.bfloat16).as_subclass(type(bad))[..., ::2]})
    with pytest.raises(TypeError, match="grad_L_XV: expected a torch.Tensor"):
        call({**good, "grad_L_XV": None})
    scratch = ext.MLP_BWD_FIELDS[11:27]
    assert len(scratch) == 16 and all(f.endswith("_group") for f in scratch)
    sizes = dict(B=_B, NH=_NH, NC=_NC, CS=_CS, F=_F, G=_G, K=_K, H=4 * _F)
    ts = {**good, **dict.fromkeys(scratch)}
    args = ext._fill_args(ext._MlpBwd, ext._MLP_BWD_SPEC, tuple(ts.values()), sizes, torch.bfloat16, optional=ext._MLP_BWD_SCRATCH)
    for f in ext.MLP_BWD_FIELDS:
        assert getattr(args, f) == (None if f in scratch else good[f].data_ptr()), f
    with pytest.raises(TypeError, match="W1_init_group: expected a torch.Tensor"):
        ext._fill_args(ext._MlpBwd, ext._MLP_BWD_SPEC, tuple(ts.values()), sizes, torch.bfloat16)


def test_forward_workspace_is_the_pair_scan_ring():
    """ABI 5 (round 6): the TTT-MLP forward at mini-batches of 64 on the MFMA scan asks for its ring of state records - per (b,h) four records of
    65.25 KiB (pack(W1'), pack(W2'), b1', b2') + two 128-byte flag lines (csrc/ttt_mfma2.hip) -, every other forward for nothing."""
    import test_time_training as ext
    lib = ext.load_library()
    d = ext._Dims(1, 48, 804, 64, 64, 16, 0, 2, 1e-8)                 # bf16, impl = MFMA
    assert lib.ttt_hip_mlp_forward_workspace(ctypes.byref(d)) == 48 * (4 * (64 * 1024 + 1024 + 256) + 256)
    d16 = ext._Dims(2, 48, 21948, 16, 64, 21948, 0, 2, 1e-8)          # the sampling geometry: mini-batches of 16
    assert lib.ttt_hip_mlp_forward_workspace(ctypes.byref(d16)) == 0
    assert lib.ttt_hip_linear_forward_workspace(ctypes.byref(d16)) == 0


def test_pipeline_part_plan_tapers_and_covers_every_group(monkeypatch):
    """ttt_amd/models/ssm/pipeline.py: the parts of the pipelined layer forward are whole checkpoint groups, cover the scan exactly, and taper
    towards the end by default (round 6); TTT_PIPELINE_WEIGHTS overrides."""
    from ttt_amd.models.ssm.pipeline import part_group_counts, plan_parts
    monkeypatch.delenv("TTT_PIPELINE_WEIGHTS", raising=False)
    assert part_group_counts(51, 5) == [16, 16, 11, 6, 2] and part_group_counts(51, 4) == [16, 17, 12, 6]
    for K, n in ((51, 5), (18, 5), (8, 4), (343, 8), (165, 5), (10, 5), (300, 7)):
        c = part_group_counts(K, n)
        assert len(c) == n and sum(c) == K and min(c) >= 1, (K, n, c)
        assert c[-1] <= c[0]
    monkeypatch.setenv("TTT_PIPELINE_WEIGHTS", "equal")
    assert part_group_counts(51, 4) == [13, 13, 13, 12]
    monkeypatch.setenv("TTT_PIPELINE_WEIGHTS", "1,1,2")
    assert part_group_counts(8, 3) == [2, 2, 4]
    monkeypatch.delenv("TTT_PIPELINE_WEIGHTS")
    parts = plan_parts(None, 804 * 64, 64, 16, 5)
    assert [p[0] for p in parts] == [0, 256, 512, 688, 784] and sum(p[1] for p in parts) == 804
    assert parts[-1][2] == [(784 * 64, 804 * 64)]

