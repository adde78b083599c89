"""Drop-in replacement for the reference's un-vendored ``test_time_training`` CUDA extension
(ttt-tk), backed by hand-written HIP kernels for MI355X / gfx950 behind the C ABI of
``include/ttt_hip.h``.

``ttt_forward`` / ``ttt_backward`` take exactly the positional tensors the reference passes at
``ttt/models/ssm/mlp_tk.py:116-133`` and ``:227-275``: every buffer (outputs, checkpoints,
re-materialisation scratch) is allocated by the caller, results are written in place, nothing
is returned, kernels are enqueued on the current torch stream without synchronising.

``ttt_linear_forward`` / ``ttt_linear_backward`` expose the TTT-Linear kernels with the tensor
contract of the reference's Triton launch sites (``ttt/models/ssm/linear_triton.py:98-129``,
``:203-246``).

There is no CPU path and no fallback: if ``lib/libttt_hip.so`` is missing or a tensor is not on
a HIP device the call raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libttt_hip.so")

IMPL_AUTO, IMPL_GENERIC, IMPL_MFMA = 0, 1, 2
_IMPL_NAMES = {"auto": IMPL_AUTO, "generic": IMPL_GENERIC, "mfma": IMPL_MFMA}

# LayerNorm epsilon of the reference's ops path (ops/utils.py:4,21); the Triton kernels use 1e-6
# (kernels/linear_forward.py:111) - SURVEY.md hazard C1.  Adjustable for experiments.
_state = {"impl": IMPL_AUTO, "eps": 1e-8}


class _Dims(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("B", "NH", "NC", "CS", "F", "G", "act_dtype", "impl")] + [("eps", ctypes.c_float)]


def _ptr_struct(name, fields):
    return type(name, (ctypes.Structure,), {"_fields_": [(f, ctypes.c_void_p) for f in fields]})


MLP_FWD_FIELDS = ("XQ", "XK", "XV", "last_eta", "ttt_norm_weight", "ttt_norm_bias", "W1_init", "b1_init", "W2_init",
                  "b2_init", "W1_checkpoints", "b1_checkpoints", "W2_checkpoints", "b2_checkpoints", "XQW")
MLP_BWD_FIELDS = ("XQ", "XK", "XV", "last_eta", "ttt_norm_weight", "ttt_norm_bias", "W1_checkpoints", "b1_checkpoints",
                  "W2_checkpoints", "b2_checkpoints", "XQW", "W1_init_group", "b1_init_group", "W2_init_group",
                  "b2_init_group", "x_hat_ln_group", "std_ln_group", "X2_group", "Z1_group", "Z1_bar_group", "X2_bar_group",
                  "grad_l_wrt_Z2_group", "grad_l_wrt_Z1_group", "x_hat_fused_group", "grad_x_hat_fused_group",
                  "grad_output_fused_group", "std_fused_group", "grad_L_W1_last", "grad_L_b1_last", "grad_L_W2_last",
                  "grad_L_b2_last", "grad_L_XQW", "grad_L_ttt_norm_weight", "grad_L_ttt_norm_bias", "grad_L_W1_init",
                  "grad_L_b1_init", "grad_L_W2_init", "grad_L_b2_init", "grad_L_last_eta", "grad_L_XQ", "grad_L_XK", "grad_L_XV")
LIN_FWD_FIELDS = ("XQ", "XK", "XV", "last_eta", "ttt_norm_weight", "ttt_norm_bias", "W1_init", "b1_init",
                  "W1_checkpoints", "b1_checkpoints", "XQW")
LIN_BWD_FIELDS = ("XQ", "XK", "XV", "last_eta", "ttt_norm_weight", "ttt_norm_bias", "W1_checkpoints", "b1_checkpoints",
                  "grad_L_W1_last", "grad_L_b1_last", "grad_L_XQW", "W1_init_group", "b1_init_group",
                  "grad_L_ttt_norm_weight", "grad_L_ttt_norm_bias", "grad_L_W1_init", "grad_L_b1_init", "grad_L_last_eta",
                  "grad_L_XQ", "grad_L_XK", "grad_L_XV")

_MlpFwd = _ptr_struct("_MlpFwd", MLP_FWD_FIELDS)
_MlpBwd = _ptr_struct("_MlpBwd", MLP_BWD_FIELDS)
_LinFwd = _ptr_struct("_LinFwd", LIN_FWD_FIELDS)
_LinBwd = _ptr_struct("_LinBwd", LIN_BWD_FIELDS)

# Tensor contract of each argument struct, keyed by its *_FIELDS names: (shape, dtype).  A shape is written in the names of
# include/ttt_hip.h - B NH NC CS F, G = checkpoint_group_size, K = ceil(NC / G), H = 4 F - and resolved per call; dtype "act" is the
# dtype of XQ (bf16 or fp32), "f32" / "bf16" are fixed.
def _contract(fields, *groups):
    spec = {name: (tuple(d if d.isalpha() else int(d) for d in shape.split()), dtype)
            for shape, dtype, names in groups for name in names.split()}
    assert set(spec) == set(fields) and len(spec) == len(fields), set(spec) ^ set(fields)
    return spec


_MLP_FWD_SPEC = _contract(
    MLP_FWD_FIELDS,
    ("B NH NC CS F", "act", "XQ XK XV XQW"), ("B NH NC CS 1", "act", "last_eta"), ("1 NH 1 F", "f32", "ttt_norm_weight ttt_norm_bias"),
    ("B NH F H", "f32", "W1_init"), ("B NH 1 H", "f32", "b1_init"), ("B NH H F", "f32", "W2_init"), ("B NH 1 F", "f32", "b2_init"),
    ("B NH K F H", "f32", "W1_checkpoints"), ("B NH K 1 H", "f32", "b1_checkpoints"),
    ("B NH K H F", "f32", "W2_checkpoints"), ("B NH K 1 F", "f32", "b2_checkpoints"))
_MLP_BWD_SPEC = _contract(
    MLP_BWD_FIELDS,
    ("B NH NC CS F", "act", "XQ XK XV XQW grad_L_XQW grad_L_XQ grad_L_XK grad_L_XV"), ("B NH NC CS 1", "act", "last_eta grad_L_last_eta"),
    ("1 NH 1 F", "f32", "ttt_norm_weight ttt_norm_bias"), ("B NH 1 F", "f32", "grad_L_ttt_norm_weight grad_L_ttt_norm_bias"),
    ("B NH K F H", "f32", "W1_checkpoints"), ("B NH K 1 H", "f32", "b1_checkpoints"),
    ("B NH K H F", "f32", "W2_checkpoints"), ("B NH K 1 F", "f32", "b2_checkpoints"),
    ("B NH G F H", "f32", "W1_init_group"), ("B NH G 1 H", "f32", "b1_init_group"),
    ("B NH G H F", "f32", "W2_init_group"), ("B NH G 1 F", "f32", "b2_init_group"),
    ("B NH G CS F", "bf16", "x_hat_ln_group grad_l_wrt_Z2_group x_hat_fused_group grad_x_hat_fused_group grad_output_fused_group"),
    ("B NH G CS H", "bf16", "X2_group Z1_group Z1_bar_group X2_bar_group grad_l_wrt_Z1_group"),
    ("B NH G CS 1", "f32", "std_ln_group std_fused_group"),
    ("B NH F H", "f32", "grad_L_W1_last grad_L_W1_init"), ("B NH 1 H", "f32", "grad_L_b1_last grad_L_b1_init"),
    ("B NH H F", "f32", "grad_L_W2_last grad_L_W2_init"), ("B NH 1 F", "f32", "grad_L_b2_last grad_L_b2_init"))
# The sixteen re-materialisation buffers of the reference contract (mlp_tk.py:192-210) may be None HERE (the reference always passes
# them; this repo's fused autograd node does not allocate what no kernel touches): the MFMA backward works in its own workspace, the
# generic kernels need the four *_init_group buffers (the C ABI refuses NULL there).
_MLP_BWD_SCRATCH = frozenset(MLP_BWD_FIELDS[11:27])
_LIN_FWD_SPEC = _contract(
    LIN_FWD_FIELDS,
    ("B NH NC CS F", "act", "XQ XK XV XQW"), ("B NH NC CS 1", "act", "last_eta"), ("NH F", "f32", "ttt_norm_weight ttt_norm_bias"),
    ("B NH F F", "f32", "W1_init"), ("B NH 1 F", "f32", "b1_init"),
    ("B NH K F F", "f32", "W1_checkpoints"), ("B NH K 1 F", "f32", "b1_checkpoints"))
_LIN_BWD_SPEC = _contract(
    LIN_BWD_FIELDS,
    ("B NH NC CS F", "act", "XQ XK XV grad_L_XQW grad_L_XQ grad_L_XK grad_L_XV"), ("B NH NC CS 1", "act", "last_eta grad_L_last_eta"),
    ("NH F", "f32", "ttt_norm_weight ttt_norm_bias"), ("B NH K F F", "f32", "W1_checkpoints"), ("B NH K 1 F", "f32", "b1_checkpoints"),
    ("B NH F F", "f32", "grad_L_W1_last grad_L_W1_init"),
    ("B NH 1 F", "f32", "grad_L_b1_last grad_L_b1_init grad_L_ttt_norm_weight grad_L_ttt_norm_bias"),
    ("B NH G F F", "f32", "W1_init_group"), ("B NH G 1 F", "f32", "b1_init_group"))

# TTT_HIP_ABI_VERSION of include/ttt_hip.h this binding was written against (the version history is kept there)
ABI_VERSION = 5


def _sig(args="", restype=ctypes.c_int):
    """(restype, argtypes) from a parameter list such as "4i f 11p": [count]kind with i int / int32_t, u unsigned, l int64_t,
    z size_t, f float, s const char*, p any other pointer (tensor data, argument struct, stream)."""
    kinds = dict(i=ctypes.c_int, u=ctypes.c_uint, l=ctypes.c_int64, z=ctypes.c_size_t, f=ctypes.c_float, s=ctypes.c_char_p, p=ctypes.c_void_p)
    return restype, [kinds[a[-1]] for a in args.split() for _ in range(int(a[:-1] or 1))]


# Prototype of every extern "C" symbol declared in include/ttt_hip.h (tests/test_abi_cpu.py compares the two); load_library() applies
# them, so that ctypes converts - and refuses - arguments by the declared parameter types.
_SCAN = _sig("3p z p")                          # dims, args, workspace, workspace_bytes, stream
_PROTOTYPES = {
    **{f"ttt_hip_{op}_workspace": _sig("p", ctypes.c_size_t) for op in ("mlp_forward", "mlp_backward", "linear_forward", "linear_backward")},
    "ttt_hip_mlp_forward": _SCAN, "ttt_hip_mlp_backward": _SCAN, "ttt_hip_linear_forward": _SCAN, "ttt_hip_linear_backward": _SCAN,
    "ttt_hip_mlp_forward_chunk": _sig("2p 2i 5p z p"),
    "ttt_hip_resolve_impl": _sig("p 2i"), "ttt_hip_abi_version": _sig(), "ttt_hip_last_error": _sig("", ctypes.c_char_p),
    # debug knobs, sweep error word, CU-masked streams
    "ttt_hip_debug_timing": _sig("p", None), "ttt_hip_debug_dump": _sig("p", None),
    "ttt_hip_debug_groups_per_chunk": _sig("i", None), "ttt_hip_debug_option": _sig("s i"),
    "ttt_hip_debug_sweep_error": _sig("", ctypes.c_uint), "ttt_hip_sweep_error_clear": _sig("", None),
    "ttt_hip_debug_occupy_cus": _sig("3i p"), "ttt_hip_debug_placement_probe": _sig("p 3i p"),
    "ttt_hip_stream_create_masked": _sig("p i p"), "ttt_hip_stream_destroy": _sig("p"),
    # fused pre / post / gate of the TTT layer: B, L, NH, F (gate: B, L, D, n_text) first, the stream last
    "ttt_hip_pre_forward": _sig("4i 12p"), "ttt_hip_pre_forward_range": _sig("4i 11p 2i p"),
    "ttt_hip_pre_backward": _sig("4i 16p"), "ttt_hip_pre_backward_ld": _sig("4i 13p l 3p"), "ttt_hip_pre_backward_partials": _sig("i"),
    "ttt_hip_post_forward": _sig("4i f 6p"), "ttt_hip_post_forward_range": _sig("4i f 5p 2i p"),
    "ttt_hip_post_backward": _sig("4i f 8p"), "ttt_hip_post_partials": _sig("2i"),
    "ttt_hip_gate_forward": _sig("4i 6p"), "ttt_hip_gate_backward": _sig("4i 7p"), "ttt_hip_gate_backward_partials": _sig("i"),
    # segment attention (argument struct, stream) and its fused LayerNorm + RoPE: B, S, NH, n_text, eps first
    "ttt_hip_attn_forward": _sig("2p"), "ttt_hip_attn_backward": _sig("2p"),
    "ttt_hip_attn_pre_forward": _sig("4i f 11p"), "ttt_hip_attn_pre_partials": _sig("3i"),
    "ttt_hip_attn_pre_backward": _sig("4i f 12p"), "ttt_hip_attn_pre_backward_ld": _sig("4i f 10p l 2p"),
    # TransformerLayer glue: B, Lt, Lv, D first
    "ttt_hip_adaln_forward": _sig("4i f 8p"), "ttt_hip_adaln_backward": _sig("4i f 10p"), "ttt_hip_adaln_backward_partials": _sig(),
    "ttt_hip_resgate_forward": _sig("4i 7p"), "ttt_hip_resgate_backward": _sig("4i 7p"), "ttt_hip_resgate_backward_partials": _sig("i"),
}
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)
# ... and of every symbol declared in include/ttt_hip_parts.h, the second header: extensions beside the reference's operator boundary
# (tests/test_abi_parts_cpu.py compares the two).  EXPORTED_SYMBOLS stays the set of the main header.
_PROTOTYPES_PARTS = {
    "ttt_hip_linear_forward_chunk": _sig("2p 2i 3p z p"),
}
# ... and of every symbol declared in include/ttt_hip_bwd_parts.h, the third header: the TTT-Linear backward over ranges of checkpoint
# groups (tests/test_abi_bwd_parts_cpu.py compares the two)
_PROTOTYPES_BWD_PARTS = {
    "ttt_hip_linear_backward_parts_slots": _sig("p i", ctypes.c_size_t),
    "ttt_hip_linear_backward_parts_carry": _sig("p", ctypes.c_size_t),
    "ttt_hip_linear_recompute_groups": _sig("2p 2i p z p"),
    "ttt_hip_linear_sweep_groups": _sig("2p 2i p z p z p"),
}
# ... and of every symbol declared in include/ttt_hip_pair16.h, the fourth header: the TTT-MLP forward scan at mini-batches of 16 as a
# pair of workgroups per (b, h) (tests/test_abi_pair16_cpu.py compares the two)
_PROTOTYPES_PAIR16 = {
    "ttt_hip_mlp_forward_pair16_workspace": _sig("p", ctypes.c_size_t),
    "ttt_hip_mlp_forward_chunk_pair16": _sig("2p 2i 5p z p"),
}
# ... and of every symbol declared in include/ttt_hip_mlp_bwd_parts.h, the fifth header: the TTT-MLP backward at mini-batches of 16 over
# ranges of checkpoint groups (tests/test_abi_mlp_bwd_parts_cpu.py compares the two)
_PROTOTYPES_MLP_BWD_PARTS = {
    "ttt_hip_mlp_backward_parts_slots": _sig("p i", ctypes.c_size_t),
    "ttt_hip_mlp_backward_parts_carry": _sig("p", ctypes.c_size_t),
    "ttt_hip_mlp_recompute_groups": _sig("2p 2i p z p"),
    "ttt_hip_mlp_sweep_groups": _sig("2p 2i p z p z p"),
}
# ... and of every symbol declared in include/ttt_hip_lin_bwd_front.h, the sixth header: the carry-free half of the TTT-Linear reverse
# steps at mini-batches of 16 as a kernel of its own, and the walk that consumes its records (tests/test_abi_lin_bwd_front_cpu.py
# compares the two)
_PROTOTYPES_LIN_BWD_FRONT = {
    "ttt_hip_linear_backward_front_records": _sig("p i", ctypes.c_size_t),
    "ttt_hip_linear_front_groups": _sig("2p 2i p z p z p"),
    "ttt_hip_linear_chain_groups": _sig("2p 2i p z p z p z p"),
}
# ... and of every symbol declared in include/ttt_hip_lin_split16.h, the seventh header: the TTT-Linear forward scan at mini-batches of
# 16 with its output path on a second wave (tests/test_abi_lin_split16_cpu.py compares the two)
_PROTOTYPES_LIN_SPLIT16 = {
    "ttt_hip_linear_forward_chunk_split16": _sig("2p 2i 3p z p"),
}
# ... and of every symbol declared in include/ttt_hip_lin64_bwd_front.h, the eighth header: the front / chain stage of the TTT-Linear
# backward in parts at mini-batches of 64 (tests/test_abi_lin64_bwd_front_cpu.py compares the two)
_PROTOTYPES_LIN64_BWD_FRONT = {
    "ttt_hip_linear_backward_front64_records": _sig("p i", ctypes.c_size_t),
    "ttt_hip_linear_front64_groups": _sig("2p 2i p z p z p"),
    "ttt_hip_linear_chain64_groups": _sig("2p 2i p z p z p z p"),
}

_lib: Optional[ctypes.CDLL] = None


def library_path() -> str:
    return _LIB_PATH


def load_library() -> ctypes.CDLL:
    """dlopen libttt_hip.so (built by ``__graft_entry__.build()`` / ``csrc/build.sh``) and give every exported function its prototype.
    Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"test_time_training: HIP library not found at {_LIB_PATH}; build it with "
            f"`python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
    lib = ctypes.CDLL(_LIB_PATH)
    if lib.ttt_hip_abi_version() != ABI_VERSION:
        raise RuntimeError(f"test_time_training: libttt_hip.so ABI version {lib.ttt_hip_abi_version()}, this binding needs {ABI_VERSION}: rebuild (csrc/build.sh)")
    for name, (restype, argtypes) in {**_PROTOTYPES, **_PROTOTYPES_PARTS, **_PROTOTYPES_BWD_PARTS, **_PROTOTYPES_PAIR16,
                                      **_PROTOTYPES_MLP_BWD_PARTS, **_PROTOTYPES_LIN_BWD_FRONT, **_PROTOTYPES_LIN_SPLIT16,
                                      **_PROTOTYPES_LIN64_BWD_FRONT}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _p(t: Optional[torch.Tensor]):
    """device pointer of a tensor, or None (a null pointer) for None"""
    return t.data_ptr() if t is not None else None


def debug_timing(buf: Optional[torch.Tensor]) -> None:
    """DEBUG: per-phase cycle counters of workgroup 0 are accumulated into ``buf`` (16 x int64, zeroed, on device)."""
    load_library().ttt_hip_debug_timing(_p(buf))


def debug_option(name: str, value: int) -> None:
    """DEBUG / A-B knobs by name, described at ttt_hip_debug_option in include/ttt_hip.h: ``groups_per_chunk``, ``overlap_tail``,
    ``fast_records``, ``sweep_fast_count`` (a query: see ``sweep_fast_count()``), ``deriver_split``, ``attn_prio``, ``scan_pair``,
    ``lin_split16_chain_alone`` and the fault injections ``sweep_fault``, ``scan_fault``."""
    if load_library().ttt_hip_debug_option(name.encode(), int(value)) != 0:
        raise ValueError(f"unknown debug option {name!r}")


def debug_groups_per_chunk(groups: int) -> None:
    """DEBUG: force the MFMA backward's chunk size in checkpoint groups (0 = automatic)."""
    debug_option("groups_per_chunk", groups)


def sweep_error() -> int:
    """0, or 1 + (b,h) of a cluster-form backward workgroup whose hand-over partner never arrived (synchronises)."""
    return int(load_library().ttt_hip_debug_sweep_error())


def debug_occupy_cus(workgroups: int, lds_bytes: int, microseconds: int, stream=None) -> None:
    """DEBUG (stress tests): hold ``workgroups`` CUs' worth of LDS for ``microseconds`` on ``stream`` (default: the current one)."""
    st = (stream or torch.cuda.current_stream()).cuda_stream
    if load_library().ttt_hip_debug_occupy_cus(int(workgroups), int(lds_bytes), int(microseconds), st) != 0:
        raise RuntimeError("ttt_hip_debug_occupy_cus: bad arguments or launch failure")


def masked_stream(cu_mask_words) -> "torch.cuda.ExternalStream":
    """A stream whose kernels run only on the compute units of ``cu_mask_words`` (sequence of 32-bit words, bit i of word w = logical CU
    32 w + i; ``ttt_hip_stream_create_masked``), as a ``torch.cuda.ExternalStream`` of the current device.  The HIP stream lives as long as
    the process (a handful per process: the sweep / side streams of a backward, a communication stream)."""
    lib = load_library()
    words = [int(w) & 0xFFFFFFFF for w in cu_mask_words]
    arr = (ctypes.c_uint * len(words))(*words)
    out = ctypes.c_void_p()
    if lib.ttt_hip_stream_create_masked(arr, len(words), ctypes.byref(out)) != 0:
        raise RuntimeError(lib.ttt_hip_last_error().decode())
    return torch.cuda.ExternalStream(out.value)


def placement_probe(workgroups: int, stream=None, lds_bytes: int = 150 * 1024, microseconds: int = 200):
    """DEBUG: where ``workgroups`` one-wave workgroups of ``stream`` run - a list of (xcd, shader engine, shader array, cu) per workgroup
    (each holds ``lds_bytes`` of LDS for ``microseconds``, so that every CU takes one).  Synchronises."""
    lib = load_library()
    st = stream or torch.cuda.current_stream()
    out = torch.zeros(workgroups, dtype=torch.int32, device="cuda")
    with torch.cuda.stream(st):
        rc = lib.ttt_hip_debug_placement_probe(out.data_ptr(), int(workgroups), int(lds_bytes), int(microseconds), st.cuda_stream)
    if rc != 0:
        raise RuntimeError("ttt_hip_debug_placement_probe: bad arguments or launch failure")
    st.synchronize()
    w = out.cpu().tolist()
    return [((v >> 16) & 0xF, (v >> 13) & 0x7, (v >> 12) & 0x1, (v >> 8) & 0xF) for v in w]


def sweep_error_clear() -> None:
    """Acknowledge a hand-over time-out (synchronises): TTT-MLP calls are accepted again."""
    load_library().ttt_hip_sweep_error_clear()


def sweep_fast_count() -> int:
    """DEBUG statistic: cluster workgroup launches that proved same-XCD placement and published plain (L2-resident) records."""
    return -2 - int(load_library().ttt_hip_debug_option(b"sweep_fast_count", 0))


def debug_dump(buf: Optional[torch.Tensor]) -> None:
    """DEBUG: step-0 intermediates of workgroup 0 of the revision-2 forward go to ``buf`` (>= 120000 fp32 on device)."""
    load_library().ttt_hip_debug_dump(_p(buf))


def set_impl(name: str) -> None:
    """Select the kernel family: 'auto' (MFMA when the geometry allows), 'generic', 'mfma'."""
    _state["impl"] = _IMPL_NAMES[name]


def get_impl() -> str:
    return {v: k for k, v in _IMPL_NAMES.items()}[_state["impl"]]


def set_ln_eps(eps: float) -> None:
    _state["eps"] = float(eps)


def get_ln_eps() -> float:
    return _state["eps"]


# ------------------------------------------------------------------------------------------------
def _check(t: torch.Tensor, name: str, shape, dtype) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor must live on a HIP device (got {t.device}); there is no CPU path")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name}: tensor must be contiguous")


def _check5(XQ) -> None:
    if not isinstance(XQ, torch.Tensor) or XQ.ndim != 5:
        raise RuntimeError("XQ: expected a 5-D tensor [B, NH, NC, CS, F]")


def _impl_code(impl) -> int:
    """selector of one call: None = the global one (``set_impl``), or 'auto' / 'generic' / 'mfma'"""
    if impl is None:
        return _state["impl"]
    if impl not in _IMPL_NAMES:
        raise ValueError(f"impl: expected None, 'auto', 'generic' or 'mfma', got {impl!r}")
    return _IMPL_NAMES[impl]


def _dims(B, NH, NC, CS, F, G, act_dtype, impl=None) -> _Dims:
    if act_dtype == torch.bfloat16:
        code = 0
    elif act_dtype == torch.float32:
        code = 1
    else:
        raise RuntimeError(f"activations must be bfloat16 or float32, got {act_dtype}")
    if G < 1:
        raise RuntimeError("checkpoint_group_size must be >= 1")
    return _Dims(B, NH, NC, CS, F, G, code, _impl_code(impl), _state["eps"])


# Workspaces (the TTT-MLP backward's step records: 2.2 GB at 48 heads) are kept per (device, stream) and grown on demand instead of
# being drawn from torch's caching allocator at every call (84 times per training step at 9 s, in the phase where HBM is fullest:
# round-3 verdict, weak #8).  Calls on one stream are ordered, so they can share the buffer; calls on different streams (two
# autograd threads) get their own.  The key is the raw stream handle; a stream that was destroyed and whose handle the runtime
# hands out again would inherit a buffer that torch's allocator associates with the old stream - harmless for ordering (the
# buffer is only ever used on the stream of the key) but the entry of a dead stream would stay: at most `_WS_MAX` entries are kept,
# the least recently used one goes first.  ``release_workspaces()`` returns the memory (sampling does, see
# ttt_amd/models/cogvideo/sampling.py).
_ws_cache = {}
_WS_MAX = 4


def _workspace(device, stream: int, nbytes: int):
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), int(stream))
    buf = _ws_cache.pop(key, None)                  # (re-inserted below: dict order = recency)
    if buf is None or buf.numel() < nbytes:
        del buf                                     # let the old block go before the larger one is requested
        while len(_ws_cache) >= _WS_MAX:
            _ws_cache.pop(next(iter(_ws_cache)))
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    _ws_cache[key] = buf
    return buf


def release_workspaces() -> None:
    """Drop the cached kernel workspaces (they are re-created by the next call that needs one)."""
    _ws_cache.clear()


def _launch(fn_name: str, dims: _Dims, args, device, suffix: str = "", extra=()) -> None:
    """``fn_name + suffix``(dims, args, *extra, workspace, workspace_bytes, stream) with the workspace ``fn_name`` asks for"""
    lib = load_library()
    ws_bytes = getattr(lib, fn_name + "_workspace")(ctypes.byref(dims))
    stream = torch.cuda.current_stream(device).cuda_stream
    ws = _workspace(device, stream, ws_bytes) if ws_bytes else None
    with torch.cuda.device(device):
        rc = getattr(lib, fn_name + suffix)(ctypes.byref(dims), ctypes.byref(args), *extra, _p(ws), ws_bytes, stream)
    if rc != 0:
        raise RuntimeError(lib.ttt_hip_last_error().decode())


def resolved_impl(B, NH, NC, CS, F, G, act_dtype=torch.bfloat16, mlp=True, backward=False, *, impl=None) -> str:
    """Name of the kernel family a call with these dims would run ('generic' / 'mfma'; 'unsupported': the selector asks for a family
    that has no kernel for them).  ``impl``: the selector of this question instead of the global one - e.g. ``impl="mfma"`` asks
    whether an explicit request would be accepted (TTT-Linear at mini-batches of 64: 'mfma' on request, 'generic' under 'auto')."""
    lib = load_library()
    d = _dims(B, NH, NC, CS, F, G, act_dtype, impl)
    r = lib.ttt_hip_resolve_impl(ctypes.byref(d), int(mlp), int(backward))
    return {1: "generic", 2: "mfma"}.get(r, "unsupported")


# ------------------------------------------------------------------------------------------------
def _fill_args(struct, spec, tensors, sizes, act, optional=()):
    """Check ``tensors`` (in the order of the struct's fields) against their contract ``spec`` at the dimensions ``sizes`` (a dict
    B .. H) and activation dtype ``act``; return the filled argument struct.  A field named in ``optional`` may be None (a null pointer)."""
    dtypes = {"act": act, "f32": torch.float32, "bf16": torch.bfloat16}
    ptrs = []
    for (name, _), t in zip(struct._fields_, tensors):
        if t is not None or name not in optional:
            shape, dtype = spec[name]
            _check(t, name, [sizes.get(d, d) for d in shape], dtypes[dtype])
        ptrs.append(_p(t))
    return struct(*ptrs)


def _scan_args(struct, spec, tensors, checkpoint_group_size, optional=(), impl=None, xq_optional=False):
    """(dims, args, device) of one scan op for ``_launch``: the sizes are XQ's, the tensors are checked against ``spec``; ``impl``
    overrides the global selector for this call.  ``xq_optional``: the sizes are XK's where XQ is None (a recompute does not need XQ)"""
    XQ = tensors[1] if xq_optional and tensors[0] is None else tensors[0]
    _check5(XQ)
    B, NH, NC, CS, F = XQ.shape
    G = int(checkpoint_group_size)
    sizes = dict(B=B, NH=NH, NC=NC, CS=CS, F=F, G=G, K=-(-NC // G), H=4 * F)
    args = _fill_args(struct, spec, tensors, sizes, XQ.dtype, optional)
    return _dims(B, NH, NC, CS, F, G, XQ.dtype, impl), args, XQ.device


def ttt_forward(XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W2_init, b2_init,
                W1_checkpoints, b1_checkpoints, W2_checkpoints, b2_checkpoints, XQW_batch, checkpoint_group_size):
    """TTT-MLP forward scan; argument list of the reference call site mlp_tk.py:116-133."""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W2_init, b2_init,
               W1_checkpoints, b1_checkpoints, W2_checkpoints, b2_checkpoints, XQW_batch)
    _launch("ttt_hip_mlp_forward", *_scan_args(_MlpFwd, _MLP_FWD_SPEC, tensors, checkpoint_group_size))


def ttt_forward_chunk(XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_state, b1_state, W2_state, b2_state,
                      W1_checkpoints, b1_checkpoints, W2_checkpoints, b2_checkpoints, XQW_batch, checkpoint_group_size, step0, nsteps):
    """The TTT-MLP forward over steps [step0, step0 + nsteps) of the sequence the (whole-sequence) tensors describe - an extension
    beside ``ttt_forward``'s 15-tensor call (``ttt_hip_mlp_forward_chunk``): started from the fp32 state in ``*_state``
    ([B,NH,F,H], [B,NH,1,H], [B,NH,H,F], [B,NH,1,F]), which it REPLACES by the state after its last step, so that consecutive
    calls walk the sequence with the bits of the one-call forward.  MFMA scan only.  At mini-batches of 64 parts start and end at
    checkpoint-group boundaries (or at the end); at mini-batches of 16 a part is any [step0, step0 + nsteps) inside [0, NC)."""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_state, b1_state, W2_state, b2_state,
               W1_checkpoints, b1_checkpoints, W2_checkpoints, b2_checkpoints, XQW_batch)
    dims, args, device = _scan_args(_MlpFwd, _MLP_FWD_SPEC, tensors, checkpoint_group_size)
    # the workspace is ttt_forward's (the pair scan's ring of state records); the final state goes where the initial one came from
    _launch("ttt_hip_mlp_forward", dims, args, device, suffix="_chunk",
            extra=(int(step0), int(nsteps), args.W1_init, args.b1_init, args.W2_init, args.b2_init))


def _launch_pair16(dims, args, device, step0, nsteps, finals) -> bool:
    """``ttt_hip_mlp_forward_chunk_pair16`` (include/ttt_hip_pair16.h) with its workspace from the per-stream cache -> True when the
    scan was enqueued as pairs, False when the library enqueued the one-workgroup kernel (the pairs do not fit the device)"""
    lib = load_library()
    ws_bytes = lib.ttt_hip_mlp_forward_pair16_workspace(ctypes.byref(dims))
    stream = torch.cuda.current_stream(device).cuda_stream
    ws = _workspace(device, stream, ws_bytes) if ws_bytes else None
    with torch.cuda.device(device):
        rc = lib.ttt_hip_mlp_forward_chunk_pair16(ctypes.byref(dims), ctypes.byref(args), int(step0), int(nsteps), *finals,
                                                  _p(ws), ws_bytes, stream)
    if rc not in (0, 1):
        raise RuntimeError(lib.ttt_hip_last_error().decode())
    return rc == 0


def ttt_forward_pair16(XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W2_init, b2_init,
                       W1_checkpoints, b1_checkpoints, W2_checkpoints, b2_checkpoints, XQW_batch, checkpoint_group_size) -> bool:
    """``ttt_forward`` at mini-batches of 16 (bf16, head dim 64, MFMA scan) as a PAIR of workgroups per (b, h) - one carries the state,
    the other computes the outputs from the records the first publishes (csrc/ttt_mlp16_pair_body.h; opt-in) - with the bits of
    ``ttt_forward``.  Returns True when pairs ran, False when the one-workgroup kernel ran instead (see ``_launch_pair16``)."""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W2_init, b2_init,
               W1_checkpoints, b1_checkpoints, W2_checkpoints, b2_checkpoints, XQW_batch)
    dims, args, device = _scan_args(_MlpFwd, _MLP_FWD_SPEC, tensors, checkpoint_group_size)
    return _launch_pair16(dims, args, device, 0, dims.NC, (None, None, None, None))


def ttt_forward_chunk_pair16(XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_state, b1_state, W2_state, b2_state,
                             W1_checkpoints, b1_checkpoints, W2_checkpoints, b2_checkpoints, XQW_batch, checkpoint_group_size, step0,
                             nsteps) -> bool:
    """``ttt_forward_chunk`` at mini-batches of 16 in pair form (``ttt_forward_pair16``): steps [step0, step0 + nsteps), the fp32 state
    in ``*_state`` REPLACED by the state after the last step.  Returns True when pairs ran."""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_state, b1_state, W2_state, b2_state,
               W1_checkpoints, b1_checkpoints, W2_checkpoints, b2_checkpoints, XQW_batch)
    dims, args, device = _scan_args(_MlpFwd, _MLP_FWD_SPEC, tensors, checkpoint_group_size)
    return _launch_pair16(dims, args, device, step0, nsteps, (args.W1_init, args.b1_init, args.W2_init, args.b2_init))


def ttt_backward(XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_checkpoints, b1_checkpoints, W2_checkpoints,
                 b2_checkpoints, XQW_batch, W1_init_group, b1_init_group, W2_init_group, b2_init_group, x_hat_ln_group,
                 std_ln_group, X2_group, Z1_group, Z1_bar_group, X2_bar_group, grad_l_wrt_Z2_group, grad_l_wrt_Z1_group,
                 x_hat_fused_group, grad_x_hat_fused_group, grad_output_fused_group, std_fused_group, grad_L_W1_last,
                 grad_L_b1_last, grad_L_W2_last, grad_L_b2_last, grad_L_XQW_batch, grad_L_ttt_norm_weight,
                 grad_L_ttt_norm_bias, grad_L_W1_init, grad_L_b1_init, grad_L_W2_init, grad_L_b2_init, grad_L_last_eta,
                 grad_L_XQ, grad_L_XK, grad_L_XV, checkpoint_group_size):
    """TTT-MLP backward; the 42 tensors + 1 int of the reference call site mlp_tk.py:227-275."""
    ttt_backward_impl(None, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_checkpoints, b1_checkpoints, W2_checkpoints,
                      b2_checkpoints, XQW_batch, W1_init_group, b1_init_group, W2_init_group, b2_init_group, x_hat_ln_group,
                      std_ln_group, X2_group, Z1_group, Z1_bar_group, X2_bar_group, grad_l_wrt_Z2_group, grad_l_wrt_Z1_group,
                      x_hat_fused_group, grad_x_hat_fused_group, grad_output_fused_group, std_fused_group, grad_L_W1_last,
                      grad_L_b1_last, grad_L_W2_last, grad_L_b2_last, grad_L_XQW_batch, grad_L_ttt_norm_weight,
                      grad_L_ttt_norm_bias, grad_L_W1_init, grad_L_b1_init, grad_L_W2_init, grad_L_b2_init, grad_L_last_eta,
                      grad_L_XQ, grad_L_XK, grad_L_XV, checkpoint_group_size)


def ttt_backward_impl(impl, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_checkpoints, b1_checkpoints, W2_checkpoints,
                      b2_checkpoints, XQW_batch, W1_init_group, b1_init_group, W2_init_group, b2_init_group, x_hat_ln_group,
                      std_ln_group, X2_group, Z1_group, Z1_bar_group, X2_bar_group, grad_l_wrt_Z2_group, grad_l_wrt_Z1_group,
                      x_hat_fused_group, grad_x_hat_fused_group, grad_output_fused_group, std_fused_group, grad_L_W1_last,
                      grad_L_b1_last, grad_L_W2_last, grad_L_b2_last, grad_L_XQW_batch, grad_L_ttt_norm_weight,
                      grad_L_ttt_norm_bias, grad_L_W1_init, grad_L_b1_init, grad_L_W2_init, grad_L_b2_init, grad_L_last_eta,
                      grad_L_XQ, grad_L_XK, grad_L_XV, checkpoint_group_size):
    """``ttt_backward`` with the selector of THIS call: ``impl`` None (the global selector) or 'auto' / 'generic' / 'mfma' - 'mfma' at
    mini-batches of 16 runs the opt-in MFMA backward of csrc/ttt_mlp16_bwd_body.h, which keeps its per-step state in the four
    ``*_init_group`` buffers (required there, as for the generic kernels).  (A function of its own, as ``ttt_linear_backward_impl``.)"""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_checkpoints, b1_checkpoints, W2_checkpoints,
               b2_checkpoints, XQW_batch, W1_init_group, b1_init_group, W2_init_group, b2_init_group, x_hat_ln_group,
               std_ln_group, X2_group, Z1_group, Z1_bar_group, X2_bar_group, grad_l_wrt_Z2_group, grad_l_wrt_Z1_group,
               x_hat_fused_group, grad_x_hat_fused_group, grad_output_fused_group, std_fused_group, grad_L_W1_last,
               grad_L_b1_last, grad_L_W2_last, grad_L_b2_last, grad_L_XQW_batch, grad_L_ttt_norm_weight,
               grad_L_ttt_norm_bias, grad_L_W1_init, grad_L_b1_init, grad_L_W2_init, grad_L_b2_init, grad_L_last_eta,
               grad_L_XQ, grad_L_XK, grad_L_XV)
    _launch("ttt_hip_mlp_backward", *_scan_args(_MlpBwd, _MLP_BWD_SPEC, tensors, checkpoint_group_size, optional=_MLP_BWD_SCRATCH, impl=impl))


def ttt_linear_forward(XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W1_checkpoints,
                       b1_checkpoints, XQW_batch, checkpoint_group_size):
    """TTT-Linear forward scan (replaces ttt_linear_scan_forward, linear_triton.py:98-129)."""
    ttt_linear_forward_impl(None, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W1_checkpoints,
                            b1_checkpoints, XQW_batch, checkpoint_group_size)


def ttt_linear_forward_impl(impl, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W1_checkpoints,
                            b1_checkpoints, XQW_batch, checkpoint_group_size):
    """``ttt_linear_forward`` with the selector of THIS call: ``impl`` None (the global selector) or 'auto' / 'generic' / 'mfma' -
    'mfma' at mini-batches of 64 runs the opt-in MFMA scan of csrc/ttt_lin64_body.h.  (A function of its own, not a keyword of
    ``ttt_linear_forward``: that one keeps the parameter list of the reference's launch site, which tests/test_reference_tkmlp_cpu.py
    counts.)"""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W1_checkpoints, b1_checkpoints, XQW_batch)
    _launch("ttt_hip_linear_forward", *_scan_args(_LinFwd, _LIN_FWD_SPEC, tensors, checkpoint_group_size, impl=impl))


def ttt_linear_forward_chunk(impl, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_state, b1_state, W1_checkpoints,
                             b1_checkpoints, XQW_batch, checkpoint_group_size, step0, nsteps):
    """The TTT-Linear forward over steps [step0, step0 + nsteps) of the sequence the (whole-sequence) tensors describe
    (``ttt_hip_linear_forward_chunk``, include/ttt_hip_parts.h): started from the fp32 state in ``W1_state`` [B,NH,F,F] / ``b1_state``
    [B,NH,1,F], which it REPLACES by the state after its last step, so that consecutive calls walk the sequence with the bits of the
    one-call forward.  MFMA scan only - mini-batches of 16, or of 64 with ``impl='mfma'`` (``impl`` as in ``ttt_linear_forward_impl``) -;
    a part is any [step0, step0 + nsteps) inside [0, NC) at either mini-batch size."""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_state, b1_state, W1_checkpoints, b1_checkpoints, XQW_batch)
    dims, args, device = _scan_args(_LinFwd, _LIN_FWD_SPEC, tensors, checkpoint_group_size, impl=impl)
    # the final state goes where the initial one came from
    _launch("ttt_hip_linear_forward", dims, args, device, suffix="_chunk", extra=(int(step0), int(nsteps), args.W1_init, args.b1_init))


linear_split16_calls = {"whole": 0, "chunk": 0}      # launches of this process (tests, tools)


def _launch_split16(dims, args, device, step0, nsteps, finals, counter) -> None:
    """``ttt_hip_linear_forward_chunk_split16`` (include/ttt_hip_lin_split16.h) on the current stream; it has no workspace"""
    lib = load_library()
    with torch.cuda.device(device):
        rc = lib.ttt_hip_linear_forward_chunk_split16(ctypes.byref(dims), ctypes.byref(args), int(step0), int(nsteps), *finals, None, 0,
                                                      torch.cuda.current_stream(device).cuda_stream)
    if rc != 0:
        raise RuntimeError(lib.ttt_hip_last_error().decode())
    linear_split16_calls[counter] += 1


def ttt_linear_forward_split16(impl, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W1_checkpoints,
                               b1_checkpoints, XQW_batch, checkpoint_group_size):
    """``ttt_linear_forward_impl`` at mini-batches of 16 (bf16, head dim 64, MFMA scan) with the output path on a second wave: one
    workgroup of two waves per (b, h) - the first carries the state, the second computes the outputs from the packed state the first
    hands over through LDS (csrc/ttt_lin16_split_body.h; opt-in) - with the bits of ``ttt_linear_forward_impl``.  ``impl``: None,
    'auto' or 'mfma'; every other geometry, dtype or selector is refused."""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_init, b1_init, W1_checkpoints, b1_checkpoints, XQW_batch)
    dims, args, device = _scan_args(_LinFwd, _LIN_FWD_SPEC, tensors, checkpoint_group_size, impl=impl)
    _launch_split16(dims, args, device, 0, dims.NC, (None, None), "whole")


def ttt_linear_forward_chunk_split16(impl, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_state, b1_state, W1_checkpoints,
                                     b1_checkpoints, XQW_batch, checkpoint_group_size, step0, nsteps):
    """``ttt_linear_forward_chunk`` at mini-batches of 16 in the two-wave form (``ttt_linear_forward_split16``): steps
    [step0, step0 + nsteps), the fp32 state in ``W1_state`` / ``b1_state`` REPLACED by the state after the last step."""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_state, b1_state, W1_checkpoints, b1_checkpoints, XQW_batch)
    dims, args, device = _scan_args(_LinFwd, _LIN_FWD_SPEC, tensors, checkpoint_group_size, impl=impl)
    _launch_split16(dims, args, device, step0, nsteps, (args.W1_init, args.b1_init), "chunk")


def ttt_linear_backward(XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_checkpoints, b1_checkpoints,
                        grad_L_W1_last, grad_L_b1_last, grad_L_XQW_batch, W1_init_group, b1_init_group,
                        grad_L_ttt_norm_weight, grad_L_ttt_norm_bias, grad_L_W1_init, grad_L_b1_init, grad_L_last_eta,
                        grad_L_XQ, grad_L_XK, grad_L_XV, checkpoint_group_size):
    """TTT-Linear backward (replaces ttt_linear_scan_backward, linear_triton.py:203-246)."""
    ttt_linear_backward_impl(None, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_checkpoints, b1_checkpoints, grad_L_W1_last,
                             grad_L_b1_last, grad_L_XQW_batch, W1_init_group, b1_init_group, grad_L_ttt_norm_weight, grad_L_ttt_norm_bias,
                             grad_L_W1_init, grad_L_b1_init, grad_L_last_eta, grad_L_XQ, grad_L_XK, grad_L_XV, checkpoint_group_size)


def ttt_linear_backward_impl(impl, XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_checkpoints, b1_checkpoints,
                             grad_L_W1_last, grad_L_b1_last, grad_L_XQW_batch, W1_init_group, b1_init_group,
                             grad_L_ttt_norm_weight, grad_L_ttt_norm_bias, grad_L_W1_init, grad_L_b1_init, grad_L_last_eta,
                             grad_L_XQ, grad_L_XK, grad_L_XV, checkpoint_group_size):
    """``ttt_linear_backward`` with the selector of this call (see ``ttt_linear_forward_impl``)."""
    tensors = (XQ, XK, XV, last_eta, ttt_norm_weight, ttt_norm_bias, W1_checkpoints, b1_checkpoints, grad_L_W1_last, grad_L_b1_last,
               grad_L_XQW_batch, W1_init_group, b1_init_group, grad_L_ttt_norm_weight, grad_L_ttt_norm_bias, grad_L_W1_init,
               grad_L_b1_init, grad_L_last_eta, grad_L_XQ, grad_L_XK, grad_L_XV)
    _launch("ttt_hip_linear_backward", *_scan_args(_LinBwd, _LIN_BWD_SPEC, tensors, checkpoint_group_size, impl=impl))


# The backward scans over ranges of checkpoint groups: six entries with one launch path.  A call is the tensor list of the one-call
# backward (``ttt_linear_backward_impl`` / ``ttt_backward``), then checkpoint_group_size, k0, nk and the raw workspaces of the entry.
# What an entry does not touch may be None; what is given is checked against the contract of the one-call backward, field by field.
def _groups_call(symbol, struct, spec, optional, impl, call, workspaces, counter):
    """``symbol``(dims, args, k0, nk, (pointer, bytes) of each of ``workspaces``, stream) on the current stream; ``counter``: the
    (dict, key) of this entry's launch count"""
    n = len(struct._fields_)
    if len(call) != n + 3 + len(workspaces):
        raise TypeError(f"{symbol}: expected {n} tensors (or None), checkpoint_group_size, k0, nk, {', '.join(workspaces)}: "
                        f"{n + 3 + len(workspaces)} arguments, got {len(call)}")
    (G, k0, nk), raw = call[n:n + 3], call[n + 3:]
    dims, args, device = _scan_args(struct, spec, call[:n], G, optional, impl, xq_optional=True)
    lib = load_library()
    sized = []
    for name, t in zip(workspaces, raw):          # raw workspaces: any dtype; the library checks the size against the range of the call
        if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
            raise RuntimeError(f"{name}: expected a contiguous tensor on a HIP device")
        if name == "ln_carry" and t.dtype != torch.float32:
            raise RuntimeError(f"ln_carry: expected dtype torch.float32, got {t.dtype}")
        sized += [_p(t), t.numel() * t.element_size()]
    with torch.cuda.device(device):
        rc = getattr(lib, symbol)(ctypes.byref(dims), ctypes.byref(args), int(k0), int(nk), *sized, torch.cuda.current_stream(device).cuda_stream)
    if rc != 0:
        raise RuntimeError(lib.ttt_hip_last_error().decode())
    counter[0][counter[1]] += 1


def _parts_bytes(symbol, B, NH, NC, CS, F, G, act_dtype, impl, *nk):
    d = _dims(B, NH, NC, CS, F, G, act_dtype, impl)
    return int(getattr(load_library(), symbol)(ctypes.byref(d), *(int(v) for v in nk)))


# TTT-Linear (include/ttt_hip_bwd_parts.h).  The recompute reads XK, XV, last_eta, the LayerNorm parameters and the checkpoints; the
# sweep reads and writes everything else of ``ttt_linear_backward``'s list.
_LIN_RECOMPUTE_FIELDS = frozenset(("XK", "XV", "last_eta", "ttt_norm_weight", "ttt_norm_bias", "W1_checkpoints", "b1_checkpoints"))
_LIN_SWEEP_UNUSED = frozenset(("W1_checkpoints", "b1_checkpoints", "W1_init_group", "b1_init_group"))
linear_bwd_parts_calls = {"recompute": 0, "sweep": 0}      # launches of this process (tests, tools)


def linear_backward_parts_slots(B, NH, NC, CS, F, G, nk, act_dtype=torch.bfloat16, *, impl=None) -> int:
    """bytes of the slot workspace of ``ttt_linear_recompute_groups`` / ``ttt_linear_sweep_groups`` for ``nk`` checkpoint groups:
    B * NH * nk * (G + 1) slots of 16384 + 256 bytes"""
    return _parts_bytes("ttt_hip_linear_backward_parts_slots", B, NH, NC, CS, F, G, act_dtype, impl, nk)


def linear_backward_parts_carry(B, NH, NC, CS, F, G, act_dtype=torch.bfloat16, *, impl=None) -> int:
    """bytes of ``ln_carry``: B * NH * 8 * lanes * 4, lanes = 64 at mini-batches of 16, 256 at mini-batches of 64"""
    return _parts_bytes("ttt_hip_linear_backward_parts_carry", B, NH, NC, CS, F, G, act_dtype, impl)


def ttt_linear_recompute_groups(impl, *call):
    """Re-run the checkpoint groups [k0, k0 + nk) of the sequence the (whole-sequence) tensors describe from their checkpoints and
    leave the state entering every step, and the state ending each group, in ``slots`` (``linear_backward_parts_slots`` bytes for
    nk groups) - ``ttt_hip_linear_recompute_groups``, include/ttt_hip_bwd_parts.h.  ``call``: the 21 tensors of
    ``ttt_linear_backward_impl``, checkpoint_group_size, k0, nk, slots; only XK, XV, last_eta, the LayerNorm parameters and the
    checkpoints are needed, the rest may be None.  MFMA sweep only."""
    _groups_call("ttt_hip_linear_recompute_groups", _LinBwd, _LIN_BWD_SPEC, frozenset(LIN_BWD_FIELDS) - _LIN_RECOMPUTE_FIELDS, impl, call,
                 ("slots",), (linear_bwd_parts_calls, "recompute"))


def ttt_linear_sweep_groups(impl, *call):
    """The reverse walk over the checkpoint groups k0 + nk - 1 .. k0 from the ``slots`` ``ttt_linear_recompute_groups`` left for the
    same range (``ttt_hip_linear_sweep_groups``).  ``call``: the 21 tensors of ``ttt_linear_backward_impl``, checkpoint_group_size, k0,
    nk, slots, ln_carry.  Carries dW1 / db1 from ``grad_L_W1_last`` / ``grad_L_b1_last`` to ``grad_L_W1_init`` / ``grad_L_b1_init`` (which
    may be the same tensors) and the LayerNorm gradients' partial sums in ``ln_carry`` (``linear_backward_parts_carry`` bytes, fp32);
    the range with k0 == 0 also writes ``grad_L_ttt_norm_weight`` / ``_bias``.  Walked from the last range to the first, the results
    are the bits of ``ttt_linear_backward_impl``.  The checkpoints and ``*_init_group`` may be None.  The caller orders a recompute
    before the sweep of its slots (same stream, or events)."""
    _groups_call("ttt_hip_linear_sweep_groups", _LinBwd, _LIN_BWD_SPEC, _LIN_SWEEP_UNUSED, impl, call,
                 ("slots", "ln_carry"), (linear_bwd_parts_calls, "sweep"))


# The third stage of the TTT-Linear backward over ranges of checkpoint groups, mini-batches of 16 (include/ttt_hip_lin_bwd_front.h).
# The front reads the four activation tiles and the LayerNorm parameters and writes grad_L_XQ; the chain is the sweep without XV,
# grad_L_XQW and grad_L_XQ.
_LIN_FRONT_FIELDS = frozenset(("XQ", "XK", "XV", "ttt_norm_weight", "ttt_norm_bias", "grad_L_XQW", "grad_L_XQ"))
_LIN_CHAIN_UNUSED = _LIN_SWEEP_UNUSED | frozenset(("XV", "grad_L_XQW", "grad_L_XQ"))
linear_bwd_front_calls = {"front": 0, "chain": 0}      # launches of this process (tests, tools)


def linear_backward_front_records(B, NH, NC, CS, F, G, nk, act_dtype=torch.bfloat16, *, impl=None) -> int:
    """bytes of the record workspace of ``ttt_linear_front_groups`` / ``ttt_linear_chain_groups`` for ``nk`` checkpoint groups:
    B * NH * nk * G records of 19456 bytes ; 0 where CS != 16"""
    return _parts_bytes("ttt_hip_linear_backward_front_records", B, NH, NC, CS, F, G, act_dtype, impl, nk)


def ttt_linear_front_groups(impl, *call):
    """The half of every reverse step of the checkpoint groups [k0, k0 + nk) that does not depend on the carried gradients, all steps
    at once, from the ``slots`` ``ttt_linear_recompute_groups`` left for the same range (``ttt_hip_linear_front_groups``,
    include/ttt_hip_lin_bwd_front.h): writes ``grad_L_XQ`` of those steps and one record per step into ``records``
    (``linear_backward_front_records`` bytes for nk groups).  ``call``: the 21 tensors of ``ttt_linear_backward_impl``,
    checkpoint_group_size, k0, nk, slots, records; only XQ, XK, XV, grad_L_XQW, the LayerNorm parameters and grad_L_XQ are needed, the
    rest may be None.  MFMA sweep at mini-batches of 16 only."""
    _groups_call("ttt_hip_linear_front_groups", _LinBwd, _LIN_BWD_SPEC, frozenset(LIN_BWD_FIELDS) - _LIN_FRONT_FIELDS, impl, call,
                 ("slots", "records"), (linear_bwd_front_calls, "front"))


def ttt_linear_chain_groups(impl, *call):
    """The reverse walk over the checkpoint groups k0 + nk - 1 .. k0 from the ``slots`` and the ``records`` of the same range
    (``ttt_hip_linear_chain_groups``): ``ttt_linear_sweep_groups`` without the work ``ttt_linear_front_groups`` has done - same carries
    (dW1 / db1 in place, ``ln_carry``), same bits.  ``call``: the 21 tensors of ``ttt_linear_backward_impl``, checkpoint_group_size, k0,
    nk, slots, records, ln_carry; XV, grad_L_XQW, grad_L_XQ, the checkpoints and ``*_init_group`` may be None.  The caller orders
    recompute -> front -> chain of a range (same stream, or events)."""
    _groups_call("ttt_hip_linear_chain_groups", _LinBwd, _LIN_BWD_SPEC, _LIN_CHAIN_UNUSED, impl, call,
                 ("slots", "records", "ln_carry"), (linear_bwd_front_calls, "chain"))


# The same stage at mini-batches of 64 (include/ttt_hip_lin64_bwd_front.h): the same tensor lists, a record of 4 x 19456 bytes per step.
def linear_backward_front64_records(B, NH, NC, CS, F, G, nk, act_dtype=torch.bfloat16, *, impl=None) -> int:
    """bytes of the record workspace of ``ttt_linear_front64_groups`` / ``ttt_linear_chain64_groups`` for ``nk`` checkpoint groups:
    B * NH * nk * G records of 77824 bytes ; 0 for anything but bf16, F = 64, CS = 64 with ``impl="mfma"``"""
    return _parts_bytes("ttt_hip_linear_backward_front64_records", B, NH, NC, CS, F, G, act_dtype, impl, nk)


def ttt_linear_front64_groups(impl, *call):
    """``ttt_linear_front_groups`` at mini-batches of 64 (``ttt_hip_linear_front64_groups``): one wave per 16-row token block of every
    step of the checkpoint groups [k0, k0 + nk), from the ``slots`` ``ttt_linear_recompute_groups`` left for the same range; writes
    ``grad_L_XQ`` of those steps and one record per step into ``records`` (``linear_backward_front64_records`` bytes).  Same ``call``
    list; ``impl="mfma"`` only."""
    _groups_call("ttt_hip_linear_front64_groups", _LinBwd, _LIN_BWD_SPEC, frozenset(LIN_BWD_FIELDS) - _LIN_FRONT_FIELDS, impl, call,
                 ("slots", "records"), (linear_bwd_front_calls, "front"))


def ttt_linear_chain64_groups(impl, *call):
    """``ttt_linear_chain_groups`` at mini-batches of 64 (``ttt_hip_linear_chain64_groups``): the reverse walk over the checkpoint
    groups k0 + nk - 1 .. k0 from the ``slots`` and the ``records`` of the same range - the carries and the bits of
    ``ttt_linear_sweep_groups`` at mini-batches of 64.  Same ``call`` list; ``impl="mfma"`` only."""
    _groups_call("ttt_hip_linear_chain64_groups", _LinBwd, _LIN_BWD_SPEC, _LIN_CHAIN_UNUSED, impl, call,
                 ("slots", "records", "ln_carry"), (linear_bwd_front_calls, "chain"))


# TTT-MLP at mini-batches of 16 (include/ttt_hip_mlp_bwd_parts.h).  The recompute reads XK, XV, last_eta, the LayerNorm parameters and
# the four checkpoint tensors; the sweep reads and writes everything else of ``ttt_backward``'s list except the sixteen
# re-materialisation buffers.
_MLP_RECOMPUTE_FIELDS = frozenset(("XK", "XV", "last_eta", "ttt_norm_weight", "ttt_norm_bias", "W1_checkpoints", "b1_checkpoints",
                                   "W2_checkpoints", "b2_checkpoints"))
_MLP_SWEEP_UNUSED = frozenset(("W1_checkpoints", "b1_checkpoints", "W2_checkpoints", "b2_checkpoints", "XQW")) | _MLP_BWD_SCRATCH
mlp_bwd_parts_calls = {"recompute": 0, "sweep": 0}      # launches of this process (tests, tools)


def mlp_backward_parts_slots(B, NH, NC, CS, F, G, nk, act_dtype=torch.bfloat16, *, impl=None) -> int:
    """bytes of the slot workspace of ``ttt_recompute_groups`` / ``ttt_sweep_groups`` for ``nk`` checkpoint groups: B * NH * nk * G
    slots of 132352 bytes (the fp32 W1, b1, W2, b2 entering a step)"""
    return _parts_bytes("ttt_hip_mlp_backward_parts_slots", B, NH, NC, CS, F, G, act_dtype, impl, nk)


def mlp_backward_parts_carry(B, NH, NC, CS, F, G, act_dtype=torch.bfloat16, *, impl=None) -> int:
    """bytes of ``ln_carry``: B * NH * 2 * 16 * 64 * 4"""
    return _parts_bytes("ttt_hip_mlp_backward_parts_carry", B, NH, NC, CS, F, G, act_dtype, impl)


def ttt_recompute_groups(*call, impl=None):
    """Re-run the state updates of the checkpoint groups [k0, k0 + nk) of the sequence the (whole-sequence) tensors describe from their
    checkpoints and leave the fp32 state entering every step in ``slots`` (``mlp_backward_parts_slots`` bytes for nk groups) -
    ``ttt_hip_mlp_recompute_groups``, include/ttt_hip_mlp_bwd_parts.h.  ``call``: the 42 tensors of ``ttt_backward``,
    checkpoint_group_size, k0, nk, slots; only XK, XV, last_eta, the LayerNorm parameters and the four checkpoint tensors are needed,
    the rest may be None.  bf16, head dim 64, mini-batches of 16; ``impl`` None (the global selector), 'auto' or 'mfma' - the parts
    exist on the MFMA body alone, 'generic' is refused."""
    _groups_call("ttt_hip_mlp_recompute_groups", _MlpBwd, _MLP_BWD_SPEC, frozenset(MLP_BWD_FIELDS) - _MLP_RECOMPUTE_FIELDS, impl, call,
                 ("slots",), (mlp_bwd_parts_calls, "recompute"))


def ttt_sweep_groups(*call, impl=None):
    """The reverse walk over the checkpoint groups k0 + nk - 1 .. k0 from the ``slots`` ``ttt_recompute_groups`` left for the same range
    (``ttt_hip_mlp_sweep_groups``).  ``call``: the 42 tensors of ``ttt_backward``, checkpoint_group_size, k0, nk, slots, ln_carry.
    Carries dW1 / db1 / dW2 / db2 from ``grad_L_*_last`` to ``grad_L_*_init`` (which may be the same tensors) and the LayerNorm
    gradients' un-reduced shares in ``ln_carry`` (``mlp_backward_parts_carry`` bytes, fp32); the range with k0 == 0 also writes
    ``grad_L_ttt_norm_weight`` / ``_bias``.  Walked from the last range to the first, the results are the bits of
    ``ttt_backward_impl('mfma', ...)``.  The checkpoints, XQW_batch and the sixteen ``*_group`` buffers may be None.  The caller orders a
    recompute before the sweep of its slots (same stream, or events)."""
    _groups_call("ttt_hip_mlp_sweep_groups", _MlpBwd, _MLP_BWD_SPEC, _MLP_SWEEP_UNUSED, impl, call,
                 ("slots", "ln_carry"), (mlp_bwd_parts_calls, "sweep"))


# ------------------------------------------------------------------------------------------------
# Fused pre- / post-processing kernels (include/ttt_hip.h, "Fused pre- / post-processing").  Thin wrappers: the
# caller (ttt_amd/models/ssm/fused.py) allocates every tensor; bf16 activations, fp32 parameters / tables.
def _req(dtype, **tensors):
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError(f"{name}: expected a contiguous {dtype} tensor on a HIP device")


def _req_rows(ld, shape, **tensors):
    """bf16 [B, L, D] tensors on a HIP device: contiguous (``ld`` None), or with token rows ``ld`` elements apart (column blocks of a
    wider buffer)"""
    if ld is None:
        return _req(torch.bfloat16, **tensors)
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.bfloat16 or tuple(t.shape) != tuple(shape) \
                or t.stride(2) != 1 or t.stride(1) != ld or (shape[0] > 1 and t.stride(0) != shape[1] * ld) or t.data_ptr() % 16:
            raise RuntimeError(f"{name}: expected a bf16 {tuple(shape)} tensor on a HIP device with token rows {ld} elements apart")


def _call(fn, *args, device):
    """``fn``(*args, stream) on the current stream of ``device``"""
    lib = load_library()
    with torch.cuda.device(device):
        rc = getattr(lib, fn)(*args, torch.cuda.current_stream(device).cuda_stream)
    if rc != 0:
        raise RuntimeError(lib.ttt_hip_last_error().decode())


def _req_maps(rope, src, pos, L, F, n_pos):
    """Token maps / RoPE table of the fused pre kernels: the kernel indexes ``rope[pos[t]]`` and ``x[src[t]]`` unchecked, so
    the table must cover every position (the reference's apply_rotary_emb raises a shape error for a video longer than
    config.compressed_num_frames, ssm/utils.py:82-108) and the maps must be int32 of length L.  ``n_pos`` = 1 + the largest
    position the maps address, as a host integer (the module caches it with the maps; no device synchronisation here).
    With ``pos`` given and ``n_pos`` unknown (a direct user of the binding, or maps that lost the module's cache through
    ``.to()`` / ``clone()``) the bound is taken from the map itself, once per map tensor (one synchronising ``max()``, cached on
    the tensor); with no ``pos`` the kernels rotate nothing (every token is text: position -1) and there is nothing to check."""
    for t, n in ((src, "src"), (pos, "pos")):
        if t is None:
            continue
        _req(torch.int32, **{n: t})
        if t.numel() != L:
            raise RuntimeError(f"{n}: expected {L} entries, got {t.numel()}")
    if rope is None:
        return
    _req(torch.float32, rope=rope)
    if rope.numel() % F != 0:
        raise RuntimeError(f"rope: expected [n_pos, {F // 2}, 2] (cos, sin) pairs, got {tuple(rope.shape)}")
    n_rows = rope.numel() // F
    if pos is None:
        return
    if n_pos is None:
        n_pos = getattr(pos, "_ttt_max_pos", None)
        if n_pos is None:
            n_pos = int(pos.max()) + 1
            try:
                pos._ttt_max_pos = n_pos
            except Exception:
                pass
    if n_pos > n_rows:
        raise RuntimeError(f"rope table has {n_rows} positions but the sequence addresses {n_pos} (video longer than "
                           f"config.compressed_num_frames?)")


def pre_forward(XQ_raw, XK_raw, XV_raw, rope, src, pos, ln_w, ln_b, XQ, XK, XV, NH, n_pos=None, t0=0, tn=None):
    """``t0``, ``tn``: the scan positions [t0, t0 + tn) only (a part of the sequence; default: all of it)"""
    B, L, D = XQ_raw.shape
    _req_maps(rope, src, pos, L, D // NH, n_pos)
    _req(torch.bfloat16, XQ_raw=XQ_raw, XK_raw=XK_raw, XV_raw=XV_raw, XQ=XQ, XK=XK, XV=XV)
    _req(torch.float32, ln_w=ln_w, ln_b=ln_b)
    _call("ttt_hip_pre_forward_range", B, L, NH, D // NH, _p(XQ_raw), _p(XK_raw), _p(XV_raw), _p(rope), _p(src), _p(pos), _p(ln_w), _p(ln_b),
          _p(XQ), _p(XK), _p(XV), int(t0), int(L - t0 if tn is None else tn), device=XQ_raw.device)


def pre_backward_partials(NH):
    return load_library().ttt_hip_pre_backward_partials(int(NH))


def pre_backward(XQ_raw, XK_raw, XV_raw, rope, src, pos, ln_w, dXQ, dXK, dXV, dXQ_raw, dXK_raw, dXV_raw, dlnw_part, dlnb_part, NH, ld_out=None):
    """``ld_out``: row stride (elements) of the three raw-gradient outputs - None: contiguous [B, L, D] tensors; 3 * D: the column
    blocks of one [B, L, 3 D] buffer (the q / k / v projections' weight gradients are then one GEMM, ttt_amd/infra/fused_linear.py)."""
    B, L, D = XQ_raw.shape
    ld = None if ld_out is None else int(ld_out)
    _req(torch.bfloat16, XQ_raw=XQ_raw, XK_raw=XK_raw, XV_raw=XV_raw, dXQ=dXQ, dXK=dXK, dXV=dXV)
    _req_rows(ld, (B, L, D), dXQ_raw=dXQ_raw, dXK_raw=dXK_raw, dXV_raw=dXV_raw)
    _req(torch.float32, ln_w=ln_w, dlnw_part=dlnw_part, dlnb_part=dlnb_part)
    _call("ttt_hip_pre_backward_ld", B, L, NH, D // NH, _p(XQ_raw), _p(XK_raw), _p(XV_raw), _p(rope), _p(src), _p(pos), _p(ln_w),
          _p(dXQ), _p(dXK), _p(dXV), _p(dXQ_raw), _p(dXK_raw), _p(dXV_raw), D if ld is None else ld, _p(dlnw_part), _p(dlnb_part),
          device=XQ_raw.device)


def post_partials(B, L):
    return load_library().ttt_hip_post_partials(int(B), int(L))


def post_forward(Y, src, w, b, out, eps, t0=0, tn=None):
    """``t0``, ``tn``: the scan positions [t0, t0 + tn) only (default: all)"""
    B, NH, L, F = Y.shape
    _req(torch.bfloat16, Y=Y, out=out)
    _req(torch.float32, w=w, b=b)
    _call("ttt_hip_post_forward_range", B, L, NH, F, eps, _p(Y), _p(src), _p(w), _p(b), _p(out),
          int(t0), int(L - t0 if tn is None else tn), device=Y.device)


def post_backward(Y, dOut, src, w, dY, dw_part, db_part, eps):
    B, NH, L, F = Y.shape
    _req(torch.bfloat16, Y=Y, dOut=dOut, dY=dY)
    _req(torch.float32, w=w, dw_part=dw_part, db_part=db_part)
    _call("ttt_hip_post_backward", B, L, NH, F, eps, _p(Y), _p(dOut), _p(src), _p(w), _p(dY), _p(dw_part), _p(db_part), device=Y.device)


def gate_forward(res, y, tanh_text, tanh_video, out, n_text):
    B, L, D = res.shape
    _req(torch.bfloat16, res=res, y=y, out=out)
    _req(torch.float32, tanh_text=tanh_text, tanh_video=tanh_video)
    _call("ttt_hip_gate_forward", B, L, D, int(n_text), _p(res), _p(y), _p(tanh_text), _p(tanh_video), _p(out), device=res.device)


def gate_backward_partials(D):
    return load_library().ttt_hip_gate_backward_partials(int(D))


def gate_backward(g, y, tanh_text, tanh_video, dy, dtanh_part, n_text):
    B, L, D = g.shape
    _req(torch.bfloat16, g=g, y=y, dy=dy)
    _req(torch.float32, tanh_text=tanh_text, tanh_video=tanh_video, dtanh_part=dtanh_part)
    _call("ttt_hip_gate_backward", B, L, D, int(n_text), _p(g), _p(y), _p(tanh_text), _p(tanh_video), _p(dy), _p(dtanh_part), device=g.device)


# ------------------------------------------------------------------------------------------------
# Segment self-attention (include/ttt_hip.h, "Segment self-attention"): strided [B, NH, S, 64] bf16 views, no copies.
class _AttnTensor(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("stride_b", ctypes.c_int64), ("stride_h", ctypes.c_int64), ("stride_s", ctypes.c_int64)]


class _AttnFwd(ctypes.Structure):
    _fields_ = [("Q", _AttnTensor), ("K", _AttnTensor), ("V", _AttnTensor), ("O", _AttnTensor), ("LSE", ctypes.c_void_p),
                ("B", ctypes.c_int32), ("NH", ctypes.c_int32), ("S", ctypes.c_int32), ("D", ctypes.c_int32), ("scale", ctypes.c_float)]


class _AttnBwd(ctypes.Structure):
    _fields_ = [(n, _AttnTensor) for n in ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV")] + [
        ("LSE", ctypes.c_void_p), ("Delta", ctypes.c_void_p),
        ("B", ctypes.c_int32), ("NH", ctypes.c_int32), ("S", ctypes.c_int32), ("D", ctypes.c_int32), ("scale", ctypes.c_float)]


def _attn_tensor(t, name, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.bfloat16:
        raise RuntimeError(f"{name}: expected a bfloat16 tensor on a HIP device (there is no CPU path)")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.stride(3) != 1:
        raise RuntimeError(f"{name}: the head dimension must be contiguous")
    return _AttnTensor(t.data_ptr(), t.stride(0), t.stride(1), t.stride(2))


def attn_forward(q, k, v, out, lse, scale):
    """O = softmax(q k^T * scale) v for [B, NH, S, 64] bf16 views (any batch/head/token strides); lse [B,NH,S] fp32 or None."""
    B, NH, S, D = q.shape
    sh = (B, NH, S, D)
    a = _AttnFwd(_attn_tensor(q, "q", sh), _attn_tensor(k, "k", sh), _attn_tensor(v, "v", sh), _attn_tensor(out, "out", sh),
                 _p(lse), B, NH, S, D, float(scale))
    if lse is not None:
        _req(torch.float32, lse=lse)
    _call("ttt_hip_attn_forward", ctypes.byref(a), device=q.device)


def attn_backward(q, k, v, out, dout, lse, delta, dq, dk, dv, scale):
    B, NH, S, D = q.shape
    sh = (B, NH, S, D)
    _req(torch.float32, lse=lse, delta=delta)
    a = _AttnBwd(_attn_tensor(q, "q", sh), _attn_tensor(k, "k", sh), _attn_tensor(v, "v", sh), _attn_tensor(out, "out", sh),
                 _attn_tensor(dout, "dout", sh), _attn_tensor(dq, "dq", sh), _attn_tensor(dk, "dk", sh), _attn_tensor(dv, "dv", sh),
                 lse.data_ptr(), delta.data_ptr(), B, NH, S, D, float(scale))
    _call("ttt_hip_attn_backward", ctypes.byref(a), device=q.device)


def attn_pre_forward(q_raw, k_raw, wq, bq, wk, bk, cos, sin, q, k, NH, n_text, eps):
    """Fused per-head LayerNorm(64) + RoPE of the attention's q and k; [B, S, NH*64] bf16 in and out."""
    B, S, D = q_raw.shape
    _req(torch.bfloat16, q_raw=q_raw, k_raw=k_raw, q=q, k=k)
    _req(torch.float32, wq=wq, bq=bq, wk=wk, bk=bk, cos=cos, sin=sin)
    if D != NH * 64 or cos.shape[-1] != 64 or cos.shape[0] < S - n_text:
        raise RuntimeError("attn_pre_forward: head_dim must be 64 and the rope tables must cover the video tokens")
    _call("ttt_hip_attn_pre_forward", B, S, NH, int(n_text), eps, _p(q_raw), _p(k_raw), _p(wq), _p(bq), _p(wk), _p(bk),
          _p(cos), _p(sin), _p(q), _p(k), device=q_raw.device)


def attn_pre_partials(B, S, NH):
    return load_library().ttt_hip_attn_pre_partials(int(B), int(S), int(NH))


def attn_pre_backward(q_raw, k_raw, dq, dk, wq, wk, cos, sin, dq_raw, dk_raw, part, NH, n_text, eps, ld_out=None):
    """``ld_out``: as in ``pre_backward`` (dq_raw / dk_raw as column blocks of one [B, S, 3 D] buffer whose third block is dV)."""
    B, S, D = q_raw.shape
    ld = None if ld_out is None else int(ld_out)
    _req(torch.bfloat16, q_raw=q_raw, k_raw=k_raw)
    _req_rows(ld, (B, S, D), dq_raw=dq_raw, dk_raw=dk_raw)
    _req(torch.float32, wq=wq, wk=wk, cos=cos, sin=sin, part=part)
    tq, tk = _attn_tensor(dq, "dq", (B, NH, S, 64)), _attn_tensor(dk, "dk", (B, NH, S, 64))
    _call("ttt_hip_attn_pre_backward_ld", B, S, NH, int(n_text), eps, _p(q_raw), _p(k_raw), ctypes.byref(tq), ctypes.byref(tk),
          _p(wq), _p(wk), _p(cos), _p(sin), _p(dq_raw), _p(dk_raw), D if ld is None else ld, _p(part), device=q_raw.device)


# ------------------------------------------------------------------------------------------------
# TransformerLayer glue (include/ttt_hip.h, "TransformerLayer glue"): bf16 activations, fp32 parameter vectors.
def adaln_forward(vid, text, w, b, shift, scale1p, out, eps):
    B, Lv, D = vid.shape
    Lt = text.shape[1]
    _req(torch.bfloat16, vid=vid, text=text, out=out)
    _req(torch.float32, w=w, b=b, shift=shift, scale1p=scale1p)
    if tuple(out.shape) != (B, Lt + Lv, D) or tuple(shift.shape) != (B, 2, D) or tuple(scale1p.shape) != (B, 2, D):
        raise RuntimeError("adaln_forward: out must be [B, Lt+Lv, D], shift / scale1p [B, 2, D]")
    _call("ttt_hip_adaln_forward", B, Lt, Lv, D, eps, _p(vid), _p(text), _p(w), _p(b), _p(shift), _p(scale1p), _p(out), device=vid.device)


def adaln_backward_partials():
    return load_library().ttt_hip_adaln_backward_partials()


def adaln_backward(vid, text, dout, w, b, scale1p, dvid, dtext, part, eps):
    B, Lv, D = vid.shape
    Lt = text.shape[1]
    _req(torch.bfloat16, vid=vid, text=text, dout=dout, dvid=dvid, dtext=dtext)
    _req(torch.float32, w=w, b=b, scale1p=scale1p, part=part)
    _call("ttt_hip_adaln_backward", B, Lt, Lv, D, eps, _p(vid), _p(text), _p(dout), _p(w), _p(b), _p(scale1p),
          _p(dvid), _p(dtext), _p(part), device=vid.device)


def resgate_forward(vid, text, y, gate, ovid, otext):
    B, Lv, D = vid.shape
    Lt = text.shape[1]
    _req(torch.bfloat16, vid=vid, text=text, y=y, ovid=ovid, otext=otext)
    _req(torch.float32, gate=gate)
    if tuple(y.shape) != (B, Lt + Lv, D) or tuple(gate.shape) != (B, 2, D):
        raise RuntimeError("resgate_forward: y must be [B, Lt+Lv, D], gate [B, 2, D]")
    _call("ttt_hip_resgate_forward", B, Lt, Lv, D, _p(vid), _p(text), _p(y), _p(gate), _p(ovid), _p(otext), device=vid.device)


def resgate_backward_partials(D):
    return load_library().ttt_hip_resgate_backward_partials(int(D))


def resgate_backward(dvid, dtext, y, gate, dy, dgate_part):
    B, Lv, D = dvid.shape
    Lt = dtext.shape[1]
    _req(torch.bfloat16, dvid=dvid, dtext=dtext, y=y, dy=dy)
    _req(torch.float32, gate=gate, dgate_part=dgate_part)
    _call("ttt_hip_resgate_backward", B, Lt, Lv, D, _p(dvid), _p(dtext), _p(y), _p(gate), _p(dy), _p(dgate_part), device=dvid.device)
