"""The TTT-MLP forward scan at mini-batches of 16 over PARTS of the sequence (sampling: the layer forward as a pipeline at CS = 16):
the chunked workgroup body of csrc/ttt_mlp16_body.h on the multi-wave emulator of tests/emul, the argument checks of
``ttt_hip_mlp_forward_chunk`` that are reached before a launch, and the layer's plan (``TTTBase._pipeline_plan``) at CS = 16."""
import ctypes
import os
import subprocess

import pytest
import torch

from helpers import rel_l2, tile_states
from oracle import ttt_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/amdclang++"


class MlpParams(ctypes.Structure):            # wv::Mlp16Params (csrc/ttt_wave_types.h)
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("XQ", "XK", "XV", "eta", "ln_w", "ln_b", "W1", "b1", "W2", "b2", "W1c", "b1c", "W2c", "b2c", "out")] + \
               [(n, ctypes.c_int) for n in ("NH", "NC", "G", "K")] + [("eps", ctypes.c_float)]


class ChunkParams(ctypes.Structure):          # wv::Mlp16ChunkParams
    _fields_ = [("p", MlpParams), ("step0", ctypes.c_int), ("NCs", ctypes.c_int)] + \
               [(n, ctypes.c_void_p) for n in ("W1f", "b1f", "W2f", "b2f")]


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(CLANG):
        pytest.skip("host clang of the ROCm toolchain not available")
    build = os.path.join(HERE, "emul", "_build")
    os.makedirs(build, exist_ok=True)
    so = os.path.join(build, "libmlp16_chunk_emul.so")
    srcs = [os.path.join(HERE, "emul", f) for f in ("mlp16_chunk_emul.cpp", "wave_emul.h")] + \
           [os.path.join(ROOT, "ttt-video-dit_amd", "csrc", f) for f in ("ttt_lin16_body.h", "ttt_mlp16_body.h", "ttt_wave_types.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call([CLANG, "-std=c++20", "-O1", "-pthread", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-psabi",
                               "-I", os.path.join(ROOT, "ttt-video-dit_amd", "csrc"), "-I", os.path.join(HERE, "emul"),
                               srcs[0], "-o", so])
    lib = ctypes.CDLL(so)
    assert lib.emul_mlp16_chunk_params_size() == ctypes.sizeof(ChunkParams)
    return lib


def _case(B, NH, NC, seed):
    d = O.make_inputs("mlp", B, NH, NC, 16, 64, seed=seed)
    for k in ("XQ", "XK", "XV", "eta", "dOut"):
        d[k] = d[k].to(torch.bfloat16).to(torch.float32)
    bf = lambda t: t.to(torch.bfloat16).contiguous()
    t = dict(XQ=bf(d["XQ"]), XK=bf(d["XK"]), XV=bf(d["XV"]), eta=bf(d["eta"][:, :, :, -1, :, None]),
             ln_w=d["ln_w"].float().contiguous(), ln_b=d["ln_b"].float().contiguous())
    t.update({k: v.float().contiguous() for k, v in tile_states(d, B).items()})
    return d, t


def _run(lib, t, B, NH, NC, G, cuts):
    """the scan as consecutive parts of the given lengths, the state carried IN PLACE (final state aliases the initial state, as
    pipeline.prepass carries it) -> out, checkpoints, final state, races"""
    K = -(-NC // G)
    nan = lambda *s: torch.full(s, float("nan"))
    cks = (nan(B, NH, K, 64, 256), nan(B, NH, K, 1, 256), nan(B, NH, K, 256, 64), nan(B, NH, K, 1, 64))
    out = torch.full((B, NH, NC, 16, 64), float("nan"), dtype=torch.bfloat16)
    state = [t[k].clone() for k in ("W1", "b1", "W2", "b2")]
    msg = ctypes.create_string_buffer(256)
    races, s0 = 0, 0
    for ns in cuts:
        c = ChunkParams()
        for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=state[0], b1=state[1],
                         W2=state[2], b2=state[3], W1c=cks[0], b1c=cks[1], W2c=cks[2], b2c=cks[3], out=out).items():
            setattr(c.p, n, v.data_ptr())
        c.p.NH, c.p.NC, c.p.G, c.p.K, c.p.eps = NH, ns, G, K, 1e-8
        c.step0, c.NCs = s0, NC
        c.W1f, c.b1f, c.W2f, c.b2f = (s.data_ptr() for s in state)
        races += lib.emul_mlp16_forward_part(ctypes.byref(c), B * NH, msg, 256)
        assert races == 0, f"LDS race between waves in the part [{s0}, {s0 + ns}): {msg.value.decode()}"
        s0 += ns
    assert s0 == NC
    return out, cks, state


@pytest.mark.parametrize("G", [7, 2, 3])
def test_emulated_mlp_scan16_in_parts_is_the_uncut_scan(emul, G):
    """A scan of 7 steps cut as (7), (3, 4), (1, 1, 5), (6, 1) - cuts on and off the checkpoint-group boundaries, parts of one
    step, a part behind the last checkpoint: outputs, checkpoints and the final state of every cutting are the BITS of the uncut
    run (the hand-over is the kernel's own fp32 state, and everything a step takes from its predecessor is rebuilt from it), no
    LDS race in any part, and the uncut run holds the 1e-2 of the one-call emulator test against the fp64 oracle."""
    B, NH, NC = 1, 2, 7
    d, t = _case(B, NH, NC, seed=73)
    out0, cks0, st0 = _run(emul, t, B, NH, NC, G, (7,))
    assert not any(torch.isnan(c).any() for c in cks0) and not torch.isnan(out0.float()).any()
    for cuts in ((3, 4), (1, 1, 5), (6, 1)):
        out, cks, st = _run(emul, t, B, NH, NC, G, cuts)
        assert torch.equal(out, out0), cuts
        for name, c, c0 in zip(("W1c", "b1c", "W2c", "b2c"), cks, cks0):
            assert torch.equal(c, c0), (cuts, name)
        for name, s, s0 in zip(("W1", "b1", "W2", "b2"), st, st0):
            assert torch.equal(s, s0), (cuts, name)
    d64 = {k: v.double() for k, v in d.items()}
    s64 = tile_states(d64, B)
    ro, rc, rf = O.mlp_forward(d64["XQ"], d64["XK"], d64["XV"], d64["eta"][:, :, :, -1, :, None], d64["ln_w"], d64["ln_b"],
                               s64["W1"], s64["b1"], s64["W2"], s64["b2"], G)
    assert rel_l2(out0, ro) < 1e-2
    for c, r in zip(cks0, rc):
        assert rel_l2(c, r) < 1e-2


def test_whole_sequence_entry_is_the_part_from_step_zero(emul):
    """``mlp16::forward`` (the entry the one-call emulator test and the one-call kernel use) is the part [0, NC) of the same body."""
    B, NH, NC, G = 1, 1, 3, 2
    _, t = _case(B, NH, NC, seed=5)
    out0, cks0, _ = _run(emul, t, B, NH, NC, G, (3,))
    K = -(-NC // G)
    nan = lambda *s: torch.full(s, float("nan"))
    cks = (nan(B, NH, K, 64, 256), nan(B, NH, K, 1, 256), nan(B, NH, K, 256, 64), nan(B, NH, K, 1, 64))
    out = torch.full((B, NH, NC, 16, 64), float("nan"), dtype=torch.bfloat16)
    p = MlpParams()
    for n, v in dict(XQ=t["XQ"], XK=t["XK"], XV=t["XV"], eta=t["eta"], ln_w=t["ln_w"], ln_b=t["ln_b"], W1=t["W1"], b1=t["b1"], W2=t["W2"],
                     b2=t["b2"], W1c=cks[0], b1c=cks[1], W2c=cks[2], b2c=cks[3], out=out).items():
        setattr(p, n, v.data_ptr())
    p.NH, p.NC, p.G, p.K, p.eps = NH, NC, G, K, 1e-8
    assert emul.emul_mlp16_forward_whole(ctypes.byref(p), B * NH, None, 0) == 0
    assert torch.equal(out, out0) and all(torch.equal(a, b) for a, b in zip(cks, cks0))


# ------------------------------------------------------------------------------------------------ C ABI: checks before a launch
def _chunk_call(lib, ext, dims, step0, nsteps, finals):
    fake = 0x1000                                  # never dereferenced: every case below is refused before the launch
    args = ext._MlpFwd(*[fake] * len(ext.MLP_FWD_FIELDS))
    vp = lambda ok: ctypes.c_void_p(fake if ok else None)
    lib.ttt_hip_mlp_forward_chunk.restype = ctypes.c_int
    rc = lib.ttt_hip_mlp_forward_chunk(ctypes.byref(dims), ctypes.byref(args), ctypes.c_int(step0), ctypes.c_int(nsteps),
                                       *[vp(f) for f in finals], ctypes.c_void_p(None), ctypes.c_size_t(0), ctypes.c_void_p(None))
    return rc, lib.ttt_hip_last_error()


def test_forward_chunk_argument_checks_at_cs16_without_gpu():
    """``ttt_hip_mlp_forward_chunk`` at mini-batches of 16: a part is any [step0, step0 + nsteps) inside [0, NC) - no
    checkpoint-group rule -, the final state comes as all four buffers or none; at mini-batches of 64 the group rule stays."""
    import test_time_training as ext
    lib = ext.load_library()
    all4 = (True, True, True, True)
    d16 = ext._Dims(1, 2, 12, 16, 64, 4, 0, 2, 1e-8)                   # bf16, impl = MFMA, G = 4
    assert lib.ttt_hip_resolve_impl(ctypes.byref(d16), 1, 0) == 2
    for step0, nsteps in ((-1, 2), (0, 0), (3, -1), (5, 8), (12, 1), (0, 13), (2 ** 31 - 1, 2)):
        rc, err = _chunk_call(lib, ext, d16, step0, nsteps, all4)
        assert rc == -1 and b"inside [0, NC)" in err, (step0, nsteps, err)
    # parts off the group boundaries pass the range checks: the next check ("all four or none") is what refuses these calls
    for step0, nsteps in ((1, 2), (0, 3), (5, 7), (11, 1)):
        rc, err = _chunk_call(lib, ext, d16, step0, nsteps, (True, True, False, True))
        assert rc == -1 and b"all four final-state buffers or none" in err, (step0, nsteps, err)
    d64 = ext._Dims(1, 2, 12, 64, 64, 4, 0, 2, 1e-8)
    rc, err = _chunk_call(lib, ext, d64, 1, 4, all4)
    assert rc == -1 and b"checkpoint-group" in err
    d32 = ext._Dims(1, 2, 12, 16, 64, 4, 0, 1, 1e-8)                   # the generic kernels do not continue from a state
    rc, err = _chunk_call(lib, ext, d32, 0, 4, all4)
    assert rc == -1 and b"only the MFMA scan" in err
    assert lib.ttt_hip_mlp_forward_workspace(ctypes.byref(d16)) == 0   # the state travels through the four fp32 arrays only


# ------------------------------------------------------------------------------------------------ the layer's plan at CS = 16
def _layer_and_meta(L_steps, scenes=1):
    from ttt_amd.models.cogvideo.utils import SequenceMetadata
    from ttt_amd.models.configs import ModelConfig
    from ttt_amd.models.ssm.ttt_layer import TTTMLP
    cfg = ModelConfig(model_dim=128, num_heads=2, num_layers=1, mini_batch_size=16, latent_height=4, latent_width=4,
                      compressed_num_frames=4, ssm_layer="ttt_mlp", scan_checkpoint_group_size=10 ** 6)
    layer = TTTMLP(cfg)
    L = 16 * L_steps
    tl = 16
    frames = (L - scenes * tl) // 16
    meta = SequenceMetadata(text_length=tl, seq_text_length=tl * scenes, num_frames=frames, num_chunks=scenes, tokens_per_frame=16,
                            latent_height=4, latent_width=4, t_emb=None)
    if scenes > 1:
        meta.init_multiscene_offsets()
    x = torch.zeros(1, 1, 128).expand(1, L, 128)          # (the plan looks at x's shape, dtype and device only)
    return layer, meta, x, L


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("steps,scenes", [(21948, 1), (2048, 1), (2500, 3), (2305, 1)])
def test_pipeline_plan_at_cs16(monkeypatch, steps, scenes, reverse):
    """Under ``no_grad`` a long TTT-MLP scan at mini-batches of 16 on the MFMA scan gets a plan whose parts cover [0, NC) exactly,
    in order, each a whole multiple of the step quantum but for the ragged tail, every token in exactly one run of one part; with
    grad enabled, for a short scan, for a head shard and with ``pipeline_parts = 0`` the layer stays one piece."""
    import test_time_training as ext
    from ttt_amd.models.ssm import pipeline
    monkeypatch.setattr(ext, "resolved_impl", lambda *a, **k: "mfma")
    monkeypatch.delenv("TTT_PIPELINE_WEIGHTS", raising=False)
    if scenes == 3:
        steps = (3 * 16 + 16 * 3 * ((steps * 16 - 48) // 48)) // 16         # frames divisible by the scenes
    layer, meta, x, L = _layer_and_meta(steps, scenes)
    NC, q = L // 16, pipeline.CS16_QUANTUM
    assert layer.pipeline_parts >= 2, "the library default must be the pipelined forward"
    with torch.enable_grad():
        assert layer._pipeline_plan(x, meta, L, reverse, False) is None
    with torch.no_grad():
        assert layer._pipeline_plan(x, meta, L, reverse, True) is None          # heads_only (tensor-parallel sampling)
        parts = layer._pipeline_plan(x, meta, L, reverse, False)
    assert parts is not None and 2 <= len(parts) <= pipeline.CS16_PARTS
    at, seen = 0, torch.zeros(L, dtype=torch.int32)
    for c, (s0, ns, runs) in enumerate(parts):
        assert s0 == at and ns >= 1 and s0 % q == 0
        assert ns % q == 0 or c == len(parts) - 1
        assert sum(r1 - r0 for r0, r1 in runs) == ns * 16
        for r0, r1 in runs:
            seen[r0:r1] += 1
        at += ns
    assert at == NC and bool((seen == 1).all())
    layer.pipeline_parts = 0
    with torch.no_grad():
        assert layer._pipeline_plan(x, meta, L, reverse, False) is None


def test_pipeline_plan_at_cs16_short_scans_stay_one_piece(monkeypatch):
    """scans below pipeline.CS16_MIN_STEPS (the small CS = 16 geometries of the suite, the 3 s video: 1 158 steps) run as one piece"""
    import test_time_training as ext
    from ttt_amd.models.ssm import pipeline
    monkeypatch.setattr(ext, "resolved_impl", lambda *a, **k: "mfma")
    assert pipeline.CS16_MIN_STEPS >= 2 * pipeline.CS16_QUANTUM
    for steps in (6, 9, 1158, pipeline.CS16_MIN_STEPS - 1):
        layer, meta, x, L = _layer_and_meta(steps)
        with torch.no_grad():
            assert layer._pipeline_plan(x, meta, L, False, False) is None, steps
    # ... and what the MFMA scan does not run (fp32 activations, the generic kernels) is never cut
    monkeypatch.setattr(ext, "resolved_impl", lambda *a, **k: "generic")
    layer, meta, x, L = _layer_and_meta(4096)
    with torch.no_grad():
        assert layer._pipeline_plan(x, meta, L, False, False) is None
