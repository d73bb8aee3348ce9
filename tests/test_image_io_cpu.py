"""CPU: the request-path entry points (tt_clip_image, tt_layernorm_block, tt_frames_out) -- symbols, every refusal (each returns before
the first HIP call, so nothing is launched: one valid argument set with fake aligned pointers, ONE fault per case, as in
tests/test_encoder_attention_refusals_cpu.py), the ops front ends on CPU tensors, and a pipeline with ``native_image_io=False`` that must
never reach the three new ops."""
import ctypes as C
import os
import re

import numpy as np
import PIL.Image
import pytest
import torch

from this_and_that_vdm_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT_BF16, TT_F16, TT_F32 = 0, 1, 2
TT_EINVAL, TT_EUNSUPPORTED = -1, -2
P = 0x10000
NEW = ("tt_clip_image_ws_bytes", "tt_clip_image", "tt_layernorm_block", "tt_frames_out")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_new_symbols_in_header_binding_and_library(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ttvdm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(tt_[a-z0-9_]+)\s*\(", text))
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.tt_abi_version() == 11                                     # additive
    assert lib.tt_clip_image_ws_bytes(2, 64, 40) == 2 * 2 * 3 * 64 * 40 * 4
    assert lib.tt_clip_image_ws_bytes(0, 64, 40) == 0


# ---- tt_clip_image: 64 x 40 -> 8 x 8 (15 / 9 taps)
CLIP = dict(src=P, src_kind=0, nimg=1, h=64, w=40, out_h=8, out_w=8, mean0=0.48, mean1=0.46, mean2=0.41, std0=0.27, std1=0.26, std2=0.28,
            dst=2 * P, dtype=TT_F32, ws=4 * P, ws_bytes=1 << 20)
CLIP_ORDER = list(CLIP)
CLIP_CASES = [
    ("null src", dict(src=None), TT_EINVAL, "null operand"),
    ("null dst", dict(dst=None), TT_EINVAL, "null operand"),
    ("null ws", dict(ws=None), TT_EINVAL, "null operand"),
    ("src_kind 2", dict(src_kind=2), TT_EINVAL, "src_kind 2"),
    ("bad dtype", dict(dtype=7), TT_EINVAL, "bad dtype"),
    ("no images", dict(nimg=0), TT_EINVAL, "empty image"),
    ("no rows", dict(h=0), TT_EINVAL, "empty image"),
    ("out_h 1", dict(out_h=1), TT_EINVAL, "at least 2"),
    ("out_w 1", dict(out_w=1), TT_EINVAL, "at least 2"),
    ("out_w 0", dict(out_w=0), TT_EINVAL, "at least 2"),
    ("std 0", dict(std1=0.0), TT_EINVAL, "std must be positive"),
    ("std nan", dict(std2=float("nan")), TT_EINVAL, "std must be positive"),
    ("65 taps", dict(h=8000, out_h=236, ws_bytes=1 << 40), TT_EUNSUPPORTED, "needs 65 x 9 taps"),        # f = 33.9: int(4 * 16.45) = 65
    ("69 taps across", dict(w=8000, out_w=224, ws_bytes=1 << 40), TT_EUNSUPPORTED, "15 x 69 taps"),
    ("reflect pad reaches a 1-row image", dict(h=1, out_h=2), TT_EINVAL, "reflect pad 1 x 4 reaches the image size 1 x 40"),
    ("reflect pad reaches a 1-column image", dict(w=1, out_w=8), TT_EINVAL, "reflect pad"),
    ("workspace too small", dict(ws_bytes=2 * 3 * 64 * 40 * 4 - 1), TT_EINVAL, "workspace too small"),
    ("workspace off a chunk", dict(ws=4 * P + 4), TT_EINVAL, "16-byte boundary"),
    ("fp32 source off an element", dict(src_kind=1, src=P + 2), TT_EINVAL, "element size"),
]


@pytest.mark.parametrize("what,fault,code,text", CLIP_CASES, ids=[c[0] for c in CLIP_CASES])
def test_clip_image_refusal(lib, what, fault, code, text):
    assert fault
    a = dict(CLIP, **fault)
    assert lib.tt_clip_image(*[a[k] for k in CLIP_ORDER], None) == code
    msg = lib.tt_last_error().decode()
    assert msg.startswith("tt_clip_image:") and text in msg, msg


def test_clip_image_tap_cap_through_the_library(lib):
    """where the 63-tap cap sits, asked of the library itself: 7400 -> 224 (in / out = 33.04: 65 taps) is refused for its taps; 7390 -> 224
    (63 taps) and 3500 -> 224 (29 taps, the header's example) get past the tap check -- shown by the NEXT refusal, the workspace size, so
    that nothing is launched."""
    def call(**kw):
        a = dict(CLIP, **kw)
        code = lib.tt_clip_image(*[a[k] for k in CLIP_ORDER], None)
        return code, lib.tt_last_error().decode()
    code, msg = call(h=7400, out_h=224, ws_bytes=1 << 40)
    assert code == TT_EUNSUPPORTED and "needs 65 x 9 taps, built for at most 63" in msg, msg
    for h in (7390, 3500):
        code, msg = call(h=h, out_h=224, ws_bytes=16)
        assert code == TT_EINVAL and "workspace too small" in msg, msg
    code, msg = call(w=7400, out_w=224, ws_bytes=1 << 40)
    assert code == TT_EUNSUPPORTED and "15 x 65 taps" in msg, msg


# ---- tt_layernorm_block: the workload, 3 x (78 x 1024)
LNB = dict(x=P, ldx=1024, nb=3, rows=78, c=1024, eps=1e-5, y=2 * P, dtype=TT_BF16)
LNB_ORDER = list(LNB)
LNB_CASES = [
    ("null x", dict(x=None), TT_EINVAL, "null operand"),
    ("null y", dict(y=None), TT_EINVAL, "null operand"),
    ("no batch", dict(nb=0), TT_EINVAL, "empty problem"),
    ("no rows", dict(rows=0), TT_EINVAL, "empty problem"),
    ("c off a chunk", dict(c=1020), TT_EINVAL, "multiples of 8"),
    ("stride off a chunk", dict(ldx=1028), TT_EINVAL, "multiples of 8"),
    ("stride < c", dict(ldx=512), TT_EINVAL, "stride >= c"),
    ("bad dtype", dict(dtype=3), TT_EINVAL, "bad dtype"),
    ("negative eps", dict(eps=-1.0), TT_EINVAL, "eps"),
    ("x off a chunk", dict(x=P + 8), TT_EINVAL, "16-byte boundaries"),
    ("y off a chunk", dict(y=2 * P + 2), TT_EINVAL, "16-byte boundaries"),
]


@pytest.mark.parametrize("what,fault,code,text", LNB_CASES, ids=[c[0] for c in LNB_CASES])
def test_layernorm_block_refusal(lib, what, fault, code, text):
    assert fault
    a = dict(LNB, **fault)
    assert lib.tt_layernorm_block(*[a[k] for k in LNB_ORDER], None) == code
    msg = lib.tt_last_error().decode()
    assert msg.startswith("tt_layernorm_block:") and text in msg, msg


# ---- tt_frames_out: one decoded chunk
FRO = dict(src=P, src_dtype=TT_F16, n=14, ch=3, h=32, w=56, kind=1, dst=2 * P)
FRO_ORDER = list(FRO)
FRO_CASES = [
    ("null src", dict(src=None), TT_EINVAL, "null operand"),
    ("null dst", dict(dst=None), TT_EINVAL, "null operand"),
    ("bad dtype", dict(src_dtype=9), TT_EINVAL, "bad dtype"),
    ("kind 2", dict(kind=2), TT_EINVAL, "kind 2"),
    ("no frames", dict(n=0), TT_EINVAL, "empty problem"),
    ("no columns", dict(w=0), TT_EINVAL, "empty problem"),
    ("5 channels", dict(ch=5), TT_EUNSUPPORTED, "5 channels"),
    ("0 channels", dict(ch=0), TT_EUNSUPPORTED, "0 channels"),
    ("src off an element", dict(src=P + 1), TT_EINVAL, "element size"),
    ("fp32 dst off an element", dict(kind=0, dst=2 * P + 2), TT_EINVAL, "element size"),
]


@pytest.mark.parametrize("what,fault,code,text", FRO_CASES, ids=[c[0] for c in FRO_CASES])
def test_frames_out_refusal(lib, what, fault, code, text):
    assert fault
    a = dict(FRO, **fault)
    assert lib.tt_frames_out(*[a[k] for k in FRO_ORDER], None) == code
    msg = lib.tt_last_error().decode()
    assert msg.startswith("tt_frames_out:") and text in msg, msg


def test_ops_refuse_cpu_tensors(lib):
    from this_and_that_vdm_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.clip_image(torch.zeros(1, 20, 28, 3, dtype=torch.uint8), (8, 12), (0.5,) * 3, (0.25,) * 3, torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.layernorm_block(torch.zeros(10, 24), 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frames_out(torch.zeros(1, 3, 2, 8), 0)


# ---- the pipeline with the option off (and, to show the trap is armed, on)
class _HostLoop:
    """stands in for DenoiseLoop (a GPU object): hands the initial latents back, so that pipe(...) runs on the CPU end to end"""

    def __init__(self, unet, controlnet, use_graph=True):
        self.unet, self.controlnet = unet, controlnet

    def begin(self, latents, **kw):
        self.latents = latents.float()

    def step(self):
        pass

    def result(self):
        return self.latents


def _pipe(monkeypatch, **kw):
    from tests.stubs import StubCLIPVision, StubVAE
    from this_and_that_vdm_amd import ops
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline, UNetSpatioTemporalConditionModel
    from this_and_that_vdm_amd.svd import pipeline_stable_video_diffusion_controlnet as mod
    monkeypatch.setattr(mod, "DenoiseLoop", _HostLoop)
    called = []

    def trap(name):
        def f(*a, **k):
            called.append(name)
            raise AssertionError(f"ops.{name} reached")
        return f
    for name in ("clip_image", "layernorm_block", "frames_out"):
        monkeypatch.setattr(ops, name, trap(name))
    unet = UNetSpatioTemporalConditionModel(block_out_channels=(64, 64, 64, 64), num_attention_heads=(1, 1, 1, 1), cross_attention_dim=64,
                                            num_frames=2)
    pipe = StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE(), image_encoder=StubCLIPVision(), unet=unet, **kw)
    pipe.set_progress_bar_config(disable=True)
    return pipe, called


def _pil():
    g = np.random.default_rng(3)
    return PIL.Image.fromarray(g.integers(0, 256, (64, 96, 3), dtype=np.uint8))


def test_pipeline_with_the_option_off_never_calls_the_new_ops(lib, monkeypatch):
    from tests.stubs import StubTextEncoder
    pipe, called = _pipe(monkeypatch)
    assert pipe.native_image_io is False
    ids = torch.arange(8).view(1, 8)
    call = dict(prompt=ids, use_text=True, text_encoder=StubTextEncoder(), height=64, width=96, num_frames=2, num_inference_steps=1,
                latents=torch.zeros(1, 2, 4, 8, 12), decode_chunk_size=1)
    frames = pipe(_pil(), output_type="np", **call).frames
    assert frames.shape == (1, 2, 64, 96, 3) and frames.dtype == np.float32
    pil = pipe(_pil(), output_type="pil", **call).frames
    assert len(pil) == 1 and len(pil[0]) == 2 and pil[0][0].size == (96, 64)
    assert called == []


@pytest.mark.parametrize("stage", ["clip_image", "layernorm_block", "frames_out"])
def test_pipeline_with_the_option_on_reaches_each_new_op(lib, monkeypatch, stage):
    """the same request with ``native_image_io=True`` (keyword of from_pretrained) runs into the trapped op of every stage: the test
    above would notice a call"""
    from tests.stubs import StubTextEncoder
    from this_and_that_vdm_amd import ops
    pipe, called = _pipe(monkeypatch, native_image_io=True)
    assert pipe.native_image_io is True
    ids = torch.arange(8).view(1, 8)
    if stage == "clip_image":
        with pytest.raises(AssertionError, match="ops.clip_image reached"):
            pipe.encode_clip(_pil(), ids, False, None, "cpu", 1, True)
    elif stage == "layernorm_block":
        with pytest.raises(AssertionError, match="ops.layernorm_block reached"):
            pipe.encode_clip(torch.rand(1, 3, 224, 224), ids, True, StubTextEncoder(), "cpu", 1, True)       # tensor image: no resize
    else:
        with pytest.raises(AssertionError, match="ops.frames_out reached"):
            pipe(torch.rand(1, 3, 64, 96), height=64, width=96, num_frames=2, num_inference_steps=1, latents=torch.zeros(1, 2, 4, 8, 12),
                 output_type="np")
    assert called == [stage]
    pipe.feature_extractor = None
    with pytest.raises(RuntimeError, match="no feature_extractor"):
        pipe.encode_clip(_pil(), ids, False, None, "cpu", 1, True)
