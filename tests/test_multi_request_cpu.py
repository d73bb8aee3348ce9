"""CPU: the host logic of several requests per pipeline call, with the stub VAE / CLIP of tests/stubs.py and a recording stand-in
for the fused loop: request ordering (image-major; batched tensors class by class), prompt and gesture-map expansion, decode chunks
that stay inside a video, the generator-list check, every ValueError; the off-path methods of the two drop-in models; the C ABI's
new entry points in header and binding."""
import os
import re

import numpy as np
import pytest
import torch

from tests.stubs import StubCLIPVision, StubTextEncoder, StubVAE
from this_and_that_vdm_amd.svd import (ControlNetModel, StableVideoDiffusionControlNetPipeline, StableVideoDiffusionPipeline,
                                       UNetSpatioTemporalConditionModel)
from this_and_that_vdm_amd.svd import pipeline_stable_video_diffusion_controlnet as pmod

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(block_out_channels=(64, 64, 64, 64), num_attention_heads=(1, 1, 1, 1), cross_attention_dim=64, num_frames=3)
NIMG, NVID, F_ = 2, 3, 3
R = NIMG * NVID


class FakeLoop:
    """stands in for DenoiseLoop: records what begin() receives, a step adds 1 to every latent"""
    last = None

    def __init__(self, unet, controlnet, use_graph=True):
        self.unet, self.controlnet = unet, controlnet
        FakeLoop.last = self

    def begin(self, **kw):
        self.kw = kw
        self.latents = kw["latents"].float().clone()
        return self

    def step(self):
        self.latents += 1.0

    def result(self):
        return self.latents


class ChunkVAE(StubVAE):
    """a decoder that mixes the frames of a chunk (as the temporal decoder does): each chunk has its own mean removed"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def decode(self, z, num_frames=None):
        self.calls.append((z.shape[0], num_frames))
        out = super().decode(z, num_frames)
        out.sample = out.sample - out.sample.mean()
        return out


@pytest.fixture()
def pipes(monkeypatch):
    monkeypatch.setattr(pmod, "DenoiseLoop", FakeLoop)
    unet = UNetSpatioTemporalConditionModel(**KW)
    vgl = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=ChunkVAE(), image_encoder=StubCLIPVision(), unet=unet)
    vl = StableVideoDiffusionPipeline.from_pretrained(None, vae=ChunkVAE(), image_encoder=StubCLIPVision(), unet=unet)
    for p in (vgl, vl):
        p.set_progress_bar_config(disable=True)
    cn_kw = dict(KW)
    cn_kw.pop("num_frames")
    return vgl, vl, ControlNetModel(**cn_kw)


def _inputs():
    g = torch.Generator().manual_seed(4)
    images = torch.rand(NIMG, 3, 32, 48, generator=g)
    conds = [torch.rand(F_, 3, 32, 48, generator=g).numpy() for _ in range(NIMG)]
    ids = torch.randint(0, 100, (NIMG, 6), generator=g)
    return images, conds, ids


CALL = dict(use_text=True, height=32, width=48, num_frames=F_, num_inference_steps=2, noise_aug_strength=0.1)


@torch.no_grad()
def test_requests_are_image_major_and_batched_tensors_class_by_class(pipes):
    vgl, _, cn = pipes
    images, conds, ids = _inputs()
    txt = StubTextEncoder()
    gens = lambda: [torch.Generator().manual_seed(50 + r) for r in range(R)]
    out = vgl(images, conds, cn, prompt=ids, text_encoder=txt, num_videos_per_prompt=NVID, generator=gens(), output_type="latent",
              guess_mode=False, **CALL).frames
    kw = FakeLoop.last.kw
    assert out.shape == (R, F_, 4, 4, 6)
    assert kw["latents"].shape == (R, F_, 4, 4, 6) and kw["guidance_scale"].shape == (R, F_, 1, 1, 1)
    ehs, il, ids_t, ges = kw["encoder_hidden_states"], kw["image_latents"], kw["added_time_ids"], kw["controlnet_cond"]
    assert ehs.shape[0] == il.shape[0] == ids_t.shape[0] == 2 * R and ges.shape == (R, F_, 4, 4, 6)
    assert float(ehs[:R].abs().max()) == 0.0 and float(il[:R].abs().max()) == 0.0          # all uncond first: torch.cat([neg, cond])
    # (the stub encoders' CPU GEMMs / convs sum in an order that depends on the batch size: 1e-5, far below the O(1) distance between requests)
    same = lambda x, y: torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-5)
    for r in range(R):
        i = r // NVID
        # ... and request r is what a call of its own builds: image i, prompt row i, gesture map i, generator r
        one = vgl(images[i:i + 1], conds[i], cn, prompt=ids[i:i + 1], text_encoder=txt, generator=torch.Generator().manual_seed(50 + r),
                  output_type="latent", guess_mode=False, **CALL).frames
        k1 = FakeLoop.last.kw
        same(ehs[R + r], k1["encoder_hidden_states"][1])
        same(il[R + r], k1["image_latents"][1])
        same(ges[r], k1["controlnet_cond"])
        torch.testing.assert_close(kw["latents"][r:r + 1], k1["latents"], rtol=0, atol=0)
        torch.testing.assert_close(out[r:r + 1], one, rtol=0, atol=0)
    assert not torch.equal(il[R], il[R + 1])                    # the videos of one image noise their own copy of it (generator r)
    # a shared [F,3,H,W] map stays one map; one prompt row serves every image; a single generator draws [R, ...] at once
    vgl(images, conds[1], cn, prompt=ids[1:], text_encoder=txt, num_videos_per_prompt=NVID, generator=torch.Generator().manual_seed(1),
        output_type="latent", guess_mode=False, **CALL)
    kw = FakeLoop.last.kw
    assert kw["controlnet_cond"].shape == (F_, 4, 4, 6) and kw["latents"].shape == (R, F_, 4, 4, 6)
    one_row = vgl.encode_clip(images, ids[1:], True, txt, "cpu", NVID, True)
    assert one_row.shape[0] == 2 * R and torch.equal(one_row, vgl.encode_clip(images, ids[1:].repeat(NIMG, 1), True, txt, "cpu", NVID, True))
    assert torch.equal(one_row, kw["encoder_hidden_states"])
    # use_instructpix2pix: three classes, (context + image, image only, nothing) -- reference :182-184, :208-211
    vgl(images, conds, cn, prompt=ids, text_encoder=txt, num_videos_per_prompt=NVID, generator=gens(), output_type="latent",
        guess_mode=False, use_instructpix2pix=True, **CALL)
    kw = FakeLoop.last.kw
    ehs, il = kw["encoder_hidden_states"], kw["image_latents"]
    assert ehs.shape[0] == il.shape[0] == 3 * R and float(ehs[R:].abs().max()) == 0.0 and float(il[2 * R:].abs().max()) == 0.0
    assert torch.equal(il[:R], il[R:2 * R]) and float(ehs[:R].abs().min(0)[0].max()) > 0.0


@torch.no_grad()
def test_callback_sees_all_requests_and_may_replace_them(pipes):
    _, vl, _ = pipes
    images, _, _ = _inputs()
    seen = []

    def cb(pipe, i, t, kw):
        seen.append(tuple(kw["latents"].shape))
        return {"latents": kw["latents"] * 0.0} if i == 0 else {}

    lat0 = torch.ones(R, F_, 4, 4, 6)
    out = vl(images, height=32, width=48, num_frames=F_, num_inference_steps=2, num_videos_per_prompt=NVID, latents=lat0,
             output_type="latent", callback_on_step_end=cb).frames
    assert seen == [(R, F_, 4, 4, 6)] * 2
    assert torch.equal(out, torch.ones_like(out))               # zeroed after step 0, + 1 in step 1


@torch.no_grad()
def test_decode_chunks_stay_inside_a_video(pipes):
    """decode_chunk_size = 2, F = 3: chunks of 2 + 1 frames per video, never a chunk of the last frame of one video and the first of
    the next (what chunking flatten(0, 1) gives) -- against a decode computed by hand, video by video."""
    vgl, _, _ = pipes
    vae = vgl.vae
    lat = torch.randn(R, F_, 4, 4, 6, generator=torch.Generator().manual_seed(0))
    out = vgl.decode_latents(lat, F_, decode_chunk_size=2)
    assert vae.calls == [(2, 2), (1, 1)] * R
    assert out.shape == (R, 3, F_, 32, 48) and out.dtype == torch.float32
    for r in range(R):
        z = lat[r] / vae.config.scaling_factor
        want = torch.cat([ChunkVAE.decode(vae, z[:2]).sample, ChunkVAE.decode(vae, z[2:]).sample], 0)
        torch.testing.assert_close(out[r], want.permute(1, 0, 2, 3).float(), rtol=0, atol=0)
        alone = vgl.decode_latents(lat[r:r + 1], F_, decode_chunk_size=2)
        assert torch.equal(out[r], alone[0])


@torch.no_grad()
def test_output_types(pipes):
    _, vl, _ = pipes
    images, _, _ = _inputs()
    call = dict(height=32, width=48, num_frames=F_, num_inference_steps=1, num_videos_per_prompt=NVID, decode_chunk_size=2)
    frames = vl(images, output_type="np", generator=torch.Generator().manual_seed(0), **call).frames
    assert isinstance(frames, np.ndarray) and frames.shape == (R, F_, 32, 48, 3)
    pil = vl(images, output_type="pil", generator=torch.Generator().manual_seed(0), **call).frames
    assert isinstance(pil, list) and len(pil) == R and all(len(v) == F_ and v[0].size == (48, 32) for v in pil)
    pt = vl(images, output_type="pt", generator=torch.Generator().manual_seed(0), **call).frames
    assert pt.shape == (R, F_, 3, 32, 48)
    lat = vl(images, output_type="latent", generator=torch.Generator().manual_seed(0), **call).frames
    assert lat.shape == (R, F_, 4, 4, 6)


def test_mismatched_counts_raise_value_errors_naming_the_counts(pipes):
    vgl, vl, cn = pipes
    images, conds, ids = _inputs()
    txt = StubTextEncoder()
    base = dict(height=32, width=48, num_frames=F_, num_inference_steps=1, num_videos_per_prompt=NVID)
    with pytest.raises(ValueError, match=rf"generators of length {R - 1}.*batch size of {R} \({NIMG} image\(s\) x {NVID} video"):
        vl(images, generator=[torch.Generator() for _ in range(R - 1)], **base)
    with pytest.raises(ValueError, match=rf"generators of length {NIMG}.*batch size of {R}"):
        vl(images, generator=[torch.Generator() for _ in range(NIMG)], **base)            # one per image is not enough: one per video
    with pytest.raises(ValueError, match=r"latents \(2, 3, 4, 4, 6\): expected \(6, 3, 4, 4, 6\)"):
        vl(images, latents=torch.zeros(NIMG, F_, 4, 4, 6), **base)
    with pytest.raises(ValueError, match=r"condition_img \(3, 3, 3, 32, 48\).*\[2,F,3,H,W\]"):
        vgl(images, conds + conds[:1], cn, guess_mode=False, **base)
    with pytest.raises(ValueError, match=r"condition_img \(2, 3, 32, 48\).*F = 3"):
        vgl(images, conds[0][:2], cn, guess_mode=False, **base)
    with pytest.raises(ValueError, match=r"prompt: 3 rows of token ids for 2 image"):
        vl(images, prompt=torch.cat([ids, ids[:1]]), use_text=True, text_encoder=txt, **base)
    with pytest.raises(ValueError, match="at least one image and one video"):
        vl(images, **dict(base, num_videos_per_prompt=0))


def test_loop_refuses_bad_request_sets_before_touching_the_device():
    from this_and_that_vdm_amd import ops
    from this_and_that_vdm_amd.svd import denoise
    unet = UNetSpatioTemporalConditionModel(**KW)                                       # on the CPU: prepare() would raise RuntimeError
    h, w, s, d, steps = 4, 6, 5, 64, 2

    def kw(nr, c, **over):
        b = nr * c
        base = dict(latents=torch.zeros(nr, F_, 4, h, w), image_latents=torch.zeros(b, F_, 4, h, w),
                    encoder_hidden_states=torch.zeros(b, s, d), added_time_ids=torch.zeros(b, 3),
                    guidance_scale=torch.ones(1, F_, 1, 1, 1) if c > 1 else None, sigmas=torch.ones(steps + 1), timesteps=torch.ones(steps))
        base.update(over)
        return base

    cap = denoise.MAX_BATCH
    assert cap >= 8 and cap <= 32                       # R = 4 with CFG 2 fits; tt_small_linear takes at most 32 rows
    for nr, c in ((cap + 1, 1), (cap // 2 + 1, 2), (cap // 3 + 1, 3)):
        with pytest.raises(ValueError, match=rf"{nr * c} batch elements.*cap is {cap}"):
            denoise.DenoiseLoop(unet).begin(**kw(nr, c))
    with pytest.raises(RuntimeError, match="no CPU fallback"):                          # the cap itself passes the check
        denoise.DenoiseLoop(unet).begin(**kw(cap // 2, 2))
    with pytest.raises(ValueError, match=r"got 8 image-latent batch elements for 3 request"):
        denoise.DenoiseLoop(unet).begin(**kw(4, 2, latents=torch.zeros(3, F_, 4, h, w)))
    with pytest.raises(ValueError, match=r"got 8 image-latent batch elements for 2 request"):
        denoise.DenoiseLoop(unet).begin(**kw(2, 4))                                     # a CFG batch of 4
    with pytest.raises(ValueError, match=r"encoder_hidden_states \(3\)"):
        denoise.DenoiseLoop(unet).begin(**kw(2, 2, encoder_hidden_states=torch.zeros(3, s, d)))
    with pytest.raises(ValueError, match=r"guidance_scale holds 9 values"):
        denoise.DenoiseLoop(unet).begin(**kw(2, 2, guidance_scale=torch.ones(3, F_, 1, 1, 1)))
    with pytest.raises(ValueError, match=r"controlnet_cond \(3, 3, 4, 4, 6\)"):
        denoise.DenoiseLoop(unet).begin(**kw(2, 2, controlnet_cond=torch.zeros(3, F_, 4, h, w)))
    with pytest.raises(ValueError, match="image_guidance_scale"):
        denoise.DenoiseLoop(unet).begin(**kw(2, 3))
    with pytest.raises(NotImplementedError, match="split_cfg"):
        denoise.DenoiseLoop(unet, split_cfg=True).begin(**kw(2, 2))
    # the ops wrappers name the counts too (host checks in front of the C entry points)
    z = torch.zeros
    with pytest.raises(ValueError, match="cond holds"):
        ops.prep_model_input_requests(z(2, F_, 4, h, w), z(4, F_, 4, h, w), z(3, F_, 4, h, w), z(3), 0, 2, 2, F_, h, w, 16, torch.float16)
    with pytest.raises(ValueError, match="guidance holds 9 values"):
        ops.cfg_euler_step_requests(z(8, 4), z(2, F_, 4, h, w), z(3, F_), z(3), 0, 2, 2, F_, h, w)
    with pytest.raises(ValueError, match="image_guidance_scale"):
        ops.cfg_euler_step_requests(z(8, 4), z(2, F_, 4, h, w), z(1, F_), z(3), 0, 2, 3, F_, h, w)


def test_geometry_and_zero_context_bookkeeping_per_request():
    """layers.Geom / StepContext: batch element c * R + r; the temporal residue classes are those of ONE request's CFG batch, and a
    class is skipped only when every request's context of that class is all-zero."""
    from this_and_that_vdm_amd.svd.layers import Geom, StepContext
    g = Geom(6, 4, 8, 16, requests=3)
    assert (g.cfg, g.ctx_batches, g.n, g.m) == (2, 6, 24, 24 * 128)
    assert Geom(2, 4, 8, 16).cfg == 2 and Geom(1, 4, 8, 16, 1, 2).cfg == 2             # one request; a split-CFG half
    sc = lambda mask: StepContext(None, None, None, 5, 8, zero_mask=mask)
    assert sc(0b000111).live_classes(g) == [1] and sc(0b000111).live_batches(g) == (3, 3)   # the three uncond contexts are zero
    assert sc(0b000011).live_classes(g) is None and sc(0b000011).live_batches(g) == (2, 4)  # request 2's uncond context is not
    assert sc(0b000101).live_batches(g) is None                                            # live elements not contiguous: general path
    assert sc(0).live_classes(g) is None and sc(0).live_batches(g) is None
    g3 = Geom(6, 4, 8, 16, requests=2)                                                      # CFG 3: 128 pixels are no multiple of 3
    assert g3.cfg == 3 and sc(0b111100).live_classes(g3) is None and sc(0b111100).live_batches(g3) == (0, 2)


@pytest.mark.parametrize("cls", ["unet", "controlnet"])
def test_off_path_model_methods(cls):
    """the five methods of the reference models a caller may touch outside the forward (unet_spatio_temporal_condition.py:254-361):
    explicit inference-only errors, or no-ops where a no-op is exact"""
    kw = dict(KW)
    if cls == "controlnet":
        kw.pop("num_frames")
    model = (UNetSpatioTemporalConditionModel if cls == "unet" else ControlNetModel)(**kw)
    keys = set(model.state_dict())
    with pytest.raises(NotImplementedError, match="inference-only build"):
        model.attn_processors
    with pytest.raises(NotImplementedError, match="inference-only build"):
        model.set_attn_processor(object())
    assert model.set_default_attn_processor() is None
    assert model.enable_forward_chunking() is None and model.enable_forward_chunking(2, dim=1) is None
    with pytest.raises(ValueError, match="either 0 or 1, not 2"):
        model.enable_forward_chunking(dim=2)
    assert model.disable_forward_chunking() is None
    assert model._set_gradient_checkpointing(model.mid_block, True) is None and not hasattr(model.mid_block, "gradient_checkpointing")
    holder = torch.nn.Module()
    holder.gradient_checkpointing = False
    model._set_gradient_checkpointing(holder, True)
    assert holder.gradient_checkpointing is True
    assert set(model.state_dict()) == keys and hasattr(model, "mid_block")      # nothing registered, attribute lookup intact


def test_abi_declares_and_binds_the_new_entry_points():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.tt_abi_version() == 11
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ttvdm.h")).read(), flags=re.S)
    for name in ("tt_prep_model_input_requests", "tt_cfg_euler_step_requests"):
        m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} not declared in ttvdm.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert len(params) == len(args), (name, params)
        for p, a in zip(params, args):
            want = _lib._vp if "*" in p or "tt_stream_t" in p else {"int32_t": _lib._i32, "int64_t": _lib._i64, "float": _lib._f32}[p.split()[0]]
            assert a is want, (name, p, a)
        assert hasattr(lib, name)
    # the single-request entry points are as they were
    assert len(_lib.SIGNATURES["tt_prep_model_input"][1]) == 13 and len(_lib.SIGNATURES["tt_cfg_euler_step"][1]) == 11
    assert len(_lib.SIGNATURES["tt_cfg3_euler_step"][1]) == 11
