"""GPU: several requests in one pipeline call -- two images x num_videos_per_prompt = 2 through both drop-in pipelines with the stub
CLIP / VAE of tests/test_pipeline_gpu.py.  Request r = image r // 2, video r % 2 (image-major); every video must be what a call of its
own with that request's image, prompt row, gesture map, latents and generator gives.  The joint launches may take other GEMM routes
than a single call's (routes depend on M), so latents are compared through the loop tests' fp16 limits (rel-L2 <= 3e-3,
cos >= 0.99999), not bitwise -- on the schedule those limits belong to (4 steps, as tests/test_denoise_loop_gpu.py: the error left at
the end of an Euler schedule scales with its last sigma step).  The stub encoders run in fp32: their outputs for an image are then
bit-identical at batch 4 and batch 1 (torch's fp16 conv rounds differently per batch size, 5e-4 on the image latents), so a batched
request and its single call really start from the same inputs and the comparison is about the loop and the host logic alone."""
import numpy as np
import pytest
import torch

from tests.parity_common import build_pair, err_stats
from tests.stubs import StubCLIPVision, StubTextEncoder, StubVAE

pytestmark = pytest.mark.gpu

NIMG, NVID, F_ = 2, 2, 4
R = NIMG * NVID
STEPS = 4


class RecordingVAE(StubVAE):
    """records the frame count of every decode call"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def decode(self, z, num_frames=None):
        self.calls.append((z.shape[0], num_frames))
        return super().decode(z, num_frames)


@pytest.fixture(scope="module")
def parts():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    p_unet, p_cn, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    return p_unet, p_cn, RecordingVAE().cuda(), StubCLIPVision().cuda(), StubTextEncoder().cuda()


def _inputs():
    g = torch.Generator().manual_seed(21)
    images = torch.rand(NIMG, 3, 64, 128, generator=g)
    conds = [torch.rand(F_, 3, 64, 128, generator=g).numpy().astype(np.float32) for _ in range(NIMG)]
    ids = torch.randint(0, 100, (NIMG, 8), generator=g)
    lat0 = torch.randn(R, F_, 4, 8, 16, generator=g)
    return images, conds, ids, lat0


def _pipes(parts):
    from this_and_that_vdm_amd.svd import (EulerDiscreteScheduler, StableVideoDiffusionControlNetPipeline,
                                           StableVideoDiffusionPipeline)
    p_unet, p_cn, vae, clip, txt = parts
    vgl = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=vae, image_encoder=clip, unet=p_unet, scheduler=EulerDiscreteScheduler())
    vl = StableVideoDiffusionPipeline.from_pretrained(None, vae=vae, image_encoder=clip, unet=p_unet, scheduler=EulerDiscreteScheduler())
    for p in (vgl, vl):
        p.set_progress_bar_config(disable=True)
    return vgl, vl


def _call(pipe, parts, images, cond, ids, **kw):
    """one __call__ of either pipeline (the VL one takes no gesture map / ControlNet)"""
    _, p_cn, _, _, txt = parts
    common = dict(prompt=ids.cuda(), use_text=True, text_encoder=txt, height=64, width=128, num_frames=F_, num_inference_steps=STEPS, fps=7,
                  motion_bucket_id=200, noise_aug_strength=0.05, **kw)
    if cond is None:
        return pipe(images.cuda(), **common).frames
    return pipe(images.cuda(), cond, p_cn, guess_mode=False, **common).frames


def _close(got, ref, what):
    s = err_stats(got, ref)
    print(what, s)
    assert s["rel_l2"] <= 3e-3 and s["cos"] >= 0.99999, (what, s)


@pytest.mark.parametrize("which", ["vgl_shared_map", "vgl_map_per_image", "vl"])
@torch.no_grad()
def test_batched_latents_equal_four_single_calls(parts, which):
    vgl, vl = _pipes(parts)
    images, conds, ids, lat0 = _inputs()
    pipe = vl if which == "vl" else vgl
    cond = None if which == "vl" else (conds[0] if which == "vgl_shared_map" else conds)
    seen = []
    gens = [torch.Generator().manual_seed(100 + r) for r in range(R)]
    got = _call(pipe, parts, images, cond, ids, num_videos_per_prompt=NVID, generator=gens, latents=lat0.clone(), output_type="latent",
                callback_on_step_end=lambda p, i, t, kw: seen.append(tuple(kw["latents"].shape)) or {})
    assert got.shape == (R, F_, 4, 8, 16) and seen == [(R, F_, 4, 8, 16)] * STEPS
    for r in range(R):
        i = r // NVID
        one_cond = None if cond is None else (conds[0] if which == "vgl_shared_map" else conds[i])
        ref = _call(pipe, parts, images[i:i + 1], one_cond, ids[i:i + 1], generator=torch.Generator().manual_seed(100 + r),
                    latents=lat0[r:r + 1].clone(), output_type="latent")
        _close(got[r:r + 1], ref, f"{which}: request {r} (image {i}, video {r % NVID}) vs a call of its own")
    # requests differ from one another: the two videos of an image through their generators (image noise) and latents
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[0], got[2])
    if which == "vgl_map_per_image":
        # one stacked [N,F,3,H,W] array is the same request set as the list
        again = _call(pipe, parts, images, np.stack(conds), ids, num_videos_per_prompt=NVID,
                      generator=[torch.Generator().manual_seed(100 + r) for r in range(R)], latents=lat0.clone(), output_type="latent")
        assert torch.equal(again, got)
    if which == "vl":
        # one prompt row serves every image; a single generator draws the [R, ...] tensors in one call
        out = _call(pipe, parts, images, None, ids[:1], num_videos_per_prompt=NVID, generator=torch.Generator().manual_seed(3),
                    output_type="latent")
        assert out.shape == (R, F_, 4, 8, 16) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("native", [False, True])
@torch.no_grad()
def test_frames_have_the_stated_shapes_and_videos_are_decoded_alone(parts, native):
    vgl, _ = _pipes(parts)
    vae = parts[2]
    vgl.native_image_io = native
    images, conds, ids, lat0 = _inputs()
    kw = dict(num_videos_per_prompt=NVID, generator=[torch.Generator().manual_seed(100 + r) for r in range(R)], decode_chunk_size=3)
    lat = _call(vgl, parts, images, conds, ids, latents=lat0.clone(), output_type="latent", **kw)
    vae.calls.clear()
    kw["generator"] = [torch.Generator().manual_seed(100 + r) for r in range(R)]
    frames = _call(vgl, parts, images, conds, ids, latents=lat0.clone(), output_type="np", **kw)
    assert isinstance(frames, np.ndarray) and frames.shape == (R, F_, 64, 128, 3) and frames.dtype == np.float32
    assert vae.calls == [(3, 3), (1, 1)] * R, "decode chunks must stay inside a video (decode_chunk_size = 3, F = 4)"
    # every video equals that video's latents decoded alone (same latents: bit for bit), through the same export path
    vgl.native_image_io = False
    from this_and_that_vdm_amd.svd.pipeline_utils import tensor2vid
    for r in range(R):
        alone = tensor2vid(vgl.decode_latents(lat[r:r + 1].to(vae.dtype), F_, 3), vgl.image_processor, output_type="np")
        np.testing.assert_array_equal(frames[r], alone[0])
    vgl.native_image_io = native
    kw["generator"] = [torch.Generator().manual_seed(100 + r) for r in range(R)]
    pil = _call(vgl, parts, images, conds, ids, latents=lat0.clone(), output_type="pil", **kw)
    assert len(pil) == R and all(len(v) == F_ and v[0].size == (128, 64) for v in pil)
    u8 = (frames * 255).round().astype("uint8")
    for r in range(R):
        np.testing.assert_array_equal(np.stack([np.asarray(im) for im in pil[r]]), u8[r])
    kw["generator"] = [torch.Generator().manual_seed(100 + r) for r in range(R)]
    pt = _call(vgl, parts, images, conds, ids, latents=lat0.clone(), output_type="pt", **kw)
    assert pt.shape == (R, F_, 3, 64, 128)
    vgl.native_image_io = False


def test_mismatched_counts_are_value_errors_with_the_counts(parts):
    vgl, vl = _pipes(parts)
    images, conds, ids, lat0 = _inputs()
    with pytest.raises(ValueError, match=r"length 3.*batch size of 4"):
        _call(vl, parts, images, None, ids, num_videos_per_prompt=NVID, generator=[torch.Generator() for _ in range(3)])
    with pytest.raises(ValueError, match=r"latents \(2, 4, 4, 8, 16\).*\(4, 4, 4, 8, 16\)"):
        _call(vl, parts, images, None, ids, num_videos_per_prompt=NVID, latents=lat0[:2])
    with pytest.raises(ValueError, match=r"condition_img \(3, 4, 3, 64, 128\).*\[2,F,3,H,W\]"):
        _call(vgl, parts, images, conds + conds[:1], ids, num_videos_per_prompt=NVID)
    with pytest.raises(ValueError, match=r"prompt: 3 rows.*2 image"):
        _call(vl, parts, images, None, torch.cat([ids, ids[:1]]), num_videos_per_prompt=NVID)
