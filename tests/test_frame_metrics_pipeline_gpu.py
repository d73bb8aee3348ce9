"""GPU: metrics.compare_frames on what the pipelines return (tiny UNet, stub VAE / CLIP of tests/test_pipeline_gpu.py): the same seed
twice is the same video (psnr inf, ssim 1 in every frame), another sampler on the same noise is a different one (finite psnr, ssim < 1),
the "pil" frames compare exactly as the device uint8 frames of the same decode do, and a batch of videos gives per-video values equal
to those of separate calls."""
import math

import numpy as np
import pytest
import torch

from tests.parity_common import build_pair
from tests.stubs import StubCLIPVision, StubVAE

pytestmark = pytest.mark.gpu
CHUNK = 4


@pytest.fixture(scope="module")
def videos():
    """(pipe, euler "pil" frames, the same call again, DPM-Solver++ 2M "pil" frames, the two samplers' final latents)"""
    from this_and_that_vdm_amd.svd import DPMSolverMultistepScheduler, EulerDiscreteScheduler, StableVideoDiffusionPipeline
    p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    pipe = StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE().cuda().half(), image_encoder=StubCLIPVision().cuda().half(), unet=p_unet)
    pipe.set_progress_bar_config(disable=True)
    image = torch.rand(1, 3, 64, 128, generator=torch.Generator().manual_seed(11))

    @torch.no_grad()
    def call(output_type):
        out = pipe(image.cuda(), height=64, width=128, num_frames=4, num_inference_steps=3, output_type=output_type,
                   decode_chunk_size=CHUNK, generator=torch.Generator().manual_seed(2)).frames
        return out.clone() if torch.is_tensor(out) else out

    euler, again, euler_lat = call("pil"), call("pil"), call("latent")
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    two_m, two_m_lat = call("pil"), call("latent")
    pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config)
    return pipe, euler, again, two_m, euler_lat, two_m_lat


def test_the_same_seed_is_the_same_video(videos):
    from this_and_that_vdm_amd import metrics
    _, euler, again, _, _, _ = videos
    m = metrics.compare_frames(euler, again)
    assert m.frame_psnr.shape == (1, 4)
    assert (m.frame_psnr == math.inf).all() and (m.frame_ssim == 1.0).all() and (m.frame_mse == 0.0).all()
    assert m.psnr[0] == math.inf and m.ssim[0] == 1.0


def test_another_sampler_is_another_video(videos):
    from this_and_that_vdm_amd import metrics
    _, euler, _, two_m, _, _ = videos
    m = metrics.compare_frames(euler, two_m)
    assert np.isfinite(m.frame_psnr).all() and (m.frame_psnr > 0).all() and (m.frame_ssim < 1.0).all() and (m.frame_mse > 0).all()
    assert math.isfinite(m.psnr[0]) and m.ssim[0] < 1.0


@torch.no_grad()
def test_pil_frames_compare_as_the_device_frames_of_the_same_decode(videos):
    from this_and_that_vdm_amd import metrics, ops
    from this_and_that_vdm_amd.svd.pipeline_utils import DevicePixels
    pipe, euler, _, two_m, euler_lat, two_m_lat = videos
    dev = [torch.cat([ops.frames_out(s, 1) for s in pipe._decode_chunks(lat.to(pipe.vae.dtype), CHUNK)], 0) for lat in (euler_lat, two_m_lat)]
    assert dev[0].dtype == torch.uint8 and tuple(dev[0].shape) == (4, 64, 128, 3) and dev[0].is_cuda
    assert np.array_equal(dev[0].cpu().numpy(), np.stack([np.asarray(im) for im in euler[0]]))     # the same decode
    on_dev = metrics.compare_frames(dev[0], dev[1])
    from_pil = metrics.compare_frames(euler, two_m)
    px = metrics.compare_frames(DevicePixels(dev[0]), DevicePixels(dev[1]))
    for name in ("frame_mse", "frame_psnr", "frame_ssim", "frame_cs"):
        assert np.array_equal(getattr(on_dev, name), getattr(from_pil, name)[0]), name
        assert np.array_equal(getattr(on_dev, name), getattr(px, name)), name
    assert on_dev.ssim == from_pil.ssim[0] and on_dev.psnr == from_pil.psnr[0]


def test_a_batch_of_videos_gives_the_values_of_separate_calls(videos):
    from this_and_that_vdm_amd import metrics
    _, euler, again, two_m, _, _ = videos
    both = metrics.compare_frames(euler + two_m, two_m + two_m)                # lists of two videos: [2, 4, 64, 128, 3]
    first, second = metrics.compare_frames(euler, two_m), metrics.compare_frames(two_m, two_m)
    assert both.frame_ssim.shape == (2, 4)
    for name in ("frame_mse", "frame_psnr", "frame_ssim", "frame_cs", "mse", "psnr", "ssim", "cs"):
        assert np.array_equal(np.asarray(getattr(both, name)), np.concatenate([np.atleast_1d(getattr(first, name)), np.atleast_1d(getattr(second, name))])), name
    assert both.psnr[1] == math.inf and both.ssim[1] == 1.0 and math.isfinite(both.psnr[0])
