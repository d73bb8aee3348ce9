"""GPU: switching the sampler of the drop-in pipelines with the diffusers idiom
``pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`` (stub VAE / CLIP of tests/test_pipeline_gpu.py):
the call hands the scheduler's coefficients to the fused loop, its result is a direct DenoiseLoop.begin(multistep=...) run on the very
constants the call built, it differs from the Euler call, the callback runs once per step, and putting the Euler scheduler back
reproduces the Euler call bit for bit."""
import numpy as np
import pytest
import torch

from tests.parity_common import build_pair
from tests.stubs import StubCLIPVision, StubTextEncoder, StubVAE

pytestmark = pytest.mark.gpu

STEPS = 6


@pytest.fixture(scope="module")
def parts():
    p_unet, p_cn, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    return p_unet, p_cn, StubVAE().cuda().half(), StubCLIPVision().cuda().half(), StubTextEncoder().cuda().half()


@pytest.fixture()
def begun(monkeypatch):
    """what every DenoiseLoop.begin() of the test received (tensors cloned: the loop's static buffers are refilled by later calls)"""
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    seen, real = [], DenoiseLoop.begin

    def begin(self, **kw):
        seen.append({k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in kw.items()})
        return real(self, **kw)

    monkeypatch.setattr(DenoiseLoop, "begin", begin)
    return seen


def _request():
    g = torch.Generator().manual_seed(11)
    image = torch.rand(1, 3, 64, 128, generator=g)
    cond = torch.rand(4, 3, 64, 128, generator=g).numpy().astype(np.float32)
    ids = torch.randint(0, 100, (1, 8), generator=g)
    return image, cond, ids


@torch.no_grad()
def test_vgl_pipeline_switches_sampler_with_from_config(parts, begun):
    from this_and_that_vdm_amd.svd import (DenoiseLoop, DPMSolverMultistepScheduler, EulerDiscreteScheduler,
                                           StableVideoDiffusionControlNetPipeline)
    p_unet, p_cn, vae, clip, txt = parts
    pipe = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=vae, image_encoder=clip, unet=p_unet)
    assert type(pipe.scheduler) is EulerDiscreteScheduler                 # from_pretrained keeps building Euler
    pipe.set_progress_bar_config(disable=True)
    image, cond, ids = _request()
    lat0 = torch.randn(1, 4, 4, 8, 16, generator=torch.Generator().manual_seed(5))

    def call(**kw):
        return pipe(image.cuda(), cond, p_cn, prompt=ids.cuda(), use_text=True, text_encoder=txt, height=64, width=128, num_frames=4,
                    num_inference_steps=STEPS, fps=7, motion_bucket_id=200, noise_aug_strength=0.0, latents=lat0.clone(),
                    output_type="latent", guess_mode=False, generator=torch.Generator().manual_seed(1), **kw).frames.clone()

    euler = call()
    assert "multistep" not in begun[-1]
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    seen = []
    two_m = call(callback_on_step_end=lambda p, i, t, kw: seen.append((i, tuple(kw["latents"].shape))) or {})
    assert seen == [(i, (1, 4, 4, 8, 16)) for i in range(STEPS)] and pipe.num_timesteps == STEPS
    assert two_m.shape == euler.shape and bool(torch.isfinite(two_m).all()) and not torch.equal(two_m, euler)
    kw = begun[-1]
    coefs = pipe.scheduler.multistep_coefficients
    assert torch.equal(kw["multistep"].cpu(), coefs.cpu()) and coefs.shape == (STEPS,) and bool((coefs[1:STEPS - 1] > 0).all())
    direct = DenoiseLoop(p_unet, p_cn, use_graph=True).begin(**kw).run()
    assert torch.equal(direct.to(two_m.dtype), two_m), "the call is a DenoiseLoop.begin(multistep=...) run on the constants it built"
    no_cb = call()
    assert torch.equal(no_cb, two_m)                                       # a callback that replaces nothing changes nothing
    pipe.scheduler = EulerDiscreteScheduler.from_config(pipe.scheduler.config)
    assert torch.equal(call(), euler) and "multistep" not in begun[-1]


@torch.no_grad()
def test_vl_pipeline_switches_sampler_with_from_config(parts, begun):
    from this_and_that_vdm_amd.svd import DPMSolverMultistepScheduler, StableVideoDiffusionPipeline
    p_unet, _, vae, clip, _ = parts
    pipe = StableVideoDiffusionPipeline.from_pretrained(None, vae=vae, image_encoder=clip, unet=p_unet)
    pipe.set_progress_bar_config(disable=True)
    image, _, _ = _request()
    call = lambda: pipe(image.cuda(), height=64, width=128, num_frames=4, num_inference_steps=3, output_type="latent",
                        generator=torch.Generator().manual_seed(2)).frames.clone()
    euler = call()
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    two_m = call()
    assert torch.equal(begun[-1]["multistep"].cpu(), pipe.scheduler.multistep_coefficients.cpu()) and "multistep" not in begun[0]
    assert bool(torch.isfinite(two_m).all()) and not torch.equal(two_m, euler)
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(dict(pipe.scheduler.config, solver_order=1))
    one = call()
    assert float(begun[-1]["multistep"].abs().max()) == 0.0 and not torch.equal(one, two_m)
