"""CPU: the two halves factored out of the pipelines' generation routine -- _request_setup (everything step-invariant of a call's
requests, on a scheduler the caller names) and _request_finish (final latents -> what the caller receives) -- with the stub CLIP / VAE.
A request set up on a scheduler instance of its own must get that instance's schedule and initial noise scale and leave the pipeline's
scheduler alone; set up on the pipeline's scheduler it is what __call__ always built."""
import copy

import torch

from tests.stubs import StubCLIPVision, StubVAE
from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline, UNetSpatioTemporalConditionModel
from this_and_that_vdm_amd.svd.pipeline_utils import tensor2vid

KW = dict(block_out_channels=(64, 64, 64, 64), num_attention_heads=(1, 1, 1, 1), cross_attention_dim=32, num_frames=3)
F_, H_, W_ = 3, 32, 48


def _pipe():
    return StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE(), image_encoder=StubCLIPVision(),
                                                        unet=UNetSpatioTemporalConditionModel(**KW))


def _setup(pipe, steps, scheduler, seed=5, max_guidance_scale=3.0):
    image = torch.rand(1, 3, H_, W_, generator=torch.Generator().manual_seed(seed))
    with torch.no_grad():
        return pipe._request_setup(image, None, None, None, False, None, H_, W_, F_, steps, 1.0, max_guidance_scale, 7, 127, 0.02, 1,
                                   torch.Generator().manual_seed(100 + seed), None, False, scheduler)


def test_a_request_on_a_scheduler_of_its_own_leaves_the_pipelines_scheduler_alone():
    pipe = _pipe()
    pipe.scheduler.set_timesteps(3)
    kept = (pipe.scheduler.timesteps.clone(), pipe.scheduler.sigmas.clone())
    own4, own2 = copy.deepcopy(pipe.scheduler), copy.deepcopy(pipe.scheduler)
    r4, r2 = _setup(pipe, 4, own4), _setup(pipe, 2, own2)
    assert len(r4.timesteps) == 4 and len(r2.timesteps) == 2 and len(r4.sigmas) == 5 and len(r2.sigmas) == 3
    assert r4.sigmas is own4.sigmas and r2.timesteps is own2.timesteps
    assert torch.equal(pipe.scheduler.timesteps, kept[0]) and torch.equal(pipe.scheduler.sigmas, kept[1])
    # the initial latents carry the request's own init_noise_sigma: the same draw, scaled by each schedule's
    noise = r4.latents / own4.init_noise_sigma
    torch.testing.assert_close(r2.latents, noise * own2.init_noise_sigma, rtol=1e-6, atol=0)
    assert r4.latents.shape == (1, F_, 4, H_ // 8, W_ // 8) and r4.nreq == 1 and r4.num_frames == F_
    assert r4.do_cfg and not r4.ip2p and r4.image_latents.shape == (2, F_, 4, H_ // 8, W_ // 8) and r4.ehs.shape[0] == 2
    assert torch.equal(r4.added_time_ids, torch.tensor([[6.0, 127.0, 0.02]] * 2, dtype=r4.added_time_ids.dtype))       # fps - 1
    assert r4.guidance.shape == (1, F_, 1, 1, 1) and r4.gesture_latents is None
    r1 = _setup(pipe, 2, copy.deepcopy(pipe.scheduler), max_guidance_scale=1.0)
    assert not r1.do_cfg and r1.image_latents.shape[0] == 1 and r1.ehs.shape[0] == 1


def test_setup_on_the_pipelines_scheduler_is_the_same_request():
    pipe = _pipe()
    own = copy.deepcopy(pipe.scheduler)
    a, b = _setup(pipe, 4, pipe.scheduler), _setup(pipe, 4, own)
    assert len(pipe.scheduler.timesteps) == 4                    # __call__'s path: the pipeline's scheduler holds the schedule
    for name in ("ehs", "image_latents", "added_time_ids", "timesteps", "sigmas", "latents", "guidance"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    # prepare_latents without the argument scales by the pipeline's scheduler, as before
    lat = torch.ones(1, F_, 4, 4, 6)
    assert torch.equal(pipe.prepare_latents(1, F_, 8, H_, W_, torch.float32, "cpu", None, lat), lat * pipe.scheduler.init_noise_sigma)
    own.set_timesteps(2)
    assert torch.equal(pipe.prepare_latents(1, F_, 8, H_, W_, torch.float32, "cpu", None, lat, scheduler=own), lat * own.init_noise_sigma)


def test_request_finish_returns_latents_or_decoded_frames():
    pipe = _pipe()
    lat = torch.randn(2, F_, 4, 4, 6, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert pipe._request_finish(lat, F_, 2, "latent") is lat
        pt = pipe._request_finish(lat, F_, 2, "pt")
        want = tensor2vid(pipe.decode_latents(lat, F_, 2), pipe.image_processor, output_type="pt")
    assert pt.shape == (2, F_, 3, H_, W_) and torch.equal(pt, want)
