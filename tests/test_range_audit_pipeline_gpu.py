"""GPU: ``range_audit=True`` on a pipeline with no stand-in model (native CLIP encoders, native VAE encoder and decoder, tiny UNet and
GestureNet): the frames of the call are bit-equal to the plain call's, and the report left in ``last_range_audit`` holds sites of all
four stages -- CLIP encode, VAE encode, the denoise loop, the decode."""
import numpy as np
import pytest
import torch

from tests import clip_reference as cr
from tests.parity_common import build_pair

pytestmark = pytest.mark.gpu

VAE_TINY = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)
PIPE_VISION = dict(cr.TINY["V257"], projection_dim=64)
PIPE_TEXT = dict(cr.TINY["T77"], hidden_size=64, num_attention_heads=1, intermediate_size=128, vocab_size=100, max_position_embeddings=77)


def _pipeline(dtype, **kw):
    from this_and_that_vdm_amd import clip
    from this_and_that_vdm_amd.svd import EulerDiscreteScheduler, StableVideoDiffusionControlNetPipeline
    from this_and_that_vdm_amd.svd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    unet, cn, _, _ = build_pair("tiny_vgl", dtype, "cuda:0", True)
    nv, nt = clip.CLIPVisionModelWithProjection(**PIPE_VISION).eval(), clip.CLIPTextModel(**PIPE_TEXT).eval()
    vae = AutoencoderKLTemporalDecoder(**VAE_TINY, native_encoder=True).eval()
    with torch.no_grad():
        for m, salt in ((nv, "clip."), (nt, "clip."), (vae, "vae.")):
            fill_parameters_(m, salt, round_to=dtype)
    nv, nt, vae = nv.to("cuda:0", dtype), nt.to("cuda:0", dtype), vae.to("cuda:0", dtype)
    pipe = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=vae, image_encoder=nv, unet=unet, scheduler=EulerDiscreteScheduler(), **kw)
    pipe.set_progress_bar_config(disable=True)
    return pipe, cn, nt


@torch.no_grad()
def test_audited_call_is_bit_equal_and_reports_all_four_stages():
    from PIL import Image
    from this_and_that_vdm_amd import audit, ops
    g = torch.Generator().manual_seed(11)
    image = Image.fromarray((torch.rand(64, 128, 3, generator=g) * 255).to(torch.uint8).numpy())
    cond = torch.rand(4, 3, 64, 128, generator=g).numpy().astype(np.float32)
    ids = torch.randint(0, 100, (1, 77), generator=g)
    lat0 = torch.randn(1, 4, 4, 8, 16, generator=torch.Generator().manual_seed(5))
    pipe, cn, nt = _pipeline(torch.float16, range_audit=True)
    assert pipe.range_audit is True and pipe.last_range_audit is None
    call = dict(output_type="np", prompt=ids.cuda(), use_text=True, text_encoder=nt, height=64, width=128, num_frames=4,
                num_inference_steps=3, fps=7, motion_bucket_id=200, noise_aug_strength=0.0, guess_mode=False, decode_chunk_size=3)
    audited = pipe(image, cond, cn, latents=lat0.clone(), **call).frames
    rep = pipe.last_range_audit
    assert isinstance(rep, audit.RangeAuditReport) and ops.AUDIT is None
    pipe.range_audit = False
    pipe.last_range_audit = None
    plain = pipe(image, cond, cn, latents=lat0.clone(), **call).frames
    assert pipe.last_range_audit is None
    assert audited.shape == (1, 4, 64, 128, 3) and np.isfinite(plain).all() and np.array_equal(audited, plain)
    sites = rep.sites()
    # (a site is named after the innermost watched module whose forward is running: the CLIP encoders run their layers inside the
    # model's own forward, so their sites carry the root's name alone)
    stages = {"CLIP encode": ("image_encoder/", "image_encoder."), "text encode": ("text_encoder/", "text_encoder."),
              "VAE encode": ("vae.encoder/", "vae.encoder."), "denoise loop": ("unet.",), "GestureNet": ("controlnet.",),
              "decode": ("vae.decoder/", "vae.decoder.")}
    found = {k: sum(s.startswith(p) for s in sites) for k, p in stages.items()}
    print(len(sites), "sites:", found, "| non-finite:", [r["site"] for r in rep.nonfinite()][:3])
    assert all(found.values()), found
    assert len(set(sites)) == len(sites) and not rep.nonfinite()
    first = {k: next(i for i, s in enumerate(sites) if s.startswith(p)) for k, p in stages.items()}
    assert first["CLIP encode"] < first["VAE encode"] < first["denoise loop"] < first["decode"]       # execution order
    # a step's sites were visited once per step, the stages around the loop once
    step = rep.row(next(s for s in sites if s.endswith("/cfg_euler_step#0")))
    assert step["record"]["count"] == 3 * 4 * 4 * 8 * 16
    # the class default and from_pretrained's default are off
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline
    assert StableVideoDiffusionPipeline.range_audit is False and type(pipe).range_audit is False
