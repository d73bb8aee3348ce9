"""GPU: ``output_type="device"`` of a pipeline built with ``native_image_io=True`` (tiny UNet, stub VAE / CLIP of
tests/test_pipeline_gpu.py): the uint8 frames stay on the device and are the "pil" output's bytes; export.write_gif writes them to a file
that Pillow decodes to the quantised frames; metrics.compare_frames takes the same tensor; without ``native_image_io`` the value raises."""
import io

import numpy as np
import pytest
import torch

from tests.parity_common import build_pair
from tests.stubs import StubCLIPVision, StubVAE

pytestmark = pytest.mark.gpu
CHUNK = 3                     # 4 frames in chunks of 3 + 1: the device output is a concatenation


@pytest.fixture(scope="module")
def outputs():
    """(pipe, the "device" output, the "pil" output and the "latent" output of the same generator)"""
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline
    p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    pipe = StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE().cuda().half(), image_encoder=StubCLIPVision().cuda().half(), unet=p_unet,
                                                        native_image_io=True)
    pipe.set_progress_bar_config(disable=True)
    image = torch.rand(1, 3, 64, 128, generator=torch.Generator().manual_seed(11))

    @torch.no_grad()
    def call(output_type):
        out = pipe(image.cuda(), height=64, width=128, num_frames=4, num_inference_steps=3, output_type=output_type,
                   decode_chunk_size=CHUNK, generator=torch.Generator().manual_seed(2)).frames
        return out.clone() if torch.is_tensor(out) else out

    return pipe, call, call("device"), call("pil"), call("latent")


def test_device_frames_are_the_pil_outputs_bytes(outputs):
    pipe, _, dev, pil, latent = outputs
    assert pipe.native_image_io is True
    assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (1, 4, 64, 128, 3)
    assert np.array_equal(dev.cpu().numpy()[0], np.stack([np.asarray(im) for im in pil[0]], 0))
    assert len(np.unique(dev.cpu().numpy())) > 16                           # a picture, not a constant
    assert torch.is_tensor(latent) and tuple(latent.shape) == (1, 4, 4, 8, 16)           # the other values behave as before


def test_write_gif_and_compare_frames_take_the_device_frames(outputs):
    from PIL import Image, ImageSequence
    from this_and_that_vdm_amd import export, metrics
    _, _, dev, pil, _ = outputs
    buf = io.BytesIO()
    q = export.write_gif(dev, buf, duration=0.05)
    im = Image.open(io.BytesIO(buf.getvalue()))
    decoded = np.stack([np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(im)], 0)
    assert im.n_frames == 4 and im.size == (128, 64) and np.array_equal(decoded, q.frames())
    again = io.BytesIO()
    export.write_gif(pil, again, duration=0.05)                              # the "pil" output of the same request: the same file
    assert again.getvalue() == buf.getvalue()
    m = metrics.compare_frames(dev, torch.from_numpy(q.frames()[None]).cuda())
    assert m.frame_psnr.shape == (1, 4) and np.allclose(m.frame_psnr[0], q.frame_psnr, rtol=1e-12, atol=0) and (m.frame_ssim <= 1.0).all()
    same = metrics.compare_frames(dev, pil)
    assert (same.frame_mse == 0.0).all() and (same.frame_ssim == 1.0).all()


def test_device_output_needs_native_image_io(outputs):
    pipe, call, _, _, _ = outputs
    pipe.native_image_io = False
    try:
        with pytest.raises(ValueError, match="native_image_io=True"):
            call("device")
    finally:
        pipe.native_image_io = True
