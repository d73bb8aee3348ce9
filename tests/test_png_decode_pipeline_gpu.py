"""GPU: the PNG import on the paths it is for (tiny UNet, stub VAE / CLIP, as tests/test_gif_decode_pipeline_gpu.py).
``DevicePixels.from_png`` hands a pipeline the tensors ``DevicePixels.from_pil(Image.open(path).convert("RGB"))`` hands it, bit for bit, for
every mode; the ``"device"`` frames of a pipeline call written by ``export.write_pngs`` and read by ``ingest.read_pngs`` are the same
frames, and ``metrics.compare_frames`` of the two reports identity."""
import numpy as np
import pytest
import torch

from tests import png_decode_reference as g
from this_and_that_vdm_amd.ingest import read_pngs          # the feature under test: without it nothing here is collected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def pipe():
    from tests.parity_common import build_pair
    from tests.stubs import StubCLIPVision, StubVAE
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline
    p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, DEV, False)
    p = StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE().to(DEV).half(), image_encoder=StubCLIPVision().to(DEV).half(), unet=p_unet, native_image_io=True)
    p.set_progress_bar_config(disable=True)
    return p


@torch.no_grad()
def test_from_png_hands_a_pipeline_what_from_pil_hands_it(pipe, tmp_path):
    from PIL import Image
    from this_and_that_vdm_amd.svd.pipeline_utils import DevicePixels
    for ch, mode in ((1, "L"), (2, "LA"), (3, "RGB"), (4, "RGBA")):
        path = str(tmp_path / f"request-{mode}.png")
        open(path, "wb").write(g.pillow_png(g.picture(64, 128, ch, ch)))
        assert Image.open(path).mode == mode
        mine, theirs = DevicePixels.from_png(path, DEV), DevicePixels.from_pil(Image.open(path).convert("RGB"), DEV)
        assert tuple(mine.shape) == (1, 64, 128, 3) and torch.equal(mine.pixels, theirs.pixels), mode
    call = dict(height=64, width=128, num_frames=4, num_inference_steps=1, output_type="latent")
    a = pipe(theirs, generator=torch.Generator().manual_seed(5), **call).frames
    b = pipe(mine, generator=torch.Generator().manual_seed(5), **call).frames
    c = pipe(Image.open(path).convert("RGB"), generator=torch.Generator().manual_seed(5), **call).frames
    assert bool(torch.isfinite(a).all()) and float(a.float().std()) > 0.0 and torch.equal(a, b) and torch.equal(a, c)


@torch.no_grad()
def test_the_device_output_written_as_pngs_reads_back_as_the_same_frames(pipe, tmp_path):
    from this_and_that_vdm_amd import export, metrics
    image = torch.rand(1, 3, 64, 128, generator=torch.Generator().manual_seed(11))
    dev = pipe(image.to(DEV), height=64, width=128, num_frames=4, num_inference_steps=2, output_type="device", generator=torch.Generator().manual_seed(2)).frames
    assert dev.is_cuda and tuple(dev.shape) == (1, 4, 64, 128, 3)
    paths = export.write_pngs(dev, str(tmp_path))
    assert len(paths) == 4
    back = read_pngs(str(tmp_path), device=DEV)
    assert back.is_cuda and tuple(back.shape) == (4, 64, 128, 3) and torch.equal(back, dev[0])
    assert np.array_equal(back.cpu().numpy()[3], g.pillow_pixels(open(paths[3], "rb").read()))
    m = metrics.compare_frames(back, dev[0])
    assert (m.frame_mse == 0.0).all() and (m.frame_ssim == 1.0).all()
