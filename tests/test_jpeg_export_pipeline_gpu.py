"""GPU: export.write_jpegs on the ``output_type="device"`` frames of a pipeline built with ``native_image_io=True`` (tiny UNet, stub VAE /
CLIP, as tests/test_png_export_pipeline_gpu.py): the files im_0.jpg .. im_{F-1}.jpg equal ``encode_jpeg`` of the "np" output's bytes, and
decode in Pillow."""
import os

import numpy as np
import pytest
import torch

from tests.parity_common import build_pair
from tests.stubs import StubCLIPVision, StubVAE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def outputs():
    """(the "device" output, the "np" output of the same generator)"""
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline
    p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    pipe = StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE().cuda().half(), image_encoder=StubCLIPVision().cuda().half(), unet=p_unet,
                                                        native_image_io=True)
    pipe.set_progress_bar_config(disable=True)
    image = torch.rand(1, 3, 64, 128, generator=torch.Generator().manual_seed(11))

    @torch.no_grad()
    def call(output_type):
        out = pipe(image.cuda(), height=64, width=128, num_frames=4, num_inference_steps=3, output_type=output_type,
                   decode_chunk_size=3, generator=torch.Generator().manual_seed(2)).frames
        return out.clone() if torch.is_tensor(out) else out

    return call("device"), call("np")


def test_write_jpegs_of_the_device_frames_equals_encode_jpeg_of_the_np_output(outputs, tmp_path):
    from PIL import Image
    from this_and_that_vdm_amd import export
    dev, arr = outputs
    assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (1, 4, 64, 128, 3)
    paths = export.write_jpegs(dev, str(tmp_path / "video"))
    assert [os.path.basename(p) for p in paths] == ["im_0.jpg", "im_1.jpg", "im_2.jpg", "im_3.jpg"]
    want = export.encode_jpeg(arr)
    for p, data in zip(paths, want):
        with open(p, "rb") as fh:
            assert fh.read() == data
        with Image.open(p) as im:
            im.load()
            assert im.mode == "RGB" and im.size == (128, 64) and im.format == "JPEG"
            assert np.asarray(im).shape == (64, 128, 3)
    with pytest.raises(ValueError, match="one video per file"):
        export.write_jpegs(torch.cat([dev, dev], 0), str(tmp_path / "two"))
