"""GPU: export.write_pngs on the ``output_type="device"`` frames of a pipeline built with ``native_image_io=True`` (tiny UNet, stub VAE /
CLIP, as tests/test_gif_export_pipeline_gpu.py): the files 0.png .. F-1.png decode in Pillow to the "pil" output's bytes, and the "pil"
output itself gives the same files."""
import os

import numpy as np
import pytest
import torch

from tests.parity_common import build_pair
from tests.stubs import StubCLIPVision, StubVAE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def outputs():
    """(the "device" output, the "pil" output of the same generator)"""
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

    return call("device"), call("pil")


def test_write_pngs_of_the_device_frames_decodes_to_the_pil_outputs_bytes(outputs, tmp_path):
    from PIL import Image
    from this_and_that_vdm_amd import export
    dev, pil = outputs
    assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (1, 4, 64, 128, 3)
    paths = export.write_pngs(dev, str(tmp_path / "video"))
    assert [os.path.basename(p) for p in paths] == ["0.png", "1.png", "2.png", "3.png"]
    for p, want in zip(paths, pil[0]):
        with Image.open(p) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), np.asarray(want))
    assert export.encode_png(pil) == export.encode_png(dev)
    with pytest.raises(ValueError, match="one video per file"):
        export.write_pngs(torch.cat([dev, dev], 0), str(tmp_path / "two"))
