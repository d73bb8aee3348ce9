"""GPU: a pipeline's ``output_type="device"`` frames (tiny UNet, stub VAE / CLIP of tests/test_pipeline_gpu.py, ``native_image_io=True``)
written by export.write_gif(lzw="device"): the index tensor is coded where the palette map left it, and Pillow decodes the file to the
frame count, the size and ``palette[indices]`` of the returned QuantizedVideo."""
import io

import numpy as np
import pytest
import torch

from tests.parity_common import build_pair
from tests.stubs import StubCLIPVision, StubVAE

pytestmark = pytest.mark.gpu


def test_device_frames_leave_as_a_gif_coded_on_the_device():
    from PIL import Image, ImageSequence
    from this_and_that_vdm_amd import export
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline
    p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    pipe = StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE().cuda().half(), image_encoder=StubCLIPVision().cuda().half(), unet=p_unet,
                                                        native_image_io=True)
    pipe.set_progress_bar_config(disable=True)
    image = torch.rand(1, 3, 64, 128, generator=torch.Generator().manual_seed(11))
    with torch.no_grad():
        dev = pipe(image.cuda(), height=64, width=128, num_frames=4, num_inference_steps=3, output_type="device", decode_chunk_size=3,
                   generator=torch.Generator().manual_seed(2)).frames
    assert torch.is_tensor(dev) and dev.is_cuda and dev.dtype == torch.uint8
    buf = io.BytesIO()
    q = export.write_gif(dev, buf, duration=0.05, lzw="device", segment=3000)          # 8192 pixels a frame: three segments each
    im = Image.open(io.BytesIO(buf.getvalue()))
    decoded = np.stack([np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(im)], 0)
    assert im.n_frames == 4 and im.size == (128, 64)
    which = range(4) if q.palettes.shape[0] == 4 else [0] * 4
    for i in range(4):
        assert np.array_equal(decoded[i], q.palettes[which[i]][q.indices[i]]), i
    host = io.BytesIO()
    export.write_gif(dev, host, duration=0.05)
    assert np.array_equal(np.stack([np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(Image.open(io.BytesIO(host.getvalue())))], 0), decoded)
