"""GPU: the GIF import on the paths it is for.  ``ingest.read_gif`` of what ``export.write_gif`` wrote -- host and device LZW, frame and
global palettes -- equals the quantised frames exactly; a Pillow-written animated file with cropped difference rectangles equals
Pillow's frames; ``metrics.compare_frames`` takes two decoded files; ``DevicePixels.from_gif`` hands a pipeline (tiny UNet, stub VAE /
CLIP, as tests/test_jpeg_decode_pipeline_gpu.py) the tensor of the Pillow frame; and the ``"device"`` output of a tiny pipeline call,
written as a GIF, reads back to the quantised frames."""
import io

import numpy as np
import pytest
import torch

from tests import gif_decode_reference as g
from this_and_that_vdm_amd.ingest import decode_gif, read_gif          # the feature under test: without it nothing here is collected

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def video(f, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // (w - 1)), (yy * 255 // (h - 1)), ((xx + yy) * 127 // (w + h - 2))], axis=-1).astype(np.uint8)
    out = np.repeat(base[None], f, axis=0)
    for i in range(f):
        out[i, 2 * i:2 * i + 6, 3 * i:3 * i + 7] = rng.integers(0, 256, size=(6, 7, 3))
    return out


def quantised(q):
    which = np.arange(q.indices.shape[0]) if q.palettes.shape[0] == q.indices.shape[0] else np.zeros(q.indices.shape[0], dtype=int)
    return np.stack([q.palettes[which[i]][q.indices[i]] for i in range(q.indices.shape[0])])


@pytest.mark.parametrize("palette", ["frame", "global"])
@pytest.mark.parametrize("lzw", ["host", "device"])
def test_read_gif_of_write_gif_equals_the_quantised_frames(lzw, palette, tmp_path):
    from this_and_that_vdm_amd import export, ingest
    frames = torch.from_numpy(video(4, 24, 40, 1)).to(DEV)
    path = str(tmp_path / "combined.gif")
    q = export.write_gif(frames, path, lzw=lzw, palette=palette)
    got, hd = ingest.decode_gif(path, DEV, info=True)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (4, 24, 40, 3) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), quantised(q)) and np.array_equal(quantised(q), q.frames())
    assert hd.frames == 4 and hd.loop == 0 and hd.durations == [0.05] * 4 and hd.local == [palette == "frame"] * 4
    assert np.array_equal(ingest.read_gif(path, DEV).cpu().numpy(), g.pillow_frames(open(path, "rb").read()))


def pillow_animation():
    """five palette frames that differ in a small block: Pillow writes frames 1 .. 4 as cropped difference rectangles"""
    from PIL import Image
    rng = np.random.default_rng(2)
    yy, xx = np.mgrid[0:60, 0:90]
    palette = rng.integers(0, 256, size=(256, 3)).astype(np.uint8)
    ims = []
    for i in range(5):
        idx = ((xx + 2 * yy) % 200).astype(np.uint8)
        idx[4 * i:4 * i + 9, 7 * i:7 * i + 11] = rng.integers(200, 256, size=(9, 11))
        ims.append(Image.fromarray(idx, "P"))
        ims[-1].putpalette(palette.tobytes())
    buf = io.BytesIO()
    ims[0].save(buf, format="GIF", save_all=True, append_images=ims[1:], duration=80, loop=3)
    return buf.getvalue()


def test_a_pillow_file_with_cropped_difference_rectangles_equals_pillows_frames():
    from this_and_that_vdm_amd import ingest
    data = pillow_animation()
    got, hd = ingest.decode_gif(data, DEV, info=True)
    assert any(tuple(r[2:]) != (90, 60) for r in hd.rectangles.tolist()), "Pillow no longer crops the difference rectangles of this video"
    assert hd.loop == 3 and hd.durations == [0.08] * 5
    assert np.array_equal(got.cpu().numpy(), g.pillow_frames(data))


def test_compare_frames_of_a_file_with_itself_reports_zero_error(tmp_path):
    from this_and_that_vdm_amd import ingest, metrics
    path = tmp_path / "a.gif"
    path.write_bytes(pillow_animation())
    m = metrics.compare_frames(ingest.read_gif(str(path), DEV), ingest.read_gif(str(path), DEV))
    assert (m.frame_mse == 0.0).all() and (m.frame_ssim == 1.0).all()


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
def test_from_gif_hands_a_pipeline_the_pillow_frame(pipe, tmp_path):
    from PIL import Image
    from this_and_that_vdm_amd.svd.pipeline_utils import DevicePixels
    path = str(tmp_path / "request.gif")
    open(path, "wb").write(pillow_animation())
    with Image.open(path) as im:
        im.seek(2)
        third = im.convert("RGB")
    pixels = DevicePixels.from_gif(path, DEV, frame=2)
    assert tuple(pixels.shape) == (1, 60, 90, 3) and np.array_equal(pixels.pixels.cpu().numpy()[0], np.asarray(third))
    assert tuple(DevicePixels.from_gif(path, DEV, frame=None).shape) == (5, 60, 90, 3) and tuple(DevicePixels.from_gif(path, DEV).shape) == (1, 60, 90, 3)
    with pytest.raises(ValueError, match="frame 5 of a file with 5 frames"):
        DevicePixels.from_gif(path, DEV, frame=5)
    call = dict(height=64, width=128, num_frames=4, num_inference_steps=1, output_type="latent")
    a = pipe(third, generator=torch.Generator().manual_seed(5), **call).frames
    b = pipe(pixels, generator=torch.Generator().manual_seed(5), **call).frames
    assert bool(torch.isfinite(a).all()) and float(a.float().std()) > 0.0 and torch.equal(a, b)


@torch.no_grad()
def test_the_device_output_written_as_a_gif_reads_back_to_the_quantised_frames(pipe, tmp_path):
    from this_and_that_vdm_amd import export, ingest
    image = torch.rand(1, 3, 64, 128, generator=torch.Generator().manual_seed(11))
    dev = pipe(image.to(DEV), height=64, width=128, num_frames=4, num_inference_steps=2, output_type="device", generator=torch.Generator().manual_seed(2)).frames
    assert dev.is_cuda and tuple(dev.shape) == (1, 4, 64, 128, 3)
    path = str(tmp_path / "combined.gif")
    q = export.write_gif(dev, path, lzw="device")
    back = ingest.read_gif(path, DEV)
    assert np.array_equal(back.cpu().numpy(), quantised(q)) and tuple(back.shape) == (4, 64, 128, 3)
