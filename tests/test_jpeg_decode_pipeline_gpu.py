"""GPU: the JPEG import on the paths it is for.  A folder ``export.write_jpegs`` wrote read back by ``ingest.read_jpegs`` -- Pillow's decode
of the same files, byte for byte --; ``metrics.compare_frames`` on it; ``ingest.read_mjpeg_video`` of a ``write_mjpeg`` file; and a
pipeline built with ``native_image_io=True`` (tiny UNet, stub VAE / CLIP, as tests/test_vae_image_pipeline_gpu.py) taking
``image=DevicePixels.from_jpeg(path, device)``: the latents of ``image=Image.open(path)``, bit for bit."""
import os

import numpy as np
import pytest
import torch

from tests import jpeg_reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pillow_pixels(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im)


def _same_metrics(a, b):
    """two VideoMetrics, field by field, bit for bit"""
    import dataclasses
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if not (np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) if x is not None and y is not None else x is y):
            return False
    return True


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """(frames uint8 [4, 40, 72, 3] on the device, the folder write_jpegs wrote them to, its paths)"""
    from this_and_that_vdm_amd import export
    frames = np.stack([ref.smooth_frame(40, 72, s) for s in range(3)] + [ref.noise_frame(40, 72, 9)], 0)
    folder = str(tmp_path_factory.mktemp("clip") / "video")
    dev = torch.from_numpy(frames).to(DEV)
    return dev, folder, export.write_jpegs(dev, folder, quality=90)


def test_read_jpegs_of_a_written_folder_equals_pillows_decode(clip):
    from this_and_that_vdm_amd import ingest
    _, folder, paths = clip
    got = ingest.read_jpegs(folder, device=DEV)
    want = np.stack([_pillow_pixels(p) for p in paths])
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (4, 40, 72, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    os.rename(paths[2], paths[2] + ".away")                                  # the first missing index ends the clip
    try:
        assert tuple(ingest.read_jpegs(folder, device=DEV).shape) == (2, 40, 72, 3)
    finally:
        os.rename(paths[2] + ".away", paths[2])


def test_compare_frames_takes_the_decoded_clip(clip):
    from this_and_that_vdm_amd import ingest, metrics
    frames, folder, paths = clip
    got = metrics.compare_frames(ingest.read_jpegs(folder, device=DEV), frames)
    want = metrics.compare_frames(torch.from_numpy(np.stack([_pillow_pixels(p) for p in paths])).to(DEV), frames)
    assert _same_metrics(got, want) and float(np.min(got.frame_mse)) > 0.0                  # JPEG is lossy: the clip differs from its source
    assert _same_metrics(metrics.compare_frames(ingest.read_jpegs(folder, device=DEV), ingest.decode_jpeg(paths, DEV)), metrics.compare_frames(frames, frames))


def test_read_mjpeg_video_gives_the_frames_of_the_file(clip, tmp_path):
    import io
    from PIL import Image
    from this_and_that_vdm_amd import export, ingest
    frames, _, _ = clip
    path = str(tmp_path / "clip.avi")
    export.write_mjpeg(frames, path, fps=4, quality=80, huffman="optimized")
    want = np.stack([np.asarray(Image.open(io.BytesIO(d))) for d in export.read_mjpeg_frames(path)])
    assert np.array_equal(ingest.read_mjpeg_video(path, DEV).cpu().numpy(), want)


@torch.no_grad()
def test_a_request_takes_its_image_from_a_jpeg_file(tmp_path, monkeypatch):
    from PIL import Image
    from tests.parity_common import build_pair
    from tests.stubs import StubCLIPVision, StubVAE
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline
    from this_and_that_vdm_amd.svd.pipeline_utils import DevicePixels
    p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", False)
    pipe = StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE().to(DEV).half(), image_encoder=StubCLIPVision().to(DEV).half(), unet=p_unet,
                                                        native_image_io=True)
    pipe.set_progress_bar_config(disable=True)
    path = str(tmp_path / "im_0.jpg")
    Image.fromarray(np.random.default_rng(3).integers(0, 256, (96, 160, 3), dtype=np.uint8)).save(path, quality=92)        # 4:2:0, larger than the request
    call = dict(height=64, width=128, num_frames=4, num_inference_steps=1, output_type="latent")
    a = pipe(Image.open(path), generator=torch.Generator().manual_seed(5), **call).frames
    pixels = DevicePixels.from_jpeg(path, DEV)
    assert tuple(pixels.shape) == (1, 96, 160, 3) and np.array_equal(pixels.pixels.cpu().numpy()[0], _pillow_pixels(path))

    def boom(*args, **kwargs):
        raise AssertionError("the host preprocessing was taken")
    monkeypatch.setattr(pipe.image_processor, "preprocess", boom)
    b = pipe(pixels, generator=torch.Generator().manual_seed(5), **call).frames
    assert a.shape == b.shape and bool(torch.isfinite(a).all()) and float(a.float().std()) > 0.0
    assert torch.equal(a, b)


def test_from_jpeg_of_a_grey_file_holds_pillows_rgb_conversion(tmp_path):
    from PIL import Image
    from this_and_that_vdm_amd.svd.pipeline_utils import DevicePixels
    path = str(tmp_path / "grey.jpg")
    Image.fromarray(ref.smooth_frame(37, 53, 2, 1)[..., 0]).save(path, quality=85)
    with Image.open(path) as im:
        assert im.mode == "L"
        want = np.asarray(im.convert("RGB"))
    pixels = DevicePixels.from_jpeg([path, path], DEV)
    assert tuple(pixels.shape) == (2, 37, 53, 3) and pixels.pixels.is_contiguous()
    assert np.array_equal(pixels.pixels.cpu().numpy()[0], want) and np.array_equal(pixels.pixels.cpu().numpy()[1], want)
