"""GPU: the pipelines with ``native_image_io=True`` take the request's pixels to the device once, as uint8, and form the VAE input there
(ops.vae_image): bit-equal to the host path's tensor, for PIL images and for ``DevicePixels``.  Tiny models as in
tests/test_image_io_gpu.py."""
import numpy as np
import PIL.Image
import pytest
import torch

from this_and_that_vdm_amd.svd import pipeline_utils
from this_and_that_vdm_amd.svd.pipeline_utils import DevicePixels

pytestmark = pytest.mark.gpu

DEV = "cuda"
CALL = dict(height=64, width=128, num_frames=4, num_inference_steps=1, output_type="latent")


@pytest.fixture(scope="module")
def pipe():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from tests.parity_common import build_pair
    from tests.stubs import StubCLIPVision, StubVAE
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline
    p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", False)
    p = StableVideoDiffusionPipeline.from_pretrained(None, vae=StubVAE().to(DEV).half(), image_encoder=StubCLIPVision().to(DEV).half(), unet=p_unet)
    p.set_progress_bar_config(disable=True)
    return p


def _image(h=96, w=160, seed=3):
    """larger than height x width = 64 x 128: the request resizes it"""
    return PIL.Image.fromarray(np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8))


def _spy_encode(p, mp):
    seen, encode = [], p.vae.encode

    def spy(x):
        seen.append(x.detach().clone())
        return encode(x)
    mp.setattr(p.vae, "encode", spy)
    return seen


def _forbid_host_preprocess(p, mp):
    def boom(*a, **k):
        raise AssertionError("the host preprocessing was taken")
    mp.setattr(p.image_processor, "preprocess", boom)


@torch.no_grad()
@pytest.mark.parametrize("gen_device, nvid, upcast", [("cpu", 1, False), ("cuda", 2, True), (None, 1, False)],
                         ids=["cpu-generator", "cuda-generator-2-videos-upcast", "no-generator"])
def test_vae_encode_input_is_bit_equal_to_the_host_path(pipe, monkeypatch, gen_device, nvid, upcast):
    p, image = pipe, _image()
    inputs = {}
    p.vae.config.force_upcast = upcast
    try:
        for native in (False, True):
            p.native_image_io = native
            if gen_device is None:
                torch.manual_seed(11)
                gen = None
            else:
                gen = torch.Generator(gen_device).manual_seed(11)
            with monkeypatch.context() as mp:
                seen = _spy_encode(p, mp)
                if native:
                    _forbid_host_preprocess(p, mp)
                p(image, generator=gen, num_videos_per_prompt=nvid, noise_aug_strength=0.02, **CALL)
            inputs[native] = seen[0]
    finally:
        p.native_image_io = False
        p.vae.config.force_upcast = False
    off, on = inputs[False], inputs[True]
    assert on.shape == off.shape == (nvid, 3, 64, 128) and on.dtype == off.dtype == (torch.float32 if upcast else torch.float16)
    assert on.is_cuda and p.vae.dtype == torch.float16
    bits = torch.int32 if upcast else torch.int16
    assert torch.equal(on.cpu().view(bits), off.cpu().view(bits))
    assert float(off.float().std()) > 0.1                                       # an image, not a constant
    if nvid > 1:
        assert not torch.equal(on[0], on[1])                                    # each video of an image has its own noise


@torch.no_grad()
def test_device_pixels_give_the_pil_request(pipe, monkeypatch):
    p, image = pipe, _image()
    p.native_image_io = True
    try:
        a = p(image, generator=torch.Generator().manual_seed(5), **CALL).frames
        with monkeypatch.context() as mp:
            _forbid_host_preprocess(p, mp)
            b = p(DevicePixels.from_pil(image, DEV), generator=torch.Generator().manual_seed(5), **CALL).frames
            c = p(DevicePixels.from_pil([image, image], DEV), generator=[torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)],
                  **CALL).frames
    finally:
        p.native_image_io = False
    assert a.shape == b.shape == (1, 4, 4, 8, 16) and bool(torch.isfinite(a).all()) and float(a.float().std()) > 0.0
    assert torch.equal(a, b)
    assert c.shape == (2, 4, 4, 8, 16) and torch.equal(c[0], c[1])              # two images, one request each


def test_device_pixels_resize_and_flip_equal_pil():
    image = _image(75, 121, 4)
    px = DevicePixels.from_pil(image, DEV)
    assert px.shape == (1, 75, 121, 3) and px.device.type == "cuda"
    got = px.resize((64, 128))                                                  # the default: the reference's callers' resize((w, h))
    assert np.array_equal(got.pixels.cpu().numpy()[0], np.asarray(image.resize((128, 64), resample=PIL.Image.BICUBIC)))
    assert np.array_equal(px.resize((40, 40), "lanczos").pixels.cpu().numpy()[0], np.asarray(image.resize((40, 40), resample=PIL.Image.LANCZOS)))
    assert np.array_equal(px.flip().pixels.cpu().numpy()[0], np.asarray(image.transpose(PIL.Image.FLIP_LEFT_RIGHT)))
    with pytest.raises(ValueError, match="RGB"):
        DevicePixels.from_pil(image.convert("L"), DEV)
    with pytest.raises(ValueError, match="device"):
        DevicePixels(torch.zeros(4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uint8"):
        DevicePixels(torch.zeros(4, 4, 3, device=DEV))


@torch.no_grad()
def test_device_pixels_need_the_option(pipe):
    assert pipe.native_image_io is False
    with pytest.raises(ValueError, match="native_image_io=True"):
        pipe(DevicePixels.from_pil(_image(), DEV), **CALL)


@torch.no_grad()
def test_pixels_are_uploaded_once(pipe, monkeypatch):
    """one host-to-device copy of the image per request, uint8: both readers (the CLIP preprocessing and the VAE input) get that tensor"""
    p, image = pipe, _image()
    uploads, readers = [], []
    upload = pipeline_utils.upload_pixels
    from this_and_that_vdm_amd import ops

    def spy_upload(arr, device):
        uploads.append(upload(arr, device))
        return uploads[-1]

    def spy_reader(name, fn):
        def f(src, *a, **k):
            readers.append((name, src.data_ptr(), src.dtype, tuple(src.shape)))
            return fn(src, *a, **k)
        return f
    monkeypatch.setattr(pipeline_utils, "upload_pixels", spy_upload)
    monkeypatch.setattr(ops, "clip_image", spy_reader("clip", ops.clip_image))
    monkeypatch.setattr(ops, "vae_image", spy_reader("vae", ops.vae_image))
    _forbid_host_preprocess(p, monkeypatch)
    p.native_image_io = True
    try:
        p(image, generator=torch.Generator().manual_seed(5), **CALL)
    finally:
        p.native_image_io = False
    assert len(uploads) == 1 and uploads[0].dtype == torch.uint8 and tuple(uploads[0].shape) == (1, 96, 160, 3)
    assert sorted(r[0] for r in readers) == ["clip", "vae"]
    assert all(r[1:] == (uploads[0].data_ptr(), torch.uint8, (1, 96, 160, 3)) for r in readers)


@torch.no_grad()
def test_uint8_arrays_give_the_pil_request(pipe, monkeypatch):
    """a list of uint8 [H, W, 3] arrays is the same request as the PIL images made of them (one upload, no host preprocessing)"""
    p, images = pipe, [_image(seed=3), _image(seed=4)]
    gens = lambda: [torch.Generator().manual_seed(5), torch.Generator().manual_seed(6)]
    p.native_image_io = True
    try:
        a = p(images, generator=gens(), **CALL).frames
        with monkeypatch.context() as mp:
            _forbid_host_preprocess(p, mp)
            b = p([np.asarray(im) for im in images], generator=gens(), **CALL).frames
    finally:
        p.native_image_io = False
    assert a.shape == (2, 4, 4, 8, 16) and bool(torch.isfinite(a).all()) and not torch.equal(a[0], a[1])
    assert torch.equal(a, b)
    # float arrays are no pixels: they keep today's path, which has no preprocessing for a list of arrays
    p.native_image_io = True
    try:
        with pytest.raises(ValueError, match="unsupported image type"):
            p([np.asarray(im).astype(np.float32) for im in images], generator=gens(), **CALL)
    finally:
        p.native_image_io = False


@torch.no_grad()
def test_controlnet_pipeline_takes_device_pixels(monkeypatch):
    """the VGL pipeline: DevicePixels give the PIL request's latents, and raise with the option off"""
    from tests.parity_common import build_pair
    from tests.stubs import StubCLIPVision, StubVAE
    from this_and_that_vdm_amd.svd import StableVideoDiffusionControlNetPipeline
    p_unet, p_cn, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    p = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=StubVAE().to(DEV).half(), image_encoder=StubCLIPVision().to(DEV).half(),
                                                               unet=p_unet, native_image_io=True)
    p.set_progress_bar_config(disable=True)
    image = _image()
    cond = torch.rand(4, 3, 64, 128, generator=torch.Generator().manual_seed(2)).numpy()
    call = dict(condition_img=cond, controlnet=p_cn, guess_mode=False, **CALL)
    a = p(image, generator=torch.Generator().manual_seed(5), **call).frames
    with monkeypatch.context() as mp:
        _forbid_host_preprocess(p, mp)
        b = p(DevicePixels.from_pil(image, DEV), generator=torch.Generator().manual_seed(5), **call).frames
    assert a.shape == (1, 4, 4, 8, 16) and bool(torch.isfinite(a).all()) and float(a.float().std()) > 0.0
    assert torch.equal(a, b)
    p.native_image_io = False
    with pytest.raises(ValueError, match="native_image_io=True"):
        p(DevicePixels.from_pil(image, DEV), **call)
