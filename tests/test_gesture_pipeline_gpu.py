"""GPU: `condition_img=GesturePoints(...)` through the VGL pipeline (tiny pair, stub VAE / CLIP as in tests/test_pipeline_gpu.py): the
frames are rasterised on the device straight to fp16 and the rest of the call is what it is for an array; get_thisthat_sam(device=).

What is bitwise and what is not: the rasterised maps of a request are bit for bit the same in a joint call and in a call of its own, and
a call given the points equals, bit for bit, the same call given the rasterised frames as an array.  The LATENTS of a request in a joint
call are not bitwise those of a single call on this project, for arrays either: the joint launches take other GEMM routes
(tests/test_multi_request_pipeline_gpu.py).  They are held to that file's limits, in its set-up (fp32 stub encoders, 4 steps)."""
import numpy as np
import pytest
import torch

from tests import gesture_cases as gc
from tests.parity_common import build_pair, err_stats
from tests.stubs import StubCLIPVision, StubVAE
from this_and_that_vdm_amd import gesture_map as gm

pytestmark = pytest.mark.gpu
H, W, F = 64, 128, 4
ORG = (48, 72)
GP_A = gm.GesturePoints(((0, 30, 20), (3, 50, 33)), ORG)
GP_B = gm.GesturePoints(((1, 10.7, 30), (-1, 60, 5.2)), ORG)


@pytest.fixture(scope="module")
def pipe_cn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd.svd import EulerDiscreteScheduler, StableVideoDiffusionControlNetPipeline
    p_unet, p_cn, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    vae, clip = StubVAE().cuda(), StubCLIPVision().cuda()      # fp32: bit-identical per image at any batch size
    pipe = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=vae, image_encoder=clip, unet=p_unet,
                                                                  scheduler=EulerDiscreteScheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe, p_cn


def _images(n):
    return torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(11)).cuda()


def _call(pipe, cn, image, cond, seed=3):
    gen = [torch.Generator().manual_seed(s) for s in seed] if isinstance(seed, (list, tuple)) else torch.Generator().manual_seed(seed)
    return pipe(image, cond, cn, height=H, width=W, num_frames=F, num_inference_steps=4, fps=7, motion_bucket_id=200,
                noise_aug_strength=0.05, output_type="latent", guess_mode=False, generator=gen).frames


def _spy(pipe, monkeypatch):
    seen = []
    inner = pipe._encode_gesture_maps
    monkeypatch.setattr(pipe, "_encode_gesture_maps", lambda cond, n: seen.append(cond) or inner(cond, n))
    return seen


def _within_fp16_of_host(cond: torch.Tensor, gp):
    host, _, _ = gm.rasterise_points(gp.points, gp.org_hw, H, W, F, dilate=gp.dilate, flip=gp.flip)
    bound = gc.BOUND32 + 0.5 * gc.ulp(host, *gc.FORMATS["float16"])
    err = np.abs(cond.float().cpu().numpy().astype(np.float64) - host.astype(np.float64))
    assert (err <= bound).all(), float(err.max())


@torch.no_grad()
def test_single_gesture_points(pipe_cn, monkeypatch):
    pipe, cn = pipe_cn
    seen = _spy(pipe, monkeypatch)
    monkeypatch.setattr(gm, "rasterise_points", None)          # the host rasteriser must not be needed by the call
    lat = _call(pipe, cn, _images(1), GP_A)
    monkeypatch.undo()
    assert lat.shape == (1, F, 4, H // 8, W // 8) and torch.isfinite(lat).all()
    cond, = seen
    assert cond.is_cuda and cond.dtype == torch.float16 and cond.shape == (F, 3, H, W)
    _within_fp16_of_host(cond, GP_A)
    # what prepare_condition_image makes of the host rasteriser's frames differs from it by the same bound
    want = pipe.prepare_condition_image(gm.rasterise_points(GP_A.points, ORG, H, W, F)[0], "cuda")
    assert (cond.float() - want.float()).abs().max() <= 2.0 ** -11 + gc.BOUND32
    # the same frames as a plain array: the new path adds nothing but the rasterisation
    again = _call(pipe, cn, _images(1), cond.cpu().numpy())
    assert torch.equal(again, lat)


@torch.no_grad()
def test_list_of_gesture_points(pipe_cn, monkeypatch):
    pipe, cn = pipe_cn
    seen = _spy(pipe, monkeypatch)
    images = _images(2)
    both = _call(pipe, cn, images, [GP_A, GP_B], seed=[5, 6])
    assert both.shape == (2, F, 4, H // 8, W // 8) and torch.isfinite(both).all()
    cond, = seen
    assert cond.is_cuda and cond.dtype == torch.float16 and cond.shape == (2, F, 3, H, W)
    for i, gp in enumerate((GP_A, GP_B)):
        _within_fp16_of_host(cond[i], gp)
        seen.clear()
        own = _call(pipe, cn, images[i:i + 1], gp, seed=5 + i)
        assert torch.equal(seen[0], cond[i]), f"request {i}: its map in the joint call is not bitwise its map in a call of its own"
        st = err_stats(both[i:i + 1], own)
        print(f"request {i} of the joint call vs a call of its own:", st)
        assert st["rel_l2"] <= 3e-3 and st["cos"] >= 0.99999, (i, st)
    # the joint call given the rasterised frames as arrays: bitwise the same latents
    again = _call(pipe, cn, images, [c.cpu().numpy() for c in cond], seed=[5, 6])
    assert torch.equal(again, both)
    with pytest.raises(ValueError, match=r"condition_img \(3, 4, 3, 64, 128\).*\[2,F,3,H,W\]"):
        _call(pipe, cn, images, [GP_A, GP_B, GP_A], seed=[5, 6])


def test_get_thisthat_sam_on_the_device(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import PIL.Image
    PIL.Image.new("RGB", (ORG[1], ORG[0])).save(tmp_path / "im_0.jpg")
    (tmp_path / "data.txt").write_text("0 30.9 20.1\n3 50 33\n")
    cfg = dict(video_seq_length=F, conditioning_channels=3, height=32, width=40, dilate=True, motion_bucket_id=127)
    h_cond, h_bucket, h_frames, h_coords = gm.get_thisthat_sam(cfg, str(tmp_path), flip=True)
    d_cond, d_bucket, d_frames, d_coords = gm.get_thisthat_sam(cfg, str(tmp_path), flip=True, device="cuda")
    assert isinstance(d_cond, torch.Tensor) and d_cond.is_cuda and d_cond.dtype == torch.float32 and d_cond.shape == h_cond.shape
    assert (d_bucket, d_frames, d_coords) == (h_bucket, h_frames, h_coords) == (127, [0, 3], [(20, 30), (33, 50)])
    assert np.abs(d_cond.cpu().numpy().astype(np.float64) - h_cond).max() <= gc.BOUND32
