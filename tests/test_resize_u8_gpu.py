"""GPU: ops.resize_u8 against PIL.Image.resize and ops.vae_image against the host statement of the VAE input
(VaeImageProcessor.preprocess, repeat_interleave, + noise_aug_strength * noise, .to(dtype)).  Every comparison is bit equality: the
resampler is integer arithmetic on fp64 tables (tests/resize_u8_reference.py restates it), and the epilogue rounds each fp32 operation
on its own, as torch does."""
import ctypes as C

import numpy as np
import PIL.Image
import pytest
import torch

from tests import resize_u8_reference as R
from this_and_that_vdm_amd.svd.pipeline_utils import VaeImageProcessor

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = sorted(R.FILTERS)
# the CPU test's shapes, and an odd output width: 3 * 41 bytes per row is no multiple of 4, so the vertical pass takes its byte-wise
# form and the last dword of the output is partial
SHAPES = R.SHAPES + [((37, 53), (24, 41))]
IDS = [f"{a}x{b}to{c}x{d}" for (a, b), (c, d) in SHAPES]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops
    return ops


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("src_hw, dst_hw", SHAPES, ids=IDS)
def test_resize_u8_equals_pil(ops, src_hw, dst_hw, name):
    imgs = np.stack([R.sample_image(*src_hw, seed) for seed in (0, 1)])
    want = np.stack([R.pil_resize(im, dst_hw, name) for im in imgs])
    one = ops.resize_u8(torch.from_numpy(imgs[0]).to(DEV), dst_hw, name)                      # [H, W, 3]: N = 1
    two = ops.resize_u8(torch.from_numpy(imgs).to(DEV), dst_hw, R.FILTERS[name][0])           # N = 2, the filter by PIL's code
    assert one.dtype == two.dtype == torch.uint8 and one.shape == (1, *dst_hw, 3) and two.shape == (2, *dst_hw, 3)
    assert np.array_equal(one.cpu().numpy()[0], want[0])
    assert np.array_equal(two.cpu().numpy(), want)
    if (src_hw, dst_hw) in R.CLAMP_SHAPES:
        assert want[0].min() == 0 and want[0].max() == 255


@pytest.mark.parametrize("n_in, n_out, first, pixels, o, pil_byte", R.HAMMING_ROWS)
def test_resize_u8_hamming_uses_pillows_fp32_constants(ops, n_in, n_out, first, pixels, o, pil_byte):
    """rows on which HAMMING tables built from the doubles 0.54 / 0.46 instead of Pillow's 0.54f / 0.46f give another byte"""
    row = R.hamming_row(n_in, first, pixels)
    want = R.pil_resize(row, (1, n_out), "hamming")
    assert want[0, o, 0] == pil_byte
    assert np.array_equal(ops.resize_u8(torch.from_numpy(row).to(DEV), (1, n_out), "hamming").cpu().numpy()[0], want)


def test_device_table_cache_is_bounded(ops, monkeypatch):
    """the least recently used tables leave; a call's own two tables survive its own insertions"""
    monkeypatch.setattr(ops, "RESAMPLE_TABLES_MAX", 2)
    img = R.sample_image(37, 53)
    src = torch.from_numpy(img).to(DEV)
    for dst_hw in ((24, 40), (20, 31), (24, 40)):
        assert np.array_equal(ops.resize_u8(src, dst_hw, "bilinear").cpu().numpy()[0], R.pil_resize(img, dst_hw, "bilinear"))
        assert len(ops._RESAMPLE_TABLES) == 2
        assert {k[:2] for k in ops._RESAMPLE_TABLES} == {(53, dst_hw[1]), (37, dst_hw[0])}


def test_device_tables_are_cached(ops):
    src = torch.from_numpy(R.sample_image(37, 53)).to(DEV)
    ops.resize_u8(src, (24, 40), "hamming")
    keys = [k for k in ops._RESAMPLE_TABLES if k[2] == R.FILTERS["hamming"][0] and k[:2] in ((53, 40), (37, 24))]
    assert len(keys) == 2
    ptrs = {k: ops._RESAMPLE_TABLES[k][0].data_ptr() for k in keys}
    ops.resize_u8(src, (24, 40), "hamming")
    assert {k: ops._RESAMPLE_TABLES[k][0].data_ptr() for k in keys} == ptrs
    tab, ksize = ops._RESAMPLE_TABLES[keys[0]]
    rk, rb, rkk = R.coeffs(keys[0][0], keys[0][1], "hamming")
    assert ksize == rk and np.array_equal(tab.cpu().numpy(), np.concatenate([rb.T, rkk.T], 0))          # the tap-major device layout


def host_vae_input(imgs, dst_hw, noise, na, dtype, nvid):
    """the pipeline's host statement (svd/pipeline_stable_video_diffusion_controlnet.py, _generate) on the same noise tensor"""
    t = VaeImageProcessor(do_convert_rgb=True).preprocess([PIL.Image.fromarray(im) for im in imgs], height=dst_hw[0], width=dst_hw[1])
    if nvid > 1:
        t = t.repeat_interleave(nvid, 0)
    if noise is not None:
        t = t + na * noise
    return t.to(dtype)


# both passes; neither; horizontal only; vertical only; an odd width (element-wise stores, byte-wise vertical pass); up-scaling
VAE_SHAPES = [((48, 64), (32, 56)), ((24, 40), (24, 40)), ((40, 33), (40, 16)), ((33, 40), (16, 40)), ((37, 53), (24, 41)),
              ((16, 24), (32, 56)), ((23, 41), (23, 41))]
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


@pytest.mark.parametrize("dtype", list(BITS), ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("nvid", [1, 2])
@pytest.mark.parametrize("src_hw, dst_hw", VAE_SHAPES, ids=[f"{a}x{b}to{c}x{d}" for (a, b), (c, d) in VAE_SHAPES])
def test_vae_image_equals_the_host_statement(ops, src_hw, dst_hw, nvid, dtype):
    imgs = np.stack([R.sample_image(*src_hw, seed) for seed in (2, 3)])
    na = 0.02
    noise = torch.randn(2 * nvid, 3, *dst_hw, generator=torch.Generator().manual_seed(src_hw[0] * 7 + nvid))
    src = torch.from_numpy(imgs).to(DEV)
    for nz in (noise, None):
        want = host_vae_input(imgs, dst_hw, nz, na, dtype, nvid)
        got = ops.vae_image(src, dst_hw, None if nz is None else nz.to(DEV), na, dtype, videos_per_image=nvid)
        assert got.dtype == dtype and got.shape == want.shape == (2 * nvid, 3, *dst_hw) and got.is_contiguous()
        assert torch.equal(got.cpu().view(BITS[dtype]), want.view(BITS[dtype])), f"noise {'given' if nz is not None else 'None'}"


def test_vae_image_filter_and_strength(ops):
    """another filter than the default, a strength that is no fp32 number's double (the kernel takes float(na), as torch's scalar
    multiplication does), and noise large enough to leave [-1, 1]"""
    imgs = R.sample_image(37, 53, 5)[None]
    noise = torch.randn(1, 3, 24, 40, generator=torch.Generator().manual_seed(9)) * 40.0
    got = ops.vae_image(torch.from_numpy(imgs).to(DEV), (24, 40), noise.to(DEV), 0.1, torch.float32, resample="bicubic")
    t = torch.from_numpy(R.pil_resize(imgs[0], (24, 40), "bicubic").astype(np.float32) / 255.0).permute(2, 0, 1)[None]
    want = (2.0 * t - 1.0) + 0.1 * noise
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


def test_foreign_table_is_clamped_to_the_image(ops):
    """a table the library did not build -- first index below 0 and past the end, more taps than the source or the table holds -- reads
    only the image: the result is what the clamped bounds give"""
    from this_and_that_vdm_amd import _lib
    lib = _lib.load()
    h, w, ow, ksize = 6, 12, 8, 5
    img = R.sample_image(h, w, 7)
    rng = np.random.default_rng(11)
    first = np.array([-3, 0, 2, w - 1, w + 2, 9, 11, 4], np.int32)
    n = np.array([ksize + 5, 3, ksize, 4, 2, 5, -1, 1 << 30], np.int32)
    kk = rng.integers(-(1 << 19), 1 << 20, (ow, ksize), dtype=np.int32)          # 5 x 255 x 2^20 stays inside int32
    want = np.empty((h, ow, 3), np.uint8)
    for o in range(ow):
        f = min(max(int(first[o]), 0), w - 1)
        m = min(max(int(n[o]), 0), ksize, w - f)
        acc = (1 << 21) + (img[:, f:f + m].astype(np.int64) * kk[o, :m, None]).sum(1)
        want[:, o] = np.clip(acc >> 22, 0, 255)
    tab = torch.from_numpy(np.ascontiguousarray(np.concatenate([first[None], n[None], kk.T], 0))).to(DEV)          # [2 + ksize, out], row-major
    src, dst = torch.from_numpy(img).to(DEV), torch.zeros(h, ow, 3, dtype=torch.uint8, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.tt_resize_u8(src.data_ptr(), 1, h, w, h, ow, tab.data_ptr(), ksize, None, 0, dst.data_ptr(), None, 0, stream) == 0
    assert np.array_equal(dst.cpu().numpy(), want)


def test_refusals(ops):
    from this_and_that_vdm_amd import _lib
    lib = _lib.load()
    src = torch.zeros(1, 8, 12, 3, dtype=torch.uint8, device=DEV)
    for bad in (src.float(), src[..., :2], src[0, 0], torch.zeros(1, 3, 8, 12, dtype=torch.uint8, device=DEV)):
        with pytest.raises(RuntimeError, match="uint8"):
            ops.resize_u8(bad, (4, 4))
    with pytest.raises(RuntimeError, match="resample"):
        ops.resize_u8(src, (4, 4), "nearest")
    with pytest.raises(RuntimeError, match="positive"):
        ops.resize_u8(src, (0, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.resize_u8(src.cpu(), (4, 4))
    with pytest.raises(RuntimeError, match="noise"):
        ops.vae_image(src, (4, 4), torch.zeros(1, 3, 4, 5, device=DEV), 0.1, torch.float32)
    with pytest.raises(RuntimeError, match="noise"):
        ops.vae_image(src, (4, 4), torch.zeros(1, 3, 4, 4, device=DEV, dtype=torch.float16), 0.1, torch.float32)
    with pytest.raises(RuntimeError, match="noise"):
        ops.vae_image(src, (4, 4), torch.zeros(1, 3, 4, 4, device=DEV), 0.1, torch.float32, videos_per_image=2)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.vae_image(src, (4, 4), torch.zeros(1, 3, 4, 4), 0.1, torch.float32)
    with pytest.raises(RuntimeError, match="videos per image"):
        ops.vae_image(src, (4, 4), None, 0.1, torch.float32, videos_per_image=0)
    with pytest.raises(RuntimeError, match="bfloat16, float16 or float32"):
        ops.vae_image(src, (4, 4), None, 0.1, torch.float64)
    # the C entry points, each refused before any launch
    tx, kx = ops._resample_table(12, 4, 1, src.device)
    ty, ky = ops._resample_table(8, 4, 1, src.device)
    dst = torch.zeros(64, dtype=torch.float32, device=DEV)
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s, d, x, y, wp = src.data_ptr(), dst.data_ptr(), tx.data_ptr(), ty.data_ptr(), ws.data_ptr()
    assert lib.tt_resize_u8_ws_bytes(1, 8, 12, 4, 4) == lib.tt_vae_image_ws_bytes(1, 8, 12, 4, 4) == 8 * 4 * 3
    assert lib.tt_resize_u8_ws_bytes(1, 8, 12, 8, 4) == lib.tt_resize_u8_ws_bytes(1, 8, 12, 4, 12) == lib.tt_resize_u8_ws_bytes(0, 8, 12, 4, 4) == 0
    EINVAL, EUNSUPPORTED = -1, -2
    resize = lambda *a: lib.tt_resize_u8(*a, st)
    assert resize(None, 1, 8, 12, 4, 4, x, kx, y, ky, d, wp, 256) == EINVAL
    assert resize(s, 1, 8, 12, 4, 4, x, kx, y, ky, None, wp, 256) == EINVAL
    assert resize(s, 0, 8, 12, 4, 4, x, kx, y, ky, d, wp, 256) == EINVAL
    assert resize(s, 1, 8, 12, 0, 4, x, kx, y, ky, d, wp, 256) == EINVAL
    assert resize(s, 1, 8, 12, 4, 4, None, 0, y, ky, d, wp, 256) == EINVAL                     # a changing axis without its table
    assert resize(s, 1, 8, 12, 8, 4, x, kx, y, ky, d, wp, 256) == EINVAL                       # a table for an axis that stays
    assert resize(s, 1, 8, 12, 4, 4, x, 0, y, ky, d, wp, 256) == EINVAL
    assert resize(s, 1, 8, 12, 4, 4, x + 2, kx, y, ky, d, wp, 256) == EINVAL
    assert resize(s, 1, 8, 12, 4, 4, x, kx, y, ky, d + 1, wp, 256) == EINVAL
    assert resize(s, 1, 8, 12, 4, 4, x, kx, y, ky, d, None, 0) == EINVAL
    assert resize(s, 1, 8, 12, 4, 4, x, kx, y, ky, d, wp, 95) == EINVAL
    assert resize(s, 1, 8, 12, 4, 4, x, kx, y, ky, d, wp + 4, 252) == EINVAL
    assert resize(s, 1, 8, (1 << 20) + 1, 4, 4, x, kx, y, ky, d, wp, 256) == EUNSUPPORTED
    assert b"tt_resize_u8" in lib.tt_last_error()
    vae = lambda *a: lib.tt_vae_image(*a, st)
    assert vae(s, 1, 8, 12, 4, 4, x, kx, y, ky, None, 0.0, 1, d, 3, wp, 256) == EINVAL          # dtype
    assert vae(s, 1, 8, 12, 4, 4, x, kx, y, ky, None, 0.0, 0, d, 2, wp, 256) == EINVAL          # videos per image
    assert vae(s, 1, 8, 12, 4, 4, x, kx, y, ky, d + 2, 0.0, 1, d, 2, wp, 256) == EINVAL         # noise off its element size
    assert vae(s, 1, 8, 12, 4, 4, x, kx, y, ky, None, 0.0, 1, d + 2, 2, wp, 256) == EINVAL      # fp32 dst off its element size
    assert vae(s, 1, 8, 12, 4, 4, x, kx, y, ky, None, 0.0, 1, d, 2, None, 0) == EINVAL
    assert b"tt_vae_image" in lib.tt_last_error()
    torch.cuda.synchronize()
    assert float(dst.abs().max()) == 0.0                                                       # nothing was launched
