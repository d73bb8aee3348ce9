"""tt_resample_coeffs and the numpy restatement of PIL's 8-bit resize (tests/resize_u8_reference.py), without a GPU.  Every
comparison is bit equality: the resampler is integer arithmetic on tables formed in fp64."""
import ctypes as C

import numpy as np
import pytest

from tests import resize_u8_reference as R
from this_and_that_vdm_amd import _lib, ops

NAMES = sorted(R.FILTERS)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("src_hw, dst_hw", R.SHAPES)
def test_reference_equals_pil(src_hw, dst_hw, name):
    img = R.sample_image(*src_hw)
    got, want = R.resize(img, dst_hw, name), R.pil_resize(img, dst_hw, name)
    assert got.shape == want.shape == (*dst_hw, 3) and got.dtype == np.uint8
    assert np.array_equal(got, want)
    if (src_hw, dst_hw) in R.CLAMP_SHAPES:
        assert got.min() == 0 and got.max() == 255          # the checkerboard quadrant reaches both ends of the clamp


def test_reference_batch_equals_single():
    imgs = np.stack([R.sample_image(37, 53, seed) for seed in (0, 1)])
    got = R.resize(imgs, (24, 40), "lanczos")
    for i in range(2):
        assert np.array_equal(got[i], R.pil_resize(imgs[i], (24, 40), "lanczos"))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("src_hw, dst_hw", R.SHAPES)
def test_library_tables_equal_reference(src_hw, dst_hw, name):
    for n_in, n_out in zip(src_hw, dst_hw):
        ksize, bounds, kk = ops.resample_coeffs(n_in, n_out, name)
        rk, rb, rkk = R.coeffs(n_in, n_out, name)
        assert ksize == rk
        assert bounds.dtype == kk.dtype == np.int32 and bounds.shape == (n_out, 2) and kk.shape == (n_out, ksize)
        assert np.array_equal(bounds, rb) and np.array_equal(kk, rkk)


@pytest.mark.parametrize("n_in, n_out, first, pixels, o, pil_byte", R.HAMMING_ROWS)
def test_hamming_uses_pillows_fp32_constants(monkeypatch, n_in, n_out, first, pixels, o, pil_byte):
    """Pillow's hamming_filter writes 0.54f + 0.46f * cos(x): float literals.  On these rows the double constants give another byte."""
    row = R.hamming_row(n_in, first, pixels)
    want = R.pil_resize(row, (1, n_out), "hamming")
    assert want[0, o, 0] == pil_byte
    assert np.array_equal(R.resize(row, (1, n_out), "hamming"), want)
    ksize, bounds, kk = ops.resample_coeffs(n_in, n_out, "hamming")
    rk, rb, rkk = R.coeffs(n_in, n_out, "hamming")
    assert ksize == rk and np.array_equal(bounds, rb) and np.array_equal(kk, rkk)
    monkeypatch.setattr(R, "_H54", 0.54)
    monkeypatch.setattr(R, "_H46", 0.46)
    assert not np.array_equal(R.coeffs(n_in, n_out, "hamming")[2], kk)           # the case tells the two apart: in a tap ...
    assert R.resize(row, (1, n_out), "hamming")[0, o, 0] != pil_byte              # ... and in the byte


def test_tables_227_taps_and_code_names():
    assert ops.resample_coeffs(300, 8, "lanczos")[0] == 227
    for name, (code, _, _) in R.FILTERS.items():
        a, b = ops.resample_coeffs(53, 40, name), ops.resample_coeffs(53, 40, code)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_ksize_only_query():
    lib = _lib.load()
    k = C.c_int32(-1)
    assert lib.tt_resample_coeffs(131, 24, 1, C.byref(k), None, None) == 0
    assert k.value == 2 * 17 + 1          # support 3 * 131 / 24 = 16.375


def test_refusals():
    lib = _lib.load()
    k = C.c_int32(0)
    buf = (C.c_int32 * 64)()
    assert lib.tt_resample_coeffs(8, 8, 1, None, None, None) == -1
    assert lib.tt_resample_coeffs(0, 8, 1, C.byref(k), None, None) == -1
    assert lib.tt_resample_coeffs(8, -3, 1, C.byref(k), None, None) == -1
    assert lib.tt_resample_coeffs(8, 4, 0, C.byref(k), None, None) == -1            # NEAREST is no filter of the resampler
    assert lib.tt_resample_coeffs(8, 4, 6, C.byref(k), None, None) == -1
    assert lib.tt_resample_coeffs(8, 4, 1, C.byref(k), buf, None) == -1             # one table without the other
    assert lib.tt_resample_coeffs((1 << 20) + 1, 4, 1, C.byref(k), None, None) == -2
    assert lib.tt_resample_coeffs(4, (1 << 20) + 1, 1, C.byref(k), None, None) == -2
    assert b"tt_resample_coeffs" in lib.tt_last_error()
    for bad in ("nearest", None, 0, 7, 3.0, True):
        with pytest.raises(RuntimeError, match="resample"):
            ops.resample_coeffs(8, 4, bad)
    with pytest.raises(RuntimeError, match="tt_resample_coeffs"):
        ops.resample_coeffs(8, 0, "lanczos")


def test_device_ops_refuse_cpu_tensors():
    import torch
    src = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.resize_u8(src, (4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.vae_image(src, (4, 4), None, 0.0, torch.float32)
