"""PIL's 8-bit resize restated in numpy: the coefficient tables of ``tt_resample_coeffs`` (Pillow's precompute_coeffs +
normalize_coeffs_8bpc, fp64 with libm through ``math``) and the two integer passes of ``tt_resize_u8`` / ``tt_vae_image``
(include/ttvdm.h).  tests/test_resize_u8_cpu.py holds it to ``PIL.Image.resize`` byte for byte; the GPU tests share its inputs."""
import math

import numpy as np
import PIL.Image


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


_H54, _H46 = float(np.float32(0.54)), float(np.float32(0.46))          # Pillow writes 0.54f / 0.46f: float literals, widened to double


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_H54 + _H46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# name -> (PIL's code, support, filter function)
FILTERS = {"box": (4, 0.5, _box), "bilinear": (2, 1.0, _bilinear), "hamming": (5, 1.0, _hamming), "bicubic": (3, 2.0, _bicubic),
           "lanczos": (1, 3.0, _lanczos)}

# (H, W) -> (h, w): down, odd sizes, up, a long down-scale, 227 taps, one pass skipped (each way), both skipped
SHAPES = [((48, 64), (32, 56)), ((37, 53), (24, 40)), ((16, 24), (32, 56)), ((97, 131), (16, 24)), ((200, 300), (8, 8)),
          ((33, 40), (16, 40)), ((40, 33), (40, 16)), ((24, 40), (24, 40))]
CLAMP_SHAPES = SHAPES[:3]          # where the 0 / 255 checkerboard must drive the result to both ends of the clamp


# HAMMING rows on which Pillow's fp32 constants 0.54f / 0.46f and the doubles 0.54 / 0.46 give tables one unit apart in a tap AND the
# accumulator sits where that unit changes the byte: (in, out, first x, pixels from there on (all channels equal, zeros elsewhere),
# output index, the byte PIL gives there)
HAMMING_ROWS = [(27, 8, 2, [207, 200, 68, 181, 206, 239], 1, 154), (34, 26, 15, [61, 169, 82], 12, 154)]


def hamming_row(n_in, first, pixels) -> np.ndarray:
    row = np.zeros((1, n_in, 3), np.uint8)
    row[0, first:first + len(pixels)] = np.asarray(pixels, np.uint8)[:, None]
    return row


def coeffs(in_size: int, out_size: int, name: str):
    """(ksize, bounds int32 [out, 2], kk int32 [out, ksize]) of one axis"""
    _, s, f = FILTERS[name]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = s * fs
    ss = 1.0 / fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds, kk = np.zeros((out_size, 2), np.int32), np.zeros((out_size, ksize), np.int32)
    for o in range(out_size):
        c = (o + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), in_size) - xmin
        w = [f((x + xmin - c + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            kk[o, x] = int(v * (1 << 22) - 0.5) if v < 0 else int(v * (1 << 22) + 0.5)       # int() truncates
        bounds[o] = (xmin, n)
    return ksize, bounds, kk


def resample_axis(img: np.ndarray, axis: int, out_size: int, name: str) -> np.ndarray:
    """one pass along `axis` of a uint8 array: int32 from 1 << 21, + pixel kk, >> 22 (arithmetic), clamp to 0 .. 255"""
    _, bounds, kk = coeffs(img.shape[axis], out_size, name)
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    out = np.empty((out_size,) + src.shape[1:], np.int32)
    for o in range(out_size):
        xmin, n = bounds[o]
        taps = kk[o, :n].reshape((n,) + (1,) * (src.ndim - 1))
        out[o] = ((1 << 21) + (src[xmin:xmin + n] * taps).sum(0, dtype=np.int32)) >> 22
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize(img: np.ndarray, size, name: str) -> np.ndarray:
    """uint8 [..., H, W, 3] -> [..., size[0], size[1], 3]: horizontal first, then vertical, a pass skipped when its size is unchanged"""
    h_axis, w_axis = img.ndim - 3, img.ndim - 2
    out = img
    if size[1] != img.shape[w_axis]:
        out = resample_axis(out, w_axis, size[1], name)
    if size[0] != img.shape[h_axis]:
        out = resample_axis(out, h_axis, size[0], name)
    return out.copy() if out is img else out


def pil_resize(img: np.ndarray, size, name: str) -> np.ndarray:
    """the yardstick: PIL.Image.resize of one [H, W, 3] image"""
    return np.asarray(PIL.Image.fromarray(img).resize((size[1], size[0]), resample=FILTERS[name][0]))


def sample_image(h: int, w: int, seed: int = 0) -> np.ndarray:
    """random bytes with the top-left quadrant a pure 0 / 255 checkerboard noise: ringing filters overshoot there on both sides"""
    rng = np.random.default_rng(seed * 1000003 + h * 1009 + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[:h // 2, :w // 2] = rng.integers(0, 2, (h // 2, w // 2, 3), dtype=np.uint8) * 255
    return img
