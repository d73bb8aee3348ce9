"""Shared by the gesture-map device tests: the ten rasteriser cases, a numpy fp64 statement of the closed form that tt_gesture_maps is
built to (include/ttvdm.h), the error bounds derived from the number formats, and a cache of the host rasteriser's results."""
import functools

import numpy as np

from this_and_that_vdm_amd import gesture_map as gm

# name -> (points (frame, horizontal, vertical), original (h, w), output (H, W), F, dilate, flip)
CASES = {
    "interior": (((0, 30, 20), (5, 50, 33)), (48, 72), (32, 40), 6, True, False),
    "corner_and_outside": (((0, 0, 0), (1, 71.9, 47.9), (2, 200, -50)), (48, 72), (32, 40), 6, True, False),
    "multi_bounce": (((0, 3, 2), (3, 11, 6)), (9, 13), (16, 24), 4, True, False),
    "one_pixel_axis": (((0, 0, 4),), (12, 1), (8, 8), 2, True, False),
    "upscale": (((0, 10, 10), (1, 20, 5)), (24, 32), (64, 96), 2, True, False),
    "flip": (((0, 10, 30), (1, 60, 5)), (48, 72), (32, 40), 2, True, True),
    "no_dilate": (((0, 30, 20), (1, 2, 46)), (48, 72), (32, 40), 2, False, False),
    "same_frame_twice": (((1, 30, 20), (1, 50, 33)), (48, 72), (32, 40), 3, True, False),
    "odd_w56": (((0, 77, 31), (6, 5, 60)), (67, 101), (24, 56), 7, True, False),
    "odd_w57": (((0, 77, 31), (6, 5, 60)), (67, 101), (24, 57), 7, True, False),
}

# ---- bounds, derived from the number formats: u = unit roundoff of fp32, A = 1.1875 = the two positive Keys weights (A = -0.75) at
# t = 0.5, 2 * 0.59375, the gain the specification of tt_gesture_maps budgets for one resize pass.  (With the two negative weights the
# absolute sum is 1.375; the same sums with it give 6.8e-7, still inside the 1e-6 condition below -- the tests hold the tighter figure.)
# In units of the final [0, 1] scale the host rounds to fp32 after the blur (<= u, amplified by A^2 through the two resize passes),
# after the resize (<= A^2 u) and after the division by 255 (<= A^2 u).  The kernel keeps the profiles in fp64 and rounds the product,
# the multiplication by d and the subtraction: <= A^2 u each.
U32 = 2.0 ** -24
_W_HALF = gm._cubic_weights(np.array(0.5))
A_CUBIC = float(_W_HALF[_W_HALF > 0].sum())
assert A_CUBIC == 1.1875 and float(np.abs(_W_HALF).sum()) == 1.375
HOST_BOUND = 3 * A_CUBIC ** 2 * U32          # 4.23 u = 2.5e-7: host rasteriser against the exact closed form
KERNEL_BOUND = 3 * A_CUBIC ** 2 * U32        # 2.5e-7: kernel against the exact closed form
BOUND32 = HOST_BOUND + KERNEL_BOUND          # 5.0e-7: kernel against the host rasteriser
assert HOST_BOUND <= 3e-7 and BOUND32 <= 1e-6, (HOST_BOUND, BOUND32)


def ulp(x: np.ndarray, mant_bits: int, emin: int) -> np.ndarray:
    """spacing of a binary format with `mant_bits` stored mantissa bits and smallest normal exponent `emin` at the magnitude of x"""
    _, e = np.frexp(np.abs(x.astype(np.float64)))
    e = np.where(x == 0, emin, np.maximum(e - 1, emin))
    return np.ldexp(1.0, e - mant_bits)


FORMATS = {"float16": (10, -14), "bfloat16": (7, -126)}


def _reflect101(j, n):
    if n == 1:
        return np.zeros_like(j)
    p = 2 * (n - 1)
    j = np.abs(j) % p
    return np.where(j >= n, p - j, j)


def profile(n: int, c: int, n_out: int, dilate: bool) -> np.ndarray:
    """r[o] of one axis (section 1 of the specification), float64"""
    i = np.arange(n)
    b = ((i >= max(0, c - 10)) & (i < min(n, c + 11))).astype(np.float64)
    if dilate:
        x = np.arange(-49, 50, dtype=np.float64)
        k = np.exp(-x * x / 200.0)
        k /= k.sum()
    else:
        k = np.ones(1)
    T = len(k)
    g = np.zeros(n)
    for t in range(T):
        g += k[t] * b[_reflect101(i + t - T // 2, n)]
    s = (np.arange(n_out) + 0.5) * n / n_out - 0.5
    base = np.floor(s)
    w = gm._cubic_weights(s - base)
    r = np.zeros(n_out)
    for tap in range(4):
        r += w[:, tap] * g[np.clip(base.astype(np.int64) - 1 + tap, 0, n - 1)]
    return r


def closed_form(points, org_hw, out_hw, num_frames, dilate, flip) -> np.ndarray:
    """[F, 3, H, W] float64: 1 - d_c ry[y] rx[x] for the last point naming each frame, zeros elsewhere"""
    out = np.zeros((num_frames, 3, out_hw[0], out_hw[1]))
    for m, f, x, y, first in gm.point_records(points, num_frames):
        ry, rx = profile(org_hw[0], y, out_hw[0], dilate), profile(org_hw[1], x, out_hw[1], dilate)
        rx = rx[::-1] if flip else rx
        d = (1.0, 1.0, 0.0) if first else (1.0, 0.0, 1.0)
        for c in range(3):
            out[f, c] = 1.0 - d[c] * np.outer(ry, rx)
    return out


@functools.lru_cache(maxsize=None)
def host(name: str) -> np.ndarray:
    """the host rasteriser's [F, 3, H, W] float32 frames of a case, computed once and never modified"""
    pts, org, out, f, dilate, flip = CASES[name]
    cond, _, _ = gm.rasterise_points(pts, org, out[0], out[1], f, dilate=dilate, flip=flip)
    cond.setflags(write=False)
    return cond
