"""GPU: tt_frame_metrics / tt_frames_pool2 and metrics.compare_frames against the fp64 restatement (tests/frame_metrics_reference.py), on
the smallest shapes at which the kernel can go wrong: one or two windows, the last window of a tile and the first of the next, rows
whose w * ch is no multiple of the 16-byte load, 1 / 3 / 4 channels, 1 / 3 frames, and one 256 x 384 x 3 pair for a real grid.  Both
sides use the library's own 11 window weights.

sse of uint8 frames must equal the integer sum exactly.  Everything else is held to a bound DERIVED from the operations the header
states, u = 2^-53, inputs in [0, L]:

  filtered moment  E = G*v: the product v = a b (1 rounding), then per pass a weight product (1) and 10 additions of non-negative
                   terms: (1 + u)^23 - 1, and sum g = 1 to a few u: |dE| <= 24 u L^2  (v = a alone: <= 24 u L)
  product of means maa = fl(mu_a mu_a):  2 * 24 u + u  ->  |d maa| <= 50 u L^2
  sigma            s = fl(E - m):  24 + 50 + 1 (|s| <= L^2)  ->  |ds| <= 75 u L^2.  THE cancellation term: absolute, however small s is.
  cs numerator     fl(fl(2 s_ab) + C2):  2 * 75 + (2 + 9e-4) u  ->  <= 153 u L^2;   denominator fl(fl(s_aa + s_bb) + C2): 150 + 2 * 2.001 -> <= 155 u L^2
  cs               |cs| <= 1 (Cauchy-Schwarz on the weighted moments), one division:  b_cs = 308 u L^2 / (D_cs - 310 u L^2) + u
                   with D_cs the reference's denominator of THAT window (itself within 155 u L^2 of the exact one, hence 310)
  luminance        numerator 2 * 50 + 2 + 1 -> 103 u L^2, denominator 100 + 5 -> 105 u L^2, |l| <= 1:  b_l = 208 u L^2 / (D_l - 210 u L^2) + u
  ssim = l cs      b_ssim = b_l + b_cs + b_l b_cs + u
  two implementations that each keep these bounds differ by at most 2 b per window.
  sums             the reference sums with math.fsum (one rounding).  The kernel adds a value along a path of 6 (lanes of a wave) + 3
                   (waves) + tiles (tile order) additions, every |term| <= 1:  (10 + tiles) u count
  => |ssim_sum - ref| <= 2 sum_windows b_ssim + (10 + tiles) u count, likewise cs_sum.
  sse of fp32      d = fl(a - b), fl(d d), then a path of at most 3 (a lane's pixels) + 9 + tiles additions of non-negative terms,
                   the reference 3 roundings:  |sse - ref| <= (20 + tiles) u ref.
  MS-SSIM          x_j the per-scale means with errors e_j = (bound of the sum) / (count ch); d(prod x_j^w_j) / prod <= sum w_j e_j / (x_j - e_j)
                   to first order (doubled here for the higher orders) plus 16 u for the five powers and products on the host.
Nothing is tuned to the observed error; each test prints what it observed beside its bound."""
import math
import os

import numpy as np
import pytest
import torch

from tests import frame_metrics_reference as ref
from this_and_that_vdm_amd import _lib, metrics, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -53

if not os.path.exists(_lib.LIB_PATH):
    _lib.build()
T, BLOCK, VEC_U8 = ops.frame_metrics_launch(torch.uint8)
VEC_F32 = ops.frame_metrics_launch(torch.float32)[2]
G = ops.frame_metrics_window()

# (n, h, w, ch)
SHAPES = [
    (1, 11, 11, 1), (1, 11, 12, 3), (3, 12, 11, 4), (1, 12, 12, 3),                       # one or two windows
    (1, T + 9, T + 11, 3), (3, T + 10, T + 9, 1), (1, T + 11, T + 10, 4), (3, T + 11, T + 11, 3),   # the last window of a tile, the first of the next
    (2, 2 * T + 13, 3 * T + 13, 3),                                                       # 3 x 4 tiles, ragged last ones
    (2, 256, 384, 3),                                                                     # a real grid: 16 x 24 tiles per frame
]
KINDS = ["noise", "near", "bright", "const", "f32"]
# rows that end in the middle of a 16-byte load, for both element sizes, on one-tile and several-tile shapes
assert sum((w * ch) % VEC_U8 != 0 and (w * ch) % VEC_F32 != 0 for _, _, w, ch in SHAPES) >= 5


def make_pair(kind, shape, seed):
    rng = np.random.default_rng(seed)
    n, h, w, ch = shape
    if kind == "noise":
        return rng.integers(0, 256, shape).astype(np.uint8), rng.integers(0, 256, shape).astype(np.uint8)
    if kind == "near":
        a = rng.integers(0, 256, shape)
        return a.astype(np.uint8), np.clip(a + rng.integers(-12, 13, shape), 0, 255).astype(np.uint8)
    if kind == "bright":                              # smooth, near 250, +-1 noise: E[x^2] - mu^2 cancels 65 025 against a variance below 1
        yy, xx = np.mgrid[0:h, 0:w]
        base = (250.0 + 3.0 * np.sin(yy / 7.0) * np.cos(xx / 9.0)).round().astype(np.int64)[None, :, :, None]
        return (base + rng.integers(-1, 2, shape)).astype(np.uint8), (base + rng.integers(-1, 2, shape)).astype(np.uint8)
    if kind == "const":
        return np.full(shape, 10, np.uint8), np.full(shape, 200, np.uint8)
    a = rng.random(shape, dtype=np.float32)
    return a, np.clip(a + np.float32(0.05) * rng.standard_normal(shape, dtype=np.float32), 0, 1).astype(np.float32)


def records(a, b, **kw):
    rec = ops.frame_metrics(a, b, **kw)
    return np.frombuffer(rec.cpu().numpy().tobytes(), dtype=metrics.REC_DTYPE)


def tiles_of(h, w):
    t = lambda v: max(1, -(-(v - 10) // T))
    return t(h) * t(w)


def sum_bounds(maps, data_range, tiles):
    """(bound of ssim_sum, bound of cs_sum) of one channel of one frame from the reference's per-window denominators"""
    s, cs, parts = maps
    l2 = data_range * data_range
    b_cs = 308 * U * l2 / (parts["cs_den"] - 310 * U * l2) + U
    b_l = 208 * U * l2 / (parts["lum_den"] - 210 * U * l2) + U
    b_ssim = b_l + b_cs + b_l * b_cs + U
    order = (10 + tiles) * U * s.size
    return 2.0 * float(b_ssim.sum()) + order, 2.0 * float(b_cs.sum()) + order


def check_against_reference(a, b, got, label=""):
    """got: the decoded records of frames a, b (numpy [n, h, w, ch]); returns (worst observed error / its bound, worst error per window)"""
    n, h, w, ch = a.shape
    data_range = 255.0 if a.dtype == np.uint8 else 1.0
    tiles = tiles_of(h, w)
    worst, per_window = 0.0, 0.0
    for i in range(n):
        want = ref.frame_record(a[i], b[i], data_range, G)
        assert got[i]["count"] == want["count"] == (h - 10) * (w - 10)
        for c in range(4):
            if c >= ch:
                assert got[i]["sse"][c] == 0.0 and got[i]["ssim_sum"][c] == 0.0 and got[i]["cs_sum"][c] == 0.0
                continue
            if a.dtype == np.uint8:
                assert got[i]["sse"][c] == float(want["sse"][c]), (i, c, got[i]["sse"][c], want["sse"][c])
            else:
                assert abs(got[i]["sse"][c] - want["sse"][c]) <= (20 + tiles) * U * want["sse"][c], (i, c)
            b_ssim, b_cs = sum_bounds(want["maps"][c], data_range, tiles)
            e_ssim, e_cs = abs(got[i]["ssim_sum"][c] - want["ssim_sum"][c]), abs(got[i]["cs_sum"][c] - want["cs_sum"][c])
            assert e_ssim <= b_ssim and e_cs <= b_cs, (label, i, c, e_ssim, b_ssim, e_cs, b_cs)
            worst = max(worst, e_ssim / b_ssim, e_cs / b_cs)
            per_window = max(per_window, e_ssim / want["count"], e_cs / want["count"])
    return worst, per_window


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_records_against_the_restatement(shape, kind):
    a, b = make_pair(kind, shape, seed=sum(shape) + KINDS.index(kind))
    got = records(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    worst, per_window = check_against_reference(a, b, got, f"{kind} {shape}")
    print(f"{kind} {shape}: worst error / bound = {worst:.3g}, worst |error of a sum| / count = {per_window:.3g}")


@pytest.mark.parametrize("kind", ["noise", "bright", "f32"])
@pytest.mark.parametrize("shape", [(3, T + 11, T + 11, 3), (2, 256, 384, 3), (1, 12, 11, 4)], ids=["seam", "grid", "tiny"])
def test_identical_frames_give_exactly_one_per_window(shape, kind):
    a = torch.from_numpy(make_pair(kind, shape, 5)[0]).to(DEV)
    got = records(a, a.clone())
    n, h, w, ch = shape
    for i in range(n):
        assert got[i]["count"] == (h - 10) * (w - 10)
        assert got[i]["sse"].tolist() == [0.0] * 4
        assert got[i]["ssim_sum"].tolist() == [float(got[i]["count"])] * ch + [0.0] * (4 - ch)
        assert got[i]["cs_sum"].tolist() == [float(got[i]["count"])] * ch + [0.0] * (4 - ch)


@pytest.mark.parametrize("kind", ["near", "f32"])
def test_same_bits_every_time_and_for_a_sub_range_of_frames(kind):
    """a frame of 27 x 21 x 3 elements is 1701 elements long: frames 1.. start off every 16-byte boundary"""
    a, b = (torch.from_numpy(v).to(DEV) for v in make_pair(kind, (4, T + 11, 21, 3), 6))
    assert a[1].data_ptr() % 16 != 0
    first = ops.frame_metrics(a, b).clone()
    again = ops.frame_metrics(a, b)
    assert torch.equal(first, again)
    part = ops.frame_metrics(a[1:3], b[1:3])
    assert torch.equal(part, first[1:3])
    big = [torch.from_numpy(v).to(DEV) for v in make_pair(kind, (2, 256, 384, 3), 7)]
    assert torch.equal(ops.frame_metrics(*big).clone(), ops.frame_metrics(*big))
    out = torch.zeros(4, ops.METRICS_BYTES, dtype=torch.uint8, device=DEV)
    assert ops.frame_metrics(a, b, out=out).data_ptr() == out.data_ptr() and torch.equal(out, first)


@pytest.mark.parametrize("kind", ["noise", "f32"])
def test_sse_only(kind):
    a, b = make_pair(kind, (2, 3, 5, 3), 8)
    got = records(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), sse_only=True)
    for i in range(2):
        want = ref.frame_record(a[i], b[i], 255.0, G, sse_only=True)
        assert got[i]["count"] == 0 and got[i]["ssim_sum"].tolist() == [0.0] * 4 and got[i]["cs_sum"].tolist() == [0.0] * 4
        if kind == "noise":
            assert got[i]["sse"].tolist() == [float(v) for v in want["sse"]] + [0.0]
        else:
            assert all(abs(got[i]["sse"][c] - want["sse"][c]) <= 21 * U * want["sse"][c] for c in range(3)) and got[i]["sse"][3] == 0.0
    with pytest.raises(RuntimeError, match="holds no 11 x 11 window"):
        ops.frame_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    # several tiles: the flag changes nothing about sse
    a, b = (torch.from_numpy(v).to(DEV) for v in make_pair(kind, (2, 2 * T + 13, 3 * T + 13, 3), 9))
    full, only = records(a, b), records(a, b, sse_only=True)
    assert np.array_equal(full["sse"], only["sse"]) and not only["count"].any()


def test_ops_refuse_what_they_cannot_serve():
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frame_metrics(a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.frames_pool2(a)
    d = a.to(DEV)
    with pytest.raises(RuntimeError, match="one shape, dtype and device"):
        ops.frame_metrics(d, d.float())
    with pytest.raises(RuntimeError, match="uint8 or float32"):
        ops.frame_metrics(d.half(), d.half())
    with pytest.raises(RuntimeError, match="must be even"):
        ops.frames_pool2(d[:, :15].contiguous())


# ---- tt_frames_pool2
@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("shape", [(2, 6, 10, 3), (1, 34, 18, 4), (3, 2, 2, 1), (1, 176, 192, 3)], ids=lambda s: "x".join(map(str, s)))
def test_pool2_is_bit_equal_to_the_fp32_statement(shape, dtype):
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, shape).astype(np.uint8) if dtype == "u8" else (rng.standard_normal(shape) * 100).astype(np.float32)
    got = ops.frames_pool2(torch.from_numpy(x).to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.pool2(x).view(np.uint32))


def test_pool2_is_exact_for_uint8_frames_through_four_levels():
    x = np.random.default_rng(12).integers(0, 256, (2, 32, 48, 3)).astype(np.uint8)
    got, want = torch.from_numpy(x).to(DEV), x.astype(np.float64)
    for _ in range(4):
        got = ops.frames_pool2(got)
        want = 0.25 * (want[:, 0::2, 0::2] + want[:, 0::2, 1::2] + want[:, 1::2, 0::2] + want[:, 1::2, 1::2])
        assert np.array_equal(got.cpu().numpy().astype(np.float64), want)


# ---- metrics.compare_frames
def smooth_noise(shape, seed):
    """uint8 noise smoothed by a 5 x 5 box"""
    n, h, w, ch = shape
    x = np.random.default_rng(seed).integers(0, 256, (n, h + 4, w + 4, ch)).astype(np.float64)
    acc = sum(x[:, i:i + h, j:j + w] for i in range(5) for j in range(5))
    return np.rint(acc / 25.0).astype(np.uint8)


@pytest.fixture(scope="module")
def ms_case():
    a = smooth_noise((2, 176, 192, 3), 13)
    b = np.clip(a.astype(np.int64) + np.random.default_rng(14).integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
    return a, b


def test_ms_ssim_against_the_restatement(ms_case):
    a, b = ms_case
    m = metrics.compare_frames(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), ms_ssim=True)
    want = ref.compare(a, b, G, ms_ssim=True)
    la, lb = [a], [b]
    for _ in range(4):
        la.append(ref.pool2(la[-1]))
        lb.append(ref.pool2(lb[-1]))
    assert m.frame_mse.tolist() == want["mse"] and m.frame_psnr.tolist() == want["psnr"]
    for i in range(a.shape[0]):
        rel = 0.0
        for lvl in range(5):
            h, w = la[lvl].shape[1:3]
            rec = ref.frame_record(la[lvl][i], lb[lvl][i], 255.0, G)
            b_ssim, b_cs = (sum(v) for v in zip(*(sum_bounds(rec["maps"][c], 255.0, tiles_of(h, w)) for c in range(3))))
            e_ssim, e_cs = b_ssim / (rec["count"] * 3) + 4 * U, b_cs / (rec["count"] * 3) + 4 * U       # (+ the host's channel sum and division)
            x_ssim, x_cs = want["scales"][i][lvl]
            assert x_ssim > 0 and x_cs > 0                            # no scale of this case falls under the nan rule
            if lvl == 0:
                assert abs(m.frame_ssim[i] - x_ssim) <= e_ssim and abs(m.frame_cs[i] - x_cs) <= e_cs
            e, x = (e_cs, x_cs) if lvl < 4 else (e_ssim, x_ssim)
            rel += ref.MS_SSIM_WEIGHTS[lvl] * e / (x - e)
        bound = want["ms_ssim"][i] * 2.0 * rel + 16 * U
        err = abs(m.frame_ms_ssim[i] - want["ms_ssim"][i])
        print(f"frame {i}: scales (ssim, cs) {[(round(s, 4), round(c, 4)) for s, c in want['scales'][i]]}, ms_ssim {want['ms_ssim'][i]:.6f}, "
              f"error {err:.3g}, bound {bound:.3g}")
        assert err <= bound
    assert m.ms_ssim == float(m.frame_ms_ssim.mean()) and m.ssim == float(m.frame_ssim.mean())


def test_ms_ssim_is_nan_where_a_scale_is_negative(ms_case):
    a = np.random.default_rng(15).integers(0, 256, (1, 176, 192, 3)).astype(np.uint8)
    m = metrics.compare_frames(torch.from_numpy(a).to(DEV), torch.from_numpy(255 - a).to(DEV), ms_ssim=True)
    want = ref.compare(a, 255 - a, G, ms_ssim=True)
    assert math.isnan(want["ms_ssim"][0]) and math.isnan(m.frame_ms_ssim[0]) and math.isnan(m.ms_ssim)
    assert m.frame_ssim[0] < 0 and m.to_dict()["ms_ssim"] == "nan"


def test_host_inputs_give_the_device_inputs_bits(ms_case):
    from PIL import Image
    a, b = (v[:, :40, :52] for v in ms_case)
    dev = metrics.compare_frames(torch.from_numpy(a.copy()).to(DEV), torch.from_numpy(b.copy()).to(DEV))
    pil = metrics.compare_frames([Image.fromarray(f) for f in a], [Image.fromarray(f) for f in b])
    arr = metrics.compare_frames(a, b)
    for other in (pil, arr):
        for name in ("frame_mse", "frame_psnr", "frame_ssim", "frame_cs"):
            assert np.array_equal(getattr(dev, name), getattr(other, name)), name
    # a batch of videos: per-video values equal those of separate calls; float frames; the thin wrappers
    both = metrics.compare_frames(np.stack([a, b]), np.stack([b, b]))
    assert both.frame_ssim.shape == (2, 2) and np.array_equal(both.frame_ssim[0], dev.frame_ssim) and both.ssim[0] == dev.ssim
    assert both.psnr[1] == math.inf and both.ssim[1] == 1.0
    fa, fb = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
    f = metrics.compare_frames(fa, fb)
    assert f.data_range == 1.0 and abs(f.ssim - dev.ssim) < 1e-5 and abs(f.psnr - dev.psnr) < 1e-4      # the same pictures, rescaled (fp32 rounding of x / 255)
    assert metrics.psnr(a, b) == dev.psnr and metrics.ssim(a, b) == dev.ssim
    assert metrics.psnr(a[:, :3, :5], b[:, :3, :5]) > 0
