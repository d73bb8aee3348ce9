"""CPU: the fp64 restatement of tt_frame_metrics (tests/frame_metrics_reference.py) against two independent formulations and against
closed forms; every refusal of the two entry points (in a child process that sees no GPU); the ctypes mirror of TtFrameMetricsRecord
against the C compiler; metrics.compare_frames refusing mismatched videos before it touches a device, and its host arithmetic on
fabricated records."""
import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import frame_metrics_reference as ref
from tests import frame_metrics_refusals as refusals

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = ref.window()


def _noise(shape, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, size=shape, dtype=np.int64).astype(np.uint8)


# ---- the restatement against independent formulations
def test_window_is_the_normalised_gaussian_and_the_library_uses_the_same_doubles():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    g = (ctypes.c_double * 11)()
    assert _lib.load().tt_frame_metrics_window(g) == 0
    assert abs(sum(G) - 1.0) <= 2.0 ** -52 and G == G[::-1]
    assert max(abs(x - y) for x, y in zip(g, G)) <= 2.0 ** -54         # one ulp of the largest weight (0.266): libm's exp on both sides


def test_filter_agrees_with_scipy_gaussian_filter():
    """scipy.ndimage.gaussian_filter(x, 1.5, truncate=3.5) has radius int(3.5 * 1.5 + 0.5) = 5: the same 11 taps; cropped by 5 it is
    the valid region whatever the boundary mode.  The two differ only in summation order: 22 taps of values below 256, so a few
    ulps of 256 (2.8e-14 each) -- 8.5e-14 observed; held to 64 * 2^-53 * 256 = 1.8e-12."""
    from scipy.ndimage import gaussian_filter
    x = _noise((64, 80), 1).astype(np.float64)
    mine = ref.filter_valid(x, G)
    theirs = gaussian_filter(x, 1.5, truncate=3.5)[5:-5, 5:-5]
    assert mine.shape == theirs.shape == (54, 70)
    err = np.abs(mine - theirs).max()
    print("filter vs scipy:", err)
    assert err <= 64 * 2.0 ** -53 * 256


def _ssim_conv2d(a, b, data_range):
    """the pytorch-msssim formulation: fp64 conv2d with the outer-product window, sigma = E[xy] - mu mu"""
    import torch.nn.functional as F
    g = torch.tensor(G, dtype=torch.float64)
    k = (g[:, None] * g[None, :])[None, None]
    a, b = (torch.from_numpy(v.astype(np.float64))[None, None] for v in (a, b))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    mu_a, mu_b = F.conv2d(a, k), F.conv2d(b, k)
    saa, sbb, sab = F.conv2d(a * a, k) - mu_a * mu_a, F.conv2d(b * b, k) - mu_b * mu_b, F.conv2d(a * b, k) - mu_a * mu_b
    cs = (2 * sab + c2) / (saa + sbb + c2)
    return (((2 * mu_a * mu_b + c1) / (mu_a * mu_a + mu_b * mu_b + c1)) * cs)[0, 0].numpy(), cs[0, 0].numpy()


@pytest.mark.parametrize("case", ["noise", "near", "bright"])
def test_ssim_agrees_with_the_conv2d_formulation(case):
    """same definition, another order of the 121 products: the per-window difference is rounding only.  Bound: the moments carry
    ~ 121 u L^2 of summation error on either side, divided by a denominator of at least C2 = 58.5: 2 * 121 * 2^-53 * 65025 / 58.5 * 4
    (numerator and denominator, both factors) = 1.2e-10."""
    a = _noise((40, 52), 2)
    if case == "noise":
        b = _noise((40, 52), 3)
    elif case == "near":
        b = np.clip(a.astype(np.int64) + np.random.default_rng(4).integers(-12, 13, a.shape), 0, 255).astype(np.uint8)
    else:
        a = (250 + np.random.default_rng(5).integers(-1, 2, a.shape)).astype(np.uint8)
        b = (250 + np.random.default_rng(6).integers(-1, 2, a.shape)).astype(np.uint8)
    s, cs, _ = ref.ssim_maps(a, b, 255.0, G)
    s2, cs2 = _ssim_conv2d(a, b, 255.0)
    err = max(np.abs(s - s2).max(), np.abs(cs - cs2).max())
    print(case, "ssim vs conv2d:", err)
    assert err <= 1.2e-10


# ---- closed forms
def test_identical_frames():
    a = _noise((2, 30, 33, 3), 7)
    out = ref.compare(a, a.copy(), G)
    assert out["mse"] == [0.0, 0.0] and out["psnr"] == [math.inf, math.inf] and out["ssim"] == [1.0, 1.0] and out["cs"] == [1.0, 1.0]


@pytest.mark.parametrize("c1c2", [(10, 200), (0, 255)])
def test_constant_frames(c1c2):
    """sigma is 0 up to the rounding of sum g = 1: cs = 1 and ssim = (2 c1 c2 + C1) / (c1^2 + c2^2 + C1)"""
    va, vb = c1c2
    a, b = np.full((1, 20, 24, 1), va, np.uint8), np.full((1, 20, 24, 1), vb, np.uint8)
    out = ref.compare(a, b, G)
    k1 = (0.01 * 255.0) ** 2
    assert abs(out["ssim"][0] - (2.0 * va * vb + k1) / (va * va + vb * vb + k1)) <= 1e-14
    # cs: each sigma is the rounding of E[x^2] - mu^2, at most 75 u L^2 (the bound of tests/test_frame_metrics_gpu.py), over C2 = 9e-4 L^2
    assert abs(out["cs"][0] - 1.0) <= 300 * 2.0 ** -53 / 9e-4
    assert out["mse"][0] == float((va - vb) ** 2)


def test_inverted_noise_has_negative_ssim():
    a = _noise((1, 48, 48, 1), 8)
    out = ref.compare(a, 255 - a, G)
    print("ssim of inverted noise:", out["ssim"][0])
    # sigma_ab = -sigma_aa and C2 is small beside the variance of uniform noise, so cs is close to -1; the luminance term of means
    # near 127 and 128 is close to 1: -0.96 for this noise (a narrower noise gives a smaller magnitude; the sign is the check)
    assert -1.0 < out["ssim"][0] < 0.0
    assert out["cs"][0] < 0


def test_pool2_statement_is_exact_for_uint8_through_four_levels():
    x = _noise((1, 32, 48, 3), 9)
    want = x.astype(np.float64)
    got = x
    for _ in range(4):
        got = ref.pool2(got)
        want = 0.25 * (want[:, 0::2, 0::2] + want[:, 0::2, 1::2] + want[:, 1::2, 0::2] + want[:, 1::2, 1::2])
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)


def test_ms_ssim_combination():
    assert ref.ms_ssim_combine([1.0] * 4, 1.0) == 1.0
    assert math.isnan(ref.ms_ssim_combine([0.9, -0.1, 0.9, 0.9], 0.9))
    want = math.exp(sum(w * math.log(v) for w, v in zip(ref.MS_SSIM_WEIGHTS, (0.84, 0.96, 0.99, 0.99, 0.998))))
    assert abs(ref.ms_ssim_combine([0.84, 0.96, 0.99, 0.99], 0.998) - want) <= 1e-15


# ---- the entry points refuse each fault, one at a time, before any launch
@pytest.fixture(scope="module")
def answers():
    return refusals.run_child()


ROWS = [("metrics", f, t) for f, t in refusals.METRICS_ROWS] + [("pool2", f, t) for f, t in refusals.POOL_ROWS]


@pytest.mark.parametrize("family,fault,text", ROWS, ids=[refusals.row_id(fam, f) for fam, f, _ in ROWS])
def test_refusal(answers, family, fault, text):
    code, msg = answers[refusals.row_id(family, fault)]
    assert code == -1, (code, msg)                                    # TT_EINVAL
    assert msg.startswith("tt_frame_metrics:" if family == "metrics" else "tt_frames_pool2:") and text in msg, msg


def test_workspace_query(answers):
    # 96 bytes per (frame, tile of 16 x 16 windows); 0 for what the entry point refuses
    assert answers["ws_bytes"] == [2 * 2 * 3 * 96, 0, 2 * 96, 0, 2 * 96, 3 * 16 * 24 * 96]


# ---- the record
def test_record_layout_matches_the_c_compiler():
    from this_and_that_vdm_amd import _lib, metrics
    fields = [n for n, _ in _lib.TtFrameMetricsRecord._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ttvdm.h"\nint main(){printf("%zu", sizeof(TtFrameMetricsRecord));' +
           "".join(f'printf(" %zu", offsetof(TtFrameMetricsRecord, {n}));' for n in fields) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "s.c"), os.path.join(d, "s")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), c, "-o", exe])
        size, *offsets = map(int, subprocess.check_output([exe]).split())
    assert size == ctypes.sizeof(_lib.TtFrameMetricsRecord) == metrics.REC_DTYPE.itemsize == 104
    for name, off in zip(fields, offsets):
        assert getattr(_lib.TtFrameMetricsRecord, name).offset == off == metrics.REC_DTYPE.fields[name][1], name


# ---- metrics.py on the host
def test_compare_frames_refuses_mismatched_videos_without_a_device():
    from this_and_that_vdm_amd import metrics
    a = np.zeros((2, 16, 16, 3), np.uint8)
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.compare_frames(a, np.zeros((2, 16, 17, 3), np.uint8))
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.compare_frames(a, a[None])
    with pytest.raises(ValueError, match="differ in kind"):
        metrics.compare_frames(a, a.astype(np.float32))
    with pytest.raises(ValueError, match="differ in kind"):
        metrics.compare_frames(torch.zeros(2, 16, 16, 3, dtype=torch.uint8), torch.zeros(2, 16, 16, 3))
    with pytest.raises(ValueError, match="1 to 4 channels"):
        metrics.compare_frames(np.zeros((2, 16, 16, 5), np.uint8), np.zeros((2, 16, 16, 5), np.uint8))
    with pytest.raises(ValueError, match="at least 11 x 11.*10 x 16"):
        metrics.compare_frames(a[:, :10], a[:, :10])
    with pytest.raises(ValueError, match="MS-SSIM.*176 x 200"):
        metrics.compare_frames(np.zeros((1, 176, 200, 3), np.uint8), np.zeros((1, 176, 200, 3), np.uint8), ms_ssim=True)
    with pytest.raises(ValueError, match="MS-SSIM.*160 x 192"):
        metrics.ms_ssim(np.zeros((1, 160, 192, 3), np.uint8), np.zeros((1, 160, 192, 3), np.uint8))
    from PIL import Image
    pil = [[Image.fromarray(a[0]), Image.fromarray(a[1])]]
    with pytest.raises(ValueError, match="differ in shape"):
        metrics.compare_frames(pil, a)                                # [1, 2, 16, 16, 3] against [2, 16, 16, 3]


def test_host_arithmetic_on_fabricated_records():
    """_from_records against the restatement's host arithmetic: the records of a 2-video batch written by the reference"""
    from this_and_that_vdm_amd import metrics
    a, b = _noise((2, 2, 20, 22, 3), 10), _noise((2, 2, 20, 22, 3), 11)
    b[1, 0] = a[1, 0]
    rec = np.zeros((1, 4), metrics.REC_DTYPE)
    want = ref.compare(a.reshape(4, 20, 22, 3), b.reshape(4, 20, 22, 3), G)
    for i in range(4):
        r = ref.frame_record(a.reshape(4, 20, 22, 3)[i], b.reshape(4, 20, 22, 3)[i], 255.0, G)
        rec[0, i]["sse"][:3], rec[0, i]["ssim_sum"][:3], rec[0, i]["cs_sum"][:3], rec[0, i]["count"] = r["sse"], r["ssim_sum"], r["cs_sum"], r["count"]
    m = metrics._from_records(rec, a.shape, 255.0)
    assert m.frame_mse.shape == (2, 2) and m.frame_ms_ssim is None and m.ms_ssim is None
    for name in ("mse", "psnr", "ssim", "cs"):
        assert getattr(m, "frame_" + name).ravel().tolist() == want[name], name
        assert np.array_equal(getattr(m, name), getattr(m, "frame_" + name).mean(axis=-1))
    assert m.frame_psnr[1, 0] == math.inf and m.psnr[1] == math.inf and m.frame_ssim[1, 0] == 1.0
    d = m.to_dict()
    assert d["psnr"][1] == "inf" and d["frame_psnr"][1][0] == "inf" and isinstance(d["ssim"][0], float)
    import json
    json.loads(json.dumps(d, allow_nan=False))
