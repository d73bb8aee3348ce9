"""fp64 numpy restatement of tt_frame_metrics / tt_frames_pool2 (include/ttvdm.h) and of the host arithmetic of
this_and_that_vdm_amd/metrics.py: direct separable sums over the "valid" windows in the header's operation order (numpy does not
fuse a product into a sum), the definitions of cs and ssim operation by operation, the fp32 2 x 2 mean, and the MS-SSIM combination.
The sums over windows are math.fsum -- correctly rounded -- so a test's bound needs to cover only the kernel's summation order.

Every function takes the 11 window weights `g`; window() restates how the library forms them, and the GPU tests hand both sides the
library's own 11 doubles."""
import math

import numpy as np

WIN = 11
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def window():
    """exp(-(k - 5)^2 / 4.5) / S, S the sum in index order"""
    e = [math.exp(-float((k - 5) * (k - 5)) / 4.5) for k in range(WIN)]
    s = 0.0
    for v in e:
        s += v
    return [v / s for v in e]


def filter_valid(v, g):
    """G*v of a 2-D fp64 array at the (H - 10) x (W - 10) valid windows: rows first, each sum left to right from its first product"""
    h, w = v.shape
    row = g[0] * v[:, 0:w - 10]
    for k in range(1, WIN):
        row = row + g[k] * v[:, k:k + w - 10]
    out = g[0] * row[0:h - 10, :]
    for k in range(1, WIN):
        out = out + g[k] * row[k:k + h - 10, :]
    return out


def ssim_maps(a, b, data_range, g):
    """(ssim, cs, parts) per window of two 2-D arrays; parts holds the denominators the error bound of the GPU test needs"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    c1, c2 = (0.01 * data_range) * (0.01 * data_range), (0.03 * data_range) * (0.03 * data_range)
    mu_a, mu_b = filter_valid(a, g), filter_valid(b, g)
    e_aa, e_ab, e_bb = filter_valid(a * a, g), filter_valid(a * b, g), filter_valid(b * b, g)
    maa, mbb, mab = mu_a * mu_a, mu_b * mu_b, mu_a * mu_b
    saa, sbb, sab = e_aa - maa, e_bb - mbb, e_ab - mab
    cs_den = (saa + sbb) + c2
    cs = (2.0 * sab + c2) / cs_den
    lum_den = (maa + mbb) + c1
    lum = (2.0 * mab + c1) / lum_den
    return lum * cs, cs, dict(cs_den=cs_den, lum_den=lum_den, lum=lum)


def frame_record(a, b, data_range, g, sse_only=False):
    """one frame pair [H, W, C] -> dict(sse, ssim_sum, cs_sum: lists per channel; count; maps: per channel (ssim, cs, parts))"""
    h, w, ch = a.shape
    rec = dict(sse=[], ssim_sum=[], cs_sum=[], count=0 if sse_only else (h - 10) * (w - 10), maps=[])
    for c in range(ch):
        if a.dtype == np.uint8:
            d = a[..., c].astype(np.int64) - b[..., c].astype(np.int64)
            rec["sse"].append(int((d * d).sum()))                     # the exact integer
        else:
            d = a[..., c].astype(np.float64) - b[..., c].astype(np.float64)
            rec["sse"].append(math.fsum((d * d).ravel()))
        if sse_only:
            rec["ssim_sum"].append(0.0)
            rec["cs_sum"].append(0.0)
            continue
        s, cs, parts = ssim_maps(a[..., c], b[..., c], data_range, g)
        rec["ssim_sum"].append(math.fsum(s.ravel()))
        rec["cs_sum"].append(math.fsum(cs.ravel()))
        rec["maps"].append((s, cs, parts))
    return rec


def pool2(x):
    """[N, H, W, C] uint8 or fp32 -> fp32 [N, H / 2, W / 2, C]: 0.25f * ((x00 + x01) + (x10 + x11)), every operation in fp32"""
    x = x.astype(np.float32)
    top = x[:, 0::2, 0::2] + x[:, 0::2, 1::2]
    bot = x[:, 1::2, 0::2] + x[:, 1::2, 1::2]
    return (np.float32(0.25) * (top + bot)).astype(np.float32)


def frame_means(rec, ch):
    """(mse numerator aside) the frame's mean ssim and cs: channel sums in index order, divided by count * ch"""
    n = float(rec["count"]) * ch
    return float(np.sum(np.array(rec["ssim_sum"][:ch]))) / n, float(np.sum(np.array(rec["cs_sum"][:ch]))) / n


def ms_ssim_combine(cs_means, ssim5):
    """prod cs_j^w_j (scales 1-4) * ssim_5^w_5; nan when a base is negative (the power is undefined; nothing is clamped)"""
    with np.errstate(invalid="ignore"):
        ms = np.float64(1.0)
        for lvl in range(4):
            ms = ms * np.power(np.float64(cs_means[lvl]), MS_SSIM_WEIGHTS[lvl])
        return float(ms * np.power(np.float64(ssim5), MS_SSIM_WEIGHTS[4]))


def compare(a, b, g, ms_ssim=False):
    """what metrics.compare_frames returns for [F, H, W, C] arrays, per frame: dict of lists mse, psnr, ssim, cs (, ms_ssim, and the
    per-scale means `scales`: [F][5] of (ssim, cs))"""
    data_range = 255.0 if a.dtype == np.uint8 else 1.0
    f, h, w, ch = a.shape
    out = dict(mse=[], psnr=[], ssim=[], cs=[], ms_ssim=[], scales=[])
    la, lb = [a], [b]
    if ms_ssim:
        for _ in range(4):
            la.append(pool2(la[-1]))
            lb.append(pool2(lb[-1]))
    for i in range(f):
        rec = frame_record(a[i], b[i], data_range, g)
        mse = float(np.sum(np.array(rec["sse"], dtype=np.float64))) / float(h * w * ch)
        out["mse"].append(mse)
        out["psnr"].append(math.inf if mse == 0.0 else 10.0 * math.log10(data_range * data_range / mse))
        s, cs = frame_means(rec, ch)
        out["ssim"].append(s)
        out["cs"].append(cs)
        if ms_ssim:
            scales = [(s, cs)] + [frame_means(frame_record(la[l][i], lb[l][i], data_range, g), ch) for l in range(1, 5)]
            out["scales"].append(scales)
            out["ms_ssim"].append(ms_ssim_combine([sc[1] for sc in scales[:4]], scales[4][0]))
    return out
