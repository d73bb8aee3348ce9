#!/usr/bin/env python
"""metrics.compare_frames timed: 14 uint8 frames at 256 x 384 and at 576 x 1024 (3 channels), with and without MS-SSIM.

  kernel_us      tt_frame_metrics alone (its two launches) on frames that are on the device, median of --iters between device events
  call_ms        the whole compare_frames call on device tensors: launches, the one device-to-host copy of the records, host fp64
                 (wall clock around a synchronised call, median of --iters)
  cpu_ms         the fp64 numpy restatement (tests/frame_metrics_reference.py) of the same comparison on this machine's CPU, one run, and a
                 scipy.ndimage.gaussian_filter formulation of the same SSIM (the fast way to do it in numpy / scipy), median of 3
  agreement      |device - restatement| of the video's ssim and psnr

A record, not a gate: nobody had measured either side.  The fp64 vector rate the kernel reaches is derived from the operation count
of the header's arithmetic (per window and channel: 11 taps x 5 moments x 2 operations x 2 passes, the horizontal pass once per row of
the tile's 26, + 3 products per tap there + 17 for the formulas), not from a counter.  Prints one JSON line; --out writes it as well."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np
import torch

SIZES = [(14, 256, 384, 3), (14, 576, 1024, 3)]


def events_us(fn, iters):
    for _ in range(3):
        fn()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


def wall_ms(fn, iters):
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def scipy_ssim(a, b):
    """the video's mean SSIM with scipy's separable Gaussian (truncate 3.5 = the same 11 taps), cropped to the valid windows"""
    from scipy.ndimage import gaussian_filter
    a, b = a.astype(np.float64), b.astype(np.float64)
    f = lambda v: gaussian_filter(v, (0, 1.5, 1.5, 0), truncate=3.5)[:, 5:-5, 5:-5]
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    mu_a, mu_b = f(a), f(b)
    saa, sbb, sab = f(a * a) - mu_a * mu_a, f(b * b) - mu_b * mu_b, f(a * b) - mu_a * mu_b
    s = ((2 * mu_a * mu_b + c1) / (mu_a * mu_a + mu_b * mu_b + c1)) * ((2 * sab + c2) / (saa + sbb + c2))
    return float(s.mean(axis=(1, 2, 3)).mean())


def flops(n, h, w, ch, tile=16):
    """fp64 operations of the header's arithmetic as the kernel does it (the horizontal pass covers the 10 halo rows of every tile)"""
    wins = (h - 10) * (w - 10) * ch * n
    halo = (tile + 10) / tile
    return wins * (11 * (5 * 2 + 3) * halo + 11 * 5 * 2 + 17)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy / scipy side")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("frame_metrics_bench: needs a GPU (there is no CPU fallback)")
    from tests import frame_metrics_reference as ref
    from this_and_that_vdm_amd import metrics, ops
    g = ops.frame_metrics_window()
    rows = []
    for shape in SIZES:
        rng = np.random.default_rng(0)
        x = rng.integers(0, 256, shape).astype(np.uint8)
        y = np.clip(x.astype(np.int64) + rng.integers(-12, 13, shape), 0, 255).astype(np.uint8)
        dx, dy = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        kernel = events_us(lambda: ops.frame_metrics(dx, dy), a.iters)
        pool = events_us(lambda: ops.frames_pool2(dx), a.iters)
        row = dict(frames=list(shape), kernel_us=round(kernel, 1), fp64_gflops=round(flops(*shape) / kernel * 1e-3, 1),
                   pool2_us=round(pool, 1),
                   call_ms=round(wall_ms(lambda: metrics.compare_frames(dx, dy), a.iters), 3),
                   call_ms_with_ms_ssim=round(wall_ms(lambda: metrics.compare_frames(dx, dy, ms_ssim=True), a.iters), 3),
                   call_ms_from_numpy=round(wall_ms(lambda: metrics.compare_frames(x, y), a.iters), 3))
        m = metrics.compare_frames(dx, dy, ms_ssim=True)
        row.update(psnr=m.psnr, ssim=m.ssim, ms_ssim=m.ms_ssim)
        if not a.no_cpu:
            t0 = time.perf_counter()
            want = ref.compare(x, y, g)
            row["cpu_ms_restatement"] = round((time.perf_counter() - t0) * 1e3, 1)
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                s = scipy_ssim(x, y)
                ts.append((time.perf_counter() - t0) * 1e3)
            row["cpu_ms_scipy_ssim"] = round(statistics.median(ts), 1)
            row["agreement"] = dict(ssim_vs_restatement=abs(m.ssim - float(np.mean(want["ssim"]))),
                                    psnr_vs_restatement=abs(m.psnr - float(np.mean(want["psnr"]))), ssim_vs_scipy=abs(m.ssim - s))
        rows.append(row)
    res = dict(tool="frame_metrics_bench", device=torch.cuda.get_device_name(0), cpu_threads=torch.get_num_threads(), iters=a.iters,
               inputs="uint8 noise and the same noise + uniform [-12, 12]", rows=rows,
               says="a record, not a gate; fp64_gflops counts the header's operations as the kernel performs them, divided by kernel_us")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
