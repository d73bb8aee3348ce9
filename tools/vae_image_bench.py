#!/usr/bin/env python
"""One request's VAE-input stage with the pipelines' ``native_image_io`` option off and on, on one GPU, for two shapes
(640 x 480 -> 256 x 384 and 1920 x 1080 -> 256 x 448, width x height -> height x width of the request):

  off   VaeImageProcessor.preprocess (PIL LANCZOS resize, / 255, 2 x - 1) + noise_aug_strength * noise on the host, then .to(fp16) and
        the upload of the result -- what _generate does with the option off
  on    the upload of the uint8 pixels, then ops.vae_image (resize, normalise, add the noise, write fp16) on the device

The noise is drawn once, outside the timed region, in both paths: a CPU generator's draw is the same host work either way.  Each path
is split into its parts -- ``*_compute`` (off: the host arithmetic; on: the kernels, tables cached) and ``*_upload`` (off: the fp16 image;
on: the uint8 pixels and the fp32 noise a CPU generator drew; a device generator's noise needs no upload) -- and timed as a whole.
Each figure is the median of --iters runs after --warmup, the paths interleaved in one process.  "wall" is a host clock around the stage
ending in a device synchronise; "device" is the time between two events recorded on the stream before and after it.  The two paths'
results are compared bit for bit before anything is timed.  Prints one JSON line.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import PIL.Image
import torch

SHAPES = [((480, 640), (256, 384)), ((1080, 1920), (256, 448))]          # (H, W) of the image -> (height, width) of the request


def measure(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--noise-aug-strength", type=float, default=0.02)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_image_bench: needs a GPU (a timing taken on the CPU says nothing about this path)")
    from this_and_that_vdm_amd import ops
    from this_and_that_vdm_amd.svd.pipeline_utils import VaeImageProcessor, upload_pixels
    dev = torch.device("cuda:0")
    proc = VaeImageProcessor(do_convert_rgb=True)
    na = a.noise_aug_strength
    results = {}
    for (ih, iw), (h, w) in SHAPES:
        image = PIL.Image.fromarray(np.random.default_rng(0).integers(0, 256, (ih, iw, 3), dtype=np.uint8))
        noise = torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(0))
        noise_dev = noise.to(dev)
        pixels = upload_pixels(np.array(image)[None], dev)
        host = {}

        def off_compute():
            host["img"] = (proc.preprocess(image, height=h, width=w) + na * noise).to(torch.float16)

        def off_upload():
            return host["img"].to(dev)

        def off():
            off_compute()
            return off_upload()

        def on_upload():
            return upload_pixels(np.array(image)[None], dev), noise.to(dev)

        def on_compute():
            return ops.vae_image(pixels, (h, w), noise_dev, na, torch.float16)

        def on():
            px, nz = on_upload()
            return ops.vae_image(px, (h, w), nz, na, torch.float16)

        def on_device_noise():                                         # a device generator's request: only the pixels travel
            return ops.vae_image(upload_pixels(np.array(image)[None], dev), (h, w), noise_dev, na, torch.float16)

        assert torch.equal(off().view(torch.int16), on().view(torch.int16)), "the two paths disagree"
        stages = {"off": off, "off_compute": off_compute, "off_upload": off_upload, "on": on, "on_upload": on_upload,
                  "on_compute": on_compute, "on_device_noise": on_device_noise}
        wall = {k: [] for k in stages}
        devt = {k: [] for k in stages}
        for _ in range(a.warmup):
            for fn in stages.values():
                measure(fn)
        for _ in range(a.iters):                                       # interleaved: one run of each per round
            for k, fn in stages.items():
                w_, d_ = measure(fn)
                wall[k].append(w_)
                devt[k].append(d_)
        results[f"{iw}x{ih}->{h}x{w}"] = {
            "wall_ms_median": {k: round(statistics.median(v), 4) for k, v in wall.items()},
            "device_ms_median": {k: round(statistics.median(v), 4) for k, v in devt.items()},
            "wall_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in wall.items()},
            "host_to_device_bytes": {"off": 3 * h * w * 2, "on": ih * iw * 3 + 3 * h * w * 4, "on_device_noise": ih * iw * 3}}
    print(json.dumps({"tool": "vae_image_bench", "iters": a.iters, "noise_aug_strength": na, "dtype": "float16", "shapes": results}))


if __name__ == "__main__":
    main()
