#!/usr/bin/env python
"""One request's image I/O with the pipelines' ``native_image_io`` option off and on, on one GPU:

  preprocess   PIL image (256 x 384, the reference's default) -> the CLIP vision model's input [1, 3, 224, 224] fp16 on the device
               off: pil_to_numpy + resize_with_antialiasing + CLIPFeatureExtractor on the CPU, then the upload (encode_clip's torch path)
               on:  upload of the uint8 pixels + ops.clip_image
  export       decoded frames [14, 3, 256, 448] fp16 on the device -> the host array the caller receives
               off: decode_latents' permute + float, tensor2vid ("np" and "pil" up to the uint8 array; PIL object construction is the
                    same host work in both paths and is left out)
               on:  ops.frames_out (kind 0 / 1) + one device-to-host copy

Each figure is the median of --iters runs after --warmup, the two paths interleaved in one process.  "wall" is a host clock around the
stage ending in a device synchronise; "device" is the time between two events recorded on the stream before and after the stage (it
includes whatever time the stream spent waiting for the host inside the stage, so for the off paths it is close to the wall clock).
Prints one JSON line.  Needs a GPU: there is no CPU fallback."""
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


def measure(fn, warmup, iters):
    wall, dev = [], []
    for i in range(warmup + iters):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
    return wall, dev


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--image", type=int, nargs=2, default=(256, 384), metavar=("H", "W"))
    ap.add_argument("--frames", type=int, nargs=3, default=(14, 256, 448), metavar=("F", "H", "W"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_io_bench: needs a GPU (a timing taken on the CPU says nothing about this path)")
    from this_and_that_vdm_amd import ops
    from this_and_that_vdm_amd.svd.pipeline_utils import CLIPFeatureExtractor, VaeImageProcessor, resize_with_antialiasing, tensor2vid
    dev = torch.device("cuda:0")
    fe, proc = CLIPFeatureExtractor(), VaeImageProcessor()
    rng = np.random.default_rng(0)
    image = PIL.Image.fromarray(rng.integers(0, 256, (*a.image, 3), dtype=np.uint8))
    f, h, w = a.frames
    decoded = (torch.randn(f, 3, h, w, generator=torch.Generator().manual_seed(0)) * 0.6).to(dev, torch.float16)

    def pre_off():
        x = proc.numpy_to_pt(proc.pil_to_numpy(image))
        x = (resize_with_antialiasing(x * 2.0 - 1.0, (224, 224)) + 1.0) / 2.0
        return fe(images=x).pixel_values.to(device=dev, dtype=torch.float16)

    def pre_on():
        return ops.clip_image(torch.from_numpy(np.array(image)[None]).to(dev), (224, 224), fe.image_mean, fe.image_std, torch.float16)

    def exp_off(kind):
        video = decoded.reshape(1, f, 3, h, w).permute(0, 2, 1, 3, 4).float()
        arr = tensor2vid(video, proc, "np")
        return arr if kind == "np" else (arr * 255).round().astype("uint8")

    def exp_on(kind):
        return ops.frames_out(decoded, 0 if kind == "np" else 1).cpu().numpy()

    assert np.array_equal(exp_off("pil")[0], exp_on("pil")) and np.array_equal(exp_off("np")[0], exp_on("np"))
    stages = {"preprocess_off": pre_off, "preprocess_on": pre_on,
              "export_pil_off": lambda: exp_off("pil"), "export_pil_on": lambda: exp_on("pil"),
              "export_np_off": lambda: exp_off("np"), "export_np_on": lambda: exp_on("np")}
    wall = {k: [] for k in stages}
    devt = {k: [] for k in stages}
    for k, fn in stages.items():                                       # warm-up of every stage first
        measure(fn, a.warmup, 0)
    for _ in range(a.iters):                                           # then interleaved: one run of each per round
        for k, fn in stages.items():
            w_, d_ = measure(fn, 0, 1)
            wall[k] += w_
            devt[k] += d_
    px = f * h * w * 3
    out = {"tool": "image_io_bench", "iters": a.iters, "image": list(a.image), "frames": list(a.frames),
           "wall_ms_median": {k: round(statistics.median(v), 4) for k, v in wall.items()},
           "device_ms_median": {k: round(statistics.median(v), 4) for k, v in devt.items()},
           "wall_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in wall.items()},
           "host_to_device_bytes": {"preprocess_off": 3 * 224 * 224 * 4, "preprocess_on": a.image[0] * a.image[1] * 3},
           "device_to_host_bytes": {"export_pil_off": px * 4, "export_pil_on": px, "export_np_off": px * 4, "export_np_on": px * 4}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
