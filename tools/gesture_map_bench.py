#!/usr/bin/env python
"""The gesture-map stage of one VGL request, host against device, on one GPU:

  host     gesture_map.rasterise_points (numpy: a canvas of the ORIGINAL image size per point, 2 x 99 shifted adds, two dense resize
           einsums) + the pipeline's prepare_condition_image (fp32 -> fp16, upload): what a caller of get_thisthat_sam pays today
  device   gesture_map.rasterise_points_device straight to fp16 (tt_gesture_maps: two launches, the points travel as kernel arguments)

for 640 x 480 -> 256 x 384 and 1920 x 1080 -> 256 x 448, 14 frames, two points each.  The host path is timed with a wall clock ending
in a device synchronise (--host-iters runs, median); the device path with two events on the stream (median of --iters after --warmup)
and with a wall clock around a synchronise.  Also reports the largest |device - host| of the fp32 frames.  Writes one JSON line to
stdout and to profiles/gesture_map_bench.json.  Needs a GPU: there is no CPU fallback."""
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

SHAPES = {"640x480_to_256x384": ((480, 640), (256, 384)), "1920x1080_to_256x448": ((1080, 1920), (256, 448))}
FRAMES = 14


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gesture_map_bench.json"))
    a = ap.parse_args()
    from this_and_that_vdm_amd import gesture_map as gm

    def to_device(cond):           # prepare_condition_image (svd/pipeline_stable_video_diffusion_controlnet.py)
        return torch.from_numpy(cond).to(torch.float16).to("cuda")

    res = {"tool": "gesture_map_bench", "device": torch.cuda.get_device_name(0), "frames": FRAMES, "points": 2, "shapes": {}}
    for name, (org, out) in SHAPES.items():
        pts = ((0, org[1] * 0.3, org[0] * 0.4), (FRAMES - 1, org[1] * 0.7, org[0] * 0.55))
        gp = gm.GesturePoints(pts, org)
        host_ms = []
        for _ in range(max(1, a.host_iters)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cond, _, _ = gm.rasterise_points(pts, org, out[0], out[1], FRAMES)
            ref16 = to_device(cond)
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        wall, dev = [], []
        for i in range(a.warmup + a.iters):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            got16 = gm.rasterise_points_device(gp, out[0], out[1], FRAMES, "cuda", torch.float16)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                wall.append((t1 - t0) * 1e3)
                dev.append(e0.elapsed_time(e1))
        got32 = gm.rasterise_points_device(gp, out[0], out[1], FRAMES, "cuda")
        res["shapes"][name] = {
            "host_wall_ms": statistics.median(host_ms), "device_event_ms": statistics.median(dev), "device_wall_ms": statistics.median(wall),
            "out_bytes_fp16": got16.numel() * 2,
            "max_abs_err_fp32_vs_host": float(np.abs(got32.cpu().numpy().astype(np.float64) - cond).max()),
            "max_abs_diff_fp16_vs_host_fp16": float((got16.float() - ref16.float()).abs().max()),
        }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
