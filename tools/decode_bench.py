#!/usr/bin/env python3
"""decode_latents through the native temporal VAE decoder at the reference's inference setting (14 frames, 256x448 output,
decode_chunk_size = 8 as test_code/inference.py:258 passes): ms per request, next to the 25-step denoise loop it follows.
python tools/decode_bench.py [--dtype bf16|fp16|f32] [--split16] [--chunk 8] [--frames 14] [--size 256x448] [--reps 5] [--wide-ab]
--size HxW: the output size (576x1024 is the pipelines' default; chunks of 8 frames and more then need tt_gemm's wide route).  Times are
medians over --reps requests after two warm-up requests, taken with device events.  --wide-ab: the same request alternately with
tt_gemm_set_wide(1) (narrow kernels wherever no operand reaches 2 GiB) and tt_gemm_set_wide(2) (wide kernels wherever they serve),
interleaved in this one process -- meaningful at a size the narrow route can run."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from this_and_that_vdm_amd import ops
from this_and_that_vdm_amd.svd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
from this_and_that_vdm_amd.utils.synthetic import fill_parameters_

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--chunk", type=int, default=8)
ap.add_argument("--frames", type=int, default=14)
ap.add_argument("--size", default="256x448")
ap.add_argument("--split16", action="store_true")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--wide-ab", action="store_true")
a = ap.parse_args()
height, width = (int(v) for v in a.size.lower().split("x"))
dt = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}[a.dtype]
with torch.device("cuda"):
    vae = AutoencoderKLTemporalDecoder().to(dt).eval()
fill_parameters_(vae, "vae.")
if dt == torch.float32:
    vae.compute_dtype = torch.float32
if a.split16:
    ops.set_f32_split(True)
vae.prepare()
lat = torch.randn(a.frames, 4, height // 8, width // 8, device="cuda")

def decode():
    out = []
    for i in range(0, a.frames, a.chunk):
        out.append(vae.decode(lat[i:i + a.chunk] / vae.config.scaling_factor, num_frames=min(a.chunk, a.frames - i)).sample)
    return torch.cat(out, 0)

def timed(reps):
    """median ms of `reps` requests (device events) and how many of one request's tt_gemm launches ran wide"""
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n0 = ops.WIDE_LAUNCHES
        e0.record()
        y = decode()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
        wide = ops.WIDE_LAUNCHES - n0
    return sorted(ms)[len(ms) // 2], wide, y


for _ in range(2):
    y = decode()
torch.cuda.synchronize()
ops.PROFILE = []
decode()
torch.cuda.synchronize()
rec, ops.PROFILE = ops.PROFILE, None
flops = sum(r[1] for r in rec)
mode = a.dtype + (" split16" if a.split16 else "")
if a.wide_ab:
    res = {1: [], 2: []}
    for _ in range(a.reps):
        for knob in (1, 2):
            ops.set_gemm_wide(knob)
            ms, wide, y = timed(1)
            res[knob].append((ms, wide))
    ops.set_gemm_wide(1)
    for knob in (1, 2):
        ms = sorted(v[0] for v in res[knob])[len(res[knob]) // 2]
        print(f"temporal VAE decode, {a.frames} frames -> {tuple(y.shape)}, {mode}, chunks of {a.chunk}, tt_gemm_set_wide({knob}): {ms:.1f} ms per "
              f"request, median of {a.reps} interleaved ({res[knob][0][1]} of {len(rec)} tt_gemm launches wide; {flops / 1e12:.2f} TFLOP = "
              f"{flops / (ms * 1e-3) / 1e12:.0f} TFLOP/s)")
else:
    ms, wide, y = timed(a.reps)
    print(f"temporal VAE decode, {a.frames} frames -> {tuple(y.shape)}, {mode}, chunks of {a.chunk}: {ms:.1f} ms per request, median of {a.reps} "
          f"({wide} of {len(rec)} tt_gemm launches wide; {flops / 1e12:.2f} TFLOP in tt_gemm launches = {flops / (ms * 1e-3) / 1e12:.0f} TFLOP/s), "
          f"finite {bool(torch.isfinite(y).all())}")
