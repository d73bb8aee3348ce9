#!/usr/bin/env python
"""Range audit of one denoise request on one GPU (this_and_that_vdm_amd/audit.py), and what the audit costs.

  1. Builds the UNet (+ GestureNet with --mode vgl) -- tiny or full size, synthetic hash-filled weights or a diffusers-format
     checkpoint folder (--checkpoint DIR: DIR/unet and, for vgl, DIR/controlnet) -- and runs one request of --steps steps through the
     hipGraph-replayed DenoiseLoop under a RangeAudit.  Prints the verdict table (fp16 / bf16 / split16 / fp8_attention, the first
     non-finite site, the largest magnitudes) and writes the whole report as JSON (--json).
  2. Times the same steps with the audit off and on, in this one process, graphs captured beforehand: device time between two events
     around the --steps replays, median of --iters requests each (the audited requests first: a loop steps only under the audit it
     began under).
  3. Times tt_tensor_stats alone on three bf16 tensors -- 784 x 1280, 50 176 x 320 and 524 288 x 1024 (1 GiB) -- against a device copy
     (torch's copy_) of the same bytes in the same call: median of --iters launches between events.  The statistics pass reads the
     bytes once, the copy reads and writes them; rates are bytes of the tensor per second for the statistics, twice that for the copy.

Magnitudes measured on the synthetic weights say nothing about a trained checkpoint: they show that the instrument runs, and what it
costs.  Prints one JSON line at the end.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

TINY = dict(block_out_channels=(64, 128, 256, 256), num_attention_heads=(1, 2, 4, 4), cross_attention_dim=64)
SIZES = {"tiny": dict(frames=4, h=8, w=16, ctx_tokens=5, ctx_dim=64), "lo": dict(frames=14, h=32, w=56, ctx_tokens=78, ctx_dim=1024)}
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
STATS_SHAPES = [(784, 1280), (50176, 320), (524288, 1024)]
HBM_PEAK = 6.3e12              # bytes / s: the ceiling the kernel guide quotes for MI355X


def build(a, dev):
    from this_and_that_vdm_amd.svd.temporal_controlnet import ControlNetModel
    from this_and_that_vdm_amd.svd.unet_spatio_temporal_condition import UNetSpatioTemporalConditionModel
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    dtype, size = DTYPES[a.dtype], SIZES[a.size]
    if a.checkpoint:
        unet = UNetSpatioTemporalConditionModel.from_pretrained(a.checkpoint, subfolder="unet", torch_dtype=dtype)
        cn = ControlNetModel.from_pretrained(a.checkpoint, subfolder="controlnet", torch_dtype=dtype) if a.mode == "vgl" else None
    else:
        with torch.device(dev):
            kw = dict(TINY) if a.size == "tiny" else dict(num_attention_heads=(5, 10, 20, 20))
            unet = UNetSpatioTemporalConditionModel(num_frames=size["frames"], **kw)
            cn = ControlNetModel(**(kw if a.size == "tiny" else {})) if a.mode == "vgl" else None
        with torch.no_grad():
            fill_parameters_(unet, "unet.")
            if cn is not None:
                fill_parameters_(cn, "controlnet.")
    models = []
    for m in (unet, cn):
        if m is not None:
            m = m.to(device=dev, dtype=dtype).eval()
            if dtype == torch.float32:
                m.compute_dtype = torch.float32
            m.attention_fp8 = a.attn == "fp8"
        models.append(m)
    return models


def request(a, dev):
    from this_and_that_vdm_amd.svd.scheduling_euler_discrete import EulerDiscreteScheduler
    from this_and_that_vdm_amd.utils.synthetic import synthetic_inputs
    s = SIZES[a.size]
    inp = {k: v.to(dev) for k, v in synthetic_inputs(2, s["frames"], s["h"], s["w"], s["ctx_tokens"], s["ctx_dim"], seed=0).items()}
    sched = EulerDiscreteScheduler()
    sched.set_timesteps(a.steps)
    return dict(latents=inp["latents"], image_latents=inp["image_latents"], encoder_hidden_states=inp["encoder_hidden_states"],
                added_time_ids=inp["added_time_ids"], guidance_scale=inp["guidance_scale"], sigmas=sched.sigmas,
                timesteps=sched.timesteps, controlnet_cond=inp["gesture_latents"] if a.mode == "vgl" else None)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats_rates(iters):
    from this_and_that_vdm_amd import ops
    out = []
    for rows, cols in STATS_SHAPES:
        x = torch.randn(rows, cols, device="cuda:0", dtype=torch.bfloat16)
        y, rec = torch.empty_like(x), torch.empty(ops.STATS_BYTES, dtype=torch.uint8, device="cuda:0")
        nbytes = x.numel() * x.element_size()
        for _ in range(3):
            ops.tensor_stats(x, out=rec)
            y.copy_(x)
        ts, tc = [], []
        for _ in range(iters):
            ts.append(timed(lambda: ops.tensor_stats(x, out=rec)))
            tc.append(timed(lambda: y.copy_(x)))
        t_s, t_c = statistics.median(ts), statistics.median(tc)
        r_s, r_c = nbytes / (t_s * 1e-3), 2 * nbytes / (t_c * 1e-3)
        out.append(dict(shape=[rows, cols], bytes=nbytes, stats_us=round(t_s * 1e3, 2), copy_us=round(t_c * 1e3, 2),
                        stats_GBps=round(r_s / 1e9, 1), copy_GBps=round(r_c / 1e9, 1), of_copy_rate=round(r_s / r_c, 3),
                        of_hbm_peak=round(r_s / HBM_PEAK, 3)))
        del x, y
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=list(SIZES), default="tiny", help="tiny models on 8 x 16 latents, or the full-size models on 32 x 56 (256 x 448)")
    ap.add_argument("--mode", choices=["vgl", "vl"], default="vgl")
    ap.add_argument("--dtype", choices=list(DTYPES), default="fp16")
    ap.add_argument("--attn", choices=["bf16", "fp8"], default="bf16", help="fp8: the e4m3 attention operands (16-bit storage only)")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--checkpoint", default=None, help="diffusers-format folder with unet/ (and controlnet/ for --mode vgl)")
    ap.add_argument("--json", default=None, help="write the report (every site's record) here")
    ap.add_argument("--no-stats-bench", action="store_true", help="skip part 3")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("range_audit: needs a GPU (there is no CPU fallback)")
    from this_and_that_vdm_amd import audit
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    dev = torch.device("cuda:0")
    with torch.no_grad():
        unet, cn = build(a, dev)
        kw = request(a, dev)
        plain, audited = DenoiseLoop(unet, cn, use_graph=True), DenoiseLoop(unet, cn, use_graph=True)
        plain.begin(**kw).run()                                   # captures the plain graph
        with audit.RangeAudit() as ra:
            audit.watch(unet, "unet")
            if cn is not None:
                audit.watch(cn, "controlnet")
            audited.begin(**kw).run()                             # captures the audited graph; this request is the report
            rep = ra.report()
            t_off, t_on = [], []
            for _ in range(a.iters):                              # (the plain loop began outside the audit and so refuses to step inside it:
                audited.begin(**kw)                               # the audited requests are timed here, the plain ones below)
                t_on.append(timed(lambda: audited.run()))
        for _ in range(a.iters):
            plain.begin(**kw)
            t_off.append(timed(lambda: plain.run()))
        same = torch.equal(plain.result(), audited.result())
    print(rep.table())
    if a.json:
        with open(a.json, "w") as f:
            f.write(rep.to_json(indent=1))
    written = sum(r["record"]["count"] * {"f32": 4, "f16": 2, "bf16": 2, "e4m3": 1}[r["dtype"]] for r in rep.rows)
    off, on = statistics.median(t_off) / a.steps, statistics.median(t_on) / a.steps
    res = dict(tool="range_audit", size=a.size, mode=a.mode, dtype=a.dtype, attn=a.attn, steps=a.steps, sites=len(rep),
               nonfinite_sites=len(rep.nonfinite()), latents_bit_equal=same, step_ms_audit_off=round(off, 3), step_ms_audit_on=round(on, 3),
               audit_cost=round(on / off, 3), audited_bytes_per_request=written,
               verdicts={s: dict(sites=len(v["sites"]), first=v["first"], flush_share=v["flush_share"])
                         for s, v in ((s, rep.verdict(s)) for s in ("fp16", "bf16", "split16", "fp8_attention"))})
    if not a.no_stats_bench:
        res["tensor_stats"] = stats_rates(max(a.iters, 10))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
