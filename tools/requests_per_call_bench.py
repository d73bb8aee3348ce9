#!/usr/bin/env python3
"""What R requests in ONE DenoiseLoop cost per request: VGL at 14x4x32x56 latents, bf16, CFG 2, hipGraph replay (bench.py's headline
workload with latents [R,14,4,32,56]).  For R in --requests: the median of three windows of 25 steps (a begin() inside every window, as
bench.py times it) -> ms/step, ms/step/request, aggregate denoise-steps/s (one "step" = one loop iteration of ONE request).

    python tools/requests_per_call_bench.py --yardstick PARENT_LINE.json [--requests 1 2 4] [--out profiles/requests_per_call.json]

The yardstick is NOT this script's own R = 1 figure: it is the headline of `python bench.py` of the commit this feature was added to,
run in the same session on the same card, handed over as the file holding its JSON line (--yardstick).  Without it the ratios are null.
Report only: nothing here gates anything."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402  (model construction, latent sizes and the kernel-source hash are bench.py's)

WINDOWS, STEPS = 3, 25


def request_set(nreq, h, w, device):
    """R seeded requests in the loop's batch order (class by class: all uncond first)"""
    from this_and_that_vdm_amd.svd.scheduling_euler_discrete import EulerDiscreteScheduler
    from this_and_that_vdm_amd.utils.synthetic import synthetic_inputs
    reqs = [synthetic_inputs(2, bench.FRAMES, h, w, bench.CTX_TOKENS, bench.CTX_DIM, seed=r) for r in range(nreq)]
    by_class = lambda k: torch.cat([r[k][c:c + 1] for c in range(2) for r in reqs]).to(device)
    sched = EulerDiscreteScheduler()
    sched.set_timesteps(bench.STEPS_PER_REQUEST)
    return dict(latents=torch.cat([r["latents"] for r in reqs]).to(device), image_latents=by_class("image_latents"),
                encoder_hidden_states=by_class("encoder_hidden_states"), added_time_ids=by_class("added_time_ids"),
                guidance_scale=reqs[0]["guidance_scale"].to(device), sigmas=sched.sigmas, timesteps=sched.timesteps,
                controlnet_cond=torch.stack([r["gesture_latents"] for r in reqs]).to(device))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--requests", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--yardstick", default=None, help="file holding the JSON line of the parent commit's `python bench.py`")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "requests_per_call.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (the denoise path has no CPU fallback)")
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    device = torch.device("cuda", 0)
    h, w = bench.LATENT["lo"]
    unet, cn, _, _ = bench.build_models("vgl", torch.bfloat16, device, 0, 1)
    yard = None
    if a.yardstick:
        lines = [ln for ln in open(a.yardstick).read().splitlines() if ln.startswith("{")]
        y = json.loads(lines[-1])
        yard = {"ms_per_step": y["ms_per_step"], "value": y["value"], "steps": y["steps"], "warmup": y["warmup"],
                "kernel_source_sha16": y["config"].get("kernel_source_sha16"), "what": "`python bench.py` of the parent commit, same session, same card"}
    rows = []
    for nreq in a.requests:
        args = request_set(nreq, h, w, device)
        loop = DenoiseLoop(unet, cn, use_graph=True).begin(**args)
        bench.advance(loop, args, a.warmup)
        windows = []
        for _ in range(WINDOWS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bench.advance(loop, args, STEPS, fresh=True)
            torch.cuda.synchronize()
            windows.append((time.perf_counter() - t0) / STEPS * 1e3)
        ms = sorted(windows)[WINDOWS // 2]
        row = {"requests": nreq, "ms_per_step": ms, "ms_per_step_per_request": ms / nreq, "denoise_steps_per_s": nreq * 1e3 / ms,
               "ms_per_step_windows": windows, "finite_output": bool(torch.isfinite(loop.result()).all().item()),
               "per_request_vs_yardstick": (yard["ms_per_step"] / (ms / nreq)) if yard else None}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del loop
    out = {"workload": f"VGL denoise step, latents [R,{bench.FRAMES},4,{h},{w}], CFG 2, {bench.CTX_TOKENS} context tokens, bf16, hipGraph replay; "
                       f"median of {WINDOWS} windows of {STEPS} steps, one begin() per window",
           "yardstick": yard, "per_request_vs_yardstick_is": "yardstick ms/step divided by this row's ms/step/request (> 1: a request is cheaper "
           "inside a batched call than alone on the parent commit)", "rows": rows, "kernel_source_sha16": bench.csrc_hash()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out, "yardstick_ms_per_step": yard and yard["ms_per_step"]}))


if __name__ == "__main__":
    main()
