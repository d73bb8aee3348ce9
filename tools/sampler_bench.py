#!/usr/bin/env python
"""The two samplers of the fused denoise loop side by side: Euler and DPM-Solver++ 2M (DenoiseLoop.begin(multistep=...)).

  (a) Cost (default).  VGL at 14 x 4 x 32 x 56 latents, bf16, CFG 2, hipGraph replay -- bench.py's headline workload -- with both
      loops in ONE process on the same models: after a warm-up, an Euler window and a 2M window alternately, three of each, 25 steps
      per window with the request's begin() inside it, device time between two events.  And the step kernel of each sampler alone
      on the loop's shapes (median of --iters launches between events).  Prints one JSON line; --out writes it to a file as well.
  (b) Solver accuracy (--accuracy tiny | full, or --checkpoint DIR).  In a reference-precision mode (--dtype f32: TT_F32, or split16),
      one request from one noise tensor: Euler at 25 steps and 2M at 12, 15, 20 and 25 steps, each against a 2M run of 200 steps.
      Reports the relative L2 distance of every candidate's final latents to that fine-step run, and next to it the distance in
      PICTURE space: every candidate's final latents and the fine-step solve's are decoded by the native AutoencoderKLTemporalDecoder
      (synthetic fill, or the checkpoint's vae/), exported with ops.frames_out(kind=1), and compared with metrics.compare_frames: psnr,
      ssim and ms_ssim (null where the frames are smaller than MS-SSIM's 176 pixels) to the fine-step video.  A report, not an assertion.

What (b) measures on synthetic (hash-filled) weights is how fast each solver converges on THAT network's ODE: solver accuracy only.  It
says nothing about pictures -- the picture-space columns included: a hash-filled decoder maps latents to noise-like frames, so they
restate the solver's error through another synthetic network.  Nobody has evaluated picture quality at fewer steps on trained This&That weights; the output of (b) says
so unless it ran on a checkpoint.  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch

TINY = dict(block_out_channels=(64, 128, 256, 256), num_attention_heads=(1, 2, 4, 4), cross_attention_dim=64)
SIZES = {"tiny": dict(frames=4, h=8, w=16, ctx_tokens=5, ctx_dim=64), "full": dict(frames=14, h=32, w=56, ctx_tokens=78, ctx_dim=1024)}
WINDOWS, STEPS = 3, 25
CANDIDATES = [("euler", 25), ("2m", 12), ("2m", 15), ("2m", 20), ("2m", 25)]
FINE_STEPS = 200


def scheduler(name):
    from this_and_that_vdm_amd.svd import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    return DPMSolverMultistepScheduler() if name == "2m" else EulerDiscreteScheduler()


def begin_args(inp, name, steps, with_cn):
    s = scheduler(name)
    s.set_timesteps(steps)
    kw = dict(latents=inp["latents"], image_latents=inp["image_latents"], encoder_hidden_states=inp["encoder_hidden_states"],
              added_time_ids=inp["added_time_ids"], guidance_scale=inp["guidance_scale"], sigmas=s.sigmas, timesteps=s.timesteps,
              controlnet_cond=inp["gesture_latents"] if with_cn else None)
    if name == "2m":
        kw["multistep"] = s.multistep_coefficients
    return kw


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def step_kernel_us(loop, iters):
    """the sampler's own launch, alone on the chip, on copies of the loop's buffers (eps: what conv_out writes, [B*F*h*w, 4] fp32)"""
    from this_and_that_vdm_amd import ops
    g = loop.geom
    eps = torch.randn(g.m, 4, dtype=torch.float32, device=loop.latents.device)
    lat = loop.latents.clone()
    if loop.x0_hist is not None:
        hist = loop.x0_hist.clone()
        coef = loop.coef_tab[1:2].clone()                        # a second-order step: the history is read
        fn = lambda: ops.cfg_multistep_step_requests(eps, lat, hist, loop.guidance, loop.cur, 0, coef, g.requests, g.cfg, g.frames, g.h,
                                                     g.w, loop.image_guidance_scale)
    else:
        fn = lambda: ops.cfg_euler_step(eps, lat, loop.guidance, loop.cur, 0, g.batch, g.frames, g.h, g.w, loop.image_guidance_scale)
    for _ in range(5):
        fn()
    return statistics.median(timed(fn) for _ in range(iters)) * 1e3


def cost(a, dev):
    import bench
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    from this_and_that_vdm_amd.utils.synthetic import synthetic_inputs
    h, w = bench.LATENT["lo"]
    unet, cn, _, _ = bench.build_models("vgl", torch.bfloat16, dev, 0, 1)
    inp = {k: v.to(dev) for k, v in synthetic_inputs(2, bench.FRAMES, h, w, bench.CTX_TOKENS, bench.CTX_DIM, seed=0).items()}
    names = ("euler", "2m")
    loops = {n: DenoiseLoop(unet, cn, use_graph=True) for n in names}
    args = {n: begin_args(inp, n, STEPS, True) for n in names}
    for n in names:
        loops[n].begin(**args[n])
        bench.advance(loops[n], args[n], a.warmup)
    torch.cuda.synchronize()
    windows = {n: [] for n in names}
    for _ in range(WINDOWS):
        for n in names:                                           # alternately: both samplers see the same clocks and neighbours
            windows[n].append(timed(lambda: bench.advance(loops[n], args[n], STEPS, fresh=True)) / STEPS)
    kernel = {n: round(step_kernel_us(loops[n], a.iters), 2) for n in names}
    med = {n: statistics.median(windows[n]) for n in names}
    spread = max(windows["euler"]) - min(windows["euler"])
    return dict(tool="sampler_bench", part="cost",
                workload=f"VGL denoise step, latents [1,{bench.FRAMES},4,{h},{w}], CFG 2, {bench.CTX_TOKENS} context tokens, bf16, hipGraph "
                         f"replay; {WINDOWS} windows of {STEPS} steps per sampler, alternating, one begin() per window, device events",
                ms_per_step_euler=round(med["euler"], 4), ms_per_step_2m=round(med["2m"], 4),
                ms_per_step_windows_euler=[round(v, 4) for v in windows["euler"]], ms_per_step_windows_2m=[round(v, 4) for v in windows["2m"]],
                euler_window_spread_ms=round(spread, 4), delta_2m_minus_euler_ms=round(med["2m"] - med["euler"], 4),
                within_euler_spread=bool(med["2m"] - med["euler"] <= spread),
                step_kernel_us_euler=kernel["euler"], step_kernel_us_2m=kernel["2m"],
                finite_output=bool(torch.isfinite(loops["2m"].result()).all().item()), kernel_source_sha16=bench.csrc_hash())


def decoded_frames(vae, latents, chunk=7):
    """final latents [1, F, 4, h, w] -> uint8 NHWC frames [F, 8h, 8w, 3] on the device, as the pipelines' "pil" output holds them"""
    from this_and_that_vdm_amd import ops
    lat = latents[0].to(torch.float32) / vae.config.scaling_factor
    return torch.cat([ops.frames_out(vae.decode(lat[i:i + chunk], num_frames=min(chunk, lat.shape[0] - i)).sample, 1)
                      for i in range(0, lat.shape[0], chunk)], 0)


def accuracy(a, dev):
    from this_and_that_vdm_amd import metrics, ops
    from this_and_that_vdm_amd.svd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    from this_and_that_vdm_amd.svd.temporal_controlnet import ControlNetModel
    from this_and_that_vdm_amd.svd.unet_spatio_temporal_condition import UNetSpatioTemporalConditionModel
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_, synthetic_inputs
    size = SIZES["full" if a.checkpoint else a.accuracy]
    if a.checkpoint:
        unet = UNetSpatioTemporalConditionModel.from_pretrained(a.checkpoint, subfolder="unet", torch_dtype=torch.float32)
        cn = ControlNetModel.from_pretrained(a.checkpoint, subfolder="controlnet", torch_dtype=torch.float32)
        vae = AutoencoderKLTemporalDecoder.from_pretrained(a.checkpoint, subfolder="vae", torch_dtype=torch.float32)
    else:
        with torch.device(dev):
            kw = dict(TINY) if a.accuracy == "tiny" else dict(num_attention_heads=(5, 10, 20, 20))
            unet = UNetSpatioTemporalConditionModel(num_frames=size["frames"], **kw)
            cn = ControlNetModel(**(kw if a.accuracy == "tiny" else {}))
            vae = AutoencoderKLTemporalDecoder()
        fill_parameters_(unet, "unet.")
        fill_parameters_(cn, "controlnet.")
        fill_parameters_(vae, "vae.")
    for m in (unet, cn, vae):
        m.to(device=dev, dtype=torch.float32).eval()
        m.compute_dtype = torch.float32                           # TT_F32: exact-fp32 products, or split16 below
    was = ops.f32_split()
    ops.set_f32_split(a.dtype == "split16")
    try:
        inp = {k: v.to(dev) for k, v in synthetic_inputs(2, size["frames"], size["h"], size["w"], size["ctx_tokens"], size["ctx_dim"],
                                                         seed=a.seed).items()}
        run = lambda name, steps: DenoiseLoop(unet, cn, use_graph=True).begin(**begin_args(inp, name, steps, True)).run().double().clone()
        fine = run("2m", FINE_STEPS)
        fine_frames = decoded_frames(vae, fine)
        ms_ok = all(v % 16 == 0 and v >= metrics.MS_SSIM_MIN_SIZE for v in fine_frames.shape[1:3])
        rows = []
        for name, steps in CANDIDATES:
            got = run(name, steps)
            pic = metrics.compare_frames(decoded_frames(vae, got), fine_frames, ms_ssim=ms_ok)
            rows.append(dict(sampler=name, steps=steps, rel_l2_to_fine=float((got - fine).norm() / fine.norm()),
                             psnr_to_fine=pic.to_dict()["psnr"], ssim_to_fine=pic.ssim, ms_ssim_to_fine=pic.to_dict()["ms_ssim"],
                             finite=bool(torch.isfinite(got).all().item())))
    finally:
        ops.set_f32_split(was)
    weights = f"checkpoint {a.checkpoint}" if a.checkpoint else f"synthetic ({a.accuracy})"
    return dict(tool="sampler_bench", part="accuracy", weights=weights, mode="TT_F32 " + ("split16" if a.dtype == "split16" else "exact fp32"),
                latents=[1, size["frames"], 4, size["h"], size["w"]], frames=list(fine_frames.shape),
                reference=f"2M at {FINE_STEPS} steps on the same noise", rows=rows,
                picture_columns="psnr / ssim / ms_ssim of the decoded uint8 frames (native temporal VAE decoder in the same TT_F32 mode, "
                                "ops.frames_out(kind=1), metrics.compare_frames) to the fine-step solve's decoded frames" + (
                                    "" if ms_ok else "; ms_ssim null: the frames are smaller than its 176 pixels"),
                says="distance of the final latents, and of the frames decoded from them, to a fine-step solve of the same ODE" + (
                    "" if a.checkpoint else ": synthetic weights (UNet, ControlNet and decoder), solver accuracy only -- nothing about picture "
                                            "quality, which nobody has evaluated at fewer steps on trained weights"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--accuracy", choices=["tiny", "full"], default=None, help="part (b) on synthetic weights of this size instead of part (a)")
    ap.add_argument("--checkpoint", default=None, help="part (b) on a diffusers-format folder with unet/ and controlnet/")
    ap.add_argument("--dtype", choices=["f32", "split16"], default="split16", help="part (b): the TT_F32 product mode")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50, help="part (a): launches of each step kernel timed alone")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench: needs a GPU (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        res = accuracy(a, dev) if (a.accuracy or a.checkpoint) else cost(a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
