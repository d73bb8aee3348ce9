#!/usr/bin/env python
"""What each precision mode's error amounts to in the decoded frames: ONE request (same noise, same sampler, same steps) run in exact
TT_F32 and in split16, fp16, bf16 and bf16 + fp8 attention; every mode's final latents decoded by the native temporal VAE decoder in
that mode's own precision, exported with ops.frames_out(kind=1), and compared with metrics.compare_frames against the exact mode's
video: PSNR / SSIM / MS-SSIM per mode, next to the relative L2 of the latents that VERDICT.md quotes.  A second line per mode decodes the
EXACT mode's latents with that mode's decoder: the decoder's own share.

  python tools/quality_compare.py [--size tiny|lo] [--checkpoint DIR] [--steps 25] [--sampler euler|2m] [--out profiles/quality_compare.json]

Weights: the synthetic fill of utils/synthetic.py (fp32 values, cast to the mode's storage type), or --checkpoint DIR (a diffusers-format
folder with unet/, controlnet/ and vae/).  On synthetic weights the frames are noise-like pictures of a hash-filled network: the numbers
say how far a mode's arithmetic moves THOSE frames, not how a trained model's pictures would look; the output says so.  Needs a GPU."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch

TINY = dict(block_out_channels=(64, 128, 256, 256), num_attention_heads=(1, 2, 4, 4), cross_attention_dim=64)
SIZES = {"tiny": dict(frames=4, h=8, w=16, ctx_tokens=5, ctx_dim=64), "lo": dict(frames=14, h=32, w=56, ctx_tokens=78, ctx_dim=1024)}
# name -> (storage dtype, split16, fp8 attention)
MODES = {"f32": (torch.float32, False, False), "split16": (torch.float32, True, False), "fp16": (torch.float16, False, False),
         "bf16": (torch.bfloat16, False, False), "bf16+fp8attn": (torch.bfloat16, False, True)}


def build(a, size, dev):
    """fp32 masters of the three models (filled or loaded once); every mode runs on a cast copy of them"""
    from this_and_that_vdm_amd.svd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
    from this_and_that_vdm_amd.svd.temporal_controlnet import ControlNetModel
    from this_and_that_vdm_amd.svd.unet_spatio_temporal_condition import UNetSpatioTemporalConditionModel
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    if a.checkpoint:
        return (UNetSpatioTemporalConditionModel.from_pretrained(a.checkpoint, subfolder="unet", torch_dtype=torch.float32).to(dev),
                ControlNetModel.from_pretrained(a.checkpoint, subfolder="controlnet", torch_dtype=torch.float32).to(dev),
                AutoencoderKLTemporalDecoder.from_pretrained(a.checkpoint, subfolder="vae", torch_dtype=torch.float32).to(dev))
    with torch.device(dev):
        kw = dict(TINY) if a.size == "tiny" else dict(num_attention_heads=(5, 10, 20, 20))
        unet = UNetSpatioTemporalConditionModel(num_frames=size["frames"], **kw)
        cn = ControlNetModel(**(kw if a.size == "tiny" else {}))
        vae = AutoencoderKLTemporalDecoder()
    for salt, m in (("unet.", unet), ("controlnet.", cn), ("vae.", vae)):
        fill_parameters_(m, salt)
    return unet, cn, vae


def decoded_frames(vae, latents, chunk=7):
    """final latents [1, F, 4, h, w] -> uint8 NHWC frames [F, 8h, 8w, 3] on the device, as the pipelines' "pil" output holds them"""
    from this_and_that_vdm_amd import ops
    lat = latents[0].to(next(vae.parameters()).dtype) / vae.config.scaling_factor
    return torch.cat([ops.frames_out(vae.decode(lat[i:i + chunk], num_frames=min(chunk, lat.shape[0] - i)).sample, 1)
                      for i in range(0, lat.shape[0], chunk)], 0)


def run_mode(name, masters, inp, a):
    """-> (final latents fp64, that mode's decoder).  The models of a mode are dropped when the next one is built."""
    import copy
    from this_and_that_vdm_amd import ops
    from this_and_that_vdm_amd.svd import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    dtype, split, fp8 = MODES[name]
    ops.set_f32_split(split)
    unet, cn, vae = (copy.deepcopy(m).to(dtype).eval() for m in masters)
    for m in (unet, cn, vae):
        if dtype == torch.float32:
            m.compute_dtype = torch.float32
    for m in (unet, cn):
        m.attention_fp8 = fp8
    s = DPMSolverMultistepScheduler() if a.sampler == "2m" else EulerDiscreteScheduler()
    s.set_timesteps(a.steps)
    kw = dict(latents=inp["latents"], image_latents=inp["image_latents"], encoder_hidden_states=inp["encoder_hidden_states"],
              added_time_ids=inp["added_time_ids"], guidance_scale=inp["guidance_scale"], sigmas=s.sigmas, timesteps=s.timesteps,
              controlnet_cond=inp["gesture_latents"])
    if a.sampler == "2m":
        kw["multistep"] = s.multistep_coefficients
    lat = DenoiseLoop(unet, cn, use_graph=True).begin(**kw).run().double().clone()
    return lat, vae


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", choices=sorted(SIZES), default="lo")
    ap.add_argument("--checkpoint", default=None, help="a diffusers-format folder with unet/, controlnet/ and vae/ (implies --size lo)")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--sampler", choices=["euler", "2m"], default="euler")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quality_compare: needs a GPU (there is no CPU fallback)")
    if a.checkpoint:
        a.size = "lo"
    from this_and_that_vdm_amd import metrics, ops
    from this_and_that_vdm_amd.utils.synthetic import synthetic_inputs
    dev = torch.device("cuda:0")
    size = SIZES[a.size]
    was = ops.f32_split()
    rows = []
    try:
        with torch.no_grad():
            masters = build(a, size, dev)
            inp = {k: v.to(dev) for k, v in synthetic_inputs(2, size["frames"], size["h"], size["w"], size["ctx_tokens"], size["ctx_dim"],
                                                             seed=a.seed).items()}
            exact_lat, exact_vae = run_mode("f32", masters, inp, a)
            exact = decoded_frames(exact_vae, exact_lat)
            del exact_vae
            ms_ok = all(v % 16 == 0 and v >= metrics.MS_SSIM_MIN_SIZE for v in exact.shape[1:3])
            for name in list(MODES)[1:]:
                lat, vae = run_mode(name, masters, inp, a)
                whole = metrics.compare_frames(decoded_frames(vae, lat), exact, ms_ssim=ms_ok).to_dict()
                alone = metrics.compare_frames(decoded_frames(vae, exact_lat), exact, ms_ssim=ms_ok).to_dict()
                rows.append(dict(mode=name, latents_rel_l2=float((lat - exact_lat).norm() / exact_lat.norm()),
                                 latents_max_abs=float((lat - exact_lat).abs().max()), finite=bool(torch.isfinite(lat).all().item()),
                                 psnr=whole["psnr"], ssim=whole["ssim"], ms_ssim=whole["ms_ssim"], worst_frame_psnr=min(
                                     (v for v in whole["frame_psnr"] if not isinstance(v, str)), default="inf"),
                                 worst_frame_ssim=min(whole["frame_ssim"]),
                                 decoder_alone=dict(psnr=alone["psnr"], ssim=alone["ssim"], ms_ssim=alone["ms_ssim"])))
                del vae
    finally:
        ops.set_f32_split(was)
    weights = f"checkpoint {a.checkpoint}" if a.checkpoint else f"synthetic ({a.size})"
    res = dict(tool="quality_compare", weights=weights, sampler=a.sampler, steps=a.steps, seed=a.seed,
               latents=[1, size["frames"], 4, size["h"], size["w"]], frames=list(exact.shape), reference="exact TT_F32 (denoise loop and decoder)",
               columns="psnr (dB) / ssim / ms_ssim: means over the frames of the mode's uint8 video against the exact mode's; "
                       "decoder_alone: the exact mode's latents through the mode's decoder" + (
                           "" if ms_ok else "; ms_ssim null: the frames are smaller than its 176 pixels"),
               rows=rows,
               says="how far each mode's arithmetic moves the decoded frames of one request" + (
                   "" if a.checkpoint else ": synthetic weights (UNet, ControlNet and decoder) -- the frames are those of a hash-filled network, "
                                           "so this measures arithmetic error in picture terms, not the picture quality of a trained model"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
