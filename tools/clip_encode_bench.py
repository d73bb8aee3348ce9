#!/usr/bin/env python3
"""One request's CLIP encodes through the native classes (this_and_that_vdm_amd/clip.py) at the shipped sizes: the image encode
(CLIPVisionModelWithProjection, ViT-H/14: 1 x 3 x 224 x 224 -> 257 tokens of 1280, 32 layers) and the text encode (CLIPTextModel,
SD-2.1: one 77-token prompt, 23 layers of 1024) -- what encode_clip runs (svd/pipeline_stable_video_diffusion_controlnet.py:130-185).
Where transformers imports, the stock modules are timed on PyTorch-ROCm in the same process with the same weights.  Prints one JSON
line per (encoder, dtype): median / all ms of >= 20 timed encodes after warm-up (device events around synchronised work), launches per
encode, algorithmic TFLOP (2 x MAC).
python tools/clip_encode_bench.py [--dtypes bf16,split16] [--iters 20] [--out profiles/NAME.json]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def encoder_flops(l, c, inner, layers, causal=False, patch_k=0, proj=0):
    attn = 4.0 * l * l * c * (0.5 if causal else 1.0)
    return layers * (2.0 * l * c * (4 * c + 2 * inner) + attn) + 2.0 * (l - 1) * patch_k * c + 2.0 * c * proj


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(max(20, iters)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def launches(fn):
    """kernel launches of one call, counted by the torch profiler (library launches and torch's own alike)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,split16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from this_and_that_vdm_amd import clip, ops
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_, hash_uniform
    try:
        import transformers
    except Exception:
        transformers = None
    rows = []
    pix = (hash_uniform(3 * 224 * 224, 224) * 2.0).view(1, 3, 224, 224).cuda()
    ids = ((hash_uniform(77, 77) + 1.0) * 0.5 * 49408).long().clamp_(0, 49407).view(1, 77).cuda()
    for name in a.dtypes.split(","):
        dt = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(name, torch.float32)
        ops.set_f32_split(name == "split16")
        for kind in ("image", "text"):
            with torch.device("cuda"):
                m = (clip.CLIPVisionModelWithProjection() if kind == "image" else clip.CLIPTextModel()).to(dt).eval()
            fill_parameters_(m, "clip.")
            if dt == torch.float32:
                m.compute_dtype = torch.float32
            m.prepare()
            x = pix.to(dt) if kind == "image" else ids
            fn = (lambda: m(x).image_embeds) if kind == "image" else (lambda: m(x)[0])
            ms = timed(fn, a.iters)
            cfg = m.config
            fl = encoder_flops(257, 1280, 5120, 32, False, 592, 1024) if kind == "image" else encoder_flops(77, 1024, 4096, 23, True)
            row = dict(tool="clip_encode_bench", encoder=kind, dtype=name, path="native", median_ms=round(statistics.median(ms), 3),
                       all_ms=[round(v, 3) for v in ms], launches=launches(fn), tflop=round(fl / 1e12, 4), finite=bool(torch.isfinite(fn().float()).all()),
                       layers=cfg.num_hidden_layers)
            rows.append(row)
            print(json.dumps(row), flush=True)
            if transformers is not None:
                from tests.golden.make_clip_golden import to_transformers
                if kind == "image":
                    sm = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(
                        hidden_size=1280, intermediate_size=5120, num_hidden_layers=32, num_attention_heads=16, image_size=224, patch_size=14,
                        projection_dim=1024, hidden_act="gelu"))
                else:
                    sm = transformers.CLIPTextModel(transformers.CLIPTextConfig(
                        vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
                        max_position_embeddings=77, hidden_act="gelu", projection_dim=512))
                sm.load_state_dict(to_transformers({k: v.float().cpu() for k, v in m.state_dict().items()}, sm), strict=True)
                sm = sm.eval().to("cuda", dt)
                with torch.no_grad():
                    sfn = (lambda: sm(pixel_values=x).image_embeds) if kind == "image" else (lambda: sm(input_ids=x)[0])
                    sms = timed(sfn, a.iters)
                    srow = dict(tool="clip_encode_bench", encoder=kind, dtype=("fp32" if name == "split16" else name), path="transformers on PyTorch-ROCm",
                                median_ms=round(statistics.median(sms), 3), all_ms=[round(v, 3) for v in sms], launches=launches(sfn),
                                max_abs_vs_native=float((sfn().float() - fn().float()).abs().max()))
                rows.append(srow)
                print(json.dumps(srow), flush=True)
                del sm
            del m
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
