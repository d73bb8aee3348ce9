#!/usr/bin/env python3
"""denoise-steps/sec of the SVD denoise hot path (GestureNet ControlNet + spatio-temporal UNet + CFG + Euler),
BASELINE.json's metric, on N MI355X GPUs of one node.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--mode vgl|vl] [--res lo|ref|hi] [--dtype bf16|fp16|f32|split16]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

One "step" = one iteration of the reference loop body
(svd/pipeline_stable_video_diffusion_controlnet.py:624-720) for one request: CFG batch 2 x 14 frames,
78 context tokens, heads (5,10,20,20), random-init weights of the real architecture (1.52 B + 0.68 B
parameters), synthetic inputs.  Each rank serves its own independent request (weak scaling,
no collective inside the step); rank 0's weights reach the other ranks by ONE RCCL broadcast at start-up.
Inputs are resident in HBM when the timed region starts.  Rank 0 prints one JSON line.

A plain run sets up, warms up, times ONE window of exactly --steps steps and prints the line.  --full adds everything else:
the median of WINDOWS windows, the per-kernel profile and roofline, the CPU oracle baseline, the per-request set-up cost and
`tolerance_mode`.  --dump-outputs DIR writes what the timed path returned after its last step (rank 0's latents; with --block,
a fixed sample of the block's output) as DIR/<name>.npy in float32; the inputs are seeded, so two builds can be compared output
for output.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

# algorithmic TFLOP per denoise step (2*MAC for conv/Linear/QK^T/PV, context K/V counted once per batch element):
# BASELINE.md section 2 / SURVEY.md 8(d)
STEP_TFLOP = {("vgl", "lo"): 20.10, ("vl", "lo"): 14.77, ("vgl", "hi"): 91.32, ("vl", "hi"): 66.89}
# "ref" = the reference's own default resolution, 256x384 (config/train_image2video_gesturenet.yaml:18-19, test_code/inference.py:135-136):
# 32x48 latents.  Its algorithmic TFLOP follow from the two figures above: per step  a * hw + b * hw^2  (everything is linear in the
# token count hw except the spatial self-attention, at every level), fitted through hw = 1792 (lo) and 7168 (hi):
# VGL a * 1792 = 19.19, b * 1792^2 = 0.91;  VL 14.119, 0.651;  hw = 1536 gives 17.12 / 12.58 (bench.py's own launch count at that size:
# `executed_tflop_per_step` in the line).
STEP_TFLOP[("vgl", "ref")] = 19.19 * (1536 / 1792) + 0.91 * (1536 / 1792) ** 2
STEP_TFLOP[("vl", "ref")] = 14.119 * (1536 / 1792) + 0.651 * (1536 / 1792) ** 2
LATENT = {"lo": (32, 56), "ref": (32, 48), "hi": (64, 112)}
PEAK_TFLOPS = 2500.0          # dense bf16/fp16 MFMA peak, MI355X_MICROARCH.md (spec ~2.5 PF; 2495 measured)
PEAK_TFLOPS_F32 = 157.3       # f32-input MFMA (v_mfma_f32_32x32x2_f32): the fp32 vector rate, same guide
PEAK_TFLOPS_SPLIT16 = PEAK_TFLOPS / 3    # split16: every product block is three fp16 MFMAs (a_lo b_hi + a_hi b_lo + a_hi b_hi)
TOLERANCE_MODE_FILE = "r6_bench_lo_split16.json"   # the bench line of the mode that meets rtol 1e-3 / atol 1e-4 (python bench.py --dtype split16)
WINDOWS = 3                   # --full: timed windows of --steps steps each; ms_per_step is their median
DUMP_BYTES = 64 << 20         # --dump-outputs: at most this many bytes over all arrays
FRAMES, CTX_TOKENS, CTX_DIM, STEPS_PER_REQUEST = 14, 78, 1024, 25
TRAFFIC_FILE = "r6_hbm_traffic.json"     # written by tools/profile_round.sh (rocprofv3 --pmc passes), stamped with the kernel-source hash


def csrc_hash() -> str:
    """sha256[:16] over the kernel sources (csrc/*.hip, *.h, *.cpp, Makefile): identifies the binary a measurement belongs to."""
    import glob
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    for f in sorted(glob.glob(os.path.join(d, "*.hip")) + glob.glob(os.path.join(d, "*.h")) + glob.glob(os.path.join(d, "*.cpp")) +
                    [os.path.join(d, "Makefile")]):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def build_models(mode, dtype, device, rank, world):
    from this_and_that_vdm_amd.svd.temporal_controlnet import ControlNetModel
    from this_and_that_vdm_amd.svd.unet_spatio_temporal_condition import UNetSpatioTemporalConditionModel
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    models = []
    with torch.device(device):
        unet = UNetSpatioTemporalConditionModel(num_attention_heads=(5, 10, 20, 20), num_frames=FRAMES).to(dtype).eval()
        models.append(("unet.", unet))
        cn = None
        if mode == "vgl":
            cn = ControlNetModel().to(dtype).eval()
            models.append(("controlnet.", cn))
    from this_and_that_vdm_amd.dist import broadcast_model_, flat_param_buffer
    bcast_s, checksum, prep_s = None, 0, 0.0
    for salt, m in models:
        flat = flat_param_buffer(m)
        if rank == 0:
            fill_parameters_(m, salt)            # zero-convs get non-zero values too
        if world > 1:
            bcast_s = (bcast_s or 0.0) + broadcast_model_(m, src=0, flat=flat)     # RCCL over xGMI, once
        if dtype == torch.float32:
            m.compute_dtype = torch.float32      # TT_F32 reference-precision mode (fp32 parameters default to bf16 compute)
        # exact integer checksum of the parameter bytes (every rank must hold rank 0's weights after the broadcast)
        bits = flat.view(torch.int16 if flat.element_size() == 2 else torch.int32)
        checksum = (checksum * 1000003 + int(bits.to(torch.int64).sum().item())) % (1 << 61)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.prepare(force=True)                    # weight packing (LayerNorm folds with exact zero row sums, conv re-layouts): once per process
        torch.cuda.synchronize()
        prep_s += time.perf_counter() - t0
    build_models.prepare_s = prep_s
    return unet, cn, bcast_s, checksum


def make_loop(unet, cn, res, device, seed):
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    from this_and_that_vdm_amd.svd.scheduling_euler_discrete import EulerDiscreteScheduler
    from this_and_that_vdm_amd.utils.synthetic import synthetic_inputs
    h, w = LATENT[res]
    inp = synthetic_inputs(2, FRAMES, h, w, CTX_TOKENS, CTX_DIM, seed=seed)
    inp = {k: v.to(device) for k, v in inp.items()}          # the request's inputs are resident in HBM before the timed region (as the
    sched = EulerDiscreteScheduler()                         # pipeline hands them over: outputs of the VAE / CLIP encoders on the device)
    sched.set_timesteps(STEPS_PER_REQUEST)
    loop = DenoiseLoop(unet, cn, use_graph=True)
    args = dict(latents=inp["latents"], image_latents=inp["image_latents"], encoder_hidden_states=inp["encoder_hidden_states"],
                added_time_ids=inp["added_time_ids"], guidance_scale=inp["guidance_scale"], sigmas=sched.sigmas,
                timesteps=sched.timesteps, controlnet_cond=inp["gesture_latents"] if cn is not None else None)
    loop.begin(**args)
    return loop, args


def advance(loop, args, n, fresh=False):
    """n steps; a request that has run out of steps is followed by the next one (same shapes -> same captured graph).
    fresh: start with a NEW request whatever the loop's position -- the timed window opens with a begin(), so the per-request
    set-up (context K/V projections, FiLM table of all steps) is inside it for every --steps / --warmup combination."""
    for i in range(n):
        if loop.step_index == loop.num_steps or (fresh and i == 0):
            loop.begin(**args)
        loop.step()


def dump_outputs(path, arrays):
    """--dump-outputs: every tensor of `arrays` as <path>/<name>.npy, float64 kept, everything else as float32.  An array larger
    than its share of DUMP_BYTES is replaced by a fixed sample of its elements (sorted indices from a seeded generator, the same
    in every run), flattened."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    share = DUMP_BYTES // len(arrays)
    for name, t in arrays.items():
        t = t.detach().to(torch.float64 if t.dtype == torch.float64 else torch.float32)
        cap = share // t.element_size()
        if t.numel() > cap:
            idx = torch.randint(t.numel(), (cap,), generator=torch.Generator().manual_seed(0)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(path, f"{name}.npy"), t.cpu().numpy())


def kernel_profile(loop, args):
    """One eager (un-captured) step with HIP events around every tt_gemm / tt_attention launch on the launch
    stream -> per kernel-instance (launch count, algorithmic flops, time)."""
    from this_and_that_vdm_amd import ops
    loop.begin(**args)
    from this_and_that_vdm_amd.svd import layers as _layers
    side_was, _layers._Side.ENABLED = _layers._Side.ENABLED, False
    loop.use_graph = False
    loop.overlap_branches = False                   # one stream: each kernel is timed alone on the chip
    loop.step()                                     # eager warm-up
    torch.cuda.synchronize()
    ops.PROFILE = []
    loop.step()
    torch.cuda.synchronize()
    rec, ops.PROFILE = ops.PROFILE, None
    loop.use_graph = True
    loop.overlap_branches = True
    _layers._Side.ENABLED = side_was
    agg = {}
    for name, flops, e0, e1, _shape in rec:
        a = agg.setdefault(name, [0, 0.0, 0.0])
        a[0] += 1
        a[1] += flops
        a[2] += e0.elapsed_time(e1) * 1e-3
    return agg


CPU_THREADS = 32      # torch-CPU on the 256-thread host of the GPU box is pathological (measured with
                      # tools/cpu_threads_probe.py: one UNet forward 4.3 s at 32 threads, 13 s at 128, 275 s at 256)


def cpu_baseline(mode, res):
    """The oracle (CPU restatement of the reference's eager op sequence, fp32, no hoists) timed on this box's host
    cores on ONE full denoise step of the same workload (ControlNet + UNet on the CFG batch of 2 x 14 frames + CFG +
    Euler), UN-WARMED (the first and only pass: BASELINE.md section 3 warms up once, which would double this leg's 30 s), with the
    thread count that is fastest for eager PyTorch on this host (32 of 256: tools/cpu_threads_probe.py).  No extrapolation."""
    from oracle import models as om
    from oracle.scheduler import EulerDiscreteScheduler as OSched
    from this_and_that_vdm_amd.utils.synthetic import synthetic_inputs
    threads = min(CPU_THREADS, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    torch.set_flush_denormal(True)
    h, w = LATENT[res]
    pat = torch.randn(1 << 20, generator=torch.Generator().manual_seed(0)) * 0.02

    def build(ctor):            # meta construction + pattern fill: avoids a minutes-long RNG init of 2.2 B parameters
        with torch.device("meta"):
            m = ctor()
        m = m.to_empty(device="cpu").eval()
        for name, p in m.named_parameters():
            n = p.numel()
            p.data.view(-1).copy_(pat.repeat((n + pat.numel() - 1) // pat.numel())[:n])
            if p.dim() == 1 and name.endswith("weight"):
                p.data.fill_(1.0)
        return m

    with torch.no_grad():
        unet = build(lambda: om.UNetSpatioTemporalConditionModel(num_attention_heads=(5, 10, 20, 20), num_frames=FRAMES))
        cn = build(lambda: om.ControlNetModel()) if mode == "vgl" else None
        inp = synthetic_inputs(2, FRAMES, h, w, CTX_TOKENS, CTX_DIM, seed=0)
        sched = OSched()
        sched.set_timesteps(STEPS_PER_REQUEST)
        t = sched.timesteps[0]
        t0 = time.perf_counter()
        x = torch.cat([sched.scale_model_input(torch.cat([inp["latents"]] * 2), t), inp["image_latents"]], dim=2)
        down = mid = None
        if cn is not None:
            down, mid = cn(x, t, inp["encoder_hidden_states"], inp["added_time_ids"],
                           controlnet_cond=torch.cat([inp["gesture_latents"]] * 2))
        eps = unet(x, t, inp["encoder_hidden_states"], inp["added_time_ids"], down_block_additional_residuals=down,
                   mid_block_additional_residual=mid)
        u, c = eps.chunk(2)
        sched.step(u + inp["guidance_scale"] * (c - u), t, inp["latents"])
        step_s = time.perf_counter() - t0
    return {"value": 1.0 / step_s, "unit": "denoise-steps/s", "cores": threads, "kind": "port",
            "sample": f"oracle fp32 eager (torch {torch.__version__}, {threads} of {os.cpu_count()} hardware threads), un-warmed: ONE full "
                      f"{mode.upper()} denoise step, CFG batch 2 x {FRAMES} frames at {h}x{w} latents = {step_s:.1f} s"}


def tolerance_mode(mode, res):
    """The committed bench line of the mode that meets BASELINE's tolerance (rtol 1e-3 / atol 1e-4 against the reference's CPU fp32
    forward on every element: tests/test_full_size_gpu.py::test_full_size_f32_mode_meets_the_north_star_tolerance[split16]) --
    `python bench.py --dtype split16`, same workload, measured on its own; None when no such file exists for this workload."""
    path = os.path.join(REPO, "profiles", TOLERANCE_MODE_FILE)
    if (mode, res) != ("vgl", "lo") or not os.path.exists(path):
        return None
    d = json.load(open(path))
    return {"dtype": d["dtype"], "ms_per_step": d["ms_per_step"], "value": d["value"], "unit": d["unit"], "source": f"profiles/{TOLERANCE_MODE_FILE}",
            "kernel_source_sha16": d["config"].get("kernel_source_sha16"), "same_kernel_sources_as_this_line": d["config"].get("kernel_source_sha16") == csrc_hash(),
            "what": "fp32 storage, split-fp16 products (three 16-bit MFMAs per product block), fp32 accumulation / norms / softmax: every element of "
                    "the UNet output and of the latents inside rtol 1e-3 / atol 1e-4 of the fp32 oracle"}


def block_main(a, dtype, device, peak) -> int:
    """--block l0hi: ONE L0 TransformerSpatioTemporalModel (C = 320, 5 heads x 64) at 64x112 latents, CFG batch 2 x 14 frames,
    78 context tokens with an all-zero uncond context as in the pipeline: the "14x4x64x112 spatio-temporal-attention block"
    BASELINE's north_star prices against the MFMA roofline (reference svd/diffusion_arch/transformer_temporal.py:323-376).
    Prints one JSON line; `roofline` is the whole block (algorithmic flops of its launches / block time)."""
    from this_and_that_vdm_amd import ops
    from this_and_that_vdm_amd.svd.diffusion_arch.transformer_temporal import TransformerSpatioTemporalModel
    from this_and_that_vdm_amd.svd.layers import Geom, PackRegistry, StepContext
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    f, h, w, c, heads, b = FRAMES, 64, 112, 320, 5, 2
    with torch.device(device):
        blk = TransformerSpatioTemporalModel(heads, c // heads, in_channels=c, cross_attention_dim=CTX_DIM).eval()
    fill_parameters_(blk, "l0tfm.")
    reg = PackRegistry()
    blk.pack(reg, dtype)
    g = torch.Generator(device="cpu").manual_seed(4)
    ehs = torch.nn.functional.layer_norm(torch.randn(b, CTX_TOKENS, CTX_DIM, generator=g), (CTX_TOKENS, CTX_DIM))
    ehs[0] = 0                                                     # the CFG uncond half (pipeline :145-152)
    sp = (CTX_TOKENS + 7) // 8 * 8
    pad = torch.zeros(b, sp, CTX_DIM, dtype=dtype, device=device)
    pad[:, :CTX_TOKENS] = ehs.to(device=device, dtype=dtype)
    pad = pad.view(b * sp, CTX_DIM)
    k_all = ops.gemm(pad, torch.cat(reg.k_w, 0).to(dtype).contiguous())
    vt_all = ops.gemm(torch.cat(reg.v_w, 0).to(dtype).contiguous(), pad)
    ctx = StepContext(None, k_all, vt_all, CTX_TOKENS, sp, attn_fp8=a.attn == "fp8", zero_mask=1)
    geom = Geom(b, f, h, w)
    tok = (torch.randn(geom.m, c, generator=g) * 1.0).to(device=device, dtype=dtype)
    run = lambda: blk(tok, geom, ctx)
    for _ in range(max(1, a.warmup)):
        run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()                                 # the block's ~45 launches replayed as in the step graph
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        graph.replay()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    if a.dump_outputs:
        dump_outputs(a.dump_outputs, {"block_out": out})
    ops.PROFILE = []
    run()
    torch.cuda.synchronize()
    rec, ops.PROFILE = ops.PROFILE, None
    flops = sum(r[1] for r in rec)
    agg = {}
    for name, fl, e0, e1, _ in rec:
        v = agg.setdefault(name, [0, 0.0, 0.0])
        v[0] += 1; v[1] += fl; v[2] += e0.elapsed_time(e1) * 1e-3
    line = {"metric": "L0 spatio-temporal transformer block at 64x112 latents (blocks/s)", "value": 1e3 / ms, "unit": "blocks/s", "n_gpus": 1,
            "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic (random-init weights, seeded inputs)",
            "config": {"workload": "one L0 TransformerSpatioTemporalModel (C 320, 5 heads x 64), CFG batch 2 x 14 frames x 7168 tokens, "
                                   "78 context tokens (uncond context all zero), hipGraph replay", "spatial_self_attention": a.attn,
                       "finite_output": bool(torch.isfinite(out.float()).all().item()), "block_tflop_algorithmic": flops / 1e12,
                       "mfma_kernels": {k: {"launches": v[0], "tflop": v[1] / 1e12, "ms": v[2] * 1e3, "tflops": v[1] / v[2] / 1e12}
                                        for k, v in sorted(agg.items(), key=lambda kv: -kv[1][2])},
                       # every GEMM / attention launch of one forward in launch order (eager, event-timed one by one): the input of
                       # DESIGN.md 6.C (ceiling analysis); shape = (mode, M, N, K, geglu, residual) or ("attn", batch x heads, Lq, Lk, mask, 0)
                       "launch_list": [{"kernel": name, "shape": list(shape) if shape else None, "gflop": fl / 1e9, "us": e0.elapsed_time(e1) * 1e3}
                                       for name, fl, e0, e1, shape in rec]},
            "roofline": {"bound": "mfma", "kernel": "whole block (all launches of one forward)", "achieved": flops / (ms * 1e-3) / 1e12,
                         "peak": peak, "unit": "TFLOP/s", "frac": flops / (ms * 1e-3) / 1e12 / peak, "traffic": None},
            "cpu_baseline": None}
    print(json.dumps(line))
    return 0


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` without a launcher: re-exec this script under torch.distributed.run with one rank per
    GPU of this node (127.0.0.1 rendezvous on a free port) -- exactly the command line the driver uses for N > 1."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def stub_cpu_main(a, world: int, rank: int) -> int:
    """The rank plumbing of main() (rendezvous, barrier-bracketed timing, max over ranks, rank-0 JSON line) with the GPU
    loop replaced by a sleep, on gloo.  Exists only so the N > 1 launcher path is testable without GPUs."""
    import torch.distributed as dist
    from this_and_that_vdm_amd.dist import RendezvousError, init_ranks, max_over_ranks
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        try:                                     # the same fail-loud start-up as the GPU path (gloo instead of RCCL)
            init_ranks("gloo", rank, world, int(os.environ.get("LOCAL_RANK", "0")),
                       timeout_s=float(os.environ.get("TT_BENCH_RENDEZVOUS_TIMEOUT_S", "180")))
        except RendezvousError as e:
            print(json.dumps({"metric": "stub (launcher self-test, no GPU work)", "value": None, "n_gpus": world, "error": f"rank {rank}: {e}"}), flush=True)
            raise SystemExit(3)
        dist.barrier()
    t0 = time.perf_counter()
    time.sleep(0.002 * a.steps * (1 + rank))
    if world > 1:
        dist.barrier()
    dt = max_over_ranks(time.perf_counter() - t0, "cpu")
    if rank == 0:
        print(json.dumps({"metric": "stub (launcher self-test, no GPU work)", "value": world * a.steps / dt,
                          "unit": "denoise-steps/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                          "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": a.dtype, "data": "none", "config": {"workload": "stub"},
                          "roofline": None, "cpu_baseline": None}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", choices=["vgl", "vl"], default="vgl")
    ap.add_argument("--res", choices=["lo", "ref", "hi"], default="lo",
                    help="lo 256x448 (BASELINE's headline), ref 256x384 (the reference's own default, config/train_image2video_gesturenet.yaml), hi 512x896")
    ap.add_argument("--dtype", choices=["bf16", "fp16", "f32", "split16"], default="bf16",
                    help="f32 = TT_F32 reference-precision mode (fp32 storage, exact-fp32 MFMA at 1/16 of the bf16 rate); split16 = the same mode with "
                         "split-fp16 products (three 16-bit MFMAs per product block): both meet rtol 1e-3 / atol 1e-4")
    ap.add_argument("--block", choices=["l0hi"], default=None,
                    help="l0hi: time ONE L0 TransformerSpatioTemporalModel at 64x112 latents (BASELINE's spatio-temporal-attention block) instead of the step")
    ap.add_argument("--attn", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: spatial self-attention on OCP e4m3 operands with fp8 MFMA (BASELINE config 5; 16-bit elsewhere)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: median of three timed windows, per-kernel profile + roofline, CPU oracle baseline, "
                         "per-request set-up cost, tolerance_mode")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU oracle baseline")
    ap.add_argument("--no-kernel-profile", action="store_true", help="--full without the per-kernel profile and roofline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--stub-cpu", action="store_true",
                    help="launcher self-test (tests/test_bench_launch_cpu.py): gloo ranks time a sleep instead of the GPU loop")
    a = ap.parse_args()

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(a.gpus))            # `python bench.py --gpus N`: spawn one rank per GPU ourselves
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}")
    if a.stub_cpu:
        return stub_cpu_main(a, world, rank)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs MI355X GPUs (the denoise path has no CPU fallback)")
    # TT_BENCH_ONE_GPU=1 (self-test on a 1-GPU box): every rank uses cuda:0 and the ranks talk over gloo -- the whole N > 1 code
    # path (launcher, weight broadcast, barrier-bracketed timing, max over ranks) runs, only the numbers mean nothing
    one_gpu = os.environ.get("TT_BENCH_ONE_GPU") == "1"
    if one_gpu:
        local = 0
    from this_and_that_vdm_amd.dist import RendezvousError, gather_floats, init_ranks
    rendezvous_s = 0.0
    try:
        # rank / LOCAL_RANK / device-count check, process group with a finite timeout, 1-element broadcast + all-reduce: a wrong
        # mapping or a dead transport ends the job HERE with its cause in the JSON line, not inside the 3 GB weight broadcast
        if not one_gpu and not (0 <= local < torch.cuda.device_count()):
            raise RendezvousError(f"LOCAL_RANK {local} has no GPU: {torch.cuda.device_count()} device(s) visible to rank {rank}")
        torch.cuda.set_device(local)
        device = torch.device("cuda", local)
        if world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            rendezvous_s = init_ranks("gloo" if one_gpu else "nccl", rank, world, local, device=None if one_gpu else device,
                                      timeout_s=float(os.environ.get("TT_BENCH_RENDEZVOUS_TIMEOUT_S", "180")))
    except RendezvousError as e:
        print(json.dumps({"metric": "denoise-steps/sec (14-frame 256x448 VGL, 25 steps)", "value": None, "unit": "denoise-steps/s",
                          "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "error": f"rank {rank}: {e}"}), flush=True)
        raise SystemExit(3)
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "split16": torch.float32}[a.dtype]
    peak = {"f32": PEAK_TFLOPS_F32, "split16": PEAK_TFLOPS_SPLIT16}.get(a.dtype, PEAK_TFLOPS)
    from this_and_that_vdm_amd import ops as _ops
    _ops.set_f32_split(a.dtype == "split16")
    if world > 1:                                # N ranks share the host's cores during prepare() / packing
        torch.set_num_threads(max(1, min(8, (os.cpu_count() or 8) // world)))
    if a.block:
        return block_main(a, dtype, device, peak)

    unet, cn, bcast_s, checksum = build_models(a.mode, dtype, device, rank, world)
    for m in (unet, cn):
        if m is not None:
            m.attention_fp8 = a.attn == "fp8"
    loop, args = make_loop(unet, cn, a.res, device, seed=rank)
    if os.environ.get("TT_NO_OVERLAP") == "1":          # experiment switches: GestureNet and UNet encoder on ONE stream
        loop.overlap_branches = False
    if os.environ.get("TT_SPLIT_CFG") == "1":           # ... the two CFG halves as separate graph branches
        loop.split_cfg = True

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    advance(loop, args, a.warmup)
    # timed windows of exactly --steps steps, each bracketed by barrier + synchronize on both sides and reduced to the MAX over ranks.
    # A plain run times one window; --full times WINDOWS of them and reports the MEDIAN (boxes of the pool differ by 3-6 %, one 0.6 s
    # window cannot resolve 0.1 ms levers), listing all of them in config.ms_per_step_windows
    from this_and_that_vdm_amd.dist import max_over_ranks
    gdev = "cpu" if one_gpu else device
    windows = WINDOWS if a.full else 1
    window_dt, window_own = [], []
    for _ in range(windows):
        fence()
        t0 = time.perf_counter()
        advance(loop, args, a.steps, fresh=True)    # >= one begin() per 25 steps inside the timed region
        fence()
        own = time.perf_counter() - t0
        window_own.append(own)
        window_dt.append(max_over_ranks(own, gdev))
    order = sorted(range(windows), key=lambda i: window_dt[i])
    mid = order[windows // 2]
    dt, dt_own = window_dt[mid], window_own[mid]
    latents = loop.result().clone()                 # what the caller of the last timed step receives (begin() below overwrites it)
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, {"latents": latents})
    begin_ms = None
    if a.full:
        tb = time.perf_counter()                    # what one request set-up costs on its own (reported, already inside dt above)
        loop.begin(**args)
        torch.cuda.synchronize()
        begin_ms = (time.perf_counter() - tb) * 1e3
    allv = gather_floats([dt_own / a.steps * 1e3, float(checksum % (1 << 52)), getattr(build_models, "prepare_s", 0.0), bcast_s or 0.0], gdev)
    per_rank_ms, checksums = [v[0] for v in allv], [int(v[1]) for v in allv]
    per_rank_pack_s, per_rank_bcast_s = [v[2] for v in allv], [v[3] for v in allv]
    rccl_ranks = None
    if world > 1:                                   # the number of ranks the collective library itself sums over (RCCL on the GPU box)
        ones = torch.ones(1, device=gdev)
        torch.distributed.all_reduce(ones)
        rccl_ranks = {"backend": torch.distributed.get_backend(), "ranks_in_all_reduce": int(ones.item()),
                      "world_size": torch.distributed.get_world_size()}
    finite = bool(torch.isfinite(latents).all().item())

    roofline, extras = None, {}
    if rank == 0 and a.full and not a.no_kernel_profile:
        agg = kernel_profile(loop, args)
        tot_flops = sum(v[1] for v in agg.values())
        name, (cnt, fl, sec) = max(agg.items(), key=lambda kv: kv[1][2])
        # HBM-side bytes per launch of that kernel: rocprofv3 PMC passes (FETCH_SIZE doubled, + WRITE_SIZE; tools/pmc_traffic.py)
        # cannot run inside this process, so the figure comes from the committed profile of the SAME kernel instance and is
        # stamped with where it was measured; it is null (not a stale number) when the dominant kernel has no entry there.
        # It is reported only when that profile was taken on THIS binary (same hash of the kernel sources); otherwise null.
        traffic, traffic_src = None, None
        tfile = os.path.join(REPO, "profiles", TRAFFIC_FILE)
        if os.path.exists(tfile):
            doc = json.load(open(tfile))
            if doc.get("_kernel_source_sha16") == csrc_hash():
                traffic = doc.get(f"{a.mode}_{a.res}", {}).get(name.replace("ttg::", ""))
                if traffic is not None:
                    traffic_src = (f"profiles/{TRAFFIC_FILE} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of tools/pmc_step.py on the "
                                   f"same kernel sources, sha16 {doc.get('_kernel_source_sha16')})")
            else:
                traffic_src = (f"null: profiles/{TRAFFIC_FILE} was measured on other kernel sources "
                               f"({doc.get('_kernel_source_sha16')} != {csrc_hash()}); re-run tools/profile_round.sh")
        roofline = {"bound": "mfma", "kernel": name, "launches_per_step": cnt,
                    "achieved": fl / sec / 1e12, "peak": peak, "unit": "TFLOP/s",
                    "frac": fl / sec / 1e12 / peak, "traffic": traffic, "traffic_source": traffic_src,
                    "algorithmic_gflop_per_launch": fl / cnt / 1e9, "avg_launch_us": sec / cnt * 1e6}
        extras["mfma_kernels"] = {k: {"launches": v[0], "tflop": v[1] / 1e12, "ms": v[2] * 1e3,
                                      "tflops": v[1] / v[2] / 1e12} for k, v in sorted(agg.items(), key=lambda kv: -kv[1][2])}
        extras["executed_tflop_per_step"] = tot_flops / 1e12
    cpu = None
    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline:
        cpu = cpu_baseline(a.mode, a.res)

    if rank == 0:
        h, w = LATENT[a.res]
        ms = dt / a.steps * 1e3
        step_tflop = STEP_TFLOP[(a.mode, a.res)]
        out = {
            "metric": "denoise-steps/sec (14-frame 256x448 VGL, 25 steps)" if (a.mode, a.res, a.attn) == ("vgl", "lo", "bf16") and a.dtype in ("bf16", "fp16")
                      else f"denoise-steps/sec (14-frame {h * 8}x{w * 8} {a.mode.upper()}{', fp8 attention' if a.attn == 'fp8' else ''}, 25 steps)",
            "value": world * a.steps / dt, "unit": "denoise-steps/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.dtype,
            "data": "synthetic (random-init weights of the real architecture, seeded inputs)",
            "config": {"workload": f"{a.mode.upper()} denoise step: {'GestureNet ControlNet + ' if a.mode == 'vgl' else ''}"
                                   f"spatio-temporal UNet + per-frame CFG + Euler, latent {FRAMES}x4x{h}x{w}, CFG batch 2, "
                                   f"{CTX_TOKENS} context tokens, heads (5,10,20,20)",
                       "mode": a.mode, "latent": [FRAMES, 4, h, w], "requests_per_gpu": 1,
                       "parallelism": f"{world} independent request(s), one per GPU; RCCL weight broadcast at start-up only",
                       "hipgraph": True, "finite_output": finite, "begin_ms_per_request": begin_ms,
                       "begins_in_timed_region": (a.steps + STEPS_PER_REQUEST - 1) // STEPS_PER_REQUEST, "spatial_self_attention": a.attn,
                       "step_tflop_algorithmic": step_tflop,
                       "step_mfma_frac_of_peak": step_tflop / (ms * 1e-3) / peak,
                       # ... and on the flops the step actually launches (the zero-context shortcut skips the uncond half's cross-attention)
                       "step_mfma_frac_executed": (extras["executed_tflop_per_step"] / (ms * 1e-3) / peak) if "executed_tflop_per_step" in extras else None,
                       "ms_per_step_windows": [d / a.steps * 1e3 for d in window_dt],
                       "ms_per_step_is": f"median of {windows} windows of {a.steps} steps" if windows > 1 else f"one window of {a.steps} steps",
                       "rccl_ranks": rccl_ranks,
                       "weight_broadcast_s": max(per_rank_bcast_s) if world > 1 else None, "rendezvous_s": rendezvous_s if world > 1 else None,
                       "weight_packing_s_per_rank": per_rank_pack_s if world > 1 else getattr(build_models, "prepare_s", None),
                       "multi_gpu_measured_on_hardware": None if world == 1 else (not one_gpu),
                       "ms_per_step_per_rank": per_rank_ms,
                       "weights_identical_on_all_ranks": len(set(checksums)) == 1, "kernel_source_sha16": csrc_hash(), **extras},
            "roofline": roofline, "cpu_baseline": cpu,
        }
        if a.full and a.dtype in ("bf16", "fp16"):  # the 16-bit modes do not meet the north-star tolerance: show the mode that does, side by side
            out["tolerance_mode"] = tolerance_mode(a.mode, a.res)
        print(json.dumps(out))
    if world > 1:
        torch.distributed.barrier()          # rank 0 profiles after the timed region; leave together
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
