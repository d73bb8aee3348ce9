"""GPU: the native VAE encoder (``AutoencoderKLTemporalDecoder(native_encoder=True).encode``; reference
svd/pipeline_stable_video_diffusion_controlnet.py:200,652) -- tt_gemm mode 3 (3x3 stride-2 conv after a bottom / right zero pad)
against F.conv2d(F.pad(x, (0, 1, 0, 1)), stride=2), the encoder against the CPU restatement (tests/vae_encoder_reference.py) on
identical weights, batch chunking, and the VGL pipeline end to end with no stand-in VAE."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.parity_common import assert_north_star, build_pair, err_stats
from tests.stubs import StubCLIPVision, StubTextEncoder
from tests.test_ops_gpu import TOL               # the mode-1 conv tests' bounds for the 16-bit storage types
from tests.vae_encoder_reference import EncoderVAE

pytestmark = pytest.mark.gpu

TINY = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    threads = torch.get_num_threads()
    torch.set_num_threads(min(32, threads))          # the CPU references: eager PyTorch is slow at hundreds of host threads
    yield o
    torch.set_num_threads(threads)


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _tok(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _conv_case(nimg, h, w, cin, cout, dtype):
    x = _rnd(nimg, cin, h, w, seed=1).to(dtype)
    wt = _rnd(cout, cin, 3, 3, seed=2, scale=(9 * cin) ** -0.5).to(dtype)
    bias = _rnd(cout, seed=3, scale=0.5)
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), wt.float(), bias, stride=2)
    return x, wt, bias, ref


def _check(out, ref, dtype):
    ref = _tok(ref)
    if dtype == torch.float32:
        assert_north_star(out, ref, "tt_gemm mode 3 (TT_F32)")
    else:
        torch.testing.assert_close(out.float().cpu(), ref, **TOL[dtype])


SHAPES = [(2, 256, 448, 128, 128), (2, 128, 224, 256, 256), (2, 64, 112, 512, 512), (3, 16, 32, 32, 32)]
MODES = ["bf16", "fp16", "f32", "split16"]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", MODES)
@torch.no_grad()
def test_gemm_mode3_matches_padded_stride2_conv(ops, shape, mode):
    from this_and_that_vdm_amd.packing import pack_conv3x3, presplit_f32
    nimg, h, w, cin, cout = shape
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(mode, torch.float32)
    x, wt, bias, ref = _conv_case(nimg, h, w, cin, cout, dtype)
    ho, wo = ref.shape[-2:]
    assert (ho, wo) == (h // 2, w // 2)
    wp = pack_conv3x3(wt).cuda()
    was = ops.f32_split()
    ops.set_f32_split(mode == "split16")
    ops.PROFILE = []
    try:
        if mode == "split16":
            wp = presplit_f32(wp)                      # packed weights arrive pre-split (TtGemmArgs.presplit bit 1), as prepare() packs them
        out = ops.gemm(_tok(x).cuda(), wp, mode=3, conv=(nimg, h, w, ho, wo, 2, 0), bias=bias.cuda())
        torch.cuda.synchronize()
        name = ops.PROFILE[0][0]
    finally:
        ops.PROFILE = None
        ops.set_f32_split(was)
    kmode = {"split16": "29"}.get(mode, "5")          # gemm_kernel.h KMODE 5 (+ 8 split products + 16 pre-split W)
    assert name.startswith("gemm_kernel<") and name.endswith(f", {kmode}>"), name
    _check(out, ref, dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@torch.no_grad()
def test_gemm_mode3_split_k_and_tile_statistics(ops, dtype):
    """the coarsest downsample (2 x 64x112 -> 32x56, 512 channels) takes a split-K plan; the 128x224 one a single pass -- both with
    stats_out: the per-tile column sums / sums of squares equal those of the stored output"""
    import ctypes as C
    from this_and_that_vdm_amd.packing import pack_conv3x3
    lib = ops._lib.load()
    for (nimg, h, w, cin, cout), want_split in (((2, 64, 112, 512, 512), True), ((2, 128, 224, 256, 256), False)):
        x, wt, bias, ref = _conv_case(nimg, h, w, cin, cout, dtype)
        ho, wo = ref.shape[-2:]
        ops.PROFILE = []
        try:
            out = ops.gemm(_tok(x).cuda(), pack_conv3x3(wt).cuda(), mode=3, conv=(nimg, h, w, ho, wo, 2, 0), bias=bias.cuda(), stats=ho * wo)
            torch.cuda.synchronize()
            name = ops.PROFILE[0][0]
        finally:
            ops.PROFILE = None
        assert name.endswith(", 5>"), name
        g = ops._lib.TtGemmArgs()
        g.a0, g.k0, g.lda0, g.w, g.ldw, g.n, g.out, g.ldo = 1, cin, cin, 1, 9 * cin, cout, 1, cout
        g.mode, g.dtype, g.m = 3, ops._code(dtype), out.shape[0]
        g.nimg, g.hin, g.win, g.hout, g.wout, g.stride = nimg, h, w, ho, wo, 2
        need = lib.tt_gemm_ws_bytes(C.byref(g))
        g.ws, g.ws_bytes = (1, need) if need else (None, 0)
        cfg = (C.c_int32 * 7)()
        assert lib.tt_gemm_plan(C.byref(g), cfg) == 0
        assert (cfg[6] > 1) == want_split, list(cfg)
        _check(out, ref, dtype)
        assert hasattr(out, "_tt_stats"), "a mode-3 launch with stats= must hand its tile sums on (the next ResnetBlock's norm1)"
        sbuf, rows = out._tt_stats[0], out._tt_stats[1]
        assert (ho * wo) % rows == 0
        o = out.float().view(-1, rows, cout)
        torch.testing.assert_close(sbuf[:, 0].cpu(), o.sum(1).cpu(), rtol=1e-4, atol=1e-3)
        torch.testing.assert_close(sbuf[:, 1].cpu(), (o * o).sum(1).cpu(), rtol=1e-4, atol=1e-3)


# ---- the encoder module
def _encoder_pair(cfg, dtype, compute=None):
    from this_and_that_vdm_amd.svd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    ref = EncoderVAE(**cfg).eval()
    fill_parameters_(ref, "vae.", round_to=dtype)
    p = AutoencoderKLTemporalDecoder(**cfg, native_encoder=True).eval()
    missing, unexpected = p.load_state_dict(ref.state_dict(), strict=False)
    assert not unexpected and all(k.startswith("decoder.") for k in missing)
    p = p.to(device="cuda:0", dtype=dtype)
    p.compute_dtype = compute
    return p, ref


def _image(n, h, w, seed, dtype):
    return (torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dtype).float()


@pytest.mark.parametrize("mode,rel", [("f32", None), ("split16", None), ("fp16", 4e-3), ("bf16", 3e-2)])
@torch.no_grad()
def test_encoder_matches_the_restatement(ops, mode, rel):
    """tiny widths (32, 64, 64, 64), 3 images of 64x128: TT_F32 (exact and split16) every element of mean and logvar inside
    rtol 1e-3 / atol 1e-4; 16-bit storage: relative L2 (bounds of the decoder's order) and cosine >= 0.999"""
    dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}.get(mode, torch.float32)
    p, ref = _encoder_pair(TINY, dtype, torch.float32 if dtype == torch.float32 else None)
    x = _image(3, 64, 128, 4, dtype)
    want = ref.encode(x)
    was = ops.f32_split()
    ops.set_f32_split(mode == "split16")
    try:
        dist = p.encode(x.cuda()).latent_dist
        tup = p.encode(x.cuda(), return_dict=False)
    finally:
        ops.set_f32_split(was)
    assert isinstance(tup, tuple) and len(tup) == 1 and torch.equal(tup[0].mean, dist.mean)
    assert dist.mean.shape == want.mean.shape == (3, 4, 8, 16) and dist.mean.dtype == dtype
    for name, got, exp in (("mean", dist.mean, want.mean), ("logvar", dist.logvar, want.logvar)):
        st = err_stats(got, exp)
        print(f"VAE encoder {mode} {name} vs the fp32 restatement: {st}")
        if rel is None:
            assert_north_star(got, exp, f"VAE encoder {name} ({mode})")
        else:
            assert st["rel_l2"] <= rel and st["cos"] >= 0.999, st
    torch.testing.assert_close(dist.std, torch.exp(0.5 * dist.logvar))


@torch.no_grad()
def test_encoder_at_the_shipped_widths_matches_the_restatement(ops):
    """(128, 256, 512, 512), one 256x448 image in TT_F32: the three mode-3 downsamples at their real sizes, the 512-channel
    single-head attention over 32x56 tokens, quant_conv folded into conv_out -- every element inside the north-star tolerance"""
    p, ref = _encoder_pair({}, torch.float32, torch.float32)
    x = _image(1, 256, 448, 7, torch.float32)
    want = ref.encode(x)
    dist = p.encode(x.cuda()).latent_dist
    assert dist.mean.shape == (1, 4, 32, 56)
    print("VAE encoder at the shipped widths (TT_F32):", err_stats(dist.parameters, want.parameters))
    assert_north_star(dist.mean, want.mean, "VAE encoder mean at (128, 256, 512, 512)")
    assert_north_star(dist.logvar, want.logvar, "VAE encoder logvar at (128, 256, 512, 512)")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@torch.no_grad()
def test_encode_chunking_does_not_change_the_result(ops, dtype):
    p, _ = _encoder_pair(TINY, dtype, torch.float32 if dtype == torch.float32 else None)
    x = _image(5, 64, 128, 9, dtype).cuda()
    whole = p.encode(x).latent_dist.parameters
    assert p.encode_chunk_size(64, 128) >= 5
    parts = p.encode(x, chunk_size=2).latent_dist.parameters
    single = p.encode(x[3:4]).latent_dist.parameters
    tol = dict(rtol=1e-3, atol=1e-4) if dtype == torch.float32 else TOL[dtype]
    torch.testing.assert_close(parts.float(), whole.float(), **tol)
    torch.testing.assert_close(single.float(), whole[3:4].float(), **tol)


# ---- the VGL pipeline with no stand-in VAE
def _request():
    g = torch.Generator().manual_seed(11)
    image = torch.rand(1, 3, 64, 128, generator=g)
    cond = torch.rand(4, 3, 64, 128, generator=g).numpy().astype(np.float32)
    ids = torch.randint(0, 100, (1, 8), generator=g)
    return image, cond, ids


@torch.no_grad()
def test_vgl_pipeline_end_to_end_through_the_native_encoder(ops):
    """`pipe(image, condition_img, controlnet, ...)` with ONE native `vae=` for both directions: the conditioning image and the
    gesture frames go through encode() on the MI355X.  TT_F32: the latents match the oracle loop fed with image / gesture latents
    from the restatement (gesture frames through fp16, quirk Q7) inside the north-star tolerance."""
    from oracle import vae as ov
    from oracle.scheduler import EulerDiscreteScheduler as OSched, denoise_loop
    from this_and_that_vdm_amd.svd import EulerDiscreteScheduler, StableVideoDiffusionControlNetPipeline
    from this_and_that_vdm_amd.svd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    dt = torch.float32
    p_unet, p_cn, o_unet, o_cn = build_pair("tiny_vgl", dt, "cuda:0", True)
    o_enc = EncoderVAE(**TINY).eval()
    fill_parameters_(o_enc, "vae.", round_to=dt)
    o_dec = ov.AutoencoderKLTemporalDecoder(**TINY).eval()
    fill_parameters_(o_dec, "vae.", round_to=dt)
    sd = dict(o_enc.state_dict())
    sd.update(o_dec.state_dict())
    vae = AutoencoderKLTemporalDecoder(**TINY, native_encoder=True).eval()
    vae.load_state_dict(sd)
    vae = vae.to("cuda:0")
    vae.compute_dtype = torch.float32
    clip, txt = StubCLIPVision().cuda(), StubTextEncoder().cuda()
    pipe = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=vae, image_encoder=clip, unet=p_unet,
                                                                  scheduler=EulerDiscreteScheduler())
    pipe.set_progress_bar_config(disable=True)
    image, cond, ids = _request()
    lat0 = torch.randn(1, 4, 4, 8, 16, generator=torch.Generator().manual_seed(5))
    call = dict(prompt=ids.cuda(), use_text=True, text_encoder=txt, height=64, width=128, num_frames=4, num_inference_steps=3, fps=7,
                motion_bucket_id=200, noise_aug_strength=0.0, guess_mode=False, decode_chunk_size=3)
    got_lat = pipe(image.cuda(), cond, p_cn, latents=lat0.clone(), output_type="latent", **call).frames
    # the oracle loop on latents from the restatement's encode(...).mode()
    ehs = pipe.encode_clip(image.cuda(), ids.cuda(), True, txt, "cuda", 1, True).float().cpu()
    img = pipe.image_processor.preprocess(image, 64, 128).float().cpu()
    il = o_enc.encode(img).mode()
    il = torch.cat([torch.zeros_like(il), il]).unsqueeze(1).repeat(1, 4, 1, 1, 1)
    ges = o_enc.encode(torch.from_numpy(cond).half().float()).mode()                   # quirk Q7: fp16 gesture frames
    sched = OSched()
    sched.set_timesteps(3)
    lat = denoise_loop(o_unet, o_cn, sched, lat0 * sched.init_noise_sigma, il, ehs, torch.tensor([[6.0, 200.0, 0.0]] * 2), ges,
                       torch.linspace(1, 3, 4).view(1, 4, 1, 1, 1), num_inference_steps=3)
    print("pipeline latents through the native encoder vs oracle loop on the restatement's latents:", err_stats(got_lat, lat))
    assert_north_star(got_lat, lat, "pipeline latents (TT_F32, native encoder) vs oracle loop")
    frames = pipe(image.cuda(), cond, p_cn, latents=lat0.clone(), output_type="np", **call).frames
    assert frames.shape == (1, 4, 64, 128, 3) and np.isfinite(frames).all()
    # fp16 storage: force_upcast (config default True) encodes the image with the VAE in fp32 and casts it back
    vae16 = AutoencoderKLTemporalDecoder(**TINY, native_encoder=True).eval()
    vae16.load_state_dict({k: v.half() for k, v in sd.items()})
    vae16 = vae16.to("cuda:0", torch.float16)
    p16, c16, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", True)
    pipe16 = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=vae16, image_encoder=StubCLIPVision().cuda().half(), unet=p16,
                                                                    scheduler=EulerDiscreteScheduler())
    pipe16.set_progress_bar_config(disable=True)
    seen = []
    enc = vae16.encode
    vae16.encode = lambda x, *a, **k: (seen.append((x.dtype, vae16.dtype)), enc(x, *a, **k))[1]
    f16 = pipe16(image.cuda(), cond, c16, latents=lat0.clone(), output_type="np", **dict(call, text_encoder=StubTextEncoder().cuda().half())).frames
    assert f16.shape == frames.shape and np.isfinite(f16).all()
    assert seen[0] == (torch.float32, torch.float32) and seen[1] == (torch.float16, torch.float16), seen
    assert vae16.dtype == torch.float16
    print("fp16 frames vs TT_F32 frames: max abs", float(np.abs(f16 - frames).max()))
