"""GPU: tt_encoder_attention and the small CLIP kernels against torch on the CPU, the native CLIP encoders (this_and_that_vdm_amd/clip.py)
against the restatement (tests/clip_reference.py) on identical weights and against transformers' recorded outputs, and the VGL pipeline
with the native VAE and the native CLIP pair (no stand-in model)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import clip_reference as cr
from tests.parity_common import assert_north_star, build_pair, err_stats
from tests.test_clip_cpu import check_against_golden
from tests.test_ops_gpu import TOL               # the project's bounds for its attention kernels in the 16-bit storage types

pytestmark = pytest.mark.gpu
MODES = ["bf16", "fp16", "f32", "split16"]
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "split16": torch.float32}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    return o


@pytest.fixture()
def mode(request, ops):
    """the storage / product mode of a case: split16 switches the process-wide TT_F32 product mode for the test's duration"""
    was = ops.f32_split()
    ops.set_f32_split(request.param == "split16")
    yield request.param
    ops.set_f32_split(was)


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _check(got, ref, m, what):
    if DT[m] == torch.float32:
        assert_north_star(got, ref, what)
    else:
        torch.testing.assert_close(got.float().cpu(), ref.float(), msg=lambda s: f"{what}: {s}", **TOL[DT[m]])


# ---- tt_encoder_attention.  (The split16 cases run the SAME exact-fp32 kernel as f32 -- this kernel has no split route and ignores
# tt_gemm_set_f32_split; they only guard against the process-wide switch leaking into it.)
ATTN_CASES = [(2, 17, 2, 80, 0), (1, 257, 2, 80, 0), (1, 64, 1, 64, 1), (1, 65, 2, 64, 1), (2, 77, 2, 64, 1), (1, 129, 2, 80, 1), (3, 77, 16, 64, 0)]
_QKV = {}


def _qkv(case, dtype):
    """(q, k, v rounded to the storage type as fp32 [nseq, l, C], the fp32 CPU reference [nseq * l, C]); computed once per case and dtype"""
    key = (case, dtype)
    if key not in _QKV:
        nseq, l, heads, d, causal = case
        c = heads * d
        q, k, v = (_rnd(nseq, l, c, seed=s + l + d).to(dtype).float() for s in (1, 2, 3))
        sp = lambda t: t.view(nseq, l, heads, d).transpose(1, 2)
        ref = F.scaled_dot_product_attention(sp(q), sp(k), sp(v), is_causal=bool(causal)).transpose(1, 2).reshape(nseq * l, c)
        _QKV[key] = (q, k, v, ref)
    return _QKV[key]


def _run_attention(ops, case, dtype, q, k, v, kpad=0, fused=False, fill=0.0):
    """q, k, v fp32 [nseq, l, C] on the CPU -> the kernel's output [nseq * l, C].  kpad: K / V get a per-sequence stride of l + kpad rows
    (columns for the fp32 V^T), the extra ones filled with +-fill; fused: q, k (and a row-major v) are slices of one [rows, 3C] buffer."""
    nseq, l, heads, d, causal = case
    c, dev = heads * d, "cuda:0"
    f32 = dtype == torch.float32
    ks = l + kpad
    vs = ks if not f32 else (ks + 3) // 4 * 4

    def padded(t, stride):
        buf = torch.empty(nseq, stride, c).fill_(fill)
        buf[:, 1::2] *= -1.0
        buf[:, :l] = t
        return buf.reshape(nseq * stride, c)
    if fused:
        assert not kpad
        buf = torch.cat([q.reshape(-1, c), k.reshape(-1, c), v.reshape(-1, c)], 1).to(dtype).to(dev)
        qd, kd, vd = buf[:, :c], buf[:, c:2 * c], buf[:, 2 * c:]
    else:
        qd, kd = q.reshape(-1, c).to(dtype).to(dev), padded(k, ks).to(dtype).to(dev)
        vd = padded(v, ks).to(dtype).to(dev)
    if f32:                                              # V^T [C, nseq * vs]: the layout tt_gemm's out_col_hw / out_col_hwp writes
        vd = padded(v, vs).view(nseq, vs, c).permute(2, 0, 1).reshape(c, nseq * vs).contiguous().to(dev)
    out = torch.full((nseq * l, c), float("nan"), dtype=dtype, device=dev)
    ops.encoder_attention(qd, kd, vd, out, nseq=nseq, l=l, heads=heads, head_dim=d, causal=bool(causal), k_seq_stride=ks, v_seq_stride=vs)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_encoder_attention_matches_sdpa(ops, case, mode):
    q, k, v, ref = _qkv(case, DT[mode])
    got = _run_attention(ops, case, DT[mode], q, k, v)
    print(f"encoder_attention {case} {mode}: {err_stats(got, ref)}")
    _check(got, ref, mode, f"encoder_attention {case} {mode}")


@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("case", [(2, 77, 2, 64, 1), (2, 17, 2, 80, 0)], ids=lambda c: "x".join(map(str, c)))
def test_encoder_attention_ignores_what_lies_past_l(ops, case, mode):
    """a per-sequence K / V stride larger than l, the rows (fp32 V^T: columns) past l filled with +-1e4: bit for bit the unpadded result"""
    q, k, v, ref = _qkv(case, DT[mode])
    plain = _run_attention(ops, case, DT[mode], q, k, v)
    padded = _run_attention(ops, case, DT[mode], q, k, v, kpad=11, fill=1e4)
    assert torch.equal(plain.view(torch.int16 if DT[mode] != torch.float32 else torch.int32),
                       padded.view(torch.int16 if DT[mode] != torch.float32 else torch.int32))
    _check(padded, ref, mode, f"padded encoder_attention {case} {mode}")


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_encoder_attention_on_slices_of_a_fused_projection(ops, mode):
    case = (2, 77, 2, 80, 0)
    q, k, v, ref = _qkv(case, DT[mode])
    got = _run_attention(ops, case, DT[mode], q, k, v, fused=True)
    _check(got, ref, mode, f"fused-buffer encoder_attention {mode}")


# ---- the small kernels
@pytest.mark.parametrize("mode", MODES, indirect=True)
@pytest.mark.parametrize("act", ["gelu", "quick_gelu"])
def test_act_rows(ops, mode, act):
    dtype = DT[mode]
    x = _rnd(34, 320, seed=5, scale=2.0).to(dtype)
    ref = cr.act_fn(act)(x.float())
    got = ops.act_rows(x.cuda(), act)
    _check(got.cpu(), ref, mode, f"act_rows {act}")
    wide = torch.full((34, 336), 7.0, dtype=dtype, device="cuda:0")       # strided, in place: columns 320.. stay untouched
    wide[:, :320] = x.cuda()
    ops.act_rows(wide[:, :320], act, out=wide[:, :320])
    assert torch.equal(wide[:, :320], got) and bool((wide[:, 320:] == 7.0).all())


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_patch_tokens_and_gemm_are_the_patch_conv(ops, mode):
    dtype = DT[mode]
    img = _rnd(2, 3, 56, 56, seed=6).to(dtype)
    w = (_rnd(160, 3, 14, 14, seed=7) / 24.0).to(dtype)
    ref = F.conv2d(img.float(), w.float(), stride=14).flatten(2).transpose(1, 2).reshape(2 * 16, 160)
    tok = ops.patch_tokens(img.float().cuda(), 14, dtype)
    assert tok.shape == (32, 592) and bool((tok[:, 588:] == 0).all())
    assert torch.equal(tok, ops.patch_tokens(img.cuda(), 14, dtype))            # fp32 and storage-typed sources agree
    want = img.float().view(2, 3, 4, 14, 4, 14).permute(0, 2, 4, 1, 3, 5).reshape(32, 588)
    assert torch.equal(tok[:, :588].float().cpu(), want)
    wp = torch.zeros(160, 592, dtype=dtype)
    wp[:, :588] = w.flatten(1)
    _check(ops.gemm(tok, wp.cuda()).cpu(), ref, mode, "patch conv")


@pytest.mark.parametrize("mode", MODES, indirect=True)
def test_embed_rows(ops, mode):
    dtype = DT[mode]
    table, pos = _rnd(1000, 128, seed=8).to(dtype), _rnd(77, 128, seed=9).to(dtype)
    ids = cr.inputs("T77")
    ids[0, 0], ids[1, 76] = 0, 999
    ref = (table.float()[ids] + pos.float()[None]).to(dtype).float().view(-1, 128)
    got = ops.embed_rows(table.cuda(), pos.cuda(), ids=ids.view(-1).cuda(), l=77)
    assert torch.equal(got.float().cpu(), ref)
    patches, cls, vpos = _rnd(2 * 16, 160, seed=10).to(dtype), _rnd(160, seed=11).to(dtype), _rnd(17, 160, seed=12).to(dtype)
    refv = (torch.cat([cls.float().expand(2, 1, 160), patches.float().view(2, 16, 160)], 1) + vpos.float()[None]).to(dtype).float().view(-1, 160)
    gotv = ops.embed_rows(patches.cuda(), vpos.cuda(), cls=cls.cuda(), l=17)
    assert torch.equal(gotv.float().cpu(), refv)


# ---- the native models
def _pair(name, dtype, compute=None, **override):
    from this_and_that_vdm_amd import clip
    ref, cfg = cr.build(name, round_to=dtype, **override)
    m = (clip.CLIPTextModel if "vocab_size" in cfg else clip.CLIPVisionModelWithProjection)(**cfg).eval()
    m.load_state_dict(ref.state_dict(), strict=True)
    m = m.to(device="cuda:0", dtype=dtype).requires_grad_(False)
    m.compute_dtype = compute
    return m, ref, cfg


_REF_OUT = {}


def _ref_out(name, dtype):
    """the fp32 restatement's outputs on weights rounded to `dtype` (once per configuration and dtype)"""
    if (name, dtype) not in _REF_OUT:
        ref, _ = cr.build(name, round_to=dtype)
        with torch.no_grad():
            _REF_OUT[(name, dtype)] = ref(cr.inputs(name))
    return _REF_OUT[(name, dtype)]


def _outputs(o):
    return [(k, getattr(o, k)) for k in ("image_embeds", "last_hidden_state") if getattr(o, k, None) is not None]


@pytest.mark.parametrize("mode", ["f32", "split16"], indirect=True)
@pytest.mark.parametrize("name", list(cr.TINY))
def test_native_model_matches_the_restatement_in_fp32(ops, name, mode):
    m, _, _ = _pair(name, torch.float32, torch.float32)
    got = m(cr.inputs(name).cuda())
    want = _ref_out(name, torch.float32)
    for k, w in _outputs(want):
        g = getattr(got, k)
        assert g.dtype == torch.float32 and g.shape == w.shape
        print(f"CLIP {name} {mode} {k} vs the restatement: {err_stats(g, w)}")
        assert_north_star(g, w, f"{name}.{k} ({mode})")
    if mode == "f32":
        check_against_golden(name, got, "native TT_F32 vs transformers")
    assert torch.equal(got[0], got.to_tuple()[0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "fp16"])
def test_text_model_on_short_prompts_and_reused_buffers(ops, dtype):
    """prompts of 1, 2 and 5 tokens (TT_F32: the padding rows of the swapped V^T launch land in pseudo-sequences past the last prompt),
    one and three prompts, and the same shape twice in a row: the buffers a model keeps between calls do not change a result"""
    m, ref, _ = _pair("T77", dtype, torch.float32 if dtype == torch.float32 else None)
    ids = cr.inputs("T77")
    last = prev = None
    for n, l in ((1, 1), (3, 1), (1, 2), (2, 5), (2, 5), (1, 77)):
        x = ids[:, :l].repeat(2, 1)[:n].contiguous()
        with torch.no_grad():
            want = ref(x).last_hidden_state
        got = m(x.cuda()).last_hidden_state
        assert got.shape == (n, l, 128) and bool(torch.isfinite(got).all())
        if dtype == torch.float32:
            assert_north_star(got, want, f"T77 with {n} prompt(s) of {l} token(s)")
        if (n, l) == last:                               # fp16's accuracy has its yardstick test below; here: reuse changes no bit
            assert torch.equal(got, prev)
        last, prev = (n, l), got.clone()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(cr.TINY))
def test_native_model_in_16_bits_is_no_worse_than_the_restatement_in_16_bits(ops, name, dtype):
    """the project's yardstick rule (tests/test_model_gpu.py): relative L2 against the fp32 restatement at most 1.25x the error the
    restatement itself makes when it runs in that dtype on the CPU (same rounded weights, measured here)"""
    m, ref, _ = _pair(name, dtype)
    x = cr.inputs(name)
    want = _ref_out(name, dtype)
    with torch.no_grad():
        yard = ref.to(dtype)(x if x.dtype == torch.int64 else x.to(dtype))
    got = m(x.cuda() if x.dtype == torch.int64 else x.to(dtype).cuda())
    for k, w in _outputs(want):
        g, y = getattr(got, k), getattr(yard, k)
        assert g.dtype == dtype
        h, ys = err_stats(g, w), err_stats(y, w)
        print(f"CLIP {name} {dtype} {k}: native rel_l2 {h['rel_l2']:.3e}, restatement in {dtype} on the CPU {ys['rel_l2']:.3e}")
        assert h["rel_l2"] <= 1.25 * ys["rel_l2"] + 1e-6, (k, h, ys)


@pytest.mark.parametrize("name,override", [
    ("V257", dict(hidden_size=1280, num_attention_heads=16, intermediate_size=5120, projection_dim=1024)),
    ("T77", dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, vocab_size=49408))], ids=["vision", "text"])
def test_shipped_widths_two_layers_fp32(ops, name, override):
    m, ref, cfg = _pair(name, torch.float32, torch.float32, **override)
    x = cr.inputs(name, cfg, batch=1)
    with torch.no_grad():
        want = ref(x)
    got = m(x.cuda())
    for k, w in _outputs(want):
        print(f"CLIP {name} at the shipped widths {k}: {err_stats(getattr(got, k), w)}")
        assert_north_star(getattr(got, k), w, f"{name}.{k} at the shipped widths")


# ---- the VGL pipeline with no stand-in model
VAE_TINY = dict(block_out_channels=(32, 64, 64, 64), layers_per_block=2)
PIPE_VISION = dict(cr.TINY["V257"], projection_dim=64)
PIPE_TEXT = dict(cr.TINY["T77"], hidden_size=64, num_attention_heads=1, intermediate_size=128, vocab_size=100, max_position_embeddings=77)


def _clip_pair(dtype):
    from this_and_that_vdm_amd import clip
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    rv, rt = cr.CLIPVisionModelWithProjection(**PIPE_VISION).eval(), cr.CLIPTextModel(**PIPE_TEXT).eval()
    with torch.no_grad():
        fill_parameters_(rv, "clip.", round_to=dtype)
        fill_parameters_(rt, "clip.", round_to=dtype)
    nv, nt = clip.CLIPVisionModelWithProjection(**PIPE_VISION).eval(), clip.CLIPTextModel(**PIPE_TEXT).eval()
    nv.load_state_dict(rv.state_dict())
    nt.load_state_dict(rt.state_dict())
    nv, nt = nv.to("cuda:0", dtype), nt.to("cuda:0", dtype)
    if dtype == torch.float32:
        nv.compute_dtype = nt.compute_dtype = torch.float32
    return nv, nt, rv, rt


def _native_vae(dtype):
    from tests.vae_encoder_reference import EncoderVAE
    from oracle import vae as ov
    from this_and_that_vdm_amd.svd.autoencoder_kl_temporal_decoder import AutoencoderKLTemporalDecoder
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    o_enc, o_dec = EncoderVAE(**VAE_TINY).eval(), ov.AutoencoderKLTemporalDecoder(**VAE_TINY).eval()
    fill_parameters_(o_enc, "vae.", round_to=dtype)
    fill_parameters_(o_dec, "vae.", round_to=dtype)
    sd = dict(o_enc.state_dict())
    sd.update(o_dec.state_dict())
    vae = AutoencoderKLTemporalDecoder(**VAE_TINY, native_encoder=True).eval()
    vae.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    vae = vae.to("cuda:0", dtype)
    if dtype == torch.float32:
        vae.compute_dtype = torch.float32
    return vae


@torch.no_grad()
def test_vgl_pipeline_with_native_vae_and_native_clip(ops):
    from PIL import Image
    from this_and_that_vdm_amd.svd import EulerDiscreteScheduler, StableVideoDiffusionControlNetPipeline
    g = torch.Generator().manual_seed(11)
    image = Image.fromarray((torch.rand(64, 128, 3, generator=g) * 255).to(torch.uint8).numpy())
    cond = torch.rand(4, 3, 64, 128, generator=g).numpy().astype(np.float32)
    ids = torch.randint(0, 100, (1, 77), generator=g)           # 77 text tokens + the image row: the real 78-token context
    lat0 = torch.randn(1, 4, 4, 8, 16, generator=torch.Generator().manual_seed(5))
    frames = {}
    for dtype in (torch.float32, torch.float16):
        unet, cn, _, _ = build_pair("tiny_vgl", dtype, "cuda:0", True)
        nv, nt, rv, rt = _clip_pair(dtype)
        pipe = StableVideoDiffusionControlNetPipeline.from_pretrained(None, vae=_native_vae(dtype), image_encoder=nv, unet=unet,
                                                                      scheduler=EulerDiscreteScheduler())
        pipe.set_progress_bar_config(disable=True)
        if dtype == torch.float32:
            ehs = pipe.encode_clip(image, ids.cuda(), True, nt, "cuda", 1, True)
            assert ehs.shape == (2, 78, 64)
            stand_in = SimpleNamespace(image_encoder=rv, image_processor=pipe.image_processor, feature_extractor=pipe.feature_extractor)
            want = type(pipe).encode_clip(stand_in, image, ids, True, lambda p: (rt(p).last_hidden_state,), "cpu", 1, True)
            print("encode_clip, native CLIP pair (TT_F32) vs the restatement through the same function:", err_stats(ehs, want))
            assert_north_star(ehs, want, "encode_clip context")
        out = pipe(image, cond, cn, latents=lat0.clone(), output_type="np", prompt=ids.cuda(), use_text=True, text_encoder=nt, height=64,
                   width=128, num_frames=4, num_inference_steps=3, fps=7, motion_bucket_id=200, noise_aug_strength=0.0, guess_mode=False,
                   decode_chunk_size=3).frames
        assert out.shape == (1, 4, 64, 128, 3) and np.isfinite(out).all()
        frames[dtype] = out
    print("fp16 frames vs TT_F32 frames: max abs", float(np.abs(frames[torch.float16] - frames[torch.float32]).max()))
