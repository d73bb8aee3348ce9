"""GPU: the request path around the models on the library's kernels -- tt_clip_image, tt_layernorm_block, tt_frames_out through their
ops front ends, and the pipelines with ``native_image_io=True`` against the same pipelines with the option off.

Yardsticks are the torch request path as it stands (pipeline_utils.resize_with_antialiasing, CLIPFeatureExtractor, nn.LayerNorm's
definition, VaeImageProcessor.postprocess / numpy_to_pil), evaluated on the CPU -- in fp64 wherever the check is a bound, in their own
fp32 where it is bit-equality.  Every bound below is derived from the arithmetic the kernels are documented to do (include/ttvdm.h),
to first order in u = 2^-24, before any measurement; the tests print worst error / bound and then assert."""
import functools

import numpy as np
import PIL.Image
import pytest
import torch
import torch.nn.functional as F

from this_and_that_vdm_amd.svd.pipeline_utils import CLIPFeatureExtractor, VaeImageProcessor, resize_with_antialiasing

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}        # unit roundoff: half an ulp relative to the stored value, at most
ABS_FLOOR = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25, torch.float32: 0.0}              # fp16 subnormals: half their spacing
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops
    return ops


# ================================================================================================ tt_clip_image
FE = CLIPFeatureExtractor()
CLIP_CONST = 20


def taps(n_in, n_out):
    s = max((n_in / n_out - 1.0) / 2.0, 0.001)
    k = int(max(4.0 * s, 3))
    return k + 1 - k % 2


def clip_bound(ref, h, w, size, dtype):
    """|got - ref| <= (kx + ky + 20) u 1.89 / std_c  (+ half an ulp of 16-bit storage), u = 2^-24.  Where the 20 comes from, following
    one output element through the kernels (all values are sums of |v| <= 1 with non-negative blur weights summing to 1 and signed bicubic
    weights whose absolute sum per axis is at most 1.375, reached at t = 1/2 with A = -0.75: 1.375^2 < 1.89):
      v = 2 x - 1                                  one rounding of |v| <= 1:                                      1 u
      blur x: k_x-term fmaf chain, sum w = 1       k_x u, + 1 u for the taps rounded from fp64 to fp32:           (k_x + 1) u
      blur y                                       the same:                                                     (k_y + 1) u
        -> the blurred value b carries (k_x + k_y + 3) u, and |b| <= 1
      bicubic  r = sum_i Wy_i sum_j Wx_j b_ij      the carried error times 1.375^2:                               1.89 (k_x + k_y + 3) u
        weights: t = rem / (out - 1) is one correctly rounded division of exact integers (<= u); the inner two weights are
        fmaf(fmaf(1.25, t, -2.25) t, t, 1): roundings 2.25 u, 1.02 u, 1 u carried to the result, + |dW/dt| <= 1.35 times the error of
        t: <= 6 u each; the outer two are the products A t (1 - t)^2: four roundings of a value <= 0.111 + 0.75 u from t: <= 1.3 u each.
        Per axis sum_j |dW_j| <= 14.6 u -> 15 u;  x axis: 15 u |b| 1.375, y axis: 15 u times a row sum <= 1.375:            41.3 u
        the two 4-term fmaf chains: 4 u 1.375 each, the inner one times 1.375:                                          13.1 u
      y = (r + 1) / 2                               |r + 1| <= 2.89: 2.9 u, then everything halves:                   y carries
                                                   [1.89 (k_x + k_y + 3) + 41.3 + 13.1 + 2.9] u / 2 = [0.945 (k_x + k_y) + 31.5] u
      (y - mean_c) / std_c                          subtraction (|y - mean| <= 1.05): 1.05 u; mean_c and std_c are the fp32 values of
                                                   the extractor's doubles: 0.5 u and 1.05 u; the division rounds once: 1.05 u  -> 3.65 u
    Sum: [0.945 (k_x + k_y) + 35.2] u / std_c  <=  1.89 (k_x + k_y + 20) u / std_c  (1.89 * 20 = 37.8; the stated form keeps the full
    1.89 on the tap counts).  A 16-bit store adds half an ulp of the stored value (fp16: at least half a subnormal step)."""
    ky, kx = taps(h, size[0]), taps(w, size[1])
    std = torch.tensor(FE.image_std, dtype=torch.float64).view(1, 3, 1, 1)
    b32 = ((kx + ky + CLIP_CONST) * U * 1.89 / std).expand_as(ref)
    return b32 + HALF_ULP[dtype] * (ref.abs() + b32) + ABS_FLOOR[dtype]


def blur_resize_fp64(v, size, align_corners=True, pad_mode="reflect"):
    """pipeline_utils.resize_with_antialiasing with its two fixed choices exposed, for the mutants (identical to it at the defaults:
    asserted in the test)"""
    from this_and_that_vdm_amd.svd.pipeline_utils import _gauss_kernel1d
    h, w = v.shape[-2:]
    ky, kx = taps(h, size[0]), taps(w, size[1])
    sy, sx = max((h / size[0] - 1.0) / 2.0, 0.001), max((w / size[1] - 1.0) / 2.0, 0.001)
    b, c = v.shape[:2]
    out = v
    for k1d, k, horizontal in ((_gauss_kernel1d(kx, sx, v.dtype), kx, True), (_gauss_kernel1d(ky, sy, v.dtype), ky, False)):
        pad = (k // 2, k // 2, 0, 0) if horizontal else (0, 0, k // 2, k // 2)
        x = F.pad(out, pad, mode=pad_mode)
        wgt = k1d.view(1, 1, 1, k) if horizontal else k1d.view(1, 1, k, 1)
        out = F.conv2d(x.reshape(b * c, 1, *x.shape[-2:]), wgt).reshape(b, c, h, w)
    return F.interpolate(out, size=size, mode="bicubic", align_corners=align_corners)


def normalise_fp64(x01):
    """CLIPFeatureExtractor's (x - image_mean) / image_std with its own constants, in fp64 (its __call__ casts to fp32 first, which would
    round the yardstick; that the formula is the class's is asserted in the test)"""
    mean = torch.tensor(FE.image_mean, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(FE.image_std, dtype=torch.float64).view(1, 3, 1, 1)
    return (x01 - mean) / std


@functools.lru_cache(maxsize=None)
def clip_case(h, w, size, nimg, kind):
    """(source as the op takes it, fp64 reference): uint8 [n, h, w, 3] or fp32 [n, 3, h, w] in [0, 1]; computed once per case"""
    g = torch.Generator().manual_seed(1000 * h + 10 * w + nimg)
    if kind == "u8":
        src = torch.randint(0, 256, (nimg, h, w, 3), generator=g, dtype=torch.uint8)
        x01 = VaeImageProcessor.numpy_to_pt(VaeImageProcessor.pil_to_numpy(list(src.numpy())))      # fp32 u / 255, as encode_clip forms it
    else:
        src = x01 = torch.rand(nimg, 3, h, w, generator=g)
    x = x01.double()
    ref = normalise_fp64((resize_with_antialiasing(x * 2.0 - 1.0, size) + 1.0) / 2.0)
    return src, x, ref


CLIP_SHAPES = [
    ((20, 28), (8, 12), False),        # 3 taps on both axes
    ((64, 40), (8, 8), True),          # 15 / 9 taps, kx != ky, reflect pad of 7 against a 64-row image
    ((6, 10), (12, 20), False),        # upscale: sigma = 1e-3 makes the blur an identity, bicubic border clamping
    ((9, 9), (9, 9), False),           # align_corners makes it the identity
    ((37, 53), (224, 224), False),     # the pipeline's output size
    ((256, 384), (224, 224), True),    # the reference's default image, taps 3 and 3
]


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("nimg", [1, 2])
@pytest.mark.parametrize("hw,size,all_dtypes", CLIP_SHAPES, ids=[f"{a[0]}x{a[1]}to{b[0]}x{b[1]}" for a, b, _ in CLIP_SHAPES])
def test_clip_image_against_the_fp64_torch_path(ops, hw, size, all_dtypes, nimg, kind):
    h, w = hw
    src, x, ref = clip_case(h, w, size, nimg, kind)
    if (h, w) == (64, 40):
        assert (taps(h, size[0]), taps(w, size[1])) == (15, 9)
    if hw == size:                                  # identity: the output is the normalised input
        assert float((ref - normalise_fp64(x)).abs().max()) <= 1e-14
    for dtype in (DTYPES if all_dtypes else (torch.float32,)):
        got = ops.clip_image(src.to(DEV), size, FE.image_mean, FE.image_std, dtype)
        assert got.shape == (nimg, 3, *size) and got.dtype == dtype and got.is_contiguous()
        err = (got.double().cpu() - ref).abs()
        bound = clip_bound(ref, h, w, size, dtype)
        print(f"clip_image {h}x{w}->{size[0]}x{size[1]} n={nimg} {kind} {dtype}: max err {float(err.max()):.3e}, worst err/bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), float((err / bound).max())
        if hw == size:
            assert bool(((got.double().cpu() - normalise_fp64(x)).abs() <= bound).all())
    if (h, w) == (64, 40):
        # CPU side of the same check: the bound the kernel has just met would flag an implementation with align_corners=False, or with
        # zero padding instead of reflect padding (each evaluated exactly, in fp64) -- and the yardstick pieces this file restates are the
        # package's own
        v = x * 2.0 - 1.0
        assert torch.equal(blur_resize_fp64(v, size), resize_with_antialiasing(v, size))
        y = (blur_resize_fp64(v, size) + 1.0) / 2.0
        assert float((FE(images=y).pixel_values.double() - normalise_fp64(y)).abs().max()) <= 2.0 ** -22      # the class's formula, in its fp32
        bound = clip_bound(ref, h, w, size, torch.float32)
        for name, kw in (("align_corners=False", dict(align_corners=False)), ("zero padding", dict(pad_mode="constant"))):
            mutant = normalise_fp64((blur_resize_fp64(v, size, **kw) + 1.0) / 2.0)
            worst = float(((mutant - ref).abs() / bound).max())
            print(f"mutant {name}: worst err/bound {worst:.1f}")
            assert worst > 1.0, name


# ================================================================================================ tt_layernorm_block
def ln_bound(y, mean, std, dtype):
    """|got - y| <= 2^-20 (1 + |y|) (1 + |mean| / std)  + half an ulp of storage.  The kernel's own budget is far inside: its fp32 mean is
    off by u |mean| (+ the pivoted sum's u-sized relative error of a std-sized quantity), which moves y by u |mean| / std; the centred
    squares and rsqrt carry a few u relative, which moves y by a few u |y|: 16 u leaves an order of magnitude."""
    b = 2.0 ** -20 * (1.0 + y.abs()) * (1.0 + mean.abs() / std)
    return b + HALF_ULP[dtype] * (y.abs() + b) + ABS_FLOOR[dtype]


def ln_reference(x, nb, rows, c, eps=1e-5):
    """x: the stored values [nb * rows, c] -> fp64 (y, mean, std) with mean / std broadcastable to y"""
    xb = x.double().reshape(nb, rows * c)
    mean = xb.mean(1, keepdim=True)
    var = ((xb - mean) ** 2).mean(1, keepdim=True)
    y = ((xb - mean) / torch.sqrt(var + eps)).reshape(nb * rows, c)
    e = lambda t: t.repeat_interleave(rows, 0)
    return y, e(mean), e(torch.sqrt(var))


LN_SHAPES = [(1, 1, 8, 8), (1, 1, 2056, 2056), (3, 78, 1024, 1024), (2, 5, 24, 40)]         # (nb, rows, c, ldx)


@pytest.mark.parametrize("dtype,inplace", [(torch.float32, False), (torch.float16, False), (torch.bfloat16, False), (torch.float32, True),
                                           (torch.bfloat16, True)], ids=["f32", "f16", "bf16", "f32-inplace", "bf16-inplace"])
@pytest.mark.parametrize("nb,rows,c,ldx", LN_SHAPES, ids=[f"{a}x{b}x{c}ld{d}" for a, b, c, d in LN_SHAPES])
def test_layernorm_block(ops, nb, rows, c, ldx, dtype, inplace):
    g = torch.Generator().manual_seed(nb * 100 + rows)
    SENT = 7.0
    buf = torch.full((nb * rows, ldx), SENT, dtype=dtype)
    buf[:, :c] = (torch.randn(nb * rows, c, generator=g) * 1.5 + 0.25).to(dtype)
    y_ref, mean, std = ln_reference(buf[:, :c], nb, rows, c)
    xd = buf.to(DEV)
    x = xd[:, :c]
    if inplace:
        got = ops.layernorm_block(x, rows, out=x)
        assert got.data_ptr() == x.data_ptr()
        full = xd
    else:
        full = torch.full((nb * rows, ldx), SENT, dtype=dtype, device=DEV)
        got = ops.layernorm_block(x, rows, out=full[:, :c])
        assert torch.equal(xd.cpu(), buf)                                      # the input is untouched
    assert bool((full[:, c:].cpu() == SENT).all())                             # padding columns are untouched
    err = (got.double().cpu() - y_ref).abs()
    bound = ln_bound(y_ref, mean, std, dtype)
    print(f"layernorm_block {nb}x{rows}x{c} ld {ldx} {dtype} inplace={inplace}: worst err/bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    if not inplace and ldx == c:                                               # the default output: x's shape and strides
        again = ops.layernorm_block(x, rows)
        assert again.stride() == x.stride() and torch.equal(again, got)


def test_layernorm_block_mean_100_std_01_needs_the_centred_form(ops):
    """The workload's shape with mean 100 and std 0.1 (fp32): the kernel is inside the bound, and the single-pass formula
    var = E[x^2] - E[x]^2 evaluated in fp32 -- shown here on the CPU -- is not: E[x^2] ~ 10000.01 has an fp32 spacing of 1e-3, a tenth of
    the variance it is meant to carry."""
    nb, rows, c = 3, 78, 1024
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(nb * rows, c, generator=g, dtype=torch.float64) * 0.1 + 100.0).float()
    y_ref, mean, std = ln_reference(x, nb, rows, c)
    assert abs(float(mean[0, 0]) - 100.0) < 1e-2 and abs(float(std[0, 0]) - 0.1) < 1e-3
    bound = ln_bound(y_ref, mean, std, torch.float32)
    xb = x.reshape(nb, rows * c)
    m1 = xb.mean(1, keepdim=True)
    var1 = (xb * xb).mean(1, keepdim=True) - m1 * m1                            # fp32 throughout
    y1 = ((xb - m1) / torch.sqrt(var1.clamp_min(0.0) + 1e-5)).reshape(nb * rows, c)
    worst1 = float(((y1.double() - y_ref).abs() / bound).max())
    print(f"single-pass fp32 formula: worst err/bound {worst1:.1f}")
    assert worst1 > 1.0
    got = ops.layernorm_block(x.to(DEV), rows)
    err = (got.double().cpu() - y_ref).abs()
    print(f"layernorm_block mean 100 / std 0.1: worst err/bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), float((err / bound).max())


# ================================================================================================ tt_frames_out
def rounding_ties():
    """every fp32 x with fl(fl(x / 2 + 0.5) * 255) == k + 0.5 exactly, k = 0 .. 254 (searched on the 2^-25 grid around 2 (k + 0.5) / 255 - 1;
    x / 2 + 0.5 lands on a grid no finer than that, so finer x only repeat the same sums).  Not every k has one: the product is rounded
    to fp32 and can step over k + 0.5."""
    out = []
    j = np.arange(-256, 257, dtype=np.float64) * 2.0 ** -25
    for k in range(255):
        x = np.unique((2.0 * (k + 0.5) / 255.0 - 1.0 + j).astype(np.float32))
        p = (x / np.float32(2) + np.float32(0.5)) * np.float32(255)
        out.append(x[p == np.float32(k + 0.5)])
    return np.concatenate(out)


def frame_inputs(shape, dtype):
    ties = rounding_ties()
    assert ties.size >= 64 and np.float32(0.0) in ties                      # k = 127 at the least: 0.5 * 255 = 127.5
    special = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 1.5, -1.5, 3.0, -7.0, 1.0 + 2.0 ** -23, -1.0 - 2.0 ** -23, 1.0 - 2.0 ** -24,
                                        -1.0 + 2.0 ** -24, 1e-30, -1e-30, 2.0 ** -140, 65504.0, -65504.0], dtype=np.float32), ties])
    sp = torch.from_numpy(special).to(dtype)
    if dtype != torch.float32:                                               # ties that survive the cast first, then the rest (rounded)
        exact = sp.float() == torch.from_numpy(special)
        sp = torch.cat([sp[exact], sp[~exact]])
    n = int(np.prod(shape))
    x = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.8).to(dtype)
    m = min(n, sp.numel())
    x[:m] = sp[:m]
    return x.reshape(shape)


FRAME_SHAPES = [(1, 2, 8), (2, 5, 7), (2, 5, 63), (14, 32, 56)]      # 2 x 5 x 63: odd width (the one-pixel-per-lane kernel), room for every tie


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("n,h,w", FRAME_SHAPES, ids=[f"{a}x{b}x{c}" for a, b, c in FRAME_SHAPES])
def test_frames_out_is_bit_equal_to_postprocess(ops, n, h, w, ch, dtype):
    x = frame_inputs((n, ch, h, w), dtype)
    want_np = VaeImageProcessor().postprocess(x.float(), "np")                 # decode_latents hands tensor2vid fp32 (.float())
    want_u8 = (want_np * 255).round().astype("uint8")                          # numpy_to_pil's rounding
    assert want_np.dtype == np.float32 and want_np.shape == (n, h, w, ch)
    xd = x.to(DEV)
    got_np = ops.frames_out(xd, 0)
    got_u8 = ops.frames_out(xd, 1)
    assert got_np.dtype == torch.float32 and got_u8.dtype == torch.uint8 and got_np.shape == got_u8.shape == (n, h, w, ch)
    assert np.array_equal(got_np.cpu().numpy().view(np.int32), want_np.view(np.int32))
    assert np.array_equal(got_u8.cpu().numpy(), want_u8)
    if n * ch * h * w >= 630:                                                  # the specials and all ties fit
        assert x.numel() >= 17 + rounding_ties().size
        assert 0 in want_u8 and 255 in want_u8 and (want_np == 0.5).any()


# ================================================================================================ the pipelines
class StubVision64(torch.nn.Module):
    """tests.stubs.StubCLIPVision in fp64 on the CPU: carries the fp64 yardstick image through the same pooling and projection"""

    def __init__(self, stub):
        super().__init__()
        self.w, self.b = stub.proj.weight.detach().double().cpu(), stub.proj.bias.detach().double().cpu()

    def forward(self, image):
        return F.adaptive_avg_pool2d(image, 8).flatten(1) @ self.w.T + self.b


@pytest.fixture(scope="module")
def pipe(ops):
    from tests.parity_common import build_pair
    from tests.stubs import StubCLIPVision, StubTextEncoder, StubVAE
    from this_and_that_vdm_amd.svd import StableVideoDiffusionPipeline
    p_unet, _, _, _ = build_pair("tiny_vgl", torch.float16, "cuda:0", False)
    vae = StubVAE().to(DEV).half()
    # two pipelines over one UNet: an fp16 one for whole requests, and one whose stub CLIP encoder is fp32 for the encode_clip comparison
    # (encode_clip touches neither the UNet nor the VAE)
    p16 = StableVideoDiffusionPipeline.from_pretrained(None, vae=vae, image_encoder=StubCLIPVision().to(DEV).half(), unet=p_unet)
    p32 = StableVideoDiffusionPipeline.from_pretrained(None, vae=vae, image_encoder=StubCLIPVision().to(DEV), unet=p_unet)
    for p in (p16, p32):
        p.set_progress_bar_config(disable=True)
    return p16, p32, StubTextEncoder().to(DEV)


def _pil_image():
    g = np.random.default_rng(3)
    return PIL.Image.fromarray(g.integers(0, 256, (64, 96, 3), dtype=np.uint8))


def _forbid_torch_path(monkeypatch):
    from this_and_that_vdm_amd.svd import pipeline_stable_video_diffusion_controlnet as mod

    def boom(*a, **k):
        raise AssertionError("the torch path was taken")
    monkeypatch.setattr(mod, "resize_with_antialiasing", boom)
    monkeypatch.setattr(mod, "tensor2vid", boom)


@torch.no_grad()
def test_encode_clip_native_agrees_with_the_torch_path(pipe, monkeypatch):
    """encode_clip of one 64 x 96 PIL image with the option on against the option off, through an fp32 stub encoder (the pipeline's
    encoder dtype is the preprocessing's output dtype).  The two paths are not compared by a fitted tolerance: the fp64 yardstick image is
    carried through an fp64 copy of the stub encoder (and, with use_text, an fp64 LayerNorm over the [5, 64] context), which gives the
    torch path's OWN error d_off per element; the native path's budget T is the kernel bounds propagated through the stub:
      pooling (a mean of 28 x 28 pixels of one channel): the per-pixel bound of that channel, + 784 u max|pixel| for the fp32 mean;
      projection e_j = sum_i W_ji p_i + b_j (192 terms):  sum_i |W_ji| dp_i + 193 u (sum_i |W_ji| |p_i| + |b_j|);
      LayerNorm over the context (only the image row moves, by at most D = max_j T_j; mean moves by <= D, std by <= D):
          (2 + |y|) D / std  (first order; D / std ~ 1e-4)  + tt_layernorm_block's own bound.
    Then |on - off| <= T + d_off by the triangle inequality."""
    _, p, txt = pipe
    image = _pil_image()
    ids = torch.arange(8).view(1, 8).to(DEV)
    x = VaeImageProcessor.numpy_to_pt(VaeImageProcessor.pil_to_numpy(image)).double()
    img64 = normalise_fp64((resize_with_antialiasing(x * 2.0 - 1.0, (224, 224)) + 1.0) / 2.0)
    enc64 = StubVision64(p.image_encoder)
    emb64 = enc64(img64)                                                                       # [1, 64]
    pix = clip_bound(img64, 64, 96, (224, 224), torch.float32)
    dpool = F.adaptive_avg_pool2d(pix, 8).flatten(1) + 784 * U * float(img64.abs().max())
    pool64 = F.adaptive_avg_pool2d(img64, 8).flatten(1)
    t_emb = dpool @ enc64.w.abs().T + 193 * U * (pool64.abs() @ enc64.w.abs().T + enc64.b.abs())
    text64 = txt(ids)[0].double().cpu()                                                        # an embedding lookup: exact
    ctx64 = torch.cat([text64, emb64.unsqueeze(1)], 1)                                         # [1, 5, 64]
    mean, std = ctx64.mean(), ctx64.std(unbiased=False)
    ln64 = (ctx64 - mean) / torch.sqrt(ctx64.var(unbiased=False) + 1e-5)
    big_d = float(t_emb.max())
    t_ln = (2.0 + ln64.abs()) * big_d / float(std) + ln_bound(ln64, mean, std, torch.float32)
    for use_text, truth, budget in ((False, emb64.unsqueeze(1), t_emb.unsqueeze(1)), (True, ln64, t_ln)):
        p.native_image_io = False
        off = p.encode_clip(image, ids, use_text, txt, DEV, 1, True).double().cpu()
        p.native_image_io = True
        with monkeypatch.context() as mp:
            _forbid_torch_path(mp)
            on = p.encode_clip(image, ids, use_text, txt, DEV, 1, True).double().cpu()
        p.native_image_io = False
        assert on.shape == off.shape == (2, *truth.shape[1:]) and float(on[0].abs().max()) == 0.0 and float(off[0].abs().max()) == 0.0
        d_off, d_on = (off[1:] - truth).abs(), (on[1:] - truth).abs()
        print(f"encode_clip use_text={use_text}: native vs fp64 worst err/budget {float((d_on / budget).max()):.3f}; torch path's own error "
              f"max {float(d_off.max()):.3e}; |on - off| max {float((on - off).abs().max()):.3e}")
        assert bool((d_on <= budget).all()), float((d_on / budget).max())
        assert bool(((on[1:] - off[1:]).abs() <= budget + d_off).all())


@torch.no_grad()
def test_pipeline_frames_native_equal_the_torch_path(pipe, monkeypatch):
    """pipe(64 x 96 PIL image, height=64, width=128, latents=...) with fixed latents, decoded in chunks of 3 (4 frames: 3 + 1): "np" frames equal the option-off
    frames exactly and "pil" frames are pixel-identical, with tensor2vid (and the torch resize) made unreachable in the native runs.
    Fixed latents alone do not make the two runs comparable bit for bit: the CLIP context enters every step, and the native preprocessing
    agrees with the torch one within a bound (the test above), not in every bit.  So both runs are given the SAME context -- the option-off
    encode_clip's, computed once -- and everything else (VAE image path, loop, chunked decode, export) runs for real in both.  One more
    native run without the pinned context covers the whole path end to end (PIL -> ops.clip_image -> loop -> ops.frames_out)."""
    p, _, _ = pipe
    image = _pil_image()
    lat0 = torch.randn(1, 4, 4, 8, 16, generator=torch.Generator().manual_seed(5))
    call = dict(height=64, width=128, num_frames=4, num_inference_steps=2, noise_aug_strength=0.0, decode_chunk_size=3)
    p.native_image_io = False
    ehs = p.encode_clip(image, None, False, None, DEV, 1, True)
    try:
        with monkeypatch.context() as mp:
            mp.setattr(p, "encode_clip", lambda *a, **k: ehs.clone())
            off_np = p(image, latents=lat0.clone(), output_type="np", **call).frames
            off_pil = p(image, latents=lat0.clone(), output_type="pil", **call).frames
            p.native_image_io = True
            _forbid_torch_path(mp)
            on_np = p(image, latents=lat0.clone(), output_type="np", **call).frames
            on_pil = p(image, latents=lat0.clone(), output_type="pil", **call).frames
        with monkeypatch.context() as mp:
            _forbid_torch_path(mp)
            whole = p(image, latents=lat0.clone(), output_type="np", **call).frames
    finally:
        p.native_image_io = False
    assert on_np.shape == off_np.shape == (1, 4, 64, 128, 3) and on_np.dtype == off_np.dtype == np.float32 and np.isfinite(off_np).all()
    assert np.array_equal(on_np.view(np.int32), off_np.view(np.int32))
    assert len(on_pil) == len(off_pil) == 1 and len(on_pil[0]) == len(off_pil[0]) == 4
    for a, b in zip(on_pil[0], off_pil[0]):
        assert isinstance(a, PIL.Image.Image) and a.size == b.size == (128, 64) and a.mode == b.mode
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert float(off_np.min()) >= 0.0 and float(off_np.max()) <= 1.0 and float(off_np.std()) > 0.0      # frames, not a constant
    assert whole.shape == off_np.shape and np.isfinite(whole).all()
    # the whole native path against the torch path: the contexts agree within encode_clip's budget (~1e-6 before the fp16 encoder rounds
    # them: a last-place step of a few context entries), the tiny UNet runs two fp16 steps on it, and the decoder's fp16 samples step by
    # 2^-11 in frame units below 1.  Not a derived bound -- the UNet has none -- but a loose one: 16 such steps.
    assert float(np.abs(whole - off_np).max()) <= 2.0 ** -7
    print("frames of the whole native path vs the torch path (contexts differ within encode_clip's bound): max abs",
          float(np.abs(whole - off_np).max()))
