"""GPU: tt_gemm's wide route (windowed descriptors, include/ttvdm.h "Operand sizes") bit for bit against the narrow route.

An operand of 2 GiB and more is a view with a large row stride into one 5 GB allocation: only the used columns are filled, so a launch
computes for microseconds while a0 / out / residual / blend really span more than 2 GiB of address space.  The same values in compact
tensors run the narrow route on the same tile configuration (tests/test_gemm_wide_cpu.py asserts the plans agree), and the outputs must
be EQUAL: same tile, ring, K order and epilogue arithmetic.  Every launch is checked to have run on the route it is meant to test
(ops.WIDE_LAUNCHES).  Last: one dense GroupNorm over a tensor beyond 2 GiB (norm.hip indexes with 64-bit pointers; the decoder at
576x1024 depends on it) under the bound of tests/test_norm_bounds_gpu.py."""
import pytest
import torch

from tests import error_bounds as eb

pytestmark = pytest.mark.gpu
G2 = 1 << 31
KINDS = ["bf16", "fp16", "f32", "split16"]
DT = dict(bf16=torch.bfloat16, fp16=torch.float16, f32=torch.float32, split16=torch.float32)


@pytest.fixture(scope="module")
def arena():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    buf = torch.empty(5 << 30, dtype=torch.uint8, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture
def ops(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    kind = request.node.callspec.params.get("kind", "bf16") if hasattr(request.node, "callspec") else "bf16"
    o.set_f32_split(kind == "split16")
    o.set_gemm_wide(1)
    yield o
    o.set_f32_split(False)
    o.set_gemm_wide(1)


def big_view(arena, slot, rows, cols, dtype, values=None, guard=8):
    """[rows, cols] view into half `slot` (0 / 1) of the arena whose rows lie far enough apart to span 2 GiB or more; the `guard`
    columns behind every row hold a sentinel (1.0) that no launch may touch"""
    es = torch.empty((), dtype=dtype).element_size()
    ld = (-(-G2 // ((rows - 1) * es)) + 7) // 8 * 8 + 8
    nbytes = rows * ld * es
    assert nbytes <= arena.numel() // 2
    half = arena[slot * (arena.numel() // 2):][:nbytes].view(dtype).view(rows, ld)
    v = half[:, :cols]
    assert ((rows - 1) * ld + cols) * es >= G2 and v.stride(0) == ld
    if values is not None:
        v.copy_(values)
    half[:, cols:cols + guard] = 1.0
    return v, half[:, cols:cols + guard]


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(dtype)


def run(ops, wide, fn):
    """fn() with the launch counter checked: exactly one launch, on the wide route or not"""
    n0 = ops.WIDE_LAUNCHES
    out = fn()
    assert ops.WIDE_LAUNCHES - n0 == (1 if wide else 0), f"expected {'the wide' if wide else 'a narrow'} launch"
    return out


def intact(guard):
    return bool((guard == 1.0).all())


# ---- mode 0: 300 x 136 x 128 (ragged row and column tiles)
M0, N0, K0 = 300, 136, 128


@pytest.mark.parametrize("kind", KINDS)
def test_linear_a0_beyond_2_gib(ops, arena, kind):
    dt = DT[kind]
    a, w, bias = rnd((M0, K0), dt, 1), rnd((N0, K0), dt, 2, 0.1), rnd((N0,), torch.float32, 3)
    a_big, guard = big_view(arena, 0, M0, K0, dt, a)
    narrow = run(ops, False, lambda: ops.gemm(a, w, bias=bias, acc_scale=0.5))
    wide = run(ops, True, lambda: ops.gemm(a_big, w, bias=bias, acc_scale=0.5))
    print(f"[wide] mode 0 a0 {kind}: max abs diff {(wide.float() - narrow.float()).abs().max().item():.3g}")
    assert torch.equal(wide, narrow) and intact(guard)
    if dt != torch.float32:                             # fp32 out of 16-bit storage (the per-fragment path: 64-bit pointers)
        o_big, og = big_view(arena, 1, M0, N0, torch.float32)
        n32 = run(ops, False, lambda: ops.gemm(a, w, bias=bias, out_f32=True))
        run(ops, True, lambda: ops.gemm(a_big, w, bias=bias, out_f32=True, out=o_big))
        assert torch.equal(o_big, n32) and intact(og)


@pytest.mark.parametrize("kind", KINDS)
def test_linear_out_beyond_2_gib_in_place_on_the_residual(ops, arena, kind):
    dt = DT[kind]
    a, w, bias, res = rnd((M0, K0), dt, 4), rnd((N0, K0), dt, 5, 0.1), rnd((N0,), torch.float32, 6), rnd((M0, N0), dt, 7)
    o_big, guard = big_view(arena, 0, M0, N0, dt, res)
    narrow = res.clone()
    run(ops, False, lambda: ops.gemm(a, w, bias=bias, residual=narrow, out=narrow))
    run(ops, True, lambda: ops.gemm(a, w, bias=bias, residual=o_big, out=o_big))
    print(f"[wide] mode 0 out = residual {kind}: max abs diff {(o_big.float() - narrow.float()).abs().max().item():.3g}")
    assert torch.equal(o_big, narrow) and intact(guard)
    assert not torch.equal(narrow, res)


@pytest.mark.parametrize("kind", KINDS)
def test_linear_blend_beyond_2_gib(ops, arena, kind):
    dt = DT[kind]
    a, w, bias = rnd((M0, K0), dt, 8), rnd((N0, K0), dt, 9, 0.1), rnd((N0,), torch.float32, 10)
    res, bl = rnd((M0, N0), dt, 11), rnd((M0, N0), dt, 12)
    bl_big, guard = big_view(arena, 0, M0, N0, dt, bl)
    res_big, rguard = big_view(arena, 1, M0, N0, dt, res)
    # a blend tensor of its own (read inside the passes), with a compact and with a wide residual
    narrow = run(ops, False, lambda: ops.gemm(a, w, bias=bias, residual=res, blend=bl, alpha=0.3))
    wide = run(ops, True, lambda: ops.gemm(a, w, bias=bias, residual=res, blend=bl_big, alpha=0.3))
    both = run(ops, True, lambda: ops.gemm(a, w, bias=bias, residual=res_big, blend=bl_big, alpha=0.3))
    print(f"[wide] mode 0 blend {kind}: max abs diff {(wide.float() - narrow.float()).abs().max().item():.3g}")
    assert torch.equal(wide, narrow) and torch.equal(both, narrow)
    # the AlphaBlender's usual form: the blend source is the residual itself
    narrow = run(ops, False, lambda: ops.gemm(a, w, bias=bias, residual=res, blend=res, alpha=0.3))
    wide = run(ops, True, lambda: ops.gemm(a, w, bias=bias, residual=res_big, blend=res_big, alpha=0.3))
    assert torch.equal(wide, narrow) and intact(guard) and intact(rguard)


# ---- mode 1: 24 images of 4 x 6, 64 -> 64 channels: a 128-row tile spans six images (borders and the zero halo inside one window)
NIMG, H1, W1, C1 = 24, 4, 6, 64


@pytest.mark.parametrize("upsample", [0, 1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_conv3x3_a0_beyond_2_gib(ops, arena, kind, upsample):
    dt = DT[kind]
    rows_in = NIMG * H1 * W1
    ho, wo = (2 * H1, 2 * W1) if upsample else (H1, W1)
    taps = 16 if upsample == 2 else 9
    a, w, bias = rnd((rows_in, C1), dt, 20 + upsample), rnd((C1, taps * C1), dt, 30, 0.05), rnd((C1,), torch.float32, 31)
    conv = (NIMG, H1, W1, ho, wo, 1, upsample)
    res = rnd((NIMG * ho * wo, C1), dt, 32) if upsample != 2 else None          # (upsample = 2: bias-only epilogue)
    a_big, guard = big_view(arena, 0, rows_in, C1, dt, a)
    narrow = run(ops, False, lambda: ops.gemm(a, w, mode=1, conv=conv, bias=bias, residual=res))
    wide = run(ops, True, lambda: ops.gemm(a_big, w, mode=1, conv=conv, bias=bias, residual=res))
    print(f"[wide] mode 1 upsample {upsample} a0 {kind}: max abs diff {(wide.float() - narrow.float()).abs().max().item():.3g}")
    assert torch.equal(wide, narrow) and intact(guard)
    if upsample == 2:                                   # ... and with `out` beyond 2 GiB: the phase slices' row map inside the out window
        o_big, og = big_view(arena, 1, NIMG * ho * wo, C1, dt)
        run(ops, True, lambda: ops.gemm(a, w, mode=1, conv=conv, bias=bias, out=o_big))
        assert torch.equal(o_big, narrow) and intact(og)
        run(ops, True, lambda: ops.gemm(a_big, w, mode=1, conv=conv, bias=bias, out=o_big.zero_()))
        assert torch.equal(o_big, narrow) and intact(og)


# ---- mode 2: 3 groups x 5 frames x 40 rows, 64 channels: tiles cross frame and group borders; first and last frames away from the ends
@pytest.mark.parametrize("kind", KINDS)
def test_tconv_a0_and_residual_beyond_2_gib(ops, arena, kind):
    dt = DT[kind]
    groups, frames, hw, c = 3, 5, 40, 64
    m = groups * frames * hw
    a, w, bias, s = rnd((m, c), dt, 40), rnd((c, 3 * c), dt, 41, 0.1), rnd((c,), torch.float32, 42), rnd((m, c), dt, 43)
    a_big, guard = big_view(arena, 0, m, c, dt, a)
    s_big, sguard = big_view(arena, 1, m, c, dt, s)
    kw = dict(mode=2, tconv=(frames, hw), bias=bias, alpha=0.25)
    narrow = run(ops, False, lambda: ops.gemm(a, w, residual=s, blend=s, **kw))
    wide = run(ops, True, lambda: ops.gemm(a_big, w, residual=s, blend=s, **kw))
    both = run(ops, True, lambda: ops.gemm(a_big, w, residual=s_big, blend=s_big, **kw))
    print(f"[wide] mode 2 {kind}: max abs diff {(wide.float() - narrow.float()).abs().max().item():.3g}")
    assert torch.equal(wide, narrow) and torch.equal(both, narrow) and intact(guard) and intact(sguard)


# ---- tt_gemm_set_wide(2): compact problems on the wide kernels
@pytest.mark.parametrize("kind", KINDS)
def test_set_wide_2_is_bit_equal_on_compact_problems(ops, kind):
    dt = DT[kind]
    cases = []
    a, w, b, r = rnd((5000, 256), dt, 50), rnd((256, 256), dt, 51, 0.1), rnd((256,), torch.float32, 52), rnd((5000, 256), dt, 53)
    cases.append(("mode 0, one block per CU", lambda: ops.gemm(a, w, bias=b, residual=r)))
    a2, w2 = rnd((25600, 128), dt, 54), rnd((256, 128), dt, 55, 0.1)
    cases.append(("mode 0, 400 tiles", lambda: ops.gemm(a2, w2, bias=b)))
    a3, w3, b3 = rnd((8 * 32 * 32, 64), dt, 56), rnd((128, 9 * 64), dt, 57, 0.05), rnd((128,), torch.float32, 58)
    cases.append(("mode 1", lambda: ops.gemm(a3, w3, mode=1, conv=(8, 32, 32, 32, 32, 1, 0), bias=b3)))
    w3u = rnd((128, 16 * 64), dt, 59, 0.05)
    cases.append(("mode 1, upsample 2", lambda: ops.gemm(a3, w3u, mode=1, conv=(8, 32, 32, 64, 64, 1, 2), bias=b3)))
    a4, w4, b4, s4 = rnd((2 * 4 * 256, 64), dt, 60), rnd((64, 3 * 64), dt, 61, 0.1), rnd((64,), torch.float32, 62), rnd((2 * 4 * 256, 64), dt, 63)
    cases.append(("mode 2", lambda: ops.gemm(a4, w4, mode=2, tconv=(4, 256), bias=b4, residual=s4, blend=s4, alpha=0.4)))
    for what, fn in cases:
        ops.set_gemm_wide(1)
        narrow = run(ops, False, fn)
        ops.set_gemm_wide(2)
        wide = run(ops, True, fn)
        assert torch.equal(wide, narrow), f"{what} ({kind})"


@pytest.mark.parametrize("kind", KINDS)
@torch.no_grad()
def test_tiny_decoder_is_bit_equal_under_set_wide_2(ops, kind):
    from tests.test_vae_decoder_gpu import _pair
    dt = DT[kind]
    p, _ = _pair(dt)
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(6, 4, 8, 4, generator=g) * 3.0).to(dt).float().cuda()
    ops.set_gemm_wide(1)
    n0 = ops.WIDE_LAUNCHES
    narrow = p.decode(z, num_frames=3).sample
    assert ops.WIDE_LAUNCHES == n0
    ops.set_gemm_wide(2)
    wide = p.decode(z, num_frames=3).sample
    assert ops.WIDE_LAUNCHES > n0
    print(f"[wide] tiny decoder {kind}: {ops.WIDE_LAUNCHES - n0} wide launches")
    assert torch.equal(wide, narrow)


# ---- GroupNorm over a dense tensor beyond 2 GiB: 42 images of 448 x 448 x 128 channels in 16-bit storage (2.16 GB)
@torch.no_grad()
def test_groupnorm_over_a_dense_tensor_beyond_2_gib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops
    from tests.test_norm_bounds_gpu import EPS, PARTIAL_ADDS, affine
    dtype, nimg, hw, c, rho, per = torch.bfloat16, 42, 448 * 448, 128, 5.0, 6
    gamma, beta = affine(c, 8)
    x = torch.empty((nimg * hw, c), dtype=dtype, device="cuda")
    assert x.numel() * x.element_size() >= G2
    for i in range(0, nimg, per):
        x[i * hw:(i + per) * hw] = eb.norm_input(per, hw, c, rho, dtype, 12 + i, device="cuda")
    y = ops.groupnorm(x, None, nimg, hw, 1, gamma, beta, EPS, True)
    torch.cuda.synchronize()
    worst = 0.0
    for i in range(0, nimg, per):
        sl = slice(i * hw, (i + per) * hw)
        b = eb.groupnorm(x[sl], gamma, beta, EPS, seg_rows=hw, silu=True, n_adds=PARTIAL_ADDS, guard=eb.GN_GUARD_RATIO)
        worst = max(worst, eb.ratio(y[sl], b, dtype))
    print(f"[wide] GroupNorm over {x.numel() * 2 / 1e9:.2f} GB: max err/bound = {worst:.3g}")
    assert worst <= 1.0
