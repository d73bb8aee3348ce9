"""GPU: tt_gemm's ``upsample = 2`` -- the nearest-x2 upsampling 3x3 conv as four 2 x 2 phase convs inside one launch of the tiled
template (phase-packed weights, packing.pack_upsample_phases) -- at the smallest shapes that exercise every index path:

  (nimg 3, h 5, w 7, Cin 64, Cout 128)    105 low-res rows: one ragged tile that spans the images, odd sizes
  (5, 6, 9, 96, 160)                      270 rows: tiles straddling images, a K tail of 32 per tap (16-bit), ragged N
  (2, 1, 1, 64, 128)                      every tap but one is zero padding

for bf16, fp16, f32 (exact-fp32 MFMA) and split16.  For every shape and storage type, on EVERY output element:
  * the per-element bound of tests/error_bounds.py against the fp64 phase conv on the STORED phase weights;
  * the upsample = 1 route on the same input, within the sum of the two routes' bounds plus what the one extra rounding of the
    pre-summed weights can move:  2^-9 sum |x| |W_eff|  (bf16; 2^-12 for fp16; nothing for the fp32 storage modes, whose packs keep
    the fp32 sum -- their difference is inside the accumulation budget);
  * a captured graph replays the eager result bit for bit;
  * every output row is written exactly once: `out` starts as NaN and none survives.
One Upsample2D forward with the route on and off, within the same bound."""
import functools

import pytest
import torch

from tests import error_bounds as eb
from tests.upsample_phases_ref import phase_conv, summed_taps, upsample_conv

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7, 64, 128), (5, 6, 9, 96, 160), (2, 1, 1, 64, 128)]
MODES = ["bf16", "fp16", "f32", "split16"]
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32, "split16": torch.float32}
PACK_ROUNDING = {"bf16": 2.0 ** -9, "fp16": 2.0 ** -12, "f32": 0.0, "split16": 0.0}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    return o


class F32Mode:
    def __init__(self, ops, split16):
        self.ops, self.split16 = ops, split16

    def __enter__(self):
        self.was = self.ops.f32_split()
        self.ops.set_f32_split(self.split16)

    def __exit__(self, *exc):
        self.ops.set_f32_split(self.was)


def limit(b: eb.Bound, dtype) -> torch.Tensor:
    """eb.check's per-element limit"""
    us = eb.UNIT[dtype]
    return us * b.ref.abs() + (1 + us) * b.err + eb.ABS_FLOOR.get(dtype, 0.0)


@functools.lru_cache(maxsize=None)
def case(shape, mode):
    """operands and both routes' fp64 references with their budgets: computed once per (shape, storage mode), shared, never modified"""
    from this_and_that_vdm_amd.packing import pack_conv3x3, pack_upsample_phases
    nimg, h, w, cin, cout = shape
    dtype, split16 = STORAGE[mode], mode == "split16"
    g = torch.Generator().manual_seed(41 + 7 * SHAPES.index(shape))
    pix = torch.exp2((torch.arange(h * w, dtype=torch.float64) % 7 - 3).reshape(h, w))          # pixel (row of A) scales 2^f
    x = (torch.randn(nimg, cin, h, w, generator=g, dtype=torch.float64) * pix).to(dtype)
    cs = torch.exp2(eb.col_exponents(cout))
    wt = (torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * (9 * cin) ** -0.5 * cs[:, None, None, None]).to(dtype)
    bias = eb.scaled((cout,), cs, torch.float32, 42)
    wp = pack_upsample_phases(wt, dtype)                      # the STORED phase weights
    b2 = eb.epilogue(eb.contract(phase_conv, x, wp, split16=split16).tokens(), bias=bias)
    b1 = eb.epilogue(eb.contract(upsample_conv, x, wt, split16=split16).tokens(), bias=bias)
    # sum |x| |W_eff|, W_eff the exact sum of the stored taps (before the pack's one rounding)
    w_eff = summed_taps(wt, torch.float64)
    s_eff = phase_conv(x.double().abs(), w_eff.abs()).movedim(1, -1).reshape(-1, cout)
    tok = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous()
    return dict(tok=tok, wp=wp, w9=pack_conv3x3(wt), bias=bias, b1=b1, b2=b2, s_eff=s_eff, dtype=dtype, split16=split16)


def run_route(ops, c, shape, upsample, out=None):
    nimg, h, w, _, _ = shape
    wgt = c["wp"] if upsample == 2 else c["w9"]
    return ops.gemm(c["tok"].cuda(), wgt.cuda(), mode=1, conv=(nimg, h, w, 2 * h, 2 * w, 1, upsample), bias=c["bias"].cuda(), out=out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_phase_route_bound_old_route_graph_and_coverage(ops, shape, mode):
    c = case(shape, mode)
    dtype = c["dtype"]
    nimg, h, w, cin, cout = shape
    with F32Mode(ops, c["split16"]):
        # the route: the tiled template, unsplit (kernel name from the profile hook)
        ops.PROFILE = []
        try:
            out = torch.full((nimg * 4 * h * w, cout), float("nan"), dtype=dtype, device="cuda")
            run_route(ops, c, shape, 2, out=out)
            torch.cuda.synchronize()
            name, flops = ops.PROFILE[-1][0], ops.PROFILE[-1][1]
        finally:
            ops.PROFILE = None
        assert name.startswith("gemm_kernel<"), name
        assert flops == 2.0 * out.shape[0] * cout * 4 * cin            # the executed products: four taps
        # every row written exactly once: a row written never leaves a NaN, and the values below are each row's own
        assert not torch.isnan(out).any(), f"{int(torch.isnan(out).any(1).sum())} output rows were not written"
        r2 = eb.check(out, c["b2"], dtype, f"upsample=2 {shape} {mode} {name}")
        # the old route on the same input
        old = run_route(ops, c, shape, 1)
        r1 = eb.check(old, c["b1"], dtype, f"upsample=1 {shape} {mode}")
        lim = limit(c["b1"], dtype) + limit(c["b2"], dtype) + PACK_ROUNDING[mode] * c["s_eff"]
        diff = (out.double().cpu() - old.double().cpu()).abs()
        worst = float(torch.where(diff == 0, torch.zeros_like(diff), diff / lim).max())
        print(f"[upsample phases] {shape} {mode}: err/bound {r2:.3g} (old route {r1:.3g}), |new - old| / allowed {worst:.3g}")
        assert worst <= 1.0, f"{shape} {mode}: the two routes differ by {worst:.3g} of what their bounds and the pack rounding allow"
        # graph replay == eager, bit for bit
        a, wgt, bias = c["tok"].cuda(), c["wp"].cuda(), c["bias"].cuda()
        gout = torch.full_like(out, float("nan"))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.gemm(a, wgt, mode=1, conv=(nimg, h, w, 2 * h, 2 * w, 1, 2), bias=bias, out=gout)            # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.gemm(a, wgt, mode=1, conv=(nimg, h, w, 2 * h, 2 * w, 1, 2), bias=bias, out=gout)
        gout.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout.view(torch.int16 if dtype != torch.float32 else torch.int32),
                           out.view(torch.int16 if dtype != torch.float32 else torch.int32))


def test_presplit_phase_pack_meets_the_same_bound(ops):
    """split16: the packed weight arrives pre-split (what prepare() does to every packed GEMM weight)"""
    from this_and_that_vdm_amd.packing import presplit_f32
    shape = SHAPES[1]
    c = case(shape, "split16")
    nimg, h, w, cin, cout = shape
    with F32Mode(ops, True):
        pre = ops.gemm(c["tok"].cuda(), presplit_f32(c["wp"]).cuda(), mode=1, conv=(nimg, h, w, 2 * h, 2 * w, 1, 2), bias=c["bias"].cuda())
        torch.cuda.synchronize()
    assert not torch.isnan(pre).any()
    eb.check(pre, c["b2"], torch.float32, f"upsample=2 {shape} split16, pre-split weight")


@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_upsample2d_forward_with_the_route_on_and_off(ops, mode, monkeypatch):
    """Upsample2D.pack / forward: the phase route and the TT_UPSAMPLE_PHASES=0 route on the same input, within the two routes' bounds
    plus the pack-rounding term"""
    from this_and_that_vdm_amd.svd import layers
    shape = SHAPES[0]
    nimg, h, w, cin, cout = shape
    c = case(shape, mode)
    dtype = c["dtype"]
    g = torch.Generator().manual_seed(41 + 7 * SHAPES.index(shape))
    # the module's own weights: the case's operands (same generator sequence as case())
    pix = torch.exp2((torch.arange(h * w, dtype=torch.float64) % 7 - 3).reshape(h, w))
    torch.randn(nimg, cin, h, w, generator=g, dtype=torch.float64)
    cs = torch.exp2(eb.col_exponents(cout))
    wt = (torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64) * (9 * cin) ** -0.5 * cs[:, None, None, None]).to(dtype)
    outs = {}
    with F32Mode(ops, False):
        for on in (True, False):
            monkeypatch.setattr(layers, "UPSAMPLE_PHASES", on)
            up = layers.Upsample2D(cin, use_conv=True, out_channels=cout)
            with torch.no_grad():
                up.conv.weight.copy_(wt.float())
                up.conv.bias.copy_(c["bias"])
            up = up.to("cuda")
            up.pack(None, dtype)
            assert up.w.shape[1] == (16 if on else 9) * cin
            y, geom = up(c["tok"].cuda(), layers.Geom(1, nimg, h, w))
            torch.cuda.synchronize()
            assert (geom.h, geom.w) == (2 * h, 2 * w)
            outs[on] = y
    eb.check(outs[True], c["b2"], dtype, f"Upsample2D phases on {mode}")
    eb.check(outs[False], c["b1"], dtype, f"Upsample2D phases off {mode}")
    lim = limit(c["b1"], dtype) + limit(c["b2"], dtype) + PACK_ROUNDING[mode] * c["s_eff"]
    diff = (outs[True].double().cpu() - outs[False].double().cpu()).abs()
    worst = float(torch.where(diff == 0, torch.zeros_like(diff), diff / lim).max())
    print(f"[upsample phases] Upsample2D on vs off, {mode}: |on - off| / allowed {worst:.3g}")
    assert worst <= 1.0
