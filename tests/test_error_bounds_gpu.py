"""GPU: every tt_gemm route (and tt_conv3x3) against an fp64 reference under the per-element error bound of tests/error_bounds.py,
on operands whose magnitudes span decades: output column j scaled by 2^e_j (e_j over -9 .. 3), A row i by 2^f_i (f_i over -3 .. 3),
the epilogue terms with their column's scale -- so a wrong term on a small output fails like one on a large output.  Every case
asserts the route it claims to test (kernel name from ops.PROFILE, tile plan from tt_gemm_plan) and restores every knob it turns.

The GELU sweep runs exact gate pre-activations through every GEGLU route (A columns 0..7 hold the sweep values, column 8 is 1; gate
row j holds 2^e_j in column j % 8, value row j holds +-1 or a power of two in column 8): every storage value in [-16, 16] with
|g| >= 2^-10, a geometric set out to +-300 and the neighbours of +-3.75, +-6.5, +-12 (the clamp and fit edges of the fast GELU
forms), each also at the gate scales 2^e."""
import ctypes as C
import time

import pytest
import torch
import torch.nn.functional as F

from tests import error_bounds as eb

pytestmark = pytest.mark.gpu

DTYPES16 = [torch.bfloat16, torch.float16]
TT_EUNSUPPORTED = -2                # include/ttvdm.h
# the tile table of gemm.hip (kCfgs): BM, BN, BK, ring stages, waves along M, waves along N -- keep in step
TILES = [(128, 128, 64, 2, 2, 2), (128, 64, 64, 3, 2, 2), (64, 64, 64, 4, 2, 2), (256, 128, 32, 3, 4, 2), (256, 256, 32, 3, 2, 4),
         (128, 128, 32, 3, 2, 2), (256, 128, 64, 3, 4, 2), (128, 160, 64, 2, 4, 1), (128, 320, 32, 3, 4, 2), (256, 256, 64, 2, 2, 4),
         (128, 128, 64, 4, 2, 2), (128, 128, 64, 2, 4, 2), (256, 160, 32, 3, 8, 1), (256, 128, 32, 4, 4, 2), (128, 128, 32, 5, 4, 2),
         (128, 128, 64, 3, 4, 2), (128, 128, 64, 4, 4, 2), (256, 256, 32, 4, 2, 4), (256, 128, 64, 2, 4, 2), (256, 128, 32, 5, 4, 2),
         (128, 128, 128, 2, 4, 2)]
PP_FORM = {torch.bfloat16: "poly", torch.float16: "sigmoid"}          # the GELU the persistent kernel evaluates per storage type
RATIOS = {}                         # route -> largest err/bound seen (printed when the module ends)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    t0 = time.time()
    yield o
    print(f"\n[error bound] module time {time.time() - t0:.1f} s; worst err/bound per route:")
    for k, v in sorted(RATIOS.items()):
        print(f"[error bound]   {k}: {v:.3g}")


def record(route, ratio):
    RATIOS[route] = max(RATIOS.get(route, 0.0), ratio)


def launch(ops, fn):
    """fn() (one ops.gemm / ops.conv3x3 call) and (its kernel instance name, the tt_gemm_plan cfg of that launch or None)"""
    lib = ops._lib.load()
    orig, plans = lib.tt_gemm_plan, []

    def plan(g, cfg):
        rc = orig(g, cfg)
        plans.append(list(cfg))
        return rc
    ops.PROFILE = []
    lib.tt_gemm_plan = plan
    try:
        out = fn()
        torch.cuda.synchronize()
        name = ops.PROFILE[-1][0]
    finally:
        lib.tt_gemm_plan = orig
        ops.PROFILE = None
    return out, name, (plans[-1] if plans else None)


class Knob:
    """a process-wide tuning knob of libttvdm set for a block and restored afterwards"""

    def __init__(self, fn, value, restore):
        self.fn, self.value, self.restore = fn, value, restore

    def __enter__(self):
        assert self.fn(self.value) == 0

    def __exit__(self, *exc):
        self.fn(self.restore)


class F32Mode:
    """TT_F32 products: split16 or the exact-fp32 MFMA for a block"""

    def __init__(self, ops, split16):
        self.ops, self.split16 = ops, split16

    def __enter__(self):
        self.was = self.ops.f32_split()
        self.ops.set_f32_split(self.split16)

    def __exit__(self, *exc):
        self.ops.set_f32_split(self.was)


# ---- the cases (each returns its err/bound; `expect(name, cfg)` asserts the route)

def case_linear(ops, dtype, expect, *, m=300, n=200, k0=64, k1=32, periodic=False, split16=False, dev="cpu", rows_per=50):
    a, w, cs = eb.decade_operands(m, n, k0 + k1, dtype, 11)
    bias = eb.scaled((n,), cs, torch.float32, 12)
    rp, mod = (1, 3) if periodic else (rows_per, 0)
    nrv = 3 if periodic else (m + rp - 1) // rp
    rv = eb.scaled((nrv, n), cs, torch.float32, 13)
    res, bl = eb.scaled((m, n), cs, dtype, 14), eb.scaled((m, n), cs, dtype, 15)
    a1 = a[:, k0:].contiguous().cuda() if k1 else None
    out, name, cfg = launch(ops, lambda: ops.gemm(a[:, :k0].contiguous().cuda(), w.cuda(), a1=a1, bias=bias.cuda(), acc_scale=0.75,
                                                  rowvec=rv.cuda(), rowvec_rows=rp, rowvec_mod=mod, residual=res.cuda(),
                                                  blend=bl.cuda(), alpha=0.3))
    expect(name, cfg)
    idx = torch.arange(m) // rp
    idx = idx % mod if mod else idx
    d = lambda t: t.to(dev)
    ref = eb.epilogue(eb.matmul(d(a), d(w), split16=split16), bias=d(bias), acc_scale=0.75, rowvec=d(rv.double()[idx]), residual=d(res),
                      blend=d(bl), alpha=0.3)
    return eb.check(out, ref, dtype, f"linear m={m} n={n} k={k0}+{k1}{' periodic' if periodic else ''} {name} {cfg}")


def case_geglu(ops, dtype, expect, form, *, m=260, h=96, k=64, split16=False):
    from this_and_that_vdm_amd.packing import pack_geglu
    a, w, cs = eb.decade_operands(m, 2 * h, k, dtype, 21)
    bias = eb.scaled((2 * h,), cs, torch.float32, 22)
    wp, bp = pack_geglu(w, bias)
    out, name, cfg = launch(ops, lambda: ops.gemm(a.cuda(), wp.cuda(), bias=bp.cuda(), geglu=True))
    expect(name, cfg)
    ref = eb.epilogue(eb.matmul(a, w, split16=split16), bias=bias, geglu=form)
    return eb.check(out, ref, dtype, f"geglu m={m} h={h} {name}")


def conv_operands(dtype, nimg, c, cout, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    pix = torch.exp2((torch.arange(h * w, dtype=torch.float64) % 7 - 3).reshape(h, w))         # pixel (row of A) scales 2^f
    x = (torch.randn(nimg, c, h, w, generator=g, dtype=torch.float64) * pix).to(dtype)
    cs = torch.exp2(eb.col_exponents(cout))
    wt = (torch.randn(cout, c, 3, 3, generator=g, dtype=torch.float64) * (9 * c) ** -0.5 * cs[:, None, None, None]).to(dtype)
    return x, wt, cs


def case_conv(ops, dtype, expect, *, mode=1, stride=1, upsample=0, split16=False):
    from this_and_that_vdm_amd.packing import pack_conv3x3
    nimg, c0, c1, cout, h, w = 2, 32, 16, 72, 9, 13
    x, wt, cs = conv_operands(dtype, nimg, c0 + c1, cout, h, w, 31)
    if mode == 3:
        op = lambda xx, ww: F.conv2d(F.pad(xx, (0, 1, 0, 1)), ww, stride=stride)
    else:
        op = lambda xx, ww: F.conv2d(F.interpolate(xx, scale_factor=2.0, mode="nearest") if upsample else xx, ww, stride=stride, padding=1)
    acc = eb.contract(op, x, wt, split16=split16)
    ho, wo = acc.ref.shape[-2:]
    acc = acc.tokens()
    bias = eb.scaled((cout,), cs, torch.float32, 32)
    res = eb.scaled((nimg * ho * wo, cout), cs, dtype, 33)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().cuda()
    out, name, cfg = launch(ops, lambda: ops.gemm(tok(x[:, :c0]), pack_conv3x3(wt).cuda(), a1=tok(x[:, c0:]), mode=mode,
                                                  conv=(nimg, h, w, ho, wo, stride, upsample), bias=bias.cuda(), residual=res.cuda()))
    expect(name, cfg)
    ref = eb.epilogue(acc, bias=bias, residual=res)
    return eb.check(out, ref, dtype, f"conv mode {mode} stride {stride} upsample {upsample} {name}")


def mode3_refused(ops, dtype):
    """True if the plan of case_conv's mode-3 problem under the current tile override is TT_EUNSUPPORTED"""
    from this_and_that_vdm_amd import _lib
    g = _lib.TtGemmArgs()
    g.m, g.n, g.k0, g.k1, g.mode = 2 * 4 * 6, 72, 32, 16, 3
    g.nimg, g.hin, g.win, g.hout, g.wout, g.stride = 2, 9, 13, 4, 6, 2
    g.dtype = ops._code(dtype)
    cfg = (C.c_int32 * 7)()
    return _lib.load().tt_gemm_plan(C.byref(g), cfg) == TT_EUNSUPPORTED


def case_tconv(ops, dtype, expect, *, split16=False):
    from this_and_that_vdm_amd.packing import pack_tconv3
    b, f, hw, c, cout = 2, 5, 12, 64, 72
    g = torch.Generator().manual_seed(41)
    rows = torch.exp2(torch.arange(f * hw, dtype=torch.float64) % 7 - 3).reshape(1, 1, f, hw, 1)
    x = (torch.randn(b, c, f, hw, 1, generator=g, dtype=torch.float64) * rows).to(dtype)
    cs = torch.exp2(eb.col_exponents(cout))
    wt = (torch.randn(cout, c, 3, 1, 1, generator=g, dtype=torch.float64) * (3 * c) ** -0.5 * cs[:, None, None, None, None]).to(dtype)
    bias = eb.scaled((cout,), cs, torch.float32, 42)
    acc = eb.contract(lambda xx, ww: F.conv3d(xx, ww, padding=(1, 0, 0)), x, wt, split16=split16).tokens()
    tok = x[..., 0].permute(0, 2, 3, 1).reshape(b * f * hw, c).contiguous().cuda()
    out, name, cfg = launch(ops, lambda: ops.gemm(tok, pack_tconv3(wt).cuda(), mode=2, tconv=(f, hw), bias=bias.cuda()))
    expect(name, cfg)
    return eb.check(out, eb.epilogue(acc, bias=bias), dtype, f"tconv {name}")


# ---- tiled template: every entry of the tile table, forced

@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("cfg", list(range(len(TILES))))
def test_tiled_every_tile_configuration(ops, dtype, cfg):
    lib = ops._lib.load()

    def expect(name, plan):
        assert name.startswith("gemm_kernel<") and tuple(plan[:6]) == TILES[cfg] and plan[6] == 1, (name, plan)
    with Knob(lib.tt_gemm_set_tile_override, cfg, -1):
        r = [case_linear(ops, dtype, expect), case_linear(ops, dtype, expect, periodic=True, m=333, n=196),
             case_geglu(ops, dtype, expect, "erf"),
             case_conv(ops, dtype, expect), case_conv(ops, dtype, expect, stride=2), case_conv(ops, dtype, expect, upsample=1),
             case_tconv(ops, dtype, expect)]
        if mode3_refused(ops, dtype):
            with pytest.raises(RuntimeError, match="tt_gemm"):
                case_conv(ops, dtype, expect, mode=3, stride=2)
        else:
            r.append(case_conv(ops, dtype, expect, mode=3, stride=2))
    record(f"tiled, forced tile table ({dtype})", max(r))


def test_tiled_mode3_is_built_for_some_configurations(ops):
    lib = ops._lib.load()
    served = []
    for cfg in range(len(TILES)):
        with Knob(lib.tt_gemm_set_tile_override, cfg, -1):
            if not mode3_refused(ops, torch.bfloat16):
                served.append(cfg)
    assert served and len(served) < len(TILES), served


# ---- tiled template on fp32 storage: exact fp32 MFMA and split16 (the default plan)

@pytest.mark.parametrize("split16", [False, True])
def test_tiled_f32(ops, split16):
    dt = torch.float32

    def expect(name, plan):
        assert name.startswith("gemm_kernel<f32_tag,"), name
    with F32Mode(ops, split16):
        r = [case_linear(ops, dt, expect, split16=split16), case_linear(ops, dt, expect, periodic=True, split16=split16),
             case_geglu(ops, dt, expect, "erf", split16=split16),
             case_conv(ops, dt, expect, split16=split16), case_conv(ops, dt, expect, stride=2, split16=split16),
             case_conv(ops, dt, expect, upsample=1, split16=split16), case_conv(ops, dt, expect, mode=3, stride=2, split16=split16),
             case_tconv(ops, dt, expect, split16=split16)]
    record(f"tiled, TT_F32 {'split16' if split16 else 'exact'}", max(r))


# ---- tiled split-K (the planner's own choice, with workspace): a coarse-level conv

@pytest.mark.parametrize("dtype", DTYPES16)
def test_tiled_split_k(ops, dtype):
    from this_and_that_vdm_amd.packing import pack_conv3x3
    nimg, cin, cout, h, w = 4, 640, 256, 7, 9                   # M = 252, K = 5760: few tiles, long K
    x, wt, cs = conv_operands(dtype, nimg, cin, cout, h, w, 51)
    bias = eb.scaled((cout,), cs, torch.float32, 52)
    rv = eb.scaled((2, cout), cs, torch.float32, 53)
    res = eb.scaled((nimg * h * w, cout), cs, dtype, 54)
    tok = x.permute(0, 2, 3, 1).reshape(-1, cin).contiguous().cuda()
    out, name, cfg = launch(ops, lambda: ops.gemm(tok, pack_conv3x3(wt).cuda(), mode=1, conv=(nimg, h, w, h, w, 1, 0), bias=bias.cuda(),
                                                  rowvec=rv.cuda(), rowvec_rows=2 * h * w, residual=res.cuda()))
    assert name.startswith("gemm_kernel<") and cfg[3] > 0 and cfg[6] >= 2, (name, cfg)
    acc = eb.contract(lambda xx, ww: F.conv2d(xx, ww, padding=1), x, wt).tokens()
    ref = eb.epilogue(acc, bias=bias, rowvec=rv.double()[torch.arange(nimg * h * w) // (2 * h * w)], residual=res)
    record(f"tiled split-K ({dtype})", eb.check(out, ref, dtype, f"split-K conv {name} {cfg}"))


# ---- the persistent ping-pong kernel (gemm_pp.hip): plain, LayerNorm fold, GEGLU, both, and the two-part launch

@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("ln,geglu,m,n,k", [(0, 0, 8192 - 200, 6144, 320), (1, 0, 8192, 6144 - 48, 192), (0, 1, 8192, 6144, 128),
                                            (1, 1, 8192 - 37, 6144 - 16, 128),
                                            (0, 0, 3072 + 130, 10240, 256)])       # 12 whole tile rows persistent + 130 rows tiled
def test_persistent_pingpong(ops, dtype, ln, geglu, m, n, k):
    from this_and_that_vdm_amd.packing import fold_layernorm, pack_geglu, zero_sum_round
    a, w, cs = eb.decade_operands(m, n, k, dtype, 61)
    bias = eb.scaled((n,), cs, torch.float32, 62)
    kw = {}
    if ln:
        g = torch.Generator().manual_seed(63)
        a = (torch.randn(m, k, generator=g) * 1.5 + torch.randn(m, 1, generator=g) * 1.5).to(dtype)
        gam, bet = torch.randn(k, generator=g) * 0.2 + 1, torch.randn(k, generator=g) * 0.3
        wf, bias = fold_layernorm(w.float(), bias, gam, bet)
        w = zero_sum_round(wf, dtype)
        rstd, rel = eb.ln_rstd(a.cuda(), 1e-5)
        kw = dict(rstd=rstd, rstd_rel=rel)
    wk, bk = pack_geglu(w, bias) if geglu else (w, bias)
    out, name, cfg = launch(ops, lambda: ops.gemm(a.cuda(), wk.cuda(), bias=bk.cuda(), geglu=bool(geglu), ln_fold=ln, ln_eps=1e-5))
    assert name.startswith(f"gemm_pp_kernel<{ops._TAG[ops._code(dtype)]}, {ln}, {geglu}>") and cfg[3] == 0, (name, cfg)
    form = (PP_FORM[dtype], "erf") if m % 256 else PP_FORM[dtype]       # (ragged rows may run on the tiled template)
    ref = eb.epilogue(eb.matmul(a.cuda(), w.cuda()), bias=bias.cuda(), geglu=form if geglu else None, **kw)
    record(f"persistent ping-pong ({dtype})", eb.check(out, ref, dtype, f"pp ln={ln} geglu={geglu} m={m} n={n} k={k}"))


# ---- the N = 320 big-tile kernels (gemm_w320.hip): 256 x 320, 128 x 320, and the 128 x 320 split-K route (long K)

@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("big,m,n,k", [(2, 46100, 320, 192), (3, 12500, 640, 192), (3, 3136, 1280, 5120)])
def test_w320(ops, dtype, big, m, n, k):
    lib = ops._lib.load()

    def expect(name, cfg):
        assert name.startswith("gemm_w320_kernel<" if big == 2 else "gemm_w320h_kernel<") and cfg[1] == 320, (name, cfg)
        assert (cfg[6] >= 2) == (k >= 4096), cfg                 # long K: the split-K variant
    with Knob(lib.tt_gemm_set_big_tile, big, 1):
        r = case_linear(ops, dtype, expect, m=m, n=n, k0=k, k1=0, dev="cuda", rows_per=1000)
    record(f"w320 big tile {big} ({dtype})", r)


# ---- the sq320 streaming kernel

@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("m", [4101, 3 * 8192 - 31])
@pytest.mark.parametrize("epi", ["bias_res", "blend", "rowvec_parity", "rowvec_two_groups"])
def test_sq320_streaming(ops, dtype, m, epi):
    lib = ops._lib.load()
    n = k = 320
    a, w, cs = eb.decade_operands(m, n, k, dtype, 71)
    bias = eb.scaled((n,), cs, torch.float32, 72)
    res = eb.scaled((m, n), cs, dtype, 73)
    rv = eb.scaled((2, n), cs, torch.float32, 74)
    r_d = res.cuda()
    kw, ekw = dict(bias=bias.cuda(), residual=r_d), dict(bias=bias.cuda(), residual=r_d)
    if epi == "bias_res":
        kw.update(acc_scale=0.5)
        ekw.update(acc_scale=0.5)
    elif epi == "blend":                                     # the self-blend the streaming kernel serves
        kw.update(blend=r_d, alpha=0.3)
        ekw.update(blend=r_d, alpha=0.3)
    else:                                                    # two distinct row vectors: even / odd rows, or two row groups
        half = (m // 2 + 31) // 32 * 32
        if epi == "rowvec_parity":
            kw.update(rowvec=rv.cuda(), rowvec_rows=1, rowvec_mod=2, acc_scale=0.5)
            sel = torch.arange(m) & 1
        else:
            kw.update(rowvec=rv.cuda(), rowvec_rows=half, acc_scale=0.5, blend=r_d, alpha=0.3)
            ekw.update(blend=r_d, alpha=0.3)
            sel = (torch.arange(m) >= half).long()
        ekw.update(rowvec=rv.double()[sel].cuda(), acc_scale=0.5)
    with Knob(lib.tt_gemm_set_streaming_square, 1, 2):
        out, name, cfg = launch(ops, lambda: ops.gemm(a.cuda(), w.cuda(), **kw))
    assert name.startswith("sq320_kernel<") and cfg[0] == 32 and cfg[1] == 320, (name, cfg)
    ref = eb.epilogue(eb.matmul(a.cuda(), w.cuda()), **ekw)
    record(f"sq320 streaming ({dtype})", eb.check(out, ref, dtype, f"sq320 m={m} {epi}"))


# ---- tt_conv3x3 (GroupNorm-activated LDS patch): two sources, explicit GroupNorm scale / shift, with and without SiLU

@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("silu", [True, False])
def test_conv3x3_patch_kernel(ops, dtype, silu):
    from this_and_that_vdm_amd.packing import pack_conv3x3
    nimg, frames, h, w, c0, c1, cout = 4, 2, 16, 28, 128, 64, 128
    assert ops.conv3x3_supported(h, w, c0, c1, cout, dtype)
    g = torch.Generator().manual_seed(81)
    x = (torch.randn(nimg, c0 + c1, h, w, generator=g) * 2.0 + 0.5).to(dtype)
    cs = torch.exp2(eb.col_exponents(cout))
    wt = (torch.randn(cout, c0 + c1, 3, 3, generator=g, dtype=torch.float64) * (9 * (c0 + c1)) ** -0.5 * cs[:, None, None, None]).to(dtype)
    scale = torch.randn(nimg, c0 + c1, generator=g) * 0.5 + 1.0
    shift = torch.randn(nimg, c0 + c1, generator=g) * 0.5
    bias = eb.scaled((cout,), cs, torch.float32, 82)
    film = eb.scaled((nimg // frames, cout), cs, torch.float32, 83)
    res = eb.scaled((nimg * h * w, cout), cs, dtype, 84)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().cuda()
    out, name, _ = launch(ops, lambda: ops.conv3x3(tok(x[:, :c0]), tok(x[:, c0:]), pack_conv3x3(wt).cuda(), nimg, h, w,
                                                   gn=(scale.cuda(), shift.cuda()), silu=silu, bias=bias.cuda(), rowvec=film.cuda(),
                                                   rowvec_rows=frames * h * w, residual=res.cuda()))
    assert name.startswith("conv_patch_kernel<"), name
    act, aerr = eb.conv3x3_formed_err(x, scale, shift, silu, dtype)
    acc = eb.contract(lambda xx, ww: F.conv2d(xx, ww, padding=1), act, wt, formed_err=aerr).tokens()
    ref = eb.epilogue(acc, bias=bias, rowvec=film.double()[torch.arange(nimg * h * w) // (frames * h * w)], residual=res)
    record(f"tt_conv3x3 ({dtype})", eb.check(out, ref, dtype, f"conv3x3 silu={silu}"))


# ---- the GELU sweep through every GEGLU route

GATE_E = [0, 0, 0, -1, -3, -6, -9, 1, 2, 3]                 # gate scales 2^e (mostly 1: every sweep value exactly)


def sweep_values(dtype) -> torch.Tensor:
    """every storage value in [-16, 16] with |g| >= 2^-10 (and 0), a geometric set out to +-300, the neighbours of +-3.75, +-6.5,
    +-12 (three storage steps each way); fp32: the bf16 and fp16 sets plus random fp32 values in [0, 16)"""
    def every(dt):
        bits = torch.arange(0, 0x7C00 if dt == torch.float16 else 0x7F80, dtype=torch.int32).to(torch.int16)
        v = bits.view(dt).double()
        return v[(v >= 2.0 ** -10) & (v <= 16.0)]
    if dtype == torch.float32:
        g = torch.Generator().manual_seed(91)
        pos = torch.cat([every(torch.bfloat16), every(torch.float16), torch.rand(12000, generator=g, dtype=torch.float64) * 16])
        pos = pos.float().double()
    else:
        pos = every(dtype)
    geo = torch.logspace(torch.log10(torch.tensor(16.0)), torch.log10(torch.tensor(300.0)), 64, dtype=torch.float64)
    edges = []
    for c in (3.75, 6.5, 12.0):
        if dtype == torch.float32:
            b = int(torch.tensor(c, dtype=torch.float32).view(torch.int32))
            edges += [float(torch.tensor(b + d, dtype=torch.int32).view(torch.float32)) for d in range(-3, 4)]
        else:
            b = int(torch.tensor(c, dtype=dtype).view(torch.int16))
            edges += [float(torch.tensor(b + d, dtype=torch.int16).view(dtype)) for d in range(-3, 4)]
    pos = torch.cat([pos, geo.to(dtype).double(), torch.tensor(edges, dtype=torch.float64)])
    return torch.unique(torch.cat([pos, -pos, torch.zeros(1, dtype=torch.float64)]))


def sweep_operands(vals, m, h, k, dtype):
    """A [m, k] (columns 0..7: the sweep values, cycling; column 8: 1) and the UNPACKED W [2h, k]"""
    cells = vals[torch.arange(8 * m) % len(vals)].reshape(m, 8)
    a = torch.zeros(m, k, dtype=torch.float64)
    a[:, :8], a[:, 8] = cells, 1.0
    w = torch.zeros(2 * h, k, dtype=torch.float64)
    j = torch.arange(h)
    sv = torch.ones(h, dtype=torch.float64)
    sv[j % 11 == 3], sv[j % 11 == 5], sv[j % 11 == 7] = -1.0, 2.0 ** -4, 4.0
    w[j, 8] = sv
    w[h + j, j % 8] = torch.exp2(torch.tensor(GATE_E, dtype=torch.float64)[(j // 8) % len(GATE_E)])
    return a.to(dtype), w.to(dtype)


def run_sweep(ops, dtype, m, h, form, expect, split16=False):
    from this_and_that_vdm_amd.packing import pack_geglu
    vals = sweep_values(dtype)
    a, w = sweep_operands(vals, m, h, 128, dtype)
    wp, _ = pack_geglu(w, torch.zeros(2 * h))
    out, name, cfg = launch(ops, lambda: ops.gemm(a.cuda(), wp.cuda(), geglu=True))
    expect(name, cfg)
    ref = eb.epilogue(eb.matmul(a.cuda(), w.cuda(), split16=split16), geglu=form)
    covered = min(len(vals), 8 * m)
    return eb.check(out, ref, dtype, f"GELU sweep ({covered} of {len(vals)} values, m={m}, {form}) {name}")


@pytest.mark.parametrize("dtype,split16", [(torch.bfloat16, False), (torch.float16, False), (torch.float32, False), (torch.float32, True)])
def test_gelu_sweep_tiled(ops, dtype, split16):
    def expect(name, cfg):
        assert name.startswith("gemm_kernel<") and cfg[3] > 0, (name, cfg)
    m = {torch.bfloat16: 4096, torch.float16: 8192, torch.float32: 12288}[dtype]     # 8 sweep values per row: all of them
    with F32Mode(ops, split16):
        r = run_sweep(ops, dtype, m, 256, "erf", expect, split16=split16)
    record(f"GELU sweep, tiled ({dtype}{' split16' if split16 else ''})", r)


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("m,h", [(8192, 3072), (3072 + 130, 5120)])      # the second: 12 whole tile rows persistent + 130 rows tiled
def test_gelu_sweep_persistent(ops, dtype, m, h):
    def expect(name, cfg):
        assert name.startswith(f"gemm_pp_kernel<{ops._TAG[ops._code(dtype)]}, 0, 1>") and cfg[3] == 0, (name, cfg)
    form = PP_FORM[dtype] if m % 256 == 0 else (PP_FORM[dtype], "erf")
    record(f"GELU sweep, persistent ({dtype})", run_sweep(ops, dtype, m, h, form, expect))
