"""GPU: every GroupNorm / LayerNorm route against an fp64 reference on the STORED input under the per-element bound of
tests/error_bounds.py (groupnorm, layernorm, tile_sums), on inputs whose group (row) mean lies rho spreads away from zero, rho over
eb.RHO_GRID = {0, 5, 50, 300}: eb.norm_input / eb.ln_input -- the spread cycles over 2^-3 .. 2^3 and differs between consecutive
segments and groups, the sign of the mean alternates by group, one group is constant, one has spread^2 near eps; gamma / beta cycle
over magnitudes like eb.col_exponents.  Every case asserts the route it claims to test, restores every knob it turns, and records
err/bound per route and storage type with the rho of the worst element (printed when the module ends).  What "asserts the route"
means: for the producers, the kernel name ops.PROFILE derives from tt_gemm_plan, and `_tt_stats` / `_tt_gn`; for the normalisation
launches, ops.NORM_TRACE -- the front end's record of the entry point it called and, for the two GroupNorm entry points that choose
between kernels, of tt_groupnorm_route's answer, which the launchers take from the same host code.  Nothing here observes a launch on
the device: the names say which entry point and which route decision a case went through, so that a change of a threshold or of
ops.groupnorm's dispatch cannot silently move a case to another kernel.

On the kernels as they were before this module existed, every uncentred GroupNorm route broke the bound in fp16 and fp32 storage from
rho = 50 on (the tile-sum route from rho = 5: up to 286 x at rho = 300), and the constant group's statistics were rounding noise; the
conditioning guard of norm.hip (GN_GUARD_RATIO) is the fix, and DESIGN.md 6.N has both tables.  eb.groupnorm's n_adds -- the fp32
additions behind one partial sum of a route, image_adds / grouped_adds / PARTIAL_ADDS / the tile height below -- is the one budget term
beyond "mean and rstd correct to one fp32 rounding", and it applies only to groups BELOW the guard, whose mean really comes from those
sums (eb.groupnorm's `guard`); at rho = 50 and 300 the budget is the issue's, term for term."""
import time

import pytest
import torch

from tests import error_bounds as eb

pytestmark = pytest.mark.gpu

DTYPES16 = [torch.bfloat16, torch.float16]
DTYPES = DTYPES16 + [torch.float32]
EPS = 1e-5
RATIOS = {}                         # (route, dtype) -> (largest err/bound, the rho it occurred at)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    t0 = time.time()
    yield o
    print(f"\n[norm bound] module time {time.time() - t0:.1f} s; worst err/bound per route and storage type (at rho):")
    for (route, dt), (r, rho) in sorted(RATIOS.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
        print(f"[norm bound]   {route} | {str(dt).replace('torch.', '')} | {r:.3g} | rho = {rho}")


def record(route, dtype, r, rho):
    if r >= RATIOS.get((route, dtype), (-1.0, 0))[0]:
        RATIOS[(route, dtype)] = (r, rho)


def traced(ops, fn):
    """fn() and what ops.NORM_TRACE recorded for it (entry point / route decision per normalisation call: see the module docstring)"""
    ops.NORM_TRACE = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, list(ops.NORM_TRACE)
    finally:
        ops.NORM_TRACE = None


def tag(ops, dtype):
    return ops._TAG[ops._code(dtype)]


def affine(c, seed):
    gamma, beta = eb.norm_affine(c, seed)
    return gamma.cuda(), beta.cuda()


# ---- the fp32 additions behind one partial sum of each statistics route (eb.groupnorm's n_adds); the launch geometry of norm.hip -- keep in step

def image_adds(c, hw):
    """gn_stats_image_kernel: 1024 / (c / 8) row lanes (fewer if [rpb][c] x 2 fp32 exceeds 96 KiB of LDS, at most hw); a lane's rows"""
    rpb = 1024 // (c // 8)
    while rpb > 1 and 2 * rpb * c * 4 > 96 * 1024:
        rpb -= 1
    rpb = min(rpb, hw)
    return -(-hw // rpb)


def grouped_adds(c, hw, dtype):
    """gn_group_kernel: gn_group_gpb groups per block, 512 / (their 8-channel vectors) row lanes (at most hw); a lane's rows"""
    cpg, es = c // 32, 4 if dtype == torch.float32 else 2
    gpb = 1
    while (gpb * cpg) & 7:
        gpb *= 2
    while gpb * 2 <= 4 and gpb * cpg * es < 128:
        gpb *= 2
    rlanes = min(512 // ((gpb * cpg) // 8), hw)
    return -(-hw // rlanes)


PARTIAL_ADDS = 8                    # gn_partial_kernel: "8 per thread row-lane" (gn_rows_per_chunk)


def sweep(route, dtype, run):
    """run(rho) -> (what, got, Bound, storage type of got) for every case at that rho; records err/bound per rho, then asserts all"""
    bad = []
    for rho in eb.RHO_GRID:
        for what, got, b, dt in run(rho):
            r = eb.ratio(got, b, dt)
            print(f"[norm bound] {route} {dtype} rho={rho} {what}: err/bound = {r:.3g}")
            record(route + (" (tile sums)" if what.startswith("sums") else ""), dtype, r, rho)
            if not r <= 1.0:
                bad.append((rho, what, r))
    assert not bad, f"{route} {dtype}: outside the bound at (rho, case, err/bound) {bad}"


# ---- tt_groupnorm_small: one block per image, and one block per (image, group slice)

def small_route(ops, dtype, shape, nimg, kernel, route):
    c0, c1, h, w = shape
    c, hw = c0 + c1, h * w
    gamma, beta = affine(c, 7)
    n_adds = image_adds(c, hw) if kernel == "gn_stats_image_kernel" else grouped_adds(c, hw, dtype)

    def run(rho):
        x = eb.norm_input(nimg, hw, c, rho, dtype, 11, device="cuda")
        x0, x1 = x[:, :c0].contiguous(), (x[:, c0:].contiguous() if c1 else None)
        for silu in (False, True):
            y, names = traced(ops, lambda: ops.groupnorm(x0, x1, nimg, hw, 1, gamma, beta, EPS, silu))
            assert names == [f"{kernel}<{tag(ops, dtype)}>"], names
            yield f"{shape} silu={silu}", y, eb.groupnorm(x, gamma, beta, EPS, seg_rows=hw, silu=silu, n_adds=n_adds, guard=eb.GN_GUARD_RATIO), dtype
    sweep(route, dtype, run)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(64, 32, 5, 3),           # cpg = 3: a group straddles the two sources
                                   (320, 0, 9, 11),          # cpg = 10
                                   (1280, 1280, 4, 7)])
def test_groupnorm_one_block_per_image(ops, dtype, shape):
    small_route(ops, dtype, shape, 5, "gn_stats_image_kernel", "one block per image")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(320, 0, 16, 16),         # 256 rows: the lower edge of the route
                                   (320, 0, 17, 19),         # 323 rows: the unrolled loops and their tails
                                   (640, 320, 16, 28)])
def test_groupnorm_grouped_one_launch(ops, dtype, shape):
    small_route(ops, dtype, shape, 9, "gn_group_kernel", "grouped one-launch")      # 9 images: the last round of the XCD mapping is ragged


# ---- tt_groupnorm_stats + tt_groupnorm_apply called directly: partial + finalize + apply

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,fpg", [((320, 0, 40, 56), 1), ((320, 0, 9, 11), 4)])
def test_groupnorm_partial_finalize_apply(ops, dtype, shape, fpg):
    c0, c1, h, w = shape
    c, hw = c0 + c1, h * w
    nimg = 2 * fpg
    gamma, beta = affine(c, 8)

    def run(rho):
        x = eb.norm_input(nimg // fpg, fpg * hw, c, rho, dtype, 12, device="cuda")
        (sc, sh), names = traced(ops, lambda: ops.groupnorm_stats(x, None, nimg, hw, fpg, gamma, beta, EPS))
        assert names == [f"gn_partial_kernel + gn_finalize_kernel<{tag(ops, dtype)}>"], names
        for silu in (False, True):
            y, names = traced(ops, lambda: ops.groupnorm_apply(x, None, nimg, hw, sc, sh, silu))
            assert names == [f"gn_apply_kernel<{tag(ops, dtype)}>"], names
            yield f"{shape} fpg={fpg} silu={silu}", y, eb.groupnorm(x, gamma, beta, EPS, seg_rows=fpg * hw, silu=silu, n_adds=PARTIAL_ADDS,
                                                                             guard=eb.GN_GUARD_RATIO), dtype
    sweep("partial + finalize + apply", dtype, run)


# ---- the opt-in cross-frame one-launch route: a video is one "image" of the grouped kernel

@pytest.mark.parametrize("dtype", DTYPES)
def test_groupnorm_cross_frame_one_launch(ops, dtype):
    c, frames, hw, videos = 1280, 14, 4 * 7, 3
    gamma, beta = affine(c, 9)

    def run(rho):
        x = eb.norm_input(videos, frames * hw, c, rho, dtype, 13, device="cuda")
        for silu in (False, True):
            keep, ops.GN_CROSS_MAX_ROWS = ops.GN_CROSS_MAX_ROWS, 512
            try:
                y, names = traced(ops, lambda: ops.groupnorm(x, None, videos * frames, hw, frames, gamma, beta, EPS, silu))
            finally:
                ops.GN_CROSS_MAX_ROWS = keep
            assert names == [f"gn_group_kernel<{tag(ops, dtype)}>"], names
            yield f"silu={silu}", y, eb.groupnorm(x, gamma, beta, EPS, seg_rows=frames * hw, silu=silu,
                                                  n_adds=grouped_adds(c, frames * hw, dtype), guard=eb.GN_GUARD_RATIO), dtype
    sweep("cross-frame one-launch", dtype, run)


# ---- producer tile sums -> tt_groupnorm_tiles: one producer per sums writer.  The producer runs with a zero weight and the wanted
# tensor as residual (out = 0 * A W^T + residual), so its STORED output has the statistics of eb.norm_input; the reference reads it.

# fpgs: the frames-per-group values each producer's sums serve (asserted in the test)
TILE_CASES = dict(
    w320_linear_res=dict(fpgs=(1, 4), rows=50176, k=128, n=320, mode=0, frames=4, kernel="gemm_w320_kernel<", stat_rows=(256,)),
    w320h_conv_64=dict(fpgs=(1, 4), nimg=28, h=16, w=28, k=64, n=640, mode=1, frames=4, per_image=True, kernel="gemm_w320h_kernel<", stat_rows=(64,)),
    tiled_linear=dict(fpgs=(1, 4), rows=3584, k=256, n=640, mode=0, frames=4, kernel="gemm_kernel<", stat_rows=(64, 128)),
    tiled_small=dict(fpgs=(1, 4), rows=1024, k=64, n=96, mode=0, frames=4, kernel="gemm_kernel<", stat_rows=(64, 128)),          # cpg = 3
    tiled_wave_rows_ragged=dict(fpgs=(14,), nimg=28, h=8, w=14, k=128, n=1280, mode=2, frames=14, blend=True, kernel="gemm_kernel<", stat_rows=(32,)),
    splitk_conv_l3=dict(fpgs=(1, 14), nimg=28, h=4, w=7, k=1280, n=1280, mode=1, frames=14, per_image=True, kernel="", stat_rows=(28,), splitk=True))


def produce(ops, g, x, stats, gn=None):
    """the producer launch of TILE_CASES entry g with the stored output x: (out, kernel name, tt_gemm_plan cfg)"""
    from tests.test_error_bounds_gpu import launch
    mode, n, k = g["mode"], g["n"], g["k"]
    rows = x.shape[0]
    taps = {0: 1, 1: 9, 2: 3}[mode]
    gen = torch.Generator(device="cuda").manual_seed(3)
    a = torch.randn(rows, k, generator=gen, device="cuda").to(x.dtype)
    w = torch.zeros(n, taps * k, dtype=x.dtype, device="cuda")
    kw = dict(mode=mode, residual=x)
    if mode == 1:
        kw["conv"] = (g["nimg"], g["h"], g["w"], g["h"], g["w"], 1, 0)
    if mode == 2:
        kw["tconv"] = (g["frames"], g["h"] * g["w"])
    if g.get("blend"):
        kw.update(blend=x, alpha=0.3)
    return launch(ops, lambda: ops.gemm(a, w, stats=stats, gn=gn, **kw))


def tile_case_params():
    for case, g in TILE_CASES.items():
        for dtype in DTYPES:
            if dtype == torch.float32 and (case.startswith("w320") or g.get("splitk")):
                continue                                     # the big-tile kernels and the split-K plans serve 16-bit storage
            yield pytest.param(case, dtype, id=f"{case}-{str(dtype).replace('torch.', '')}")


@pytest.mark.parametrize("case,dtype", list(tile_case_params()))
def test_groupnorm_from_producer_tile_sums(ops, case, dtype):
    g = TILE_CASES[case]
    n, frames = g["n"], g["frames"]
    if g["mode"] == 0:
        rows = g["rows"]
        hw = rows // 28 if rows % 28 == 0 else rows // 8
    else:
        hw = g["h"] * g["w"]
        rows = g["nimg"] * hw
    nimg = rows // hw
    seg0 = hw if g.get("per_image") else frames * hw          # the segment the producer is told about
    gamma, beta = affine(n, 10)
    assert ops.GN_TILES and ops.GN_TILES_SEG, "the producer hand-off is the default route"

    def run(rho):
        x = eb.norm_input(rows // seg0, seg0, n, rho, dtype, 14, device="cuda")
        out, name, cfg = produce(ops, g, x, seg0)
        st = getattr(out, "_tt_stats", None)
        assert st is not None, f"{case}: route without statistics epilogue"
        r = st[1]
        if dtype != torch.float32:                           # (the fp32 template has its own tile shapes)
            assert name.startswith(g["kernel"]) and r in g["stat_rows"], (name, cfg, r)
            assert (cfg[6] >= 2) == bool(g.get("splitk")), cfg
        else:
            assert name.startswith("gemm_kernel<f32_tag") and seg0 % r == 0, (name, r)
        yield f"sums of {r}-row tiles", st[0], eb.tile_sums(out, r), torch.float32
        # `fpgs`: the segment lengths that are whole numbers of this producer's statistics tiles -- per image and across `frames` images, except
        # tiled_wave_rows_ragged, whose 112-row images are no whole number of its 32-row wave rows (cross-frame only).  Stated, not derived
        # from r: a change of tile height must fail here, not quietly empty the sweep
        assert tuple(f for f in (1, frames) if (f * hw) % r == 0 and nimg % f == 0) == g["fpgs"], (case, r, g["fpgs"])
        for fpg in g["fpgs"]:
            seg = fpg * hw
            b = {silu: eb.groupnorm(out, gamma, beta, EPS, seg_rows=seg, silu=silu, n_adds=r, guard=eb.GN_GUARD_RATIO_TILES) for silu in (False, True)}      # a tile's chain of r rows
            for silu in (False, True):
                y, names = traced(ops, lambda: ops.groupnorm(out, None, nimg, hw, fpg, gamma, beta, EPS, silu))
                assert names == [f"gn_tiles_kernel<{tag(ops, dtype)}>"], names
                yield f"fpg={fpg} silu={silu}", y, b[silu], dtype
    sweep(f"tile sums -> tt_groupnorm_tiles, {case}", dtype, run)


# ---- GroupNorm inside the split-K reduction pass (TtGemmArgs.gn_out)

GN_OUT_CASES = dict(conv_l3_per_image=dict(nimg=28, h=4, w=7, k=1280, n=1280, mode=1, frames=14, fpg=1),
                    tconv_l3_cross_frame_film=dict(nimg=28, h=4, w=7, k=1280, n=1280, mode=2, frames=14, fpg=14))


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("case", list(GN_OUT_CASES))
def test_groupnorm_inside_the_splitk_reduction(ops, dtype, case):
    g = GN_OUT_CASES[case]
    hw, n, fpg, nimg = g["h"] * g["w"], g["n"], g["fpg"], g["nimg"]
    seg = fpg * hw
    gamma, beta = affine(n, 15)
    assert ops.GN_FUSED

    def run(rho):
        x = eb.norm_input(nimg // fpg, seg, n, rho, dtype, 16, device="cuda")
        for silu in (False, True):
            out, name, cfg = produce(ops, g, x, seg, gn=(gamma, beta, EPS, silu))
            fz = getattr(out, "_tt_gn", None)
            assert fz is not None and cfg[6] >= 2, f"{case}: no split-K reduction pass on this plan ({name}, {cfg})"
            y, names = traced(ops, lambda: ops.groupnorm(out, None, nimg, hw, fpg, gamma, beta, EPS, silu))
            assert names == [] and y.data_ptr() == fz[0].data_ptr(), "groupnorm() must hand out the reduction pass's result without a launch"
            assert torch.equal(out, x), "a zero product plus the residual stores the residual"
            yield f"silu={silu}", y, eb.groupnorm(out, gamma, beta, EPS, seg_rows=seg, silu=silu), dtype
    sweep(f"gn_out in the split-K reduction, {case}", dtype, run)


# ---- LayerNorm: ln_kernel (with and without the fused row vector) and ln_block_kernel

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [64, 320, 1280])
def test_layernorm(ops, dtype, c):
    rows = 37 * 6
    gamma, beta = affine(c, 17)
    gen = torch.Generator().manual_seed(18)
    emb = (torch.randn(3, c, generator=gen) * 0.125).cuda()

    def run(rho):
        x = eb.ln_input(rows, c, rho, dtype, 19).cuda()
        y, names = traced(ops, lambda: ops.layernorm(x, gamma, beta, EPS))
        assert names == [f"ln_kernel<{tag(ops, dtype)}>"], names
        yield "plain", y, eb.layernorm(x, gamma, beta, EPS, n_adds=eb.ln_adds(c)), dtype
        (xs, y2), names = traced(ops, lambda: ops.layernorm(x, gamma, beta, EPS, rowvec=emb, rows_per_vec=37, nvec=3))
        assert names == [f"ln_kernel<{tag(ops, dtype)}>"], names
        idx = (torch.arange(rows) // 37) % 3
        xsum = eb.Bound(x.double() + emb.double()[idx.cuda()], eb.U * (x.double().abs() + emb.double()[idx.cuda()].abs()))
        yield "x + row vector", xs, xsum, dtype
        yield "fused row vector", y2, eb.layernorm(xs, gamma, beta, EPS, n_adds=eb.ln_adds(c)), dtype      # normalises the STORED sum
    sweep("ln_kernel", dtype, run)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [64, 320, 1280])
def test_layernorm_block(ops, dtype, c):
    nb, rows = 12, 37                                        # twelve blocks: the constant one and the one with spread 2^-9 among them

    def run(rho):
        xb = eb.ln_input(nb, rows * c, rho, dtype, 20).cuda()
        y, names = traced(ops, lambda: ops.layernorm_block(xb.view(nb * rows, c), rows, EPS))
        assert names == [f"ln_block_kernel<{tag(ops, dtype)}>"], names
        yield "block", y.view(nb, rows * c), eb.layernorm(xb, None, None, EPS, n_adds=eb.ln_block_adds(rows, c), pivot=xb[:, 0]), dtype
    sweep("ln_block_kernel", dtype, run)
