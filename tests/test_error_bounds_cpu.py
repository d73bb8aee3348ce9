"""CPU: the per-element error bound of tests/error_bounds.py has teeth.  A "correct kernel" is emulated in fp32 -- products summed in
16-wide K blocks taken in a shuffled order, the epilogue in fp32, the result rounded to the storage type -- and must pass its bound;
every mutant below (a slip a tile kernel can make: one tile, one column, one row, one block) must fail it.  Beside each mutant the
test prints whether the flat tolerances of tests/test_ops_gpu.py (bf16 rtol 1.6e-2 / atol 3.2e-2, fp16 rtol = atol = 1e-3) would
have noticed it: reported, not asserted.  Also the fp32 emulations of the fast GELU forms of the persistent kernel (common.h)
against their budgets over the whole real line."""
import pytest
import torch
import torch.nn.functional as F

from tests import error_bounds as eb

DTYPES16 = [torch.bfloat16, torch.float16]
FLAT = {torch.bfloat16: dict(rtol=1.6e-2, atol=3.2e-2), torch.float16: dict(rtol=1e-3, atol=1e-3)}
T = 32                              # the tile the mutants hit: 32 x 32
M, N, K = 100, 72, 64               # ragged against 32 x 32 tiles: 3 whole tile rows + 4 rows, 2 whole tile columns + 8


def flat_verdict(got, ref, dtype) -> str:
    ok = torch.allclose(got.double(), ref, rtol=FLAT[dtype]["rtol"], atol=FLAT[dtype]["atol"])
    return "MISSED by the flat tolerance" if ok else "caught by the flat tolerance"


def emu_acc(a, w, seed=0, drop=None):
    """fp32 accumulation of a @ w.T over 16-wide K blocks in a shuffled order (a, w: storage values, [m, K] / [n, K]);
    drop = (row tile, column tile, block): that K block is skipped inside that 32 x 32 tile"""
    a32, w32 = a.float(), w.float()
    nb = a.shape[1] // 16
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    for b in torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).tolist():
        part = a32[:, 16 * b:16 * b + 16] @ w32[:, 16 * b:16 * b + 16].T
        if drop is not None and drop[2] == b:
            part[drop[0] * T:(drop[0] + 1) * T, drop[1] * T:(drop[1] + 1) * T] = 0
        acc = acc + part
    return acc


def rowvec_index(m, rows_per, mod):
    i = torch.arange(m) // rows_per
    return i % mod if mod else i


# ---- fp32 emulations of the GELU forms (common.h), the constants as written there

def gelu_erf32(x):
    x = x.float()
    t = 1.0 / (x.abs() * (0.3275911 * 0.70710678118654752) + 1.0)
    p = t * (0.5 * 1.061405429) + (0.5 * -1.453152027)
    p = p * t + 0.5 * 1.421413741
    p = p * t + 0.5 * -0.284496736
    p = p * t + 0.5 * 0.254829592
    u = p * t * torch.exp2(x * x * -0.72134752044448170)
    return x * torch.where(x >= 0, 1.0 - u, u)


def gelu_sig32(x):
    x = x.float()
    x2 = x * x
    q = x2 * -4.111726866540266e-06 + 1.0587536235107109e-04
    q = q * x2 + 2.534117375034839e-04
    q = q * x2 + -0.10500594228506088
    q = q * x2 + -2.3021652698516846
    return x * (1.0 / (torch.exp2(x * q) + 1.0))


def gelu_poly32(x, leak=False):
    """gelu_poly_pk; leak=True: the form before the fix, x * Phi(clamp(x)) -- 3.2e-5 x for x < -3.75 where gelu is 0"""
    x = x.float()
    xc = x.clamp(-3.75, 3.75)
    t = xc * xc
    q = t * 3.9124383732769275e-08 + -2.3762543150951387e-06
    q = q * t + 6.234781903913245e-05
    q = q * t + -0.0009441798320040107
    q = q * t + 0.009362553246319294
    q = q * t + -0.06578987091779709
    q = q * t + 0.39870646595954895
    phi = xc * q + 0.5
    return (x if leak else x.clamp_min(-3.75)) * phi


FORMS = {"erf": gelu_erf32, "sigmoid": gelu_sig32, "poly": gelu_poly32}


# ---- the emulated kernel: Linear with the full epilogue

def operands(dtype, seed=1, n=N, k=K):
    a, w, cs = eb.decade_operands(M, n, k, dtype, seed)
    bias = eb.scaled((n,), cs, torch.float32, seed + 1)
    rv = eb.scaled((3, n), cs, torch.float32, seed + 2)
    res = eb.scaled((M, n), cs, dtype, seed + 3)
    bl = eb.scaled((M, n), cs, dtype, seed + 4)
    return a, w, bias, rv, res, bl


ROWS_PER, MOD, S, ALPHA = 1, 3, 0.75, 0.3        # row r takes rowvec[r % 3]


def emu_full(dtype, mut=None):
    a, w, bias, rv, res, bl = operands(dtype)
    acc = emu_acc(a, w, drop=(1, 1, 2) if mut == "drop_k_block" else None)
    b = bias.clone().expand(M, N).clone()
    if mut == "bias_shift":                          # tile (2, 0): columns read bias[c + 1]
        b[2 * T:3 * T, 0:T] = bias[1:T + 1]
    s = torch.tensor(S, dtype=torch.float32)
    idx = rowvec_index(M, ROWS_PER, MOD)
    if mut == "rowvec_period":
        idx = rowvec_index(M, ROWS_PER, 2)
    rvm = rv[idx]
    if mut == "rowvec_off_by_one":                   # the first row of tile row 2 (row 64) takes the previous row's vector
        rvm[2 * T] = rv[(2 * T - 1) % MOD]
    if mut == "scale_not_on_bias":                   # acc_scale applied to acc only, the bias added unscaled
        v = acc * s + b
    else:
        v = (acc + b) * s
    if mut == "scale_on_rowvec":                     # acc_scale applied to the row vector as well
        v = v + rvm * s
    else:
        v = v + rvm
    r = res.float()
    if mut == "residual_next_row":                   # the ragged last tile row (rows 96..99) reads the residual of the next row
        r[3 * T:] = res.float()[torch.clamp(torch.arange(3 * T, M) + 1, max=M - 1)]
    v = v + r
    al = torch.tensor(ALPHA, dtype=torch.float32)
    v = al * bl.float() + (1.0 - al) * v
    got = v.to(dtype)
    ref = eb.epilogue(eb.matmul(a, w), bias=bias, acc_scale=S, rowvec=rv.double()[rowvec_index(M, ROWS_PER, MOD)],
                      residual=res, blend=bl, alpha=ALPHA)
    return got, ref


def emu_geglu(dtype, form, mut=None):
    h = 48
    a, w, cs = eb.decade_operands(M, 2 * h, K, dtype, 7)
    bias = eb.scaled((2 * h,), cs, torch.float32, 8)
    v = emu_acc(a, w) + bias
    val, gate = v[:, :h], v[:, h:]
    if mut == "geglu_swap":                          # one column pair with value and gate exchanged
        val, gate = val.clone(), gate.clone()
        val[:, 5], gate[:, 5] = v[:, h + 5], v[:, 5]
    g = gelu_poly32(gate, leak=True) if mut == "gelu_leak" else FORMS[form](gate)
    got = (val * g).to(dtype)
    ref = eb.epilogue(eb.matmul(a, w), bias=bias, geglu=form)
    return got, ref


def emu_mode3(dtype, mut=None):
    """tt_gemm mode 3: 3x3 conv, stride 2, zero padding on the bottom / right only"""
    nimg, c, cout, hh, ww = 2, 16, 40, 9, 12
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(nimg, c, hh, ww, generator=g, dtype=torch.float64) * 2.0 ** (torch.arange(hh * ww) % 7 - 3).reshape(hh, ww)).to(dtype)
    cs = torch.exp2(eb.col_exponents(cout))
    wt = (torch.randn(cout, c, 3, 3, generator=g, dtype=torch.float64) * (9 * c) ** -0.5 * cs[:, None, None, None]).to(dtype)
    pad = (1, 0, 1, 0) if mut == "mode3_top_left" else (0, 1, 0, 1)
    cols = F.unfold(F.pad(x.float(), pad), 3, stride=2)                      # [nimg, c*9, L]
    a = cols.transpose(1, 2).reshape(-1, c * 9)
    got = emu_acc(a, wt.float().reshape(cout, -1)).to(dtype)
    op = lambda xx, ww_: F.conv2d(F.pad(xx, (0, 1, 0, 1)), ww_, stride=2)
    return got, eb.contract(op, x, wt).tokens()


def emu_ln(dtype):
    """LayerNorm fold: rows with large means, folded zero-sum-rounded weights, fp32 statistics as ln_stat accumulates them"""
    from this_and_that_vdm_amd.packing import fold_layernorm, zero_sum_round
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(M, K, generator=g) * 1.5 + torch.randn(M, 1, generator=g) * 4.0).to(dtype)
    w = torch.randn(N, K, generator=g) * K ** -0.5 * torch.exp2(eb.col_exponents(N)).float()[:, None]
    bias = torch.randn(N, generator=g) * torch.exp2(eb.col_exponents(N)).float()
    gam, bet = torch.randn(K, generator=g) * 0.2 + 1, torch.randn(K, generator=g) * 0.3
    wf, bf = fold_layernorm(w, bias, gam, bet)
    wq = zero_sum_round(wf, dtype)
    xf = x.float()
    sm, sq = xf.sum(1) * (1.0 / K), (xf * xf).sum(1) * (1.0 / K)
    rs = torch.rsqrt(torch.clamp(sq - sm * sm, min=0.0) + 1e-5)
    got = (emu_acc(x, wq) * rs[:, None] + bf).to(dtype)
    rstd, rel = eb.ln_rstd(x, 1e-5)
    return got, eb.epilogue(eb.matmul(x, wq), rstd=rstd, rstd_rel=rel, bias=bf)


def emu_split16(mut=None):
    """TT_F32 split16: operands split into fp16 h = fp16(x 2^-8), l = fp16((x - 2^8 h) 2^3), products 2^16 hh + 2^5 (hl + lh)"""
    a, w, cs = eb.decade_operands(M, N, K, torch.float32, 31)

    def split(x):
        h = (x * 2.0 ** -8).half()
        lo = ((x - h.float() * 2.0 ** 8) * 2.0 ** 3).half()
        return h.float(), lo.float()
    (ah, al), (wh, wl) = split(a), split(w)
    acc = emu_acc(ah, wh) * 2.0 ** 16 + (emu_acc(ah, wl) + emu_acc(al, wh)) * 2.0 ** 5
    return acc, eb.matmul(a, w, split16=True)


# ---- a correct kernel passes

@pytest.mark.parametrize("dtype", DTYPES16)
def test_correct_kernel_passes_full_epilogue(dtype):
    got, ref = emu_full(dtype)
    assert eb.check(got, ref, dtype, f"emulated full epilogue {dtype}") <= 1.0


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("form", ["erf", "sigmoid", "poly"])
def test_correct_kernel_passes_geglu(dtype, form):
    got, ref = emu_geglu(dtype, form)
    eb.check(got, ref, dtype, f"emulated GEGLU ({form}) {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
def test_correct_kernel_passes_mode3_and_layernorm_fold(dtype):
    got, ref = emu_mode3(dtype)
    eb.check(got, ref, dtype, f"emulated mode 3 {dtype}")
    got, ref = emu_ln(dtype)
    eb.check(got, ref, dtype, f"emulated LayerNorm fold {dtype}")


def test_correct_kernel_passes_split16_and_exact_f32():
    got, ref = emu_split16()
    eb.check(got, ref, torch.float32, "emulated split16")
    a, w, _ = eb.decade_operands(M, N, K, torch.float32, 32)
    eb.check(emu_acc(a, w), eb.matmul(a, w), torch.float32, "emulated exact fp32")


# ---- every mutant fails

MUTANTS_FULL = ["drop_k_block", "bias_shift", "scale_not_on_bias", "scale_on_rowvec", "rowvec_off_by_one", "rowvec_period",
                "residual_next_row"]


def _must_fail(got, ref, dtype, what):
    with pytest.raises(AssertionError, match="breaks its error bound"):
        eb.check(got, ref, dtype, what)
    print(f"[mutant] {what}: flagged by the bound; {flat_verdict(got, ref.ref, dtype)}")


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("mut", MUTANTS_FULL)
def test_mutant_of_the_linear_epilogue_is_flagged(dtype, mut):
    got, ref = emu_full(dtype, mut)
    _must_fail(got, ref, dtype, f"{mut} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
@pytest.mark.parametrize("mut,form", [("geglu_swap", "erf"), ("geglu_swap", "poly"), ("gelu_leak", "poly")])
def test_mutant_of_the_geglu_epilogue_is_flagged(dtype, mut, form):
    got, ref = emu_geglu(dtype, form, mut)
    _must_fail(got, ref, dtype, f"{mut} ({form}) {dtype}")


@pytest.mark.parametrize("dtype", DTYPES16)
def test_mutant_mode3_padded_top_left_is_flagged(dtype):
    got, ref = emu_mode3(dtype, "mode3_top_left")
    _must_fail(got, ref, dtype, f"mode3_top_left {dtype}")


# ---- the fast GELU forms against their budgets on the whole line (fp32 emulation of common.h)

def _gelu_sweep():
    g = torch.linspace(-16, 16, 64001, dtype=torch.float64)
    geo = torch.logspace(-3, 4, 2000, dtype=torch.float64)
    edges = torch.tensor([3.75, 6.5, 12.0], dtype=torch.float64)
    edges = (edges[:, None] + torch.linspace(-1e-3, 1e-3, 41, dtype=torch.float64)[None]).reshape(-1)
    g = torch.cat([g, geo, -geo, edges, -edges])
    return g.float().double()                        # exact fp32 arguments


@pytest.mark.parametrize("form", ["erf", "sigmoid", "poly"])
def test_gelu_form_meets_its_budget_everywhere(form):
    g = _gelu_sweep()
    G = eb.gelu_exact(g)
    err = (FORMS[form](g).double() - G).abs()
    ratio = float((err / eb.gelu_budget(form, g, G)).max())
    print(f"[gelu] {form}: max err/budget = {ratio:.3g}, max |err| over |g| <= 12: {float(err[g.abs() <= 12].max()):.3g}")
    assert ratio <= 1.0
    if form == "poly":                               # the maximum over |g| <= 12 (3.9e-4, at g = 12) is not raised by the fix
        old = (gelu_poly32(g, leak=True).double() - G).abs()
        assert float(err[g.abs() <= 12].max()) <= float(old[g.abs() <= 12].max())


def test_gelu_poly_leak_breaks_its_budget():
    g = _gelu_sweep()
    G = eb.gelu_exact(g)
    err = (gelu_poly32(g, leak=True).double() - G).abs()
    assert float((err / eb.gelu_budget("poly", g, G)).max()) > 1.0
    assert float(err[g == -300.0].max() if (g == -300.0).any() else err[g < -290].max()) > 5e-3


# ---- GroupNorm / LayerNorm: the normalisation bounds (eb.groupnorm, eb.layernorm, eb.tile_sums) against an emulated correct kernel
# -- fp64 statistics, then the fp32 arithmetic norm.hip states: s_mean / s_rstd rounded to fp32, sc = s_rstd * gamma,
# sh = beta - s_mean * sc, t = fmaf(x, sc, sh), silu_f, the store -- and against the slips a normalisation kernel can make.  Inputs:
# eb.norm_input (|group mean| = rho x group spread, rho over eb.RHO_GRID; a constant group; a group with spread^2 near eps).

DTYPES = DTYPES16 + [torch.float32]
OPS_TOL = {torch.float16: (1e-3, 1e-3), torch.bfloat16: (1.6e-2, 3.2e-2), torch.float32: (2e-5, 2e-5)}   # close(.., scale=2.0) of tests/test_ops_gpu.py
EPS = 1e-5
G = eb.GN_GROUPS


def ops_flat_ok(got, ref, dtype) -> bool:
    """what tests/test_ops_gpu.py asserts for every GroupNorm: assert_close against the fp32 reference, one flat rtol / atol per type"""
    rtol, atol = OPS_TOL[dtype]
    return bool(torch.allclose(got.float(), ref.float(), rtol=rtol, atol=atol))


def fma32(a, b, c):
    """fmaf: the product of two fp32 numbers is exact in fp64 and the fp64 sum rounds at 2^-53 before the fp32 rounding"""
    return (a.double() * b.double() + c.double()).float()


def strip_sums32(x, tile_rows):
    """colstat_strip: per column, the rows of a 32-row strip added one after the other from 0 in fp32 (squares through fmaf), the strips
    of a tile chained (`a += srow_sum`) -> fp32 sums [tiles, C] x 2"""
    rows, c = x.shape
    xt = x.float().view(rows // tile_rows, tile_rows, c)
    ts = tq = None
    for r0 in range(0, tile_rows, 32):
        a = torch.zeros(xt.shape[0], c)
        b = torch.zeros(xt.shape[0], c)
        for r in range(r0, min(r0 + 32, tile_rows)):
            a = a + xt[:, r]
            b = fma32(xt[:, r], xt[:, r], b)
        ts, tq = (a, b) if ts is None else (a + ts, b + tq)
    return ts, tq


def emu_groupnorm(x, gamma, beta, seg_rows, silu, dtype, mut=None, frames=1, tile_rows=128, guard=None):
    """x [nseg * seg_rows, C] storage values -> what a GroupNorm kernel stores.  Mutants: see GN_MUTANTS.  guard (with mut =
    "fp32_tile_sums"): the kernel as norm.hip has it -- the fp32 sums, and the exact centred statistics for a group with E[x^2] > guard var"""
    rows, c = x.shape
    cpg, nseg = c // G, rows // seg_rows
    stat_rows = seg_rows // frames if mut == "one_frame" else seg_rows          # the statistics of each frame, not of the video
    xg = x.double().view(rows // stat_rows, stat_rows, G, cpg)
    cnt = stat_rows * cpg
    if mut in ("fp32_tile_sums", "no_clamp"):        # uncentred sums whose lowest level is fp32; fp64 across tiles and channels
        ts, tq = strip_sums32(x, tile_rows)
        s = ts.double().view(nseg, -1, G, cpg).sum((1, 3))
        q = tq.double().view(nseg, -1, G, cpg).sum((1, 3))
        mean = s / cnt
        var = q / cnt - mean * mean
        if mut != "no_clamp":
            var = var.clamp_min(0.0)
        if guard is not None:
            redo = q / cnt > guard * var
            m_exact = xg.mean((1, 3))
            mean = torch.where(redo, m_exact, mean)
            var = torch.where(redo, (xg - m_exact[:, None, :, None]).square().mean((1, 3)), var)
    else:
        mean = xg.mean((1, 3))
        var = (xg - mean[:, None, :, None]).square().mean((1, 3))
    if mut == "sample_variance":
        var = var * cnt / (cnt - 1)
    e32 = eb.f32(EPS)
    r = 1.0 / (var.sqrt() + e32) if mut == "eps_outside_sqrt" else 1.0 / (var + e32).sqrt()
    if mut == "one_frame":
        nseg, seg_rows = rows // stat_rows, stat_rows
    if mut == "previous_segment":
        mean, r = mean.roll(1, 0), r.roll(1, 0)
    ch = torch.arange(c)
    gi = ((ch + 1) // cpg).clamp_max(G - 1) if mut == "group_off_by_one" else ch // cpg
    mean32, r32 = mean.float()[:, gi], r.float()[:, gi]                         # [nseg, C]
    sc = r32 * gamma
    sh = beta - mean32 * sc
    t = fma32(x.float().view(nseg, seg_rows, c), sc[:, None], sh[:, None])
    y = t / (1.0 + torch.exp(-t)) if (silu and mut != "no_silu") else t
    return y.reshape(rows, c).to(dtype)


def gn_case(dtype, rho, c=96, hw=15, nseg=3, seed=5):
    """the smallest shapes: C = 96 (cpg = 3: a group is no whole number of 4-channel quads), 15 rows"""
    x = eb.norm_input(nseg, hw, c, rho, dtype, seed)
    gamma, beta = eb.norm_affine(c, seed + 1)
    return x, gamma, beta


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [False, True])
def test_correct_groupnorm_passes_at_every_ratio(dtype, silu):
    worst = 0.0
    for rho in eb.RHO_GRID:
        for c, hw, nseg in ((96, 15, 3), (320, 99, 2)):
            x, gamma, beta = gn_case(dtype, rho, c, hw, nseg)
            got = emu_groupnorm(x, gamma, beta, hw, silu, dtype)
            worst = max(worst, eb.check(got, eb.groupnorm(x, gamma, beta, EPS, seg_rows=hw, silu=silu), dtype,
                                        f"emulated GroupNorm C={c} hw={hw} rho={rho} silu={silu} {dtype}"))
    print(f"[norm bound] correct GroupNorm {dtype} silu={silu}: largest err/bound over the rho grid = {worst:.3g}")
    assert worst <= 1.0


# mutant -> (rho, what it needs): each at the smallest shape it can occur at
GN_MUTANTS = ["sample_variance", "eps_outside_sqrt", "group_off_by_one", "previous_segment", "one_frame", "no_silu", "no_clamp",
              "fp32_tile_sums"]


def gn_mutant(dtype, mut, rho=None):
    """(got, Bound, fp32 reference) of one mutant.  fp32_tile_sums / no_clamp: C = 320, two 128-row tiles per segment, the largest rho
    (no_clamp: fp32 storage, where the squares of the constant group round -- in 16 bits they are exact and its variance is exactly 0)"""
    silu = True
    if mut in ("fp32_tile_sums", "no_clamp"):
        rho = eb.RHO_GRID[-1] if rho is None else rho
        c, hw, nseg, frames = 320, 256, 4, 1
    elif mut == "one_frame":
        rho = 5 if rho is None else rho
        c, hw, nseg, frames = 96, 2 * 15, 2, 2          # a video of two 15-row frames
    else:
        rho = 5 if rho is None else rho
        c, hw, nseg, frames = 96, 15, 3, 1
    x, gamma, beta = gn_case(dtype, rho, c, hw, nseg)
    got = emu_groupnorm(x, gamma, beta, hw, silu, dtype, mut=mut, frames=frames)
    b = eb.groupnorm(x, gamma, beta, EPS, seg_rows=hw, silu=silu)
    return got, b


# (no_clamp on fp32 storage only: the squares of a constant 16-bit group are exact in fp32 and its variance is exactly 0 with or without the clamp)
# (... and fp32_tile_sums not on bf16 storage, whose own half ulp, 2^-9 |y|, is of the size of that error, u rho^2 / 2 ~ 3e-3 of t - beta)
@pytest.mark.parametrize("dtype,mut", [(d, m) for d in DTYPES for m in GN_MUTANTS
                                       if (m != "no_clamp" or d == torch.float32) and (m != "fp32_tile_sums" or d != torch.bfloat16)])
def test_mutant_of_groupnorm_is_flagged(dtype, mut):
    got, b = gn_mutant(dtype, mut)
    with pytest.raises(AssertionError, match="breaks its error bound"):
        eb.check(got, b, dtype, f"{mut} {dtype}")
    print(f"[mutant] {mut} {dtype}: flagged by the bound; the flat tolerance of test_ops_gpu.py "
          f"{'MISSES' if ops_flat_ok(got, b.ref, dtype) else 'catches'} it")


def _benign(dtype, shift=0.0, c=320, hw=256, nimg=4):
    """the inputs of tests/test_ops_gpu.py's GroupNorm tests (randn * 3 + 1.5, gamma = randn + 1, beta = randn); shift: a mean further out"""
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(nimg * hw, c, generator=g) * 3.0 + 1.5 + shift).to(dtype)
    return x, torch.randn(c, generator=g) + 1, torch.randn(c, generator=g)


@pytest.mark.parametrize("dtype,mut,shift", [(torch.bfloat16, "sample_variance", 0.0), (torch.float16, "eps_outside_sqrt", 0.0),
                                             (torch.float32, "eps_outside_sqrt", 0.0),
                                             (torch.float16, "fp32_tile_sums", 150.0)])      # |mean| = 50 spreads
def test_flat_tolerance_is_blind_where_the_bound_is_not(dtype, mut, shift):
    """the same wrong output passes the flat rtol / atol of tests/test_ops_gpu.py (on its own kind of input) and breaks the bound"""
    hw = 256
    x, gamma, beta = _benign(dtype, shift)
    got = emu_groupnorm(x, gamma, beta, hw, True, dtype, mut=mut)
    b = eb.groupnorm(x, gamma, beta, EPS, seg_rows=hw, silu=True)
    assert eb.ratio(emu_groupnorm(x, gamma, beta, hw, True, dtype), b, dtype) <= 1.0          # (the correct kernel passes both)
    assert ops_flat_ok(got, b.ref, dtype), "the flat tolerance was expected to miss this mutant"
    r = eb.ratio(got, b, dtype)
    print(f"[mutant] {mut} {dtype} on randn * 3 + {1.5 + shift}: passes the flat tolerance, err/bound = {r:.3g}")
    assert r > 1.0


@pytest.mark.parametrize("tile_rows", [32, 64, 128, 256])
def test_tile_sums_bound(tile_rows):
    """the colstat_strip order passes the summation bound at the largest rho (where the sums are largest against their terms' spread);
    a tile that misses its last row, or takes the first row of the next tile, breaks it"""
    x = eb.norm_input(2, 2 * tile_rows, 96, eb.RHO_GRID[-1], torch.float32, 9)
    b = eb.tile_sums(x, tile_rows)
    ts, tq = strip_sums32(x, tile_rows)
    got = torch.stack([ts, tq], 1)
    assert eb.check(got, b, torch.float32, f"emulated tile sums, {tile_rows}-row tiles") <= 1.0
    xs = x.clone().view(-1, tile_rows, 96)
    xs[1, -1] = xs[2, 0]                                       # tile 1 reads one row too far
    ts, tq = strip_sums32(xs.view(-1, 96), tile_rows)
    with pytest.raises(AssertionError, match="breaks its error bound"):
        eb.check(torch.stack([ts, tq], 1), b, torch.float32, "tile sums, one row from the next tile")


# ---- LayerNorm (the centred form of ln_kernel / ln_block_kernel)

def emu_layernorm(x, gamma, beta, dtype, mut=None, pivot=False):
    xf = x.float()
    n = x.shape[1]
    if pivot:                                                  # ln_block_kernel: pivot + mean of (x - pivot)
        p = xf[:, :1]
        mean = (p.double() + (xf - p).sum(1, keepdim=True).double() / n).float()
    else:
        mean = xf.sum(1, keepdim=True) / n
    d = xf - mean
    var = (d * d).sum(1, keepdim=True) / (n - 1 if mut == "sample_variance" else n)
    rstd = torch.rsqrt(var + EPS)
    y = d * rstd
    if gamma is not None:
        y = y * gamma + beta
    return y.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [64, 320, 1280])
def test_correct_layernorm_passes_and_sample_variance_is_flagged(dtype, n):
    gamma, beta = eb.norm_affine(n, 3)
    worst = 0.0
    for rho in eb.RHO_GRID:
        x = eb.ln_input(37, n, rho, dtype, 4)
        b = eb.layernorm(x, gamma, beta, EPS, n_adds=eb.ln_adds(n))
        worst = max(worst, eb.check(emu_layernorm(x, gamma, beta, dtype), b, dtype, f"emulated LayerNorm n={n} rho={rho} {dtype}"))
        xb = eb.ln_input(12, 5 * n, rho, dtype, 5)            # twelve blocks of 5 rows (the constant and the tiny one among them)
        bb = eb.layernorm(xb, None, None, EPS, n_adds=eb.ln_block_adds(5, n), pivot=xb[:, 0])
        worst = max(worst, eb.check(emu_layernorm(xb, None, None, dtype, pivot=True), bb, dtype,
                                    f"emulated block LayerNorm 5 x {n} rho={rho} {dtype}"))
        if n == 64:
            with pytest.raises(AssertionError, match="breaks its error bound"):
                eb.check(emu_layernorm(x, gamma, beta, dtype, mut="sample_variance"), b, dtype, f"LayerNorm sample variance rho={rho}")
    print(f"[norm bound] correct LayerNorm n={n} {dtype}: largest err/bound over the rho grid = {worst:.3g}")
    assert worst <= 1.0


# ---- the bound AS THE GPU MODULE USES IT: eb.groupnorm(n_adds=.., guard=..) with the module's own values -- the tile heights 32 .. 256
# under GN_GUARD_RATIO_TILES, and a thread's 4 / 8 / 13 rows of the statistics-pass kernels under GN_GUARD_RATIO.  The kernel as norm.hip
# has it (fp32 sums of that chain length, a group above the guard recomputed centred) must stay under 1 at every rho; the same sums
# WITHOUT the guard must break the bound at rho = 50 and 300 -- the mean term of n_adds applies to groups below the guard only and
# cannot pay for them.

CHAINS = [(32, eb.GN_GUARD_RATIO_TILES, 1792), (64, eb.GN_GUARD_RATIO_TILES, 1792), (128, eb.GN_GUARD_RATIO_TILES, 1792),
          (256, eb.GN_GUARD_RATIO_TILES, 1792), (4, eb.GN_GUARD_RATIO, 104), (8, eb.GN_GUARD_RATIO, 104), (13, eb.GN_GUARD_RATIO, 104)]


def _chain_case(dtype, rho, n, guard, seg, guarded):
    x, gamma, beta = gn_case(dtype, rho, 320, seg, 2)
    got = emu_groupnorm(x, gamma, beta, seg, True, dtype, mut="fp32_tile_sums", tile_rows=n, guard=guard if guarded else None)
    return eb.ratio(got, eb.groupnorm(x, gamma, beta, EPS, seg_rows=seg, silu=True, n_adds=n, guard=guard), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,guard,seg", CHAINS)
def test_guarded_kernel_passes_the_bound_the_gpu_module_uses(dtype, n, guard, seg):
    worst = max(_chain_case(dtype, rho, n, guard, seg, True) for rho in eb.RHO_GRID)
    print(f"[norm bound] guarded fp32 sums, chains of {n}, guard {guard}, {dtype}: largest err/bound over the rho grid = {worst:.3g}")
    assert worst <= 1.0


# (fp16 storage with chains of 4 and 8: the squares of 16-bit values are exact in fp32 and so few additions round less than fp16's own
# half ulp shows -- left out, like bf16 storage throughout)
@pytest.mark.parametrize("dtype,n,guard,seg", [(d, *c) for d in (torch.float32, torch.float16) for c in CHAINS
                                               if d == torch.float32 or c[0] >= 13])
@pytest.mark.parametrize("rho", [50, 300])
def test_unguarded_fp32_sums_break_the_bound_the_gpu_module_uses(dtype, n, guard, seg, rho):
    r = _chain_case(dtype, rho, n, guard, seg, False)
    print(f"[mutant] fp32 sums without the guard, chains of {n}, {dtype}, rho = {rho}: err/bound = {r:.3g}")
    assert r > 1.0
