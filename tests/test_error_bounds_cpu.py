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
