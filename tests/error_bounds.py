"""Per-element error bounds for the dense contractions of libttvdm (tt_gemm's routes, tt_conv3x3) and for its normalisations (every
GroupNorm / LayerNorm route, the producers' tile sums: see groupnorm(), layernorm(), tile_sums() below), derived beforehand from the operands
a kernel read and the arithmetic it is documented to do -- never fitted to measured errors.  A plain module (not a conftest): used by
tests/test_error_bounds_cpu.py (the bound against emulated correct and deliberately wrong kernels), tests/test_error_bounds_gpu.py
(every GEMM route against it) and tests/test_norm_bounds_gpu.py (every normalisation route against it).

For one output element with storage unit roundoff u_s (bf16 2^-8, fp16 2^-11, fp32 2^-24), u = 2^-24, K products a_k w_k and
S = sum_k |a_k| |w_k|:

* reference: fp64, from the exact storage-type operands the kernel received (inputs, packed / folded / zero-sum-rounded weights);
* accumulation (fp32 MFMA chain, any K order, split-K slabs included):  E_acc = 2 sqrt(K) u S.  The cdna guide measured
  0.75-1.5e-7 S at K <= 1024 and 3.5e-7 S at K = 4096 for this chain: a margin of 10x or more;
* split16 (TT_F32 with tt_gemm_set_f32_split(1)): each operand is carried to max(2^-22 |x|, 2^-28) (include/ttvdm.h), so a product
  is off by at most 2^-22 (|a||w| + |a||w|) + 2^-28 (|w| + |a|):  + 2^-21 S + 2^-28 sum_k (|a_k| + |w_k|);
* operands the kernel forms itself before the MFMA (tt_conv3x3's GroupNorm-activated input, rounded to 16 bits):  + sum_k e_k |w_k|,
  e_k = u_s |act_k| + the fp32 budget of forming act_k (conv3x3_formed_err);
* epilogue: + 4u (sum of the absolute values of the fp32 epilogue terms: acc_scale * acc, bias, row vector, the GEGLU product,
  residual, alpha * blend, (1 - alpha) * v);
* LayerNorm fold: the kernel's 1/sigma carries the relative error ln_rstd() derives from the statistics algorithm it runs;
* GEGLU  y = v gelu(g), gelu with exact erf in fp64:  |v| (dG(g) + 1.13 E_g) + |gelu(g)| E_v + E_v 1.13 E_g  (1.13 > max |gelu'|),
  dG the budget of the GELU form the route evaluates (gelu_budget);
* final check:  |got - ref| <= u_s |ref| + (1 + u_s) (sum of the above) + abs_floor,  abs_floor = 2^-25 for fp16 (subnormal
  outputs: half their spacing), 0 otherwise.

Every term scales with the element's own operands, so a wrong term that lands on a small output fails as surely as one on a large
output -- what the flat rtol / atol of the older kernel tests cannot promise."""
import math

import torch

U = 2.0 ** -24
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
ABS_FLOOR = {torch.float16: 2.0 ** -25}
GELU_SLOPE = 1.13                  # > max |gelu'(x)| = 1.1289 (at x = sqrt 2)


def f32(x: float) -> float:
    """a Python scalar as the kernel sees it (TtGemmArgs holds fp32 scalars)"""
    return float(torch.tensor(x, dtype=torch.float32))


class Bound:
    """an fp64 reference tensor and the error budget of the kernel's fp32 value of it, carried through the epilogue"""

    def __init__(self, ref: torch.Tensor, err: torch.Tensor):
        self.ref, self.err = ref, err

    def tokens(self) -> "Bound":
        """[nimg, C, h, w] (or [b, C, f, hw, 1]) -> token-major rows [nimg*h*w, C], the layout tt_gemm writes"""
        t = lambda x: x.movedim(1, -1).reshape(-1, x.shape[1])
        return Bound(t(self.ref), t(self.err))


def contract(op, a: torch.Tensor, w: torch.Tensor, *, split16: bool = False, formed_err=None, k=None) -> Bound:
    """op(a, w): the route's contraction written as an fp64 torch op on the storage values -- a @ w.T for a Linear, F.conv2d with the
    route's padding / stride (upsampling applied to `a` inside op) for a conv.  S = op(|a|, |w|); K per element = op(1, 1) (taps
    that fall into zero padding add exact zeros and do not count) unless `k` gives it.  formed_err: per-operand budget e_k of an
    operand the kernel forms itself (same shape as `a`)."""
    a, w = a.double(), w.double()
    aa, wa = a.abs(), w.abs()
    s = op(aa, wa)
    if k is None:
        kk = op(torch.ones_like(a), torch.ones_like(w)).clamp_min(1.0).sqrt()
    else:
        kk = math.sqrt(k)
    err = 2.0 * kk * U * s
    if split16:
        err = err + 2.0 ** -21 * s + 2.0 ** -28 * (op(aa, torch.ones_like(w)) + op(torch.ones_like(a), wa))
    if formed_err is not None:
        err = err + op(formed_err.double(), wa)
    return Bound(op(a, w), err)


def matmul(a, w, **kw) -> Bound:
    """Linear: a [m, K] (two sources already concatenated), w [n, K]"""
    return contract(lambda x, y: x @ y.T, a, w, k=a.shape[1], **kw)


def ln_rstd(x: torch.Tensor, eps: float):
    """exact 1/sigma of every row of x (fp64, population variance of the STORED 16-bit row) and the relative error budget of the
    kernel's fp32 value of it.

    Derivation, for the algorithm the 16-bit kernels run (gemm_kernel.h ln_stat<bf16_tag / f16_tag>, used by the tiled template,
    gemm_pp.hip and gemm_w320.hip): s = sum_k x_k and q = sum_k x_k^2 are accumulated in fp32 by v_dot2 instructions against 1 and
    against the fragment itself (products of 16-bit values are exact in fp32); a partial sum then passes per-lane and cross-lane
    fp32 additions, at most K - 1 roundings on any path, so |ds| <= g sum|x_k| and |dq| <= g sum x_k^2 with g = K u (deterministic,
    and q has no cancellation).  mean = s * (1/K), E2 = q * (1/K): the rounded 1/K and the product add 2u each.  var = E2 - mean^2:
    the square adds u + 2 |dmean / mean| relative on mean^2, the subtraction u (E2 + mean^2).  With g' = g + 2u and A = sum|x| / K:
        |d var| <= g' E2 + 2 |mean| g' A + 3u mean^2 + u (E2 + mean^2)
    rstd = rsqrtf(max(var, 0) + eps): the addition rounds (u (var + eps)), v_rsq_f32 is faithful (<= 2u relative), and to first
    order d rstd / rstd = d var / (2 (var + eps)):
        rel = (|d var| + u (var + eps)) / (2 (var + eps)) + 2u
    (The fp32 mode shifts its sums by the row's first element, ln_stat_shifted: not covered here.)"""
    x = x.double()
    k = x.shape[1]
    mean = x.mean(1)
    e2 = (x * x).mean(1)
    var = (x - mean[:, None]).square().mean(1)
    a = x.abs().mean(1)
    g = (k + 2) * U
    dvar = g * e2 + 2 * mean.abs() * g * a + 3 * U * mean.square() + U * (e2 + mean.square())
    rel = (dvar + U * (var + eps)) / (2 * (var + eps)) + 2 * U
    return (var + eps).rsqrt(), rel


def gelu_exact(g: torch.Tensor) -> torch.Tensor:
    return 0.5 * g * (1.0 + torch.erf(g * 0.5 ** 0.5))


def gelu_budget(form, g: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """allowed |computed gelu(g) - gelu(g)| of the GELU form a route evaluates in fp32, for an exact argument g (G = gelu(g)):
      erf      Abramowitz-Stegun 7.1.26 (|d erf| <= 1.5e-7, so 7.5e-8 |g| on g Phi(g)): gelu_erf_f / gelu_erf_pk (common.h), the
               tiled template, every dtype.  Plus 8u |g|: Phi is formed in fp32 by about eight roundings of quantities of magnitude
               <= 1 (t = rcp(..) <= 1, the Horner chain's partial sums <= 0.73, exp2 <= 1, the products and 0.5 +- (0.5 - u)), each
               <= u absolute.  Without this term the fp32 evaluation alone breaks the bound near g = 0, where the 0.5 a_k terms
               cancel to Phi = 1/2 (2.3e-7 |g| measured in tests/test_error_bounds_cpu.py against 7.5e-8 + 4u/2 = 1.9e-7)
      sigmoid  Phi ~ 1 / (1 + exp(-g P(g^2))), gelu_sig_pk: the persistent kernel, fp16 storage
      poly     Phi ~ 0.5 + gc P(gc^2), gc = g clamped to +-3.75, gelu_poly_pk: the persistent kernel, bf16 storage -- its comment's
               own figure (4e-4 absolute) for EVERY g, plus 4e-5 relative beyond the clamp
    A tuple of forms: the largest of their budgets (a launch whose rows run on two kernels)."""
    if isinstance(form, (tuple, list)):
        return torch.stack([gelu_budget(f, g, G) for f in form]).amax(0)
    if form == "erf":
        return (7.5e-8 + 8 * U) * g.abs() + 4 * U * G.abs()
    if form == "sigmoid":
        return 8e-6 + 8 * U * G.abs()
    if form == "poly":
        return 4e-4 + 4e-5 * G.abs()
    raise ValueError(form)


def epilogue(acc: Bound, *, rstd=None, rstd_rel=None, bias=None, acc_scale: float = 1.0, rowvec=None, geglu=None, residual=None,
             blend=None, alpha: float = 0.0) -> Bound:
    """tt_gemm's epilogue in the order include/ttvdm.h states it, in fp64, with the budget carried along:
        acc *= rstd (ln_fold);  v = (acc + bias) * acc_scale + rowvec;  geglu: v = v_value * gelu(v_gate);  v += residual;
        v = alpha * blend + (1 - alpha) * v
    rowvec is already expanded to one row per output row ([m, n]); with geglu the columns of acc / bias are in the UNPACKED order
    (values 0 .. n/2 - 1, their gates n/2 .. n - 1) and `geglu` names the GELU form (gelu_budget)."""
    v, e = acc.ref, acc.err
    if rstd is not None:
        r = rstd.double()[:, None]
        v = v * r
        e = e * r + rstd_rel.double()[:, None] * v.abs()
    s = f32(acc_scale)
    v = v * s
    e = e * abs(s)
    terms = v.abs()
    if bias is not None:
        b = bias.double()[None, :] * s
        v = v + b
        terms = terms + b.abs()
    if rowvec is not None:
        rv = rowvec.double()
        v = v + rv
        terms = terms + rv.abs()
    e = e + 4 * U * terms
    if geglu is not None:
        h = v.shape[1] // 2
        val, gate, ev, eg = v[:, :h], v[:, h:], e[:, :h], e[:, h:]
        G = gelu_exact(gate)
        v = val * G
        e = val.abs() * (gelu_budget(geglu, gate, G) + GELU_SLOPE * eg) + G.abs() * ev + ev * GELU_SLOPE * eg + 4 * U * v.abs()
    if residual is not None:
        r = residual.double()
        e = e + 4 * U * (v.abs() + r.abs())
        v = v + r
    if blend is not None:
        al = f32(alpha)
        bl, v1 = al * blend.double(), (1.0 - al) * v
        e = abs(1.0 - al) * e + 4 * U * (bl.abs() + v1.abs())
        v = bl + v1
    return Bound(v, e)


def conv3x3_formed_err(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, silu: bool, dtype):
    """tt_conv3x3 forms its operand act = silu?(x * scale + shift) in fp32 (one fma; silu_f = t / (1 + __expf(-t))) and rounds it to
    `dtype` before the MFMA.  x [nimg, C, h, w] (stored values), scale / shift [nimg, C].  Returns (exact act in fp64, per-element
    budget): u_s |act| for the rounding; the fma's u |t| through |silu'| <= 1.1; the SiLU itself 8u |act| (division, 1 + e, exp2)
    plus u |t| |act| (the argument of exp2 is -t log2 e, rounded: a relative u |t| on exp(-t))."""
    x = x.double()
    t = x * scale.double()[:, :, None, None] + shift.double()[:, :, None, None]
    act = t * torch.sigmoid(t) if silu else t
    err = UNIT[dtype] * act.abs() + 1.1 * U * t.abs()
    if silu:
        err = err + (8 * U + U * t.abs()) * act.abs()
    return act, err


def check(got: torch.Tensor, b: Bound, dtype, what: str = "") -> float:
    """max over the elements of |got - ref| / limit; raises with the worst element (index, got, ref, bound, ratio) if it exceeds 1.
    Non-finite outputs fail."""
    us = UNIT[dtype]
    ref = b.ref
    g = got.to(ref.device).double()
    lim = us * ref.abs() + (1 + us) * b.err + ABS_FLOOR.get(dtype, 0.0)
    err = (g - ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / lim)
    flat = int(torch.argmax(ratio.reshape(-1)))
    worst = float(ratio.reshape(-1)[flat])
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    print(f"[error bound] {what}: max err/bound = {worst:.3g} at {idx}")
    if not worst <= 1.0:
        raise AssertionError(f"{what}: element {idx} breaks its error bound: got {float(g[idx]):.9g}, ref {float(ref[idx]):.9g}, "
                             f"|err| {float(err[idx]):.3g} > bound {float(lim[idx]):.3g} (ratio {worst:.3g})")
    return worst


def ratio(got: torch.Tensor, b: Bound, dtype) -> float:
    """check()'s figure without the assertion: max over the elements of |got - ref| / limit (inf for a non-finite output) -- for tests that
    record every case of a sweep before they assert"""
    us = UNIT[dtype]
    g = got.to(b.ref.device).double()
    lim = us * b.ref.abs() + (1 + us) * b.err + ABS_FLOOR.get(dtype, 0.0)
    err = (g - b.ref).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, math.inf))
    return float(torch.where(err == 0, torch.zeros_like(err), err / lim).max())


# ---- operands whose magnitudes span decades

def col_exponents(n: int) -> torch.Tensor:
    """e_j cycling over -9 .. 3: output column j gets the scale 2^e_j"""
    return torch.tensor([-9 + j % 13 for j in range(n)], dtype=torch.float64)


def row_exponents(m: int) -> torch.Tensor:
    """f_i cycling over -3 .. 3: A row i gets the scale 2^f_i"""
    return torch.tensor([-3 + i % 7 for i in range(m)], dtype=torch.float64)


def decade_operands(m: int, n: int, k: int, dtype, seed: int):
    """A [m, k] with row i scaled by 2^f_i, W [n, k] (randn * k^-1/2) with row j scaled by 2^e_j, and the column scales 2^e_j [n]
    for the epilogue terms (bias, row vector, residual, blend get the same scale per column: a small column is small in every
    term)."""
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(m, k, generator=g, dtype=torch.float64) * torch.exp2(row_exponents(m))[:, None]).to(dtype)
    cs = torch.exp2(col_exponents(n))
    w = (torch.randn(n, k, generator=g, dtype=torch.float64) * k ** -0.5 * cs[:, None]).to(dtype)
    return a, w, cs


def scaled(shape, cs: torch.Tensor, dtype, seed: int) -> torch.Tensor:
    """randn of `shape` with the last dim scaled by the column scales cs"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * cs).to(dtype)


# ---- GroupNorm / LayerNorm: reference and budget

GN_GROUPS = 32
RHO_GRID = (0, 5, 50, 300)         # |group mean| / group spread: the ratios of the fused-LayerNorm analysis in gemm_kernel.h and of its test
GN_GUARD_RATIO, GN_GUARD_RATIO_TILES = 64.0, 4.0      # the conditioning guard of norm.hip -- keep in step
GUARD_MARGIN = 1.0 + 2.0 ** -8
SECOND_ORDER = 1.0 + 2.0 ** -10    # the budgets below are first order in u; the products of two roundings they drop are < 2^-20 of them


def _activate(t: torch.Tensor, e_t: torch.Tensor, silu: bool):
    """y = silu?(t) and its fp32 budget from the budget e_t of t: through |silu'| <= 1.1, plus silu_f's own 8u |y| (division, 1 + e,
    exp2) and u |t| |y| (the rounded argument of exp2) -- the figures conv3x3_formed_err states"""
    if not silu:
        return t, e_t
    y = t * torch.sigmoid(t)
    return y, 1.1 * e_t + (8 * U + U * t.abs()) * y.abs()


def groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, *, seg_rows: int, silu: bool,
              n_adds: int = 0, guard: float = math.inf, groups: int = GN_GROUPS) -> Bound:
    """GroupNorm of the token-major tensor x [nseg * seg_rows, C] (STORED values; two sources already concatenated), statistics per
    (segment of seg_rows rows, group of C / groups channels) -- one image, or the frames x hw rows of one video.

    Reference (fp64): the exact population mean mu and variance s2 of each (segment, group), r = 1 / sqrt(s2 + eps) with eps the fp32
    number the kernel receives, t = (x - mu) r gamma + beta, y = silu?(t).

    Budget, from the arithmetic norm.hip and gemm_kernel.h state for EVERY GroupNorm route ("statistics in fp32 with fp64 block / group
    combination", then s_mean = (float)mean, s_rstd = (float)(1 / sqrt(var + eps)), sc = s_rstd * gamma, sh = beta - s_mean * sc,
    t = fmaf(x, sc, sh)): the fp64 statistics are taken as exact, so mu and r each carry ONE fp32 rounding, |d| <= u = 2^-24:
        mu^ = mu (1 + d1),  r^ = r (1 + d2)
        sc  = fl(r^ gamma)      = r gamma (1 + d2)(1 + d3)
        m   = fl(mu^ sc)        = mu r gamma (1 + d1)(1 + d2)(1 + d3)(1 + d4)
        sh  = fl(beta - m)      = (beta - m)(1 + d5)            (an fma here drops d4: covered)
        t^  = fl(x sc + sh)     = (x sc + sh)(1 + d6)
    With P = |x r gamma| and M = |mu r gamma|, to first order:  |x sc - x r gamma| <= 2u P,  |m - mu r gamma| <= 4u M,
    |sh - (beta - mu r gamma)| <= 4u M + u (|beta| + M),  and the last rounding adds u |t|:
        |t^ - t| <= u (2 P + 5 M + |beta| + |t|)
    Linear in rho = |mu| / sigma (M <= rho |gamma|), never quadratic: a kernel whose variance loses digits to E[x^2] - mean^2 in fp32
    -- an error of order u rho^2 -- is outside it by construction.  Through SiLU: _activate().  check() adds the half ulp of the
    storage type at |y|.

    n_adds and guard, the one term beyond "mu correct to one fp32 rounding".  The lowest level of every route's sums but one IS fp32 -- a
    thread's running sum over its n_adds rows in the statistics-pass kernels, a producer's chain over the n_adds rows of a tile -- and a
    sum of values x_i formed that way is off by up to n_adds u sum |x_i| (the fp64 levels above add nothing), so the mean such sums give is
        |mean^ - mu| <= n_adds u A,   A = the group's mean |x|,   which enters t as   n_adds u A r |gamma|
    That holds ONLY for a group whose statistics the kernel takes from those sums: one below the conditioning guard of norm.hip,
    E[x^2] <= guard x var (guard = GN_GUARD_RATIO for the statistics-pass kernels, GN_GUARD_RATIO_TILES for tt_groupnorm_tiles).  Above
    the guard the kernel recomputes the group centred, in fp64, and its mean carries the one rounding again: no term.  So A <= sqrt(guard)
    sigma wherever the term applies -- it cannot grow with rho, and at rho = 50 or 300 the budget is the one above, unchanged.  The
    reference decides from its own exact E[x^2] / var, widened by GUARD_MARGIN (the kernel's ratio comes from the fp32 sums, off by up to
    2 n_adds u E[x^2] / var <= 2^-9 of itself at 256 additions and guard 64; a group that close to the guard may be on either side).
    n_adds = 0: fp64 from the first addition (splitk_epilogue_gn_kernel).  The SAME sums cost the variance n_adds u (s2 + mu^2): that is
    the rho^2 term, and it stays out."""
    x = x.double()
    rows, c = x.shape
    cpg, nseg = c // groups, rows // seg_rows
    assert c % groups == 0 and rows % seg_rows == 0, (rows, c, seg_rows)
    xg = x.view(nseg, seg_rows, groups, cpg)
    mu = xg.mean((1, 3), keepdim=True)
    s2 = (xg - mu).square().mean((1, 3), keepdim=True)
    r = (s2 + f32(eps)).rsqrt()
    g, b = gamma.double().to(x.device).view(1, 1, groups, cpg), beta.double().to(x.device).view(1, 1, groups, cpg)
    t = (xg - mu) * r * g + b
    from_fp32_sums = (s2 + mu * mu) <= guard * GUARD_MARGIN * s2              # (never true for a constant group: s2 = 0 < E[x^2])
    a_mean = torch.where(from_fp32_sums, xg.abs().mean((1, 3), keepdim=True), torch.zeros_like(s2))
    e = U * SECOND_ORDER * (2 * (xg * r * g).abs() + 5 * (mu * r * g).abs() + b.abs() + t.abs() + n_adds * a_mean * r * g.abs())
    y, e = _activate(t, e, silu)
    return Bound(y.reshape(rows, c), e.reshape(rows, c))


def layernorm(x: torch.Tensor, gamma, beta, eps: float, *, n_adds: int, pivot=None) -> Bound:
    """LayerNorm of every row of x [rows, n] (STORED values) in the CENTRED form ln_kernel (norm.hip) and ln_block_kernel (image.hip; one
    "row" = one [rows, c] block, gamma = beta = None) run:  mean = sum / n,  d = x - mean,  var = sum d^2 / n,
    rstd = 1 / sqrt(var + eps),  y = d rstd gamma + beta, all in fp32.

    n_adds: the fp32 additions on the longest path of the kernel's sums (ln_kernel: 8 values per 8-channel vector, ceil(n / 512)
    vectors per lane, then 6 xor-shuffle levels -- ln_adds(); ln_block_kernel: 8 ceil(n / 2048) per thread plus the subtraction of the
    pivot, fp64 across threads -- ln_block_adds()).  pivot [rows] or None: ln_block_kernel sums x - pivot (the block's first element).
    With A = mean |x - pivot| (pivot 0 for ln_kernel), mu the exact mean, d = x - mu, s2 = mean d^2, r = 1 / sqrt(s2 + eps):
        dm   = n_adds u A + u |mu|                       |mean^ - mu|: the sum, then the division (or the fp64 -> fp32 conversion)
        d^   = fl(x - mean^):  |d^ - d| <= dm + u |d|
        sum d^^2 - sum d^2 = n dm'^2 - 2 dm' sum d + O(u) sum d^2 and sum d = 0 EXACTLY: the error of the mean enters the variance
                              only squared -- the centred form has no cancellation, which is why this budget is tighter than the
                              GroupNorm one wherever the mean is large: its var term is u s2, not u (s2 + mu^2)
        dvar = (n_adds + 3) u (s2 + dm^2) + dm^2         2u for d^^2, n_adds u for the chain, u for the division
        rel  = (dvar + u (s2 + eps)) / (2 (s2 + eps)) + 2u       relative error of rstd (the addition rounds; rsqrt is faithful), as ln_rstd
        |y^ - y| <= (dm + u |d|) r |gamma| + |d r gamma| (rel + 2u) + u |y|        two products and the final addition (or one fma)
    """
    x = x.double()
    n = x.shape[1]
    p = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device) if pivot is None else pivot.double().to(x.device)
    mu = x.mean(1, keepdim=True)
    d = x - mu
    s2 = d.square().mean(1, keepdim=True)
    e32 = f32(eps)
    r = (s2 + e32).rsqrt()
    g = torch.ones(n, dtype=torch.float64, device=x.device) if gamma is None else gamma.double().to(x.device)
    b = torch.zeros(n, dtype=torch.float64, device=x.device) if beta is None else beta.double().to(x.device)
    dm = n_adds * U * (x - p[:, None]).abs().mean(1, keepdim=True) + U * mu.abs()
    dvar = (n_adds + 3) * U * (s2 + dm * dm) + dm * dm
    rel = (dvar + U * (s2 + e32)) / (2 * (s2 + e32)) + 2 * U
    drg = (d * r * g).abs()
    y = d * r * g + b
    e = SECOND_ORDER * ((dm + U * d.abs()) * r * g.abs() + drg * (rel + 2 * U) + U * y.abs())
    return Bound(y, e)


def ln_adds(n: int) -> int:
    """ln_kernel: a lane adds the 8 values of each of its ceil(n / 512) vectors in turn, then 6 xor-shuffle levels"""
    return 8 * ((n // 8 + 63) // 64) + 6


def ln_block_adds(rows: int, n: int) -> int:
    """ln_block_kernel: thread t adds the 8 values of vectors t, t + 256, .. of the block (fp32), each after subtracting the pivot (one
    more rounding per value, counted once on the path); the 256 threads then meet in fp64"""
    return 8 * ((rows * (n // 8) + 255) // 256) + 1


def tile_sums(x: torch.Tensor, tile_rows: int, n_adds=None) -> Bound:
    """the producers' GroupNorm tile sums (TtGemmArgs.stats_out): [rows / R, 2, C] = per tile of R rows and per column the sum and the
    sum of squares of the STORED output.  Summation orders, from the producers' comments: colstat_strip (gemm_kernel.h; the tiled
    template and both 320-wide kernels) adds the 32 rows of a strip one after the other from 0, a wave chains its fragment rows
    (read-add-store), w3_stats_tile / the tiled template's tile step chain the waves of a tile column; splitk_epilogue_stats_kernel gives
    row r to lane r % 32 and then adds the 32 lanes in order.  Every one of them is a fixed tree over the R values of a column, so no
    value passes more than R - 1 additions (the fully sequential chain), and for ANY order of n_adds roundings on the longest path
        |S^ - S| <= n_adds u sum |x|,      |Q^ - Q| <= n_adds u sum x^2      (x^2 enters through an fma: no rounding of its own)
    n_adds defaults to R (R - 1 additions and the store).  check(..., torch.float32) adds the last half ulp."""
    x = x.double()
    rows, c = x.shape
    n_adds = tile_rows if n_adds is None else n_adds
    xt = x.view(rows // tile_rows, tile_rows, c)
    ref = torch.stack([xt.sum(1), xt.square().sum(1)], 1)
    err = n_adds * U * SECOND_ORDER * torch.stack([xt.abs().sum(1), xt.square().sum(1)], 1)
    return Bound(ref, err)


# ---- normalisation inputs: per (segment, group) mean and spread, the mean rho spreads away from zero

CONST_FACTOR = math.pi / 3
CONST_GROUP, TINY_GROUP = 5, 11     # group 5 of every segment is constant; group 11 has spread 2^-9 (spread^2 = 3.8e-6, eps = 1e-5)


def norm_input(nseg: int, seg_rows: int, c: int, rho: float, dtype, seed: int, device="cpu", groups: int = GN_GROUPS) -> torch.Tensor:
    """x [nseg * seg_rows, c] = spread * randn + mean per (segment s, group g), rounded to `dtype`: spread 2^((g + 3 s) % 7 - 3) (2^-3 .. 2^3;
    consecutive segments and consecutive groups differ), mean = (-1)^g rho spread.  Group CONST_GROUP is constant, at
    (-1)^g max(rho, 1) spread (pi / 3) (1 + s / 7) (full fp32 mantissas, another one in every segment: their fp32 squares and sums round), group TINY_GROUP has spread 2^-9."""
    cpg = c // groups
    gen = torch.Generator(device=device).manual_seed(seed)
    z = torch.randn(nseg, seg_rows, groups, cpg, generator=gen, dtype=torch.float64, device=device)
    s = torch.arange(nseg, device=device)[:, None]
    k = torch.arange(groups, device=device)[None, :]
    spread = torch.exp2(((k + 3 * s) % 7 - 3).double())
    sign = 1.0 - 2.0 * (k % 2).double()
    mean = sign * rho * spread
    tiny, const = (k == TINY_GROUP).expand_as(spread), (k == CONST_GROUP).expand_as(spread)
    mean = torch.where(tiny, sign * rho * 2.0 ** -9, mean)
    mean = torch.where(const, sign * max(rho, 1.0) * spread * CONST_FACTOR * (1.0 + s.double() / 7.0), mean)
    spread = torch.where(tiny, torch.full_like(spread, 2.0 ** -9), spread)
    spread = torch.where(const, torch.zeros_like(spread), spread)
    x = z * spread[:, None, :, None] + mean[:, None, :, None]
    return x.reshape(nseg * seg_rows, c).to(dtype)


def norm_affine(c: int, seed: int):
    """gamma, beta (fp32 [c]) with magnitudes cycled like col_exponents: gamma_j = +-2^e_j (1 + randn / 4), beta_j = 2^e_(j+4) randn"""
    gen = torch.Generator().manual_seed(seed)
    e = col_exponents(c)
    sign = 1.0 - 2.0 * ((torch.arange(c) % 5) == 3).double()
    gamma = sign * torch.exp2(e) * (1.0 + 0.25 * torch.randn(c, generator=gen, dtype=torch.float64))
    beta = torch.exp2(col_exponents(c + 4)[4:]) * torch.randn(c, generator=gen, dtype=torch.float64)
    return gamma.float(), beta.float()


def ln_input(rows: int, n: int, rho: float, dtype, seed: int) -> torch.Tensor:
    """LayerNorm rows: row i = 2^f_i randn + (-1)^i rho 2^f_i (f_i over -3 .. 3); row CONST_GROUP is constant (as in norm_input), row
    TINY_GROUP has spread 2^-9"""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, n, generator=gen, dtype=torch.float64)
    i = torch.arange(rows)
    spread = torch.exp2(row_exponents(rows))
    sign = 1.0 - 2.0 * (i % 2).double()
    mean = sign * rho * spread
    mean = torch.where(i == TINY_GROUP, sign * rho * 2.0 ** -9, mean)
    mean = torch.where(i == CONST_GROUP, sign * max(rho, 1.0) * spread * CONST_FACTOR * (8.0 / 7.0), mean)
    spread = torch.where(i == TINY_GROUP, torch.full_like(spread, 2.0 ** -9), spread)
    spread = torch.where(i == CONST_GROUP, torch.zeros_like(spread), spread)
    return (z * spread[:, None] + mean[:, None]).to(dtype)
