"""Per-element error bounds for the dense contractions of libttvdm (tt_gemm's routes, tt_conv3x3), derived beforehand from the operands
a kernel read and the arithmetic it is documented to do -- never fitted to measured errors.  A plain module (not a conftest): used by
tests/test_error_bounds_cpu.py (the bound against emulated correct and deliberately wrong kernels) and tests/test_error_bounds_gpu.py
(every GEMM route against it).

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
