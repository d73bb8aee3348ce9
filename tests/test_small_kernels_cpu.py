"""CPU: the case tables of tests/small_kernels.py have teeth.  Every small kernel of csrc/elementwise.hip is emulated in plain torch fp32
-- the documented arithmetic in the kernel's order of operations, the kernel's geometry (tiles, quads, lanes, grid passes) where a slip
in it would show, rounding through .to(dtype) -- behind the signatures of this_and_that_vdm_amd.ops.  The correct emulation must pass
every case (its worst err / bound is printed and must stay below 1); every named wrong variant must fail at least one case, and a variant
that is a slip at a geometry edge must be caught by the cases that exist for that edge and by no other.  Mirrors
tests/test_error_bounds_cpu.py."""
import math

import pytest
import torch

from tests import small_kernels as sk

F32 = torch.float32
NAN = float("nan")


def f32c(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=F32)


def gelu_erf32(x):
    """gelu_erf_f (common.h), the constants as written there"""
    x = x.float()
    t = 1.0 / (x.abs() * (0.3275911 * 0.70710678118654752) + 1.0)
    p = t * (0.5 * 1.061405429) + (0.5 * -1.453152027)
    p = p * t + 0.5 * 1.421413741
    p = p * t + 0.5 * -0.284496736
    p = p * t + 0.5 * 0.254829592
    u = p * t * torch.exp2(x * x * -0.72134752044448170)
    return x * torch.where(x >= 0, 1.0 - u, u)


def silu32(x):
    return x / (1.0 + torch.exp(-x))


class Emu:
    """the kernels of elementwise.hip in torch fp32; `variant` names ONE deliberate slip (None: the correct kernel)"""

    def __init__(self, variant=None):
        self.v = variant

    # ---- storage
    def store(self, x, dtype):
        x = x.float()
        if dtype == F32:
            return x
        y = x.to(dtype)
        if self.v == "truncating_store":                 # round towards zero: step back wherever nearest-even went away from zero
            over = (y.float().abs() > x.abs()) & torch.isfinite(y.float())
            y = torch.where(over, (y.view(torch.int16) - 1).view(dtype), y)
        return y

    def first_pass(self, total: int, blocks: int):
        """which of `total` grid-stride items are served: all of them, or (the slip) those of the first pass of the grid only"""
        m = torch.ones(total, dtype=torch.bool)
        if self.v == "first_pass_only":
            m[blocks * sk.BLOCK:] = False
        return m

    # ---- transposes
    def tile_mask(self, n, c, hw):
        """[n, hw, c]: the elements a 32 x 32 tile's store guard lets through"""
        if self.v != "tile_swapped_edge":
            return torch.ones(n, hw, c, dtype=torch.bool)
        p, cc = torch.arange(hw)[:, None], torch.arange(c)[None, :]
        p0, c0 = p // 32 * 32, cc // 32 * 32
        return (((c0 + (p - p0)) < c) & ((p0 + (cc - c0)) < hw))[None].expand(n, hw, c)

    def nchw_to_tokens(self, src, dtype, ld=None, out=None):
        n, c, h, w = src.shape
        val = self.store(src.float().permute(0, 2, 3, 1).reshape(n * h * w, c), dtype)
        if out is None:
            out = torch.full((n * h * w, c), NAN, dtype=dtype)
        out.copy_(torch.where(self.tile_mask(n, c, h * w).reshape(n * h * w, c), val, out))
        return out

    def tokens_to_nchw(self, src, n, c, h, w, out_dtype):
        hw = h * w
        val = self.store(src.float().view(n, hw, c), out_dtype)
        val = torch.where(self.tile_mask(n, c, hw), val, torch.full_like(val, NAN))
        return val.permute(0, 2, 1).reshape(n, c, h, w).contiguous()

    # ---- elementwise
    def add_scaled(self, a, b, scale=1.0, out=None):
        n = a.numel()
        val = self.store((a.double() + float(f32c(scale)) * b.double()).float(), a.dtype)       # one fma: the fp64 sum of the exact product, rounded
        if out is None:
            out = torch.full_like(a, NAN)
        m = self.first_pass(n // 8, 4096).repeat_interleave(8)
        out.copy_(torch.where(m.view(a.shape), val, out))
        return out

    def add_rowvec(self, x, rowvec, rows_per_vec, nvec, out=None):
        rows, c = x.shape
        r = torch.arange(rows)
        idx = r % nvec if self.v == "row_mod_nvec" else (r // rows_per_vec) % nvec
        val = self.store(x.float() + rowvec[idx], x.dtype)
        if out is None:
            out = torch.full((rows, c), NAN, dtype=x.dtype)
        m = self.first_pass(rows * c // 8, 4096).repeat_interleave(8).view(rows, c)
        out.copy_(torch.where(m, val, out))
        return out

    def act_rows(self, x, act="gelu", out=None):
        f = x.float()
        if act == "gelu":
            y = gelu_erf32(f)
        else:
            t = f32c(-1.702) * f
            y = f / (1.0 + torch.exp(t))
            if self.v != "quick_gelu_overflow":          # beyond t = 80 the quotient is x e^-t to 1e-35 relative: two half-size factors stay finite
                hh = torch.exp(t * -0.5)
                y = torch.where(t > 80.0, f * hh * hh, y)
        val = self.store(y, x.dtype)
        if out is None:
            return val
        out.copy_(val)
        return out

    # ---- softmax_rows: one wave per row; lane l holds the quads at columns 4 l + 256 p
    def softmax_rows(self, x, dtype, cols=None, out=None):
        rows = x.shape[0]
        cols = x.shape[1] if cols is None else cols
        npass = (cols + 255) // 256
        q = (cols + 3) // 4 * 4                          # the last quad is read whole: its tail holds whatever lies behind the row
        raw = torch.full((rows, npass * 256), -math.inf, dtype=F32)
        raw[:, :q] = torch.as_strided(x, (rows, q), (x.stride(0), 1))
        live = (torch.arange(npass * 256) < cols)[None, :]
        read = (torch.arange(npass * 256) < q)[None, :]
        mx_in = raw if self.v == "max_unmasked" else torch.where(live, raw, f32c(-math.inf))
        mx = torch.where(torch.isnan(mx_in), f32c(-math.inf), mx_in).amax(1, keepdim=True)      # fmaxf drops a NaN
        if self.v == "no_max_subtraction":
            mx = torch.zeros_like(mx)
        e = torch.exp(raw - mx)
        counted = read if self.v == "sum_unmasked" else live
        if self.v == "partial_quad_dropped":
            counted = live & (torch.arange(npass * 256) < cols // 4 * 4)[None, :]
        terms = torch.where(counted, e, f32c(0.0)).view(rows, npass, 64, 4).permute(0, 2, 1, 3).reshape(rows, 64, npass * 4)
        s = torch.zeros(rows, 64, dtype=F32)
        for i in range(npass * 4):                       # the lane's serial sum, then the xor-shuffle tree
            s = s + terms[:, :, i]
        for o in (32, 16, 8, 4, 2, 1):
            s = s[:, :o] + s[:, o:2 * o]
        inv = 1.0 / s
        y = torch.where(live, e * inv, f32c(0.0))
        cols_pad = out.shape[1]
        val = torch.zeros(rows, cols_pad, dtype=F32)
        val[:, :cols] = y[:, :cols]
        out.copy_(self.store(val, dtype))
        return out

    # ---- small_linear: one wave per column; lane l runs an fma chain over the 8-vectors l, l + 64, ..; rows staged four at a time
    def small_linear(self, x, w, bias=None, act_in=False, act_out=False, out=None, accumulate=False):
        rows, k = x.shape
        n = w.shape[0]
        xs = x.float()
        if act_in and self.v != "act_in_on_product":
            xs = silu32(xs)
        if self.v == "stale_rows":                       # every chunk of four rows is served from the first chunk's staging
            xs = xs[torch.arange(rows) % 4 % rows]
        wf = w.float()
        kv = k // 8
        npass = 1 if self.v == "k_tail_dropped" else (kv + 63) // 64
        acc = torch.zeros(rows, n, 64, dtype=F32)
        for p in range(npass):
            lanes = min(64, kv - p * 64)
            for e in range(8):
                col = (p * 64 + torch.arange(lanes)) * 8 + e
                prod = xs[:, None, col] * wf[None, :, col]
                if act_in and self.v == "act_in_on_product":
                    prod = silu32(prod)
                acc[:, :, :lanes] += prod
        s = acc
        for o in (32, 16, 8, 4, 2, 1):
            s = s[..., :o] + s[..., o:2 * o]
        s = s[..., 0]
        if bias is not None:
            s = s + bias[None, :]
        if act_out:
            s = silu32(s)
        if accumulate:
            s = out + s
            if bias is not None and self.v == "bias_twice_on_accumulate":
                s = s + bias[None, :]
        if out is None:
            out = torch.full((rows, n), NAN, dtype=F32)
        served = torch.ones(n, dtype=torch.bool)
        if self.v == "first_pass_only":
            served[1024 * 4:] = False                    # the column loop does not wrap its 1024-block grid
        out.copy_(torch.where(served[None, :], s, out))
        return out

    # ---- timestep_embedding
    def timestep_embedding(self, t, dim):
        half = dim // 2
        den = half - 1 if self.v == "half_minus_one" else half
        freq = torch.exp(f32c(-9.210340371976184) * torch.arange(half, dtype=F32) / f32c(float(max(den, 1))))
        arg = t[:, None] * freq[None, :]
        parts = [torch.sin(arg), torch.cos(arg)] if self.v == "sin_cos_swapped" else [torch.cos(arg), torch.sin(arg)]
        return torch.cat(parts, 1)

    # ---- the single-request loop glue
    def prep_model_input(self, latents, image_latents, cond, sigmas, step, batch, frames, h, w, cpad, dtype):
        sg = sigmas[step]
        c_in = 1.0 / torch.sqrt(sg * sg + 1.0)
        tok = lambda t: t.permute(0, 1, 3, 4, 2)
        x = torch.zeros(batch, frames, h, w, cpad, dtype=F32)
        x[..., 0:4] = tok(latents.view(1, frames, 4, h, w)) * c_in
        x[..., 4:8] = tok(image_latents.view(batch, frames, 4, h, w))
        if cond is not None:
            x[..., 8:12] = tok(cond.view(1, frames, 4, h, w))
        val = self.store(x.view(-1, cpad), dtype)
        m = self.first_pass(val.shape[0], 2048)[:, None]
        return torch.where(m, val, torch.full_like(val, NAN))

    def cfg_euler_step(self, eps, latents, guidance, sigmas, step, batch, frames, h, w, image_guidance_scale=None):
        sg = sigmas[step]
        sn = sigmas[step] if self.v == "sigma_next_is_sigma" else sigmas[step + 1]
        c_out, c_skip = -sg / torch.sqrt(sg * sg + 1.0), 1.0 / (sg * sg + 1.0)
        e = eps[:, :4].reshape(batch, frames, h, w, 4).permute(0, 1, 4, 2, 3)
        g = torch.ones(frames) if guidance is None else guidance
        g = g.view(frames, 1, 1, 1)
        if batch == 3:
            e1, cd, u = e[0], e[1], e[2]
            if self.v == "cond_uncond_swapped":
                cd, u = u, cd
            v = u + g * (cd - u) + f32c(image_guidance_scale) * (cd - e1)
        elif batch == 2:
            u, cd = e[0], e[1]
            v = u + g * (cd - u)
        else:
            v = e[0]
        xv = latents.view(frames, 4, h, w)
        x0 = v * c_out + xv * c_skip
        new = xv + (xv - x0) / sg * (sn - sg)
        m = self.first_pass(frames * h * w, 2048).view(frames, 1, h, w)
        xv.copy_(torch.where(m, new, xv))
        return latents

    # ---- the CLIP plumbing
    def patch_tokens(self, src, patch, dtype, kpad=None):
        n, c, h, w = src.shape
        p, gh, gw = patch, h // patch, w // patch
        kk = c * p * p
        kpad = (kk + 7) // 8 * 8 if kpad is None else kpad
        patches = src.float().view(n, c, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(n, gh, gw, kk)
        t = torch.arange(n * gh * gw)
        img, r = t // (gw * gh), t % (gw * gh)
        if self.v == "gw_gh_swapped":
            px, py = r % gh % gw, (r // gh) % gw % gh    # (kept inside the image)
        else:
            px, py = r % gw, r // gw
        out = torch.zeros(n * gh * gw, kpad, dtype=F32)
        out[:, :kk] = patches[img, py, px]
        return self.store(out, dtype)

    def embed_rows(self, table, pos, *, ids=None, cls=None, l, out=None):
        if ids is not None:
            rows = ids.numel()
            inside = (ids >= 0) & (ids < table.shape[0])
            a = table[ids.clamp(0, table.shape[0] - 1)].float()
            if self.v != "ids_clamped":
                a = torch.where(inside[:, None], a, f32c(0.0))
        else:
            nimg = table.shape[0] // (l - 1)
            rows = nimg * l
            a = torch.cat([cls.float()[None, None].expand(nimg, 1, -1), table.float().view(nimg, l - 1, -1)], 1).reshape(rows, -1)
        out.copy_(self.store(a + pos.float()[torch.arange(rows) % l], table.dtype))
        return out


def sweep(kernel, impl, dtype):
    """(case, ratio or None when the case failed) for every case of the kernel"""
    out = []
    for case in sk.all_cases(kernel, dtype):
        try:
            out.append((case, sk.run(kernel, impl, case, dtype)))
        except AssertionError:
            out.append((case, None))
    return out


@pytest.mark.parametrize("dtype", sk.DTYPES, ids=sk.name_of)
@pytest.mark.parametrize("kernel", list(sk.KERNELS))
def test_the_correct_emulation_passes_every_case(kernel, dtype):
    cases = sk.all_cases(kernel, dtype)
    if not cases:
        return                                           # (a kernel without a storage type runs once, under fp32)
    worst = 0.0
    for case in cases:
        worst = max(worst, sk.run(kernel, Emu(), case, dtype))
    print(f"[small kernels] {kernel} {sk.name_of(dtype)}: {len(cases)} cases, worst err/bound of the correct emulation = {worst:.3g}")
    assert worst < 1.0


# variant -> (kernels, storage types, the predicate of the cases meant to catch it, how strictly: True -- every one of them catches it and
# every other case still passes; "some" -- at least one of them and no other case; False -- at least one of them)
B16, H16 = torch.bfloat16, torch.float16
edge = lambda *names: (lambda c: c["edge"] in names)
VARIANTS = {
    "truncating_store": (["nchw_to_tokens", "tokens_to_nchw", "add_scaled", "add_rowvec", "prep_model_input", "softmax_rows", "act_rows"],
                         [B16, H16], lambda c: True, False),
    "max_unmasked": (["softmax_rows"], [B16], lambda c: c["quad"] == "partial", True),
    "sum_unmasked": (["softmax_rows"], [B16], lambda c: c["quad"] == "partial", True),
    "partial_quad_dropped": (["softmax_rows"], [B16], lambda c: c["quad"] == "partial", "some"),   # (a ramp's last quad holds e^-200 = 0)
    "no_max_subtraction": (["softmax_rows"], [B16, F32], edge("offset"), False),
    "k_tail_dropped": (["small_linear"], [B16], lambda c: c["shape"][1] > 512, True),
    "stale_rows": (["small_linear"], [B16], lambda c: c["shape"][0] > 4, True),
    "bias_twice_on_accumulate": (["small_linear"], [B16], lambda c: c["flags"]["bias"] and c["flags"]["accumulate"], True),
    "act_in_on_product": (["small_linear"], [B16], lambda c: c["flags"]["act_in"], "some"),      # (a row of scale 1e-2: SiLU is linear there)
    "sin_cos_swapped": (["timestep_embedding"], [F32], lambda c: True, False),
    "half_minus_one": (["timestep_embedding"], [F32], lambda c: c["dim"] > 2, True),
    "tile_swapped_edge": (["nchw_to_tokens", "tokens_to_nchw"], [B16, F32], edge("ragged"), True),
    "row_mod_nvec": (["add_rowvec"], [B16], lambda c: c["shape"][3] > 1, True),
    "cond_uncond_swapped": (["cfg_euler_step"], [F32], edge("batch3"), True),
    "sigma_next_is_sigma": (["cfg_euler_step"], [F32], lambda c: True, False),
    "gw_gh_swapped": (["patch_tokens"], [B16, F32], edge("oblong"), True),
    "ids_clamped": (["embed_rows"], [B16], edge("ids"), True),
    "quick_gelu_overflow": (["act_rows"], [B16, F32], lambda c: c["act"] == "quick_gelu", True),
    "first_pass_only": (["add_scaled", "add_rowvec", "prep_model_input", "cfg_euler_step", "small_linear"], [B16, F32],
                        edge("wrap", "grid_wrap"), True),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_wrong_variant_is_caught_by_the_cases_of_its_edge(variant):
    kernels, dtypes, catches, exclusive = VARIANTS[variant]
    for kernel in kernels:
        for dtype in dtypes:
            res = sweep(kernel, Emu(variant), dtype)
            if not res:
                continue
            meant = [(c, r) for c, r in res if catches(c)]
            other = [(c, r) for c, r in res if not catches(c)]
            caught = [c["id"] for c, r in meant if r is None]
            print(f"[small kernels] {variant} in {kernel} {sk.name_of(dtype)}: caught by {len(caught)} of its {len(meant)} cases"
                  f" ({len(other)} other cases)")
            assert meant, (variant, kernel)
            assert caught, f"{variant} passes every case of {kernel} {sk.name_of(dtype)}"
            if exclusive is True:                        # a slip at an edge: every case of the edge catches it ...
                assert len(caught) == len(meant), [c["id"] for c, r in meant if r is not None]
            if exclusive:                                # ... and no other case does
                assert all(r is not None for _, r in other), [c["id"] for c, r in other if r is None]


def test_timestep_oracle_b():
    """TS_B is twice what the fp32 CPU oracle needs under the form A u |t f| + B u (A = TS_A) on the grid of the cases: measured here,
    printed, and held against the constant written in tests/small_kernels.py"""
    from oracle.leaves import get_timestep_embedding
    need = 0.0
    for case in sk.timestep_cases():
        t = sk.timestep_values(case["rows"])
        got = get_timestep_embedding(t, case["dim"], True, 0).double()
        b = sk.timestep_bound(t, case["dim"], b=0.0)
        # the form alone, without the storage term check() adds on top:  |err| <= A u |arg| + B u
        need = max(need, float(((got - b.ref).abs() - b.err).max()) / sk.U)
    print(f"[small kernels] timestep_embedding: the fp32 CPU oracle needs B = {need:.4f} with A = {sk.TS_A}; TS_B_ORACLE = {sk.TS_B_ORACLE}")
    assert need <= sk.TS_B_ORACLE <= need + 0.1 and sk.TS_B == 2 * sk.TS_B_ORACLE
