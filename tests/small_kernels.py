"""Case tables, input builders, fp64 references and exact answers / per-element budgets for the small kernels of csrc/elementwise.hip.
A plain module (not a conftest), in the manner of tests/error_bounds.py, whose UNIT, U, Bound, check, ratio and gelu_budget it reuses.
Used by tests/test_small_kernels_cpu.py (fp32 emulations of the documented arithmetic, and deliberately wrong variants of them, run
through the same cases) and tests/test_small_kernels_gpu.py (this_and_that_vdm_amd.ops through the same cases).

run(kernel, impl, case, dtype, device) builds the case's inputs on the CPU, calls impl.<kernel>(...) -- `impl` has the signatures of
this_and_that_vdm_amd.ops -- and either compares bits (torch.equal) or applies error_bounds.check(); it returns the worst err / bound
(0.0 for a case that is exact) and raises AssertionError on a miss.  Every case carries an `edge`: the geometry edge or value family it
exists for (the CPU test asserts that a wrong variant is caught by the cases of its edge).

Budgets (u = 2^-24, the fp32 unit roundoff; check() adds the storage rounding u_s |ref| on top; FLOOR = 2^-126 is added to every
budget: a result below the smallest normal fp32 may flush to zero):

  nchw_to_tokens, tokens_to_nchw, patch_tokens, embed_rows   exact: the torch permutation / gather / one fp32 sum, then .to(dtype)
  add_scaled    y = fma(b, scale, a): exact wherever a + scale b is exact in fp32 (scale 1, -1, 0, 0.5 on operands of one binade, the
                ties); otherwise one rounding, u |ref|
  add_rowvec    one fp32 add: u |ref|
  softmax_rows  y_j = e_j / S, relative: e_j = __expf(d_j), d_j = x_j - max: the subtraction and the product d_j log2(e) inside __expf
                round (u |d_j| each, absolute on the argument = relative on e_j), v_exp_f32 2u:  r_j = (2 |d_j| + 2) u;
                S: every term carries its r_j, then one u per level of the sum (4 ceil(cols / 256) lane-serial terms, 6 shuffle levels):
                sum_j e_j r_j / S + L u;  the reciprocal and the product: 3u.   Padding and -inf entries: exactly 0.
  small_linear  depth u sum_k |act(x_k)| |w_k|, depth = 8 ceil(k / 512) + 6 + 1 (the lane's fma chain, the shuffle tree, the bias);
                act_in: + sum_k e_k |w_k|, e_k = (8u + u |x_k|) |silu(x_k)| (error_bounds.conv3x3_formed_err's SiLU term; x is exact);
                act_out: 1.1 e + (8u + u |s|) |silu(s)|;  accumulate: + u |y_old + s| for the last addition
  timestep_embedding   A u |t f_j| + B u, see TS_A / TS_B below
  prep_model_input     pass-through channels and the zero tail exact; latents * c_in, c_in = 1 / sqrtf(s s + 1): the square, the sum,
                the root, the division (<= 4u relative on c_in) and the product: 5u |ref|
  cfg_euler_step       first-order propagation through the kernel's statements, cfg_euler_bound()
  act_rows      gelu: gelu_budget("erf");  quick_gelu y = x / (1 + __expf(-t)) with the FORMED argument t = fl(1.702f x): the SiLU form's
                8u |y| + u |t| |y| for an exact t, plus the forming error u |t| of t through |dy/dt| = |y| (1 - sigmoid(t)) <= |y| -- the
                way error_bounds.conv3x3_formed_err carries the fma that forms silu_f's argument.  (In silu_f itself the argument is the
                operand, exact: one rounding of magnitude |t| in front of exp2; here there are two.)
"""
import functools
import itertools
import math

import torch

from tests.error_bounds import ABS_FLOOR, U, UNIT, Bound, check, gelu_budget, gelu_exact, ratio  # noqa: F401  (re-exported)

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
FLOOR = 2.0 ** -126
CANARY = 7.5
LEAD = 8                      # canary columns in front of a window: 16 bytes of a 16-bit type, 32 of fp32 (vector accesses stay aligned)
BLOCK = 256


def name_of(dtype) -> str:
    return {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[dtype]


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def window(rows: int, cols: int, dtype, dev, tail: int = 8):
    """a [rows, cols] column window of a wider buffer filled with CANARY; returns (buffer, window)"""
    buf = torch.full((rows, LEAD + cols + tail), CANARY, dtype=dtype, device=dev)
    return buf, buf[:, LEAD:LEAD + cols]


def canaries_untouched(buf: torch.Tensor, cols: int, what: str) -> None:
    b = buf.cpu()
    if not (bool((b[:, :LEAD] == CANARY).all()) and bool((b[:, LEAD + cols:] == CANARY).all())):
        raise AssertionError(f"{what}: a canary column beside the output window was overwritten")


def same(got: torch.Tensor, want: torch.Tensor, what: str) -> float:
    got = got.cpu()
    if got.dtype != want.dtype or got.shape != want.shape or not torch.equal(got, want):
        bad = (got != want) | (torch.isnan(got.float()) != torch.isnan(want.float())) if got.shape == want.shape else None
        n = int(bad.sum()) if bad is not None else -1
        first = tuple(int(i) for i in bad.nonzero()[0]) if n > 0 else ()
        raise AssertionError(f"{what}: {n} elements differ from the exact answer; first at {first}: got "
                             f"{float(got[first]) if n > 0 else '?'!r}, want {float(want[first]) if n > 0 else '?'!r}")
    return 0.0


def bounded(got: torch.Tensor, b: Bound, dtype, what: str) -> float:
    return check(got.cpu(), Bound(b.ref, b.err + FLOOR), dtype, what)


def silu_budget(t: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """silu_f / the quick-GELU quotient for an exact argument t: 8u |y| (division, 1 + e, exp2) + u |t| |y| (the rounded argument of exp2)"""
    return (8 * U + U * t.abs()) * y.abs()


# ================================================================ nchw_to_tokens / tokens_to_nchw (32 x 32 LDS tile, grid.z = images)
TRANSPOSE_SHAPES = [((1, 1, 1), "one"), ((2, 33, 31), "ragged"), ((3, 64, 64), "whole"), ((2, 40, 1025), "ragged")]


def special_values(src_dtype, dst_dtype) -> torch.Tensor:
    """exact rounding ties of the 16-bit destination (both parities, both signs), +-0, fp16 subnormals and their ties, the largest finite value"""
    v = []
    if dst_dtype != torch.float32:
        bits = 7 if dst_dtype == torch.bfloat16 else 10
        v += [s * (2 ** bits + m + 0.5) * 2.0 ** -bits for m in range(4) for s in (1.0, -1.0)]
    v += [0.0, -0.0, 2.0 ** -24, 3 * 2.0 ** -24, -(2.0 ** -20), 2.0 ** -25, 3 * 2.0 ** -25, -5 * 2.0 ** -25]
    big = min(torch.finfo(src_dtype).max, torch.finfo(dst_dtype).max)
    v += [big, -big]
    return torch.tensor(v, dtype=torch.float64)


def transpose_values(numel: int, src_dtype, dst_dtype, seed: int) -> torch.Tensor:
    x = torch.randn(numel, generator=gen(seed), dtype=torch.float64) * 4
    sp = special_values(src_dtype, dst_dtype)
    k = min(numel, sp.numel())
    pos = torch.linspace(0, numel - 1, k).long()
    x[pos] = sp[:k]
    return x.to(src_dtype)


def transpose_cases():
    out = []
    for (shape, edge), src, dst, layout in itertools.product(TRANSPOSE_SHAPES, ("f32", "st"), ("f32", "st"), ("plain", "window")):
        out.append(dict(id=f"{'x'.join(map(str, shape))}-{src}-{dst}-{layout}", shape=shape, src=src, dst=dst, layout=layout, edge=edge))
    return out


def run_nchw_to_tokens(impl, case, dtype, dev):
    """the destination is always the storage type `dtype`: the fp32 destinations are the cases of dtype = fp32 (applies())"""
    n, c, hw = case["shape"]
    src_dtype = torch.float32 if case["src"] == "f32" else dtype
    src = transpose_values(n * c * hw, src_dtype, dtype, 11).view(n, c, hw, 1)
    want = src.permute(0, 2, 3, 1).reshape(-1, c).to(dtype)
    what = f"nchw_to_tokens {case['id']} {name_of(dtype)}"
    if case["layout"] == "window":
        buf, view = window(n * hw, c, dtype, dev)
        impl.nchw_to_tokens(src.to(dev), dtype, out=view)
        canaries_untouched(buf, c, what)
        return same(view, want, what)
    return same(impl.nchw_to_tokens(src.to(dev), dtype), want, what)


def run_tokens_to_nchw(impl, case, dtype, dev):
    n, c, hw = case["shape"]
    src_dtype = torch.float32 if case["src"] == "f32" else dtype
    out_dtype = torch.float32 if case["dst"] == "f32" else dtype
    tok = transpose_values(n * hw * c, src_dtype, out_dtype, 12).view(n * hw, c)
    want = tok.view(n, hw, c).permute(0, 2, 1).reshape(n, c, hw, 1).to(out_dtype)
    if case["layout"] == "window":                      # ld_src > c
        buf, view = window(n * hw, c, src_dtype, dev)
        view.copy_(tok)
        tok_d = view
    else:
        tok_d = tok.to(dev)
    return same(impl.tokens_to_nchw(tok_d, n, c, hw, 1, out_dtype), want, f"tokens_to_nchw {case['id']} {name_of(dtype)}")


# ================================================================ add_scaled (8 elements per lane, 4096 blocks x 256 threads)
ADD_SCALED_WRAP = 8 * (4096 * BLOCK + 3)


def add_scaled_cases():
    out = []
    for n, edge in ((8, "one"), (8 * 257, "blocks"), (ADD_SCALED_WRAP, "wrap")):
        small = n != ADD_SCALED_WRAP
        kinds = ["one", "minus_one", "zero", "half", "tie", "budget"] if small else ["tie", "budget"]
        for kind in kinds:
            for place in (("new", "in_a", "in_b") if small else ("new",) if kind == "tie" else ("in_a",)):
                out.append(dict(id=f"{n}-{kind}-{place}", n=n, kind=kind, place=place, edge=edge))
    return out


@functools.lru_cache(maxsize=8)
def add_scaled_operands(n: int, kind: str, dtype):
    g = gen(n % 1000 + 17)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    a = (sign * (1.0 + torch.rand(n, generator=g, dtype=torch.float64))).to(dtype)          # one binade: [1, 2)
    if kind == "minus_one":
        return a, a.clone(), -1.0
    if kind == "tie":                                   # a + half an ulp of its binade: halfway between two storage values, both parities
        return a, (torch.sign(a.double()) * UNIT[dtype]).to(dtype), 1.0
    if kind == "budget":
        return a, (torch.randn(n, generator=g, dtype=torch.float64) * 3).to(dtype), 0.37
    b = (sign * (1.0 + torch.rand(n, generator=g, dtype=torch.float64))).to(dtype)
    return a, b, {"one": 1.0, "zero": 0.0, "half": 0.5}[kind]


def run_add_scaled(impl, case, dtype, dev):
    a, b, scale = add_scaled_operands(case["n"], case["kind"], dtype)
    what = f"add_scaled {case['id']} {name_of(dtype)}"
    ad, bd = a.to(dev).clone(), b.to(dev).clone()
    out = {"new": None, "in_a": ad, "in_b": bd}[case["place"]]
    got = impl.add_scaled(ad, bd, scale, out=out)
    s32 = float(torch.tensor(scale, dtype=torch.float32))
    ref = a.double() + s32 * b.double()
    if case["kind"] == "budget":
        return bounded(got, Bound(ref, U * ref.abs()), dtype, what)
    if case["kind"] == "minus_one":
        assert float(ref.abs().max()) == 0.0
    return same(got, ref.to(dtype), what)


# ================================================================ add_rowvec (8 elements per lane, 4096 blocks x 256 threads)
ADD_ROWVEC_SHAPES = [((1, 8, 1, 1), "one"), ((37 * 6 + 5, 328, 37, 3), "ragged"), ((3300, 2560, 7, 5), "wrap")]


def add_rowvec_cases():
    out = []
    for (shape, edge), layout in itertools.product(ADD_ROWVEC_SHAPES, ("plain", "strided", "in_place")):
        out.append(dict(id=f"{'x'.join(map(str, shape))}-{layout}", shape=shape, layout=layout, edge=edge))
    return out


@functools.lru_cache(maxsize=4)
def add_rowvec_operands(shape, dtype):
    rows, c, rpv, nvec = shape
    g = gen(rows + c)
    x = torch.randn(rows, c, generator=g, dtype=torch.float64).to(dtype)
    rv = (torch.randn(nvec, c, generator=g, dtype=torch.float64) * (10.0 ** torch.arange(nvec).double())[:, None]).float()   # rows differ by decades
    ref = x.double() + rv.double()[(torch.arange(rows) // rpv) % nvec]
    return x, rv, ref


def run_add_rowvec(impl, case, dtype, dev):
    rows, c, rpv, nvec = case["shape"]
    x, rv, ref = add_rowvec_operands(case["shape"], dtype)
    what = f"add_rowvec {case['id']} {name_of(dtype)}"
    b = Bound(ref, U * ref.abs())
    if case["layout"] == "plain":
        return bounded(impl.add_rowvec(x.to(dev), rv.to(dev), rpv, nvec), b, dtype, what)
    if case["layout"] == "in_place":
        xd = x.to(dev).clone()
        got = impl.add_rowvec(xd, rv.to(dev), rpv, nvec, out=xd)
        return bounded(got, b, dtype, what)
    xbuf, xv = window(rows, c, dtype, dev)              # strided x, strided out with canary columns, ld_rowvec > c
    xv.copy_(x)
    rbuf, rvv = window(nvec, c, torch.float32, dev)
    rvv.copy_(rv)
    obuf, ov = window(rows, c, dtype, dev, tail=16)
    impl.add_rowvec(xv, rvv, rpv, nvec, out=ov)
    canaries_untouched(obuf, c, what)
    return bounded(ov, b, dtype, what)


# ================================================================ softmax_rows (one wave per row, 4 rows per block, 256 columns per pass)
SOFTMAX_COLS = [1, 3, 5, 37, 255, 257, 301, 1030]
SOFTMAX_ROWS = [1, 5, 130]
SOFTMAX_FAMILIES = ["randn4", "equal", "dominant", "offset", "ramp", "neg_inf"]
IGNORED = [3e38, math.inf, math.nan]                   # what the columns cols .. ldx hold, in turn: a lone ignored column holds the finite one


def softmax_cases():
    out = []
    for cols, rows, fam in itertools.product(SOFTMAX_COLS, SOFTMAX_ROWS, SOFTMAX_FAMILIES):
        edge = {"offset": "offset", "neg_inf": "neg_inf"}.get(fam, "values")
        out.append(dict(id=f"{rows}x{cols}-{fam}", rows=rows, cols=cols, family=fam, quad="partial" if cols % 4 else "whole", edge=edge))
    return out


def softmax_scores(rows: int, cols: int, fam: str) -> torch.Tensor:
    g = gen(rows * 10007 + cols)
    z = torch.randn(rows, cols, generator=g, dtype=torch.float64)
    if fam == "randn4":
        x = z * 4
    elif fam == "equal":
        x = torch.full((rows, cols), 1.0, dtype=torch.float64) * torch.randn(rows, 1, generator=g, dtype=torch.float64)
    elif fam == "dominant":
        x = torch.zeros(rows, cols, dtype=torch.float64)
        x[torch.arange(rows), torch.randint(0, cols, (rows,), generator=g)] = 80.0
    elif fam == "offset":
        x = z + 1e4
    elif fam == "ramp":
        x = -200.0 * torch.arange(cols).double()[None, :].expand(rows, cols) / max(cols - 1, 1) + 0.0 * z
    else:
        x = z * 4
        x[:, 1::3] = -math.inf                          # (column 0 stays finite: a row of -inf alone has no softmax)
    return x.float()


def softmax_bound(x: torch.Tensor) -> Bound:
    """x fp32 [rows, cols] (the live columns)"""
    cols = x.shape[1]
    xd = x.double()
    d = xd - xd.amax(1, keepdim=True)
    e = d.exp()
    s = e.sum(1, keepdim=True)
    ad = torch.where(torch.isfinite(d), d.abs(), torch.zeros_like(d))          # an -inf entry is exactly 0: no error
    r = (2 * ad + 2) * U
    levels = 4 * ((cols + 255) // 256) + 6
    rel = r + (e * r).sum(1, keepdim=True) / s + (levels + 3) * U
    y = e / s
    return Bound(y, rel * y)


def run_softmax_rows(impl, case, dtype, dev):
    rows, cols = case["rows"], case["cols"]
    what = f"softmax_rows {case['id']} {name_of(dtype)}"
    x = softmax_scores(rows, cols, case["family"])
    cols_pad = (cols + 7) // 8 * 8 + (8 if rows == 5 else 0)
    ldx = cols_pad + 12
    xbuf = torch.tensor(IGNORED, dtype=torch.float32)[(torch.arange(ldx) - cols) % 3][None, :].repeat(rows, 1)
    xbuf[:, :cols] = x
    xd = xbuf.to(dev)
    obuf, ov = window(rows, cols_pad, dtype, dev)       # ldy > cols_pad, canaries on both sides
    impl.softmax_rows(xd[:, :cols_pad], dtype, cols=cols, out=ov)
    canaries_untouched(obuf, cols_pad, what)
    got = ov.cpu()
    if not bool((got[:, cols:] == 0).all()):
        raise AssertionError(f"{what}: a padding column is not exactly zero")
    dead = torch.isinf(x) & (x < 0)
    if not bool((got[:, :cols][dead] == 0).all()):
        raise AssertionError(f"{what}: an -inf score did not give exactly zero")
    return bounded(got[:, :cols], softmax_bound(x), dtype, what)


# ================================================================ small_linear (one wave per column, 4 rows staged at a time, 1024-block cap)
SMALL_LINEAR_SHAPES = [((1, 8, 1), "one"), ((5, 520, 7), "combos"), ((32, 1280, 4100), "grid_wrap"), ((25, 5120, 64), "lds_opt_in"),
                       ((4, 8192, 8), "lds_max")]
FLAGS = ("bias", "act_in", "act_out", "accumulate")


def small_linear_cases():
    out = []
    for shape, edge in SMALL_LINEAR_SHAPES:
        if edge == "combos":
            combos = list(itertools.product((0, 1), repeat=4))
        elif edge == "one":
            combos = [(0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 1, 1)]
        elif edge == "grid_wrap":
            combos = [(1, 1, 0, 0)]                      # the FiLM projections: SiLU on the way in, bias
        elif edge == "lds_opt_in":
            combos = [(1, 0, 1, 0), (1, 0, 0, 1)]        # the hidden layer of an MLP; emb + aug_emb
        else:
            combos = [(1, 0, 0, 1), (0, 1, 0, 0)]
        for fl in combos:
            tag = "+".join(n for n, f in zip(FLAGS, fl) if f) or "plain"
            out.append(dict(id=f"{'x'.join(map(str, shape))}-{tag}", shape=shape, flags=dict(zip(FLAGS, fl)), edge=edge))
    return out


@functools.lru_cache(maxsize=16)
def small_linear_operands(shape, wdtype):
    rows, k, n = shape
    g = gen(rows * 31 + k + n)
    x = (torch.randn(rows, k, generator=g, dtype=torch.float64) * (10.0 ** ((torch.arange(rows) % 5) - 2).double())[:, None]).float()   # rows by decades
    w = (torch.randn(n, k, generator=g, dtype=torch.float64) * k ** -0.5 * torch.exp2(((torch.arange(n) % 7) - 3).double())[:, None]).to(wdtype)
    bias = torch.randn(n, generator=g, dtype=torch.float64).float()
    y0 = torch.randn(rows, n, generator=g, dtype=torch.float64).float()
    return x, w, bias, y0


def small_linear_bound(x, w, bias, y0, flags) -> Bound:
    k = x.shape[1]
    xd, wd = x.double(), w.double()
    a, e_a = xd, torch.zeros_like(xd)
    if flags["act_in"]:
        a = xd * torch.sigmoid(xd)
        e_a = silu_budget(xd, a)
    depth = 8 * ((k + 511) // 512) + 6 + 1
    s = a @ wd.T
    e = depth * U * (a.abs() @ wd.abs().T) + e_a @ wd.abs().T
    if flags["bias"]:
        s = s + bias.double()[None, :]
        e = e + depth * U * bias.double().abs()[None, :]
    if flags["act_out"]:
        y = s * torch.sigmoid(s)
        e = 1.1 * e + silu_budget(s, y)
        s = y
    if flags["accumulate"]:
        s = s + y0.double()
        e = e + U * s.abs()
    return Bound(s, e)


def run_small_linear(impl, case, wdtype, dev):
    rows, k, n = case["shape"]
    fl = case["flags"]
    what = f"small_linear {case['id']} w {name_of(wdtype)}"
    x, w, bias, y0 = small_linear_operands(case["shape"], wdtype)
    xbuf, xv = window(rows, k, torch.float32, dev)      # ldx > k, ldw > k, ldy > n
    xv.copy_(x)
    wbuf, wv = window(n, k, wdtype, dev)
    wv.copy_(w)
    obuf, ov = window(rows, n, torch.float32, dev, tail=5)
    if fl["accumulate"]:
        ov.copy_(y0)
    impl.small_linear(xv, wv, bias.to(dev) if fl["bias"] else None, act_in=bool(fl["act_in"]), act_out=bool(fl["act_out"]), out=ov,
                      accumulate=bool(fl["accumulate"]))
    canaries_untouched(obuf, n, what)
    return bounded(ov, small_linear_bound(x, w, bias, y0, fl), torch.float32, what)


# ================================================================ timestep_embedding
# out[r] = [cos(t_r f_j) | sin(t_r f_j)],  f_j = expf(-9.210340371976184f * (float)j / (float)half).  Roundings in front of the sine:
#   the constant: fp32(ln 1e4) is off by 1.5e-8 relative = 0.25u: 0.25u ln(1e4) on the exponent                      <= 2.3u
#   the product with j and the quotient by half: u each, relative, on an exponent of magnitude <= ln(1e4) = 9.2104   <= 18.5u
#   expf: <= 1 ulp = 2u;   the product t f_j: u
# every one of them a relative error of the phase t f_j:  A = 2.3 + 18.5 + 2 + 1 = 23.8, rounded up.
TS_A = 24.0
# B u: the last-place error of the device's sinf / cosf on top of that, absolute (|sin|, |cos| <= 1).  No document at hand states it, so it
# is set to TWICE what the fp32 CPU oracle (oracle.leaves.get_timestep_embedding: the same roundings in front of its sine, the CPU's fp32 sine /
# cosine behind them) needs under the same form on the same grid -- tests/test_small_kernels_cpu.py measures and prints that figure:
TS_B_ORACLE = 0.6             # measured 0.593 (torch's fp32 sin / cos on the CPU, 58 values x 5 dims): test_timestep_oracle_b holds this line to it
TS_B = 2 * TS_B_ORACLE
TS_DIMS = [2, 6, 256, 320, 1280]
TS_ROWS = [1, 3, 25, 300]


@functools.lru_cache(maxsize=1)
def timestep_grid() -> torch.Tensor:
    """0, +-1e-3, the model's own inputs (0.25 ln sigma over the 25-step schedule, fps 6, motion bucket 127, noise level 0.02, the frame
    indices 0 .. 24), 200 and 999"""
    from oracle.scheduler import EulerDiscreteScheduler
    s = EulerDiscreteScheduler()
    s.set_timesteps(25)
    t = [0.0, 1e-3, -1e-3] + [float(v) for v in s.timesteps] + [6.0, 127.0, 0.02] + [float(i) for i in range(25)] + [200.0, 999.0]
    return torch.tensor(t, dtype=torch.float32)


def timestep_cases():
    return [dict(id=f"{rows}x{dim}", rows=rows, dim=dim, edge="values") for dim, rows in itertools.product(TS_DIMS, TS_ROWS)]


def timestep_values(rows: int) -> torch.Tensor:
    """300 rows hold the whole grid; fewer rows take every seventh value of it (58 values: 7 visits them all)"""
    g = timestep_grid()
    i = torch.arange(rows)
    return g[(i if rows >= g.numel() else 7 * i + 3) % g.numel()]


def timestep_bound(t: torch.Tensor, dim: int, b: float = None) -> Bound:
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    arg = t.double()[:, None] * f[None, :]
    e = TS_A * U * arg.abs() + (TS_B if b is None else b) * U
    return Bound(torch.cat([arg.cos(), arg.sin()], 1), torch.cat([e, e], 1))


def run_timestep_embedding(impl, case, dtype, dev):
    t = timestep_values(case["rows"])
    got = impl.timestep_embedding(t.to(dev), case["dim"])
    return bounded(got, timestep_bound(t, case["dim"]), torch.float32, f"timestep_embedding {case['id']}")


# ================================================================ the single-request loop glue (2048 blocks x 256 threads, grid-stride)
GLUE_WRAP = (1, 725, 725)                              # f h w = 525 625 > 2048 * 256


@functools.lru_cache(maxsize=1)
def sigmas() -> torch.Tensor:
    from oracle.scheduler import EulerDiscreteScheduler
    s = EulerDiscreteScheduler()
    s.set_timesteps(25)
    return s.sigmas.float().clone()                     # 25 values and the final 0


def prep_cases():
    out = []
    for batch, (shape, edge), cond, step in itertools.product((1, 2, 3), (((1, 1, 1), "one"), ((5, 6, 7), "small"), (GLUE_WRAP, "wrap")),
                                                              (0, 1), (0, 12)):
        if edge == "wrap" and (batch != 1 or step != 12):
            continue
        for cpad in ((16 if cond else 8), 64):
            if edge == "wrap" and cpad == 64:
                continue
            out.append(dict(id=f"b{batch}-{'x'.join(map(str, shape))}-{'cond' if cond else 'nocond'}-cpad{cpad}-step{step}", batch=batch,
                            shape=shape, cond=cond, cpad=cpad, step=step, edge=edge))
    return out


@functools.lru_cache(maxsize=4)
def glue_fields(batch: int, shape):
    f, h, w = shape
    g = gen(batch * 100 + f + h + w)
    lat = (torch.randn(1, f, 4, h, w, generator=g, dtype=torch.float64) * 300).float()
    img = torch.randn(batch, f, 4, h, w, generator=g, dtype=torch.float64).float()
    cond = torch.randn(f, 4, h, w, generator=g, dtype=torch.float64).float()
    return lat, img, cond


def run_prep_model_input(impl, case, dtype, dev):
    f, h, w = case["shape"]
    batch, cpad, step = case["batch"], case["cpad"], case["step"]
    what = f"prep_model_input {case['id']} {name_of(dtype)}"
    lat, img, cond = glue_fields(batch, case["shape"])
    sg = sigmas()
    x = impl.prep_model_input(lat.to(dev), img.to(dev), cond.to(dev) if case["cond"] else None, sg.to(dev), step, batch, f, h, w, cpad, dtype)
    got = x.cpu().view(batch, f, h, w, cpad)
    tok = lambda t: t.permute(0, 1, 3, 4, 2)            # [b, f, 4, h, w] -> [b, f, h, w, 4]
    same(got[..., 4:8], tok(img).to(dtype), what + " image latents")
    c0 = 8
    if case["cond"]:
        same(got[..., 8:12], tok(cond[None]).expand(batch, f, h, w, 4).to(dtype), what + " cond")
        c0 = 12
    if not bool((got[..., c0:] == 0).all()):
        raise AssertionError(f"{what}: the zero tail is not exactly zero")
    s = sg[step].double()
    ref = tok(lat).double().expand(batch, f, h, w, 4) / torch.sqrt(s * s + 1.0)
    return bounded(got[..., :4], Bound(ref, 5 * U * ref.abs()), dtype, what)


def cfg_cases():
    out = []
    for batch, guided, ld, step in itertools.product((1, 2, 3), (0, 1), (4, 8), (0, 12, 24)):
        if batch == 3 and not guided:
            continue                                    # the InstructPix2Pix combination needs its guidance
        out.append(dict(id=f"b{batch}-{'g' if guided else 'nog'}-ld{ld}-step{step}", batch=batch, guided=guided, ld=ld, step=step,
                        shape=(5, 6, 7), edge="small" if batch < 3 else "batch3"))
    out.append(dict(id="b1-nog-ld4-step12-wrap", batch=1, guided=0, ld=4, step=12, shape=GLUE_WRAP, edge="wrap"))
    return out


IMAGE_GUIDANCE = 7.5


def cfg_euler_bound(eps, lat, g, sg: float, sn: float, batch: int) -> Bound:
    """eps [batch, f, 4, h, w] fp32, lat [f, 4, h, w], g [f] or None -- the statements of cfg_euler_kernel in fp64, each with the sum of
    the absolute values of its terms times the roundings behind them (first order; contraction into fmas only removes roundings):
        t1 = cd - u (u |t1|);  t2 = g t1 (u |t2| more);  v = u + t2 (u |v|)                       batch 3: + ig (cd - e1), likewise
        c_out = -s / sqrtf(s s + 1), c_skip = 1 / (s s + 1): <= 4u relative each (square, sum, root, quotient)
        a = v c_out: |c_out| e_v + 5u |a|;  b = x c_skip: 5u |b|;  x0 = a + b: + u |x0|
        d = x - x0: e_x0 + u |d|  (the cancellation: e_x0 stays absolute);  q = d / s: e_d / s + u |q|
        r = q (s' - s): the difference and the product round, e_q |s' - s| + 2u |r|;  x' = x + r: + u |x'|"""
    e = eps.double()
    x = lat.double()
    gg = torch.ones(eps.shape[1], dtype=torch.float64) if g is None else g.double()
    gg = gg.view(-1, 1, 1, 1)
    if batch == 1:
        v, ev = e[0], torch.zeros_like(x)
    else:
        e1, cd, u = (e[0], e[1], e[2]) if batch == 3 else (None, e[1], e[0])
        t2 = gg * (cd - u)
        v = u + t2
        ev = 2 * U * t2.abs() + U * v.abs()
        if batch == 3:
            t4 = IMAGE_GUIDANCE * (cd - e1)
            ev = ev + 2 * U * t4.abs() + U * (v + t4).abs()
            v = v + t4
    c_out, c_skip = -sg / math.sqrt(sg * sg + 1.0), 1.0 / (sg * sg + 1.0)
    a, b = v * c_out, x * c_skip
    x0 = a + b
    e0 = abs(c_out) * ev + 5 * U * a.abs() + 5 * U * b.abs() + U * x0.abs()
    d = x - x0
    ed = e0 + U * d.abs()
    q = d / sg
    eq = ed / sg + U * q.abs()
    r = q * (sn - sg)
    er = eq * abs(sn - sg) + 2 * U * r.abs()
    out = x + r
    return Bound(out, er + U * out.abs())


def run_cfg_euler_step(impl, case, dtype, dev):
    f, h, w = case["shape"]
    batch, ld, step = case["batch"], case["ld"], case["step"]
    lat, _, _ = glue_fields(1, case["shape"])
    lat = lat[0]
    eps = torch.randn(batch, f, 4, h, w, generator=gen(batch + f * h), dtype=torch.float64).float()
    g = torch.linspace(1.0, 3.0, f) if case["guided"] else None
    sg = sigmas()
    tok = torch.full((batch * f * h * w, ld), CANARY, dtype=torch.float32)
    tok[:, :4] = eps.permute(0, 1, 3, 4, 2).reshape(-1, 4)
    lat_d = lat.to(dev).clone()
    impl.cfg_euler_step(tok.to(dev), lat_d, None if g is None else g.to(dev), sg.to(dev), step, batch, f, h, w,
                        image_guidance_scale=IMAGE_GUIDANCE if batch == 3 else None)
    b = cfg_euler_bound(eps, lat, g, float(sg[step]), float(sg[step + 1]), batch)
    return bounded(lat_d, b, torch.float32, f"cfg_euler_step {case['id']}")


# ================================================================ act_rows
def act_values(dtype) -> torch.Tensor:
    """every storage value in [-16, 16] of a 16-bit type (a dense grid for fp32), +-50, +-300, and the neighbourhood of 1.702 |x| = 88.7,
    where __expf overflows: |x| in [50, 56]"""
    if dtype == torch.float32:
        v = torch.cat([torch.linspace(-16, 16, 1 << 16, dtype=torch.float64), torch.linspace(50, 56, 4096, dtype=torch.float64),
                       -torch.linspace(50, 56, 4096, dtype=torch.float64)]).float()
    else:
        pos = torch.arange(0, 1 << 15, dtype=torch.int32).to(torch.int16).view(dtype)
        pos = pos[torch.isfinite(pos.float())]
        fl = pos.float()
        keep = pos[(fl <= 16) | ((fl >= 50) & (fl <= 56))]
        v = torch.cat([keep, -keep])
    v = torch.cat([v, torch.tensor([50.0, -50.0, 300.0, -300.0], dtype=torch.float32).to(dtype)])
    pad = (-v.numel()) % 64
    return torch.cat([v, torch.zeros(pad, dtype=dtype)]).view(-1, 64)


def act_cases():
    return [dict(id=f"{act}-{layout}", act=act, layout=layout, edge="values") for act in ("gelu", "quick_gelu")
            for layout in ("plain", "strided", "in_place")]


def act_bound(x: torch.Tensor, act: str) -> Bound:
    xd = x.double()
    if act == "gelu":
        y = gelu_exact(xd)
        return Bound(y, gelu_budget("erf", xd, y))
    t = 1.702 * xd
    y = xd * torch.sigmoid(t)
    return Bound(y, silu_budget(t, y) + U * t.abs() * y.abs())          # the SiLU form + the forming error of t = fl(1.702f x)


def run_act_rows(impl, case, dtype, dev):
    x = act_values(dtype)
    what = f"act_rows {case['id']} {name_of(dtype)}"
    b = act_bound(x, case["act"])
    if case["layout"] == "plain":
        return bounded(impl.act_rows(x.to(dev), case["act"]), b, dtype, what)
    if case["layout"] == "in_place":
        xd = x.to(dev).clone()
        return bounded(impl.act_rows(xd, case["act"], out=xd), b, dtype, what)
    xbuf, xv = window(x.shape[0], x.shape[1], dtype, dev)
    xv.copy_(x)
    obuf, ov = window(x.shape[0], x.shape[1], dtype, dev, tail=16)
    impl.act_rows(xv, case["act"], out=ov)
    canaries_untouched(obuf, x.shape[1], what)
    return bounded(ov, b, dtype, what)


# ================================================================ patch_tokens, embed_rows (exact)
def patch_cases():
    return [dict(id=f"{'x'.join(map(str, s))}-{src}-kpad{kp}", shape=s, src=src, kpad=kp, edge=edge)
            for (s, kp, edge) in (((2, 3, 28, 42, 14), None, "oblong"), ((1, 5, 6, 4, 2), None, "oblong"), ((1, 5, 6, 4, 2), 48, "oblong"),
                                  ((2, 3, 28, 28, 14), 600, "square")) for src in ("f32", "st")]


def run_patch_tokens(impl, case, dtype, dev):
    n, c, h, w, p = case["shape"]
    src_dtype = torch.float32 if case["src"] == "f32" else dtype
    src = transpose_values(n * c * h * w, src_dtype, dtype, 21).view(n, c, h, w)
    got = impl.patch_tokens(src.to(dev), p, dtype, kpad=case["kpad"])
    kk = c * p * p
    kpad = (kk + 7) // 8 * 8 if case["kpad"] is None else case["kpad"]
    want = torch.zeros(n * (h // p) * (w // p), kpad, dtype=dtype)
    want[:, :kk] = src.view(n, c, h // p, p, w // p, p).permute(0, 2, 4, 1, 3, 5).reshape(-1, kk).to(dtype)
    return same(got, want, f"patch_tokens {case['id']} {name_of(dtype)}")


def embed_cases():
    return [dict(id="text-ids-outside-the-table", mode="text", edge="ids"), dict(id="vision-l2", mode="vision", edge="l2")]


def run_embed_rows(impl, case, dtype, dev):
    c = 24
    g = gen(5)
    what = f"embed_rows {case['id']} {name_of(dtype)}"
    if case["mode"] == "text":
        l, nseq, table_rows = 5, 3, 11
        table = torch.randn(table_rows, c, generator=g, dtype=torch.float64).to(dtype)
        pos = torch.randn(l, c, generator=g, dtype=torch.float64).to(dtype)
        ids = torch.randint(0, table_rows, (nseq * l,), generator=g)
        ids[1], ids[6], ids[12], ids[14] = -1, table_rows, 1 << 40, table_rows - 1
        inside = (ids >= 0) & (ids < table_rows)
        rows = torch.where(inside[:, None], table[ids.clamp(0, table_rows - 1)].float(), torch.zeros(1))
        want = (rows + pos.float().repeat(nseq, 1)).to(dtype)
        assert torch.equal(want[1], pos[1]) and torch.equal(want[6], pos[1]) and torch.equal(want[12], pos[2])   # the position row alone
        obuf, ov = window(nseq * l, c, dtype, dev)
        impl.embed_rows(table.to(dev), pos.to(dev), ids=ids.to(dev), l=l, out=ov)
    else:
        l, nimg = 2, 7
        table = torch.randn(nimg, c, generator=g, dtype=torch.float64).to(dtype)
        pos = torch.randn(l, c, generator=g, dtype=torch.float64).to(dtype)
        cls = torch.randn(c, generator=g, dtype=torch.float64).to(dtype)
        rows = torch.stack([cls[None].expand(nimg, c), table], 1).reshape(nimg * l, c)
        want = (rows.float() + pos.float().repeat(nimg, 1)).to(dtype)
        obuf, ov = window(nimg * l, c, dtype, dev)
        impl.embed_rows(table.to(dev), pos.to(dev), cls=cls.to(dev), l=l, out=ov)
    canaries_untouched(obuf, c, what)
    return same(ov, want, what)


# ================================================================ the table of tables
# kernel -> (cases, run, whether the storage type matters: False runs once, in fp32)
KERNELS = {
    "nchw_to_tokens": (transpose_cases, run_nchw_to_tokens, True),
    "tokens_to_nchw": (transpose_cases, run_tokens_to_nchw, True),
    "add_scaled": (add_scaled_cases, run_add_scaled, True),
    "add_rowvec": (add_rowvec_cases, run_add_rowvec, True),
    "softmax_rows": (softmax_cases, run_softmax_rows, True),
    "small_linear": (small_linear_cases, run_small_linear, True),
    "timestep_embedding": (timestep_cases, run_timestep_embedding, False),
    "prep_model_input": (prep_cases, run_prep_model_input, True),
    "cfg_euler_step": (cfg_cases, run_cfg_euler_step, False),
    "act_rows": (act_cases, run_act_rows, True),
    "patch_tokens": (patch_cases, run_patch_tokens, True),
    "embed_rows": (embed_cases, run_embed_rows, True),
}


def applies(kernel: str, case, dtype) -> bool:
    """fp32 storage has no fp32 sibling: the duplicates of a transpose / patch case are dropped"""
    if dtype == torch.float32 and kernel in ("nchw_to_tokens", "tokens_to_nchw", "patch_tokens"):
        return case.get("src", "st") == "st" and case.get("dst", "st") == "st"
    if kernel == "nchw_to_tokens" and case["dst"] == "f32":
        return False                                    # the destination of nchw_to_tokens IS the storage type: covered by dtype = fp32
    return True


def all_cases(kernel: str, dtype):
    cases, _, typed = KERNELS[kernel]
    if not typed and dtype != torch.float32:
        return []
    return [c for c in cases() if applies(kernel, c, dtype)]


def run(kernel: str, impl, case, dtype, dev="cpu") -> float:
    return KERNELS[kernel][1](impl, case, dtype, dev)
