"""The cases of tests/test_gemm_w320_bits_gpu.py, shared with tests/golden/make_gemm_w320_bits.py (which records their output hashes from
the library of the commit that is the reference).  gemm_w320_kernel (256 x 320 tiles) and gemm_w320h_kernel (128 x 320, optional split-K)
are built from shared pieces (producer, strip transposition / exchange, epilogue, LayerNorm 1/sigma; gemm_w320.hip), so a change to one
piece moves both.  Shapes are those of tests/test_gemm_w320_gpu.py and of the big-tile cases of tests/test_ops_gpu.py with K cut to <= 640
outside the split-K route; M stays where the planner picks the kernel under tt_gemm_set_big_tile(3) (40-50 k rows: 256-row tiles,
12.5-25 k: 128-row tiles).  Between them the cases reach: all 16 instances (2 kernels x {linear, conv3x3, temporal conv, linear + ln_fold}
x {bf16, f16}); every arm of w3_epilogue_dispatch (statistics with / without residual x with / without row vector, distinct blend x
with / without row vector, residual only x with / without row vector, plain with bias == NULL); the even / odd row vector and a row-vector
group boundary inside a fragment row (groups of 3000 rows); a ragged last row tile on each kernel; two channel sources; a strided A view and
in-place over the residual; K = 128 (two slabs: the ring never reaches its steady state) and odd slab counts >= 5; the split-K route with a
slice that starts inside a tap of the SECOND source, an odd slab split and the 9-slice coarsest level; two statistics tiles per output
tile (128-row kernel, 448-row segments).

run_case(ops, case) -> (output on the device, tile sums or None, fp32 reference on the CPU, rtol, atol); it asserts the kernel the launch
ran on (ops.PROFILE), so a planner change cannot silently move a case.  Operands are seeded (utils/synthetic.py) and the reference is
fp32 torch on the operands the kernel gets."""
import hashlib

import torch
import torch.nn.functional as F

from this_and_that_vdm_amd.utils.synthetic import hash_uniform

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
# tests/test_gemm_w320_gpu.py: fp16 rtol = atol = 1e-3, bf16 1.6e-2 with atol x 2 (outputs are O(4))
TOL = {"f16": (1e-3, 1e-3), "bf16": (1.6e-2, 3.2e-2)}
BOTH = ("bf16", "f16")


def _cases():
    out = []
    for dt in BOTH:
        # bias, scale, row vector in groups of 3000 rows, residual, DISTINCT blend; ragged last row tile; K = 192: 3 slabs
        out += [dict(kind="linear", dt=dt, m=46100, n=320, k=192, epi="full"), dict(kind="linear", dt=dt, m=12500, n=640, k=192, epi="full")]
        # ln_fold + residual; 5 slabs; ragged
        out += [dict(kind="ln", dt=dt, m=50176 - 100, n=320, k=320), dict(kind="ln", dt=dt, m=25088 - 60, n=320, k=320)]
        # conv3x3, two channel sources, bias + FiLM row + residual (18 slabs); 16 x 28: the second level, 128-row tiles
        out += [dict(kind="conv", dt=dt, h=32, w=56, c0=64, c1=64, n=320, epi="film_res"), dict(kind="conv", dt=dt, h=16, w=28, c0=64, c1=64, n=640, epi="film_res")]
        # temporal conv + bias + AlphaBlender with the residual as its source
        out += [dict(kind="tconv", dt=dt, hw=1792, n=320), dict(kind="tconv", dt=dt, hw=448, n=640)]
    # the remaining epilogue arms, one storage type each
    out += [dict(kind="linear", dt="bf16", m=47000, n=320, k=128, epi="none"), dict(kind="linear", dt="f16", m=12000, n=640, k=128, epi="none")]      # bias == NULL; two slabs
    out += [dict(kind="linear", dt="f16", m=50176, n=320, k=128, epi="blend"), dict(kind="linear", dt="bf16", m=12544, n=640, k=128, epi="blend")]     # distinct blend, no row vector
    out += [dict(kind="linear", dt="f16", m=50176 - 77, n=320, k=128, epi="parity"), dict(kind="linear", dt="bf16", m=12544, n=640, k=320, epi="parity")]      # even / odd row vector + residual
    out += [dict(kind="linear", dt="bf16", m=50176, n=320, k=320, epi="film"), dict(kind="linear", dt="f16", m=25088, n=320, k=320, epi="film")]       # row vector only
    # the 1x1 shortcut over a skip concat: two sources, strided A, in place over the residual which is also the blend source
    out += [dict(kind="inplace", dt="bf16", m=50176, n=320), dict(kind="inplace", dt="f16", m=12544, n=640)]
    # statistics: residual x row vector; the 128-row kernel with one statistics tile per 64-row wave row (448-row segments)
    out += [dict(kind="conv", dt="bf16", h=32, w=56, c0=64, c1=0, n=320, epi="bias", stats=4 * 1792, srows=256),
            dict(kind="linear", dt="f16", m=50176, n=320, k=128, epi="res", stats=4 * 1792, srows=256),
            dict(kind="linear", dt="bf16", m=50176, n=320, k=128, epi="film_res", stats=4 * 1792, srows=256),
            dict(kind="conv", dt="f16", h=16, w=28, c0=64, c1=0, n=640, epi="film", stats=4 * 448, srows=128),
            dict(kind="conv", dt="bf16", h=16, w=28, c0=64, c1=0, n=640, epi="film_res", stats=448, srows=64)]
    # split-K (128-row kernel + reduction pass): 63 slabs in two slices, the second starts inside tap 4 in the SECOND source; 2912 rows
    # (ragged) and 45 slabs, 22 + 23; the coarsest level, 28 tiles x 9 slices
    out += [dict(kind="conv", dt="bf16", h=8, w=14, c0=128, c1=320, n=1280, epi="film_res", split=True),
            dict(kind="conv", dt="f16", h=8, w=13, c0=320, c1=0, n=1280, epi="film_res", split=True),
            dict(kind="conv", dt="bf16", h=4, w=7, c0=640, c1=640, n=1280, epi="film_res", split=True)]
    return out


def case_id(c):
    return "-".join(f"{k}={v}" for k, v in c.items())


CASES = _cases()


def _u(*shape, seed, dtype=torch.float32, scale=1.7):
    """seeded uniform values on the GPU (unit variance at scale 1.7), rounded through the storage type"""
    n = 1
    for s in shape:
        n *= s
    return (hash_uniform(n, seed, device="cuda").view(*shape) * scale).to(dtype)


def _f(t):
    return t.float().cpu()


def _epilogue(case, m, n, dtype, rows_per_vec):
    """(keyword arguments of ops.gemm, reference epilogue lin -> out) of the case's operand set"""
    epi = case.get("epi", "none")
    kw, bias = {}, None
    if epi != "none":
        bias = _u(n, seed=3)
        kw["bias"] = bias
    rv = res = bl = None
    scale, alpha = 1.0, 0.0
    if epi in ("full", "film", "film_res"):
        rv = _u((m + rows_per_vec - 1) // rows_per_vec, n, seed=4)
        kw.update(rowvec=rv, rowvec_rows=rows_per_vec)
    if epi == "parity":
        rv = _u(2, n, seed=4)
        kw.update(rowvec=rv, rowvec_rows=1, rowvec_mod=2)
    if epi in ("full", "res", "film_res", "parity"):
        res = _u(m, n, seed=5, dtype=dtype)
        kw["residual"] = res
    if epi in ("full", "blend"):
        bl = _u(m, n, seed=6, dtype=dtype)
        alpha = 0.3
        kw.update(blend=bl, alpha=alpha)
    if epi == "full":
        scale = 0.75
        kw["acc_scale"] = scale

    def ref(lin):
        v = lin
        if bias is not None:
            v = v + _f(bias)
        v = v * scale
        if epi == "parity":
            v = v + _f(rv)[torch.arange(m) % 2]
        elif rv is not None:
            v = v + _f(rv).repeat_interleave(rows_per_vec, 0)[:m]
        if res is not None:
            v = v + _f(res)
        if bl is not None:
            v = alpha * _f(bl) + (1.0 - alpha) * v
        return v

    return kw, ref


def _run(ops, a, w, **kw):
    """one launch under tt_gemm_set_big_tile(3) (the 128-row kernel for every gather mode and its split-K route), with its kernel name"""
    lib = ops._lib.load()
    lib.tt_gemm_set_big_tile(3)
    ops.PROFILE = []
    try:
        out = ops.gemm(a, w, **kw)
        torch.cuda.synchronize()
        name = ops.PROFILE[0][0]
    finally:
        ops.PROFILE = None
        lib.tt_gemm_set_big_tile(1)
    return out, name


def run_case(ops, case):
    kind, dtype = case["kind"], DT[case["dt"]]
    rtol, atol = TOL[case["dt"]]
    tag = f"{case['dt']}_tag"
    if kind in ("linear", "ln"):
        m, n, k = case["m"], case["n"], case["k"]
        kern, mode, ln = ("gemm_w320_kernel" if m > 40000 else "gemm_w320h_kernel"), 0, int(kind == "ln")
        w = _u(n, k, seed=2, dtype=dtype, scale=1.7 * k ** -0.5)
        if kind == "ln":
            from this_and_that_vdm_amd.packing import fold_layernorm, zero_sum_round
            a = (_u(m, k, seed=1, scale=2.6) + _u(m, 1, seed=9, scale=2.6)).to(dtype)
            g, be = _u(k, seed=7, scale=0.35) + 1, _u(k, seed=8, scale=0.5)
            wf, bf = fold_layernorm(w.float().cpu(), _u(n, seed=3).cpu(), g.cpu(), be.cpu())
            wq, bf, res = zero_sum_round(wf, dtype).cuda(), bf.cuda(), _u(m, n, seed=5, dtype=dtype)
            out, name = _run(ops, a, wq, bias=bf, ln_fold=1, ln_eps=1e-5, residual=res)
            # fp32 on the operands the kernel gets: 1/sigma of the stored rows times the product with the folded, rounded weights
            x = _f(a)
            rs = torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
            ref = (x @ _f(wq).T) * rs + _f(bf) + _f(res)
        else:
            a = _u(m, k, seed=1, dtype=dtype)
            kw, epi = _epilogue(case, m, n, dtype, 3000 if case["epi"] == "full" else 14 * 1792)
            out, name = _run(ops, a, w, stats=case.get("stats", 0), **kw)
            ref = epi(_f(a) @ _f(w).T)
    elif kind == "inplace":
        m, n, k0, k1 = case["m"], case["n"], 128, 64
        kern, mode, ln = ("gemm_w320_kernel" if m > 40000 else "gemm_w320h_kernel"), 0, 0
        a0 = _u(2 * m, k0, seed=1, dtype=dtype)[0::2]
        a1 = _u(m, k1, seed=7, dtype=dtype)
        w = _u(n, k0 + k1, seed=2, dtype=dtype, scale=1.7 * (k0 + k1) ** -0.5)
        bias = _u(n, seed=3)
        x = _u(m + 64, n + 16, seed=5, dtype=dtype)
        view = x[32:32 + m, 8:8 + n]
        xr = _f(view)
        ref = _f(x)                                         # the whole buffer: what lies around the [m, n] window stays as it was
        ref[32:32 + m, 8:8 + n] = 0.4 * xr + 0.6 * (torch.cat([_f(a0), _f(a1)], 1) @ _f(w).T + _f(bias) + xr)
        _, name = _run(ops, a0, w, a1=a1, bias=bias, residual=view, blend=view, alpha=0.4, out=view)
        out = x
    elif kind == "conv":
        from this_and_that_vdm_amd.packing import pack_conv3x3
        nimg, frames, h, wd, c0, c1, n = 28, 14, case["h"], case["w"], case["c0"], case["c1"], case["n"]
        m, c = nimg * h * wd, c0 + c1
        kern, mode, ln = ("gemm_w320_kernel" if h == 32 else "gemm_w320h_kernel"), 1, 0
        x0 = _u(m, c0, seed=1, dtype=dtype)
        x1 = _u(m, c1, seed=2, dtype=dtype) if c1 else None
        wt = _u(n, c, 3, 3, seed=3, dtype=dtype, scale=1.7 * (9 * c) ** -0.5)
        kw, epi = _epilogue(case, m, n, dtype, frames * h * wd)
        out, name = _run(ops, x0, pack_conv3x3(wt.cpu()).cuda(), a1=x1, mode=1, conv=(nimg, h, wd, h, wd, 1, 0), stats=case.get("stats", 0), **kw)
        xin = torch.cat([_f(x0), _f(x1)], 1) if c1 else _f(x0)
        xin = xin.view(nimg, h, wd, c).permute(0, 3, 1, 2)
        ref = epi(F.conv2d(xin, _f(wt), None, padding=1).permute(0, 2, 3, 1).reshape(m, n))
    else:
        from this_and_that_vdm_amd.packing import pack_tconv3
        b, f, c, hw, n = 2, 14, 64, case["hw"], case["n"]
        m = b * f * hw
        kern, mode, ln = ("gemm_w320_kernel" if hw == 1792 else "gemm_w320h_kernel"), 2, 0
        x = _u(m, c, seed=1, dtype=dtype)
        wt = _u(n, c, 3, 1, 1, seed=2, dtype=dtype, scale=1.7 * (3 * c) ** -0.5)
        bias, res = _u(n, seed=3), _u(m, n, seed=5, dtype=dtype)
        out, name = _run(ops, x, pack_tconv3(wt.cpu()).cuda(), mode=2, tconv=(f, hw), bias=bias, residual=res, blend=res, alpha=0.35)
        xin = _f(x).view(b, f, hw, 1, c).permute(0, 4, 1, 2, 3)
        conv = F.conv3d(xin, _f(wt), _f(bias), padding=(1, 0, 0))[..., 0].permute(0, 2, 3, 1).reshape(m, n)
        ref = 0.35 * _f(res) + 0.65 * (conv + _f(res))
    sums = None
    if case.get("stats"):
        st = getattr(out, "_tt_stats", None)
        assert st is not None and st[1] == case["srows"], f"no tile sums, or not on tiles of {case['srows']} rows: {st and st[1]}"
        sums = st[0]
        xs = out.float()
        want = torch.stack([xs.view(-1, st[1], n).sum(1), (xs * xs).view(-1, st[1], n).sum(1)], 1)
        torch.testing.assert_close(sums, want, rtol=2e-5, atol=2e-4)      # (tests/test_ops_gpu.py's bound for the tile sums)
    want_name = f"{kern}<{tag}, {mode}, {ln}>"
    assert name == want_name, f"the planner moved this case to {name} (expected {want_name})"
    return out, sums, ref, rtol, atol


def output_hash(out, sums=None):
    """sha256 of the stored output (and of the tile sums where there are any)"""
    torch.cuda.synchronize()
    h = hashlib.sha256(out.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    if sums is not None:
        h.update(sums.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()
