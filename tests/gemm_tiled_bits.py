"""The cases of tests/test_gemm_tiled_bits_gpu.py and tests/test_gemm_tiled_bits_cpu.py, shared with tests/golden/make_gemm_tiled_bits.py
(which records their output hashes from the library of the commit that is the reference).  They pin the tiled template of tt_gemm
(gemm_kernel: every tile of TT_GEMM_TILES / TT_GEMM_TILES_F32, every KMODE_ of TT_GEMM_KMODES on the tiles it is built for), its split-K
reduction kernels and sq320_kernel.  Shapes are the smallest at which each piece can still go wrong:

  * per tile: m = BM + 33 (the second tile row is ragged inside a live 32-row fragment), n = BN + 36 (the second tile column ends inside
    a quad row; BN + 48 / BN + 32 where n % 16 / n % 32 is required), K steps KT in {1, NST - 1, NST, 2 NST + 1} (the ring never fills,
    just fills, reaches its steady state) with k0 = KT BK - 24 (dead chunks in the last step), one two-source case with k1 = BK + 8;
  * gathers: conv3x3 on 2 images of 5 x 7 (a tile straddles the images) with stride 1 / 2, upsample 1 / 2 (the four phase slices),
    mode 3 on 6 x 8 with stride 2, the temporal conv on 2 x 3 frames of 40 rows (a tile spans frame and group borders), 24 channels
    (every tap ends in a K tail); ln_fold 1 / 2, with row means 12 sigma from zero (ln_stat_shifted for fp32); split16 plain, with W / A /
    both pre-split and its conv / tconv / LN / mode-3 forms; the wide forms;
  * every arm of the pass epilogue's dispatch (EPIS below), on one tile per wave-tile shape;
  * the tile order with tiles_n > 8 and a ragged last group; split-K plans the planner makes by itself (a forced tile never splits) into
    all three reduction kernels, one slice starting inside a tap of the second source, one launch without its workspace;
  * sq320_kernel's three instances, m = 260 ragged 32-row tiles on the 256-block grid (blocks own 1 and 2 tiles).

run_case(ops, case) -> (what is hashed: the stored output or the buffer around it, extra tensors hashed with it, fp32 reference on the
CPU, rtol, atol); it asserts the kernel the launch ran on (ops.PROFILE), so a planner change cannot silently move a case.  Operands are
seeded (utils/synthetic.py) and the reference is fp32 torch on the operands the kernel gets.  plan_case(ops, case) builds the same
TtGemmArgs on the CPU (ops.gemm with the launch replaced by the host-only queries) for the _cpu test."""
import contextlib
import ctypes as C
import hashlib

import torch
import torch.nn.functional as F

from tests.gemm_w320_bits import TOL as TOL16
from this_and_that_vdm_amd.utils.synthetic import hash_uniform

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "split16": torch.float32}
TAG = {"bf16": "bf16_tag", "f16": "f16_tag", "f32": "f32_tag", "split16": "f32_tag"}
# 16-bit: TOL of tests/gemm_w320_bits.py.  fp32: tests/test_ops_gpu.py (exact-fp32 MFMA, only the summation order differs).  split16: a
# product carries 2^-21 relative (the dropped lo x lo term); |a| <= 1.7 and |w| <= 1.7 K^-1/2 give sum |a w| <= 2.9 sqrt(K) <= 80 for
# the K <= 720 used here, i.e. <= 4e-5 absolute: the mode's own target, atol 1e-4, holds with room and is what is asserted.
TOL = dict(TOL16, f32=(2e-5, 2e-5), split16=(1e-4, 1e-4))
# (BM, BN, BK, NST, WGM, WGN, LNOK, M3OK): TT_GEMM_TILES / TT_GEMM_TILES_F32 (the _cpu test holds every expected name to tt_gemm_kernel)
TILES = [(128, 128, 64, 2, 2, 2, 0, 0), (128, 64, 64, 3, 2, 2, 1, 1), (64, 64, 64, 4, 2, 2, 1, 1), (256, 128, 32, 3, 4, 2, 1, 0),
         (256, 256, 32, 3, 2, 4, 0, 0), (128, 128, 32, 3, 2, 2, 0, 0), (256, 128, 64, 3, 4, 2, 0, 0), (128, 160, 64, 2, 4, 1, 1, 0),
         (128, 320, 32, 3, 4, 2, 0, 0), (256, 256, 64, 2, 2, 4, 1, 0), (128, 128, 64, 4, 2, 2, 0, 0), (128, 128, 64, 2, 4, 2, 1, 1),
         (256, 160, 32, 3, 8, 1, 0, 0), (256, 128, 32, 4, 4, 2, 0, 0), (128, 128, 32, 5, 4, 2, 0, 0), (128, 128, 64, 3, 4, 2, 0, 0),
         (128, 128, 64, 4, 4, 2, 1, 1), (256, 256, 32, 4, 2, 4, 0, 0), (256, 128, 64, 2, 4, 2, 0, 0), (256, 128, 32, 5, 4, 2, 0, 0),
         (128, 128, 128, 2, 4, 2, 0, 0)]
TILES_F32 = [(128, 128, 32, 2, 2, 2, 1, 1), (64, 64, 32, 4, 2, 2, 1, 1)]
WIDE16 = (11, 16)
# one 16-bit tile per wave-tile shape of the pass epilogue: 32 x 32 (2), 32 x 64 (11), 64 x 64 (0), the 256-row tile that reads the
# residual in-pass (3), and 32 x 160 with its odd number of 64-column chunks (7)
EPI_TILES = (2, 11, 0, 3, 7)
# the arms of the pass epilogue's dispatch and the paths beside it
EPIS = ("none",          # plain, bias == NULL
        "film",          # row vector held in registers, a group boundary inside a fragment row (groups of 40 rows)
        "film_mod",      # ... periodic (rowvec_mod = 3)
        "parity",        # ... the even / odd form
        "blend",         # in-pass: a blend tensor of its own (+ residual, scale)
        "short",         # in-pass: row-vector groups of 5 rows
        "res",           # residual: preloaded, or in-pass on a 256-row tile and in split16
        "blend_res",     # AlphaBlender with the residual as its source
        "fp8",           # out_fp8
        "geglu",         # the GEGLU epilogue
        "f32out",        # the direct path: fp32 out of 16-bit storage
        "colpad",        # ... and out_col_hw
        "inplace",       # in place over the residual, strided A, two sources
        "stats", "stats_wave", "stats_film_res")      # statistics: one tile per BM rows / per wave row; with row vector + residual


def tile_of(case):
    return (TILES_F32 if DT[case["dt"]] == torch.float32 else TILES)[case["tile"]]


def _kmode(case):
    kind, split = case["kind"], 8 if case["dt"] == "split16" else 0
    pre = case.get("pre", 0)
    if case.get("wide"):
        return 64 + split + {"linear": 0, "conv": 1, "tconv": 2}[kind]
    base = {"linear": 0, "conv": 1, "tconv": 2, "ln1": 3, "ln2": 4, "m3": 5}[kind]
    return base + split + (16 if pre & 2 else 0) + (32 if pre & 1 else 0)


def kernel_of(case):
    """the kernel instance the case must run on, as ops.PROFILE and tt_gemm_kernel name it"""
    if case["kind"] == "sq320":
        return "sq320_kernel<%s, %s, %s>" % (TAG[case["dt"]], "true" if case["epi"] != "bias" else "false", "true" if case["epi"] == "parity_res" else "false")
    t = tile_of(case)
    return "gemm_kernel<%s, %d, %d, %d, %d, %d, %d, %d>" % ((TAG[case["dt"]],) + t[:6] + (_kmode(case),))


def _wide_n(case, m):
    """TT_F32 picks its tile by the tile count: 128 x 128 from 256 tiles on (the un-split threshold, above split16's 160) -- reached
    here with columns --, else 64 x 64; the 16-bit tiles are forced"""
    if DT[case["dt"]] != torch.float32 or case["tile"] != 0 or case.get("splitk") or case.get("stats"):
        return 0                                                    # (the statistics cases reach it with rows: GroupNorm widths stay small)
    return -(-256 // -(-m // 128)) * 128 - 128


def _n_for(bn, epi):
    """BN + 36; n % 16 for GEGLU, whole groups of 20 columns for out_col_hw"""
    return bn + 48 if epi == "geglu" else ((bn + 55) // 20 * 20 if epi == "colpad" else bn + 36)


def _cases():
    out = []

    def add(kind, dt, tile, **kw):
        out.append(dict(kind=kind, dt=dt, tile=tile, **kw))

    def tiles(dt):
        return range(len(TILES_F32 if DT[dt] == torch.float32 else TILES))

    for dt in DT:
        for t in tiles(dt):
            bm, bn, bk, nst, _, _, lnok, m3ok = (TILES_F32 if DT[dt] == torch.float32 else TILES)[t]
            # the ring: K steps, K tail, ragged second tile row and column; two sources
            for kt in sorted({1, nst - 1, nst, 2 * nst + 1}):
                add("linear", dt, t, m=bm + 33, n=bn + 36, k0=kt * bk - 24, epi="bias")
            add("linear", dt, t, m=bm + 33, n=bn + 36, k0=bk - 24, k1=bk + 8, epi="bias")
            # the gathers on every tile they are built for
            add("conv", dt, t, n=bn + 36, c0=24, epi="bias")
            add("tconv", dt, t, n=bn + 36, c0=24, epi="blend_res")
            if lnok:                                                # (fp32 storage: whole K steps -- ln_stat_shifted counts the zero fill of a K tail)
                add("ln1", dt, t, m=bm + 33, n=bn + 36, k0=2 * bk + (8 if DT[dt] != torch.float32 else 0))
                add("ln2", dt, t, m=bm + 33, n=bn + 36, k0=2 * bk + (8 if DT[dt] != torch.float32 else 0))
            if m3ok:
                add("m3", dt, t, n=bn + 36, c0=24, epi="bias")
    # the conv forms: stride 2, two sources, the fused upsample and the phase store
    for dt, ts in (("bf16", (2, 16)), ("f16", (11, 3)), ("f32", (0, 1)), ("split16", (0, 1))):
        for t in ts:
            bn = tile_of(dict(dt=dt, tile=t))[1]
            add("conv", dt, t, n=bn + 36, c0=24, stride=2, epi="film_res")
            add("conv", dt, t, n=bn + 36, c0=16, c1=24, epi="res")
            add("conv", dt, t, n=bn + 36, c0=24, ups=1, epi="bias")
            add("conv", dt, t, n=bn + 36, c0=24, ups=2, epi="bias")
            add("tconv", dt, t, n=bn + 36, c0=16, c1=24, epi="bias")
    # split16 with pre-split operands: every KMODE_ + 16 / + 32 that is built
    for t in (0, 1):
        bm, bn, bk = TILES_F32[t][:3]
        for pre in (1, 2, 3):
            add("linear", "split16", t, m=bm + 33, n=bn + 36, k0=3 * bk - 24, pre=pre, epi="res")
        add("conv", "split16", t, n=bn + 36, c0=24, pre=2, epi="bias")
        add("tconv", "split16", t, n=bn + 36, c0=24, pre=2, epi="bias")
        add("m3", "split16", t, n=bn + 36, c0=24, pre=2, epi="bias")
        add("ln1", "split16", t, m=bm + 33, n=bn + 36, k0=2 * bk, pre=2)
        add("ln2", "split16", t, m=bm + 33, n=bn + 36, k0=2 * bk, pre=1)
    # the wide forms (tt_gemm_set_wide(2)): their own epilogue arms
    for dt in DT:
        for t in (tiles(dt) if DT[dt] == torch.float32 else WIDE16):
            bm, bn, bk = tile_of(dict(dt=dt, tile=t))[:3]
            add("linear", dt, t, m=bm + 33, n=bn + 36, k0=3 * bk - 24, epi="blend", wide=1)
            add("linear", dt, t, m=(128 if bm == 128 and DT[dt] == torch.float32 else 2) * bm, n=bn + 32, k0=bk - 24,
                epi="bias" if dt == "split16" else "res", stats=bm, srows=bm, wide=1)
            add("conv", dt, t, n=bn + 36, c0=24, epi="res", wide=1)
            add("conv", dt, t, n=bn + 36, c0=24, ups=2, epi="bias", wide=1)
            add("tconv", dt, t, n=bn + 36, c0=24, epi="blend_res", wide=1)
    # the epilogue arms
    for i, t in enumerate(EPI_TILES):
        bm, bn, bk, _, wgm = TILES[t][:5]
        for j, epi in enumerate(EPIS):
            dt = ("bf16", "f16")[(i + j) & 1]
            if epi.startswith("stats"):
                rows = bm // wgm if epi == "stats_wave" else bm
                add("linear", dt, t, m=2 * bm, n=bn + 32, k0=bk - 24, epi={"stats": "bias", "stats_wave": "film", "stats_film_res": "film_res" if bm <= 128 else "film"}[epi],      # (a 256-row tile reads the residual in-pass: no sums)
                    stats=rows, srows=rows)
            else:
                add("linear", dt, t, m=bm + 33, n=_n_for(bn, epi), k0=bk + 8, epi=epi)
    for dt in ("f32", "split16"):                                   # fp32 storage: no fp8 / fp32-out forms; split16 reads every residual in-pass
        for t in (0, 1):
            bm, bn, bk, _, wgm = TILES_F32[t][:5]
            for epi in ("none", "film", "parity", "blend", "short", "res", "blend_res", "geglu", "colpad", "inplace"):
                add("linear", dt, t, m=bm + 33, n=_n_for(bn, epi), k0=bk + 8, epi=epi)
            rows = (128 if t == 0 else 2) * bm
            add("linear", dt, t, m=rows, n=bn + 32, k0=bk - 24, epi="bias", stats=bm, srows=bm)
            add("linear", dt, t, m=rows, n=bn + 32, k0=bk - 24, epi="film", stats=bm // wgm, srows=bm // wgm)
    # the tile order: tiles_n > 8 and a ragged last group of tile rows
    for dt, t in (("bf16", 2), ("f16", 1), ("bf16", 11), ("f16", 3), ("bf16", 7), ("f32", 1)):
        bm, bn = tile_of(dict(dt=dt, tile=t))[:2]
        add("linear", dt, t, m=3 * bm, n=9 * bn + 4, k0=40, epi="bias")
    # split-K by the planner's own choice (one 128 x 128 x 64 tile on the 4-deep ring, 40 / 45 K steps in 5 slices) into the three
    # reduction kernels; slice 1 of the conv starts at K step 9 = tap 1, second source; one launch without its workspace
    for dt in ("bf16", "f16"):
        add("linear", dt, 16, m=100, n=128, k0=2560, epi="film_res", splitk=5)
        add("linear", dt, 16, m=96, n=128, k0=2560, epi="res", splitk=5, stats=48, srows=48)
        add("linear", dt, 16, m=96, n=128, k0=2560, epi="bias", splitk=5, stats=48, gn=1)
        add("conv", dt, 16, n=128, c0=128, c1=192, epi="res", splitk=5)
    add("linear", "bf16", 2, m=100, n=128, k0=2560, epi="res", nows=1)
    add("linear", "split16", 0, m=100, n=128, k0=2560, epi="bias", splitk=5)
    # the streaming 320 x 320 kernel (tt_gemm_set_streaming_square(1)): 260 tiles of 32 rows, the last one ragged
    for dt in ("bf16", "f16"):
        for epi in ("bias", "blend_res", "parity_res"):
            add("sq320", dt, -1, m=32 * 259 + 5, n=320, k0=320, epi=epi)
    return out


def case_id(c):
    return "-".join(f"{k}={v}" for k, v in c.items())


CASES = _cases()


def _u(*shape, seed, dtype=torch.float32, scale=1.7, dev="cuda"):
    """seeded uniform values (unit variance at scale 1.7), rounded through the storage type"""
    n = 1
    for s in shape:
        n *= s
    return (hash_uniform(n, seed, device=dev).view(*shape) * scale).to(dtype)


def _f(t):
    return t.float().cpu()


def _epilogue(case, m, n, dtype, dev):
    """(keyword arguments of ops.gemm, reference epilogue lin -> out, rtol, atol) of the case's operand set"""
    epi = case.get("epi", "none")
    rtol, atol = TOL[case["dt"]]
    kw, bias = {}, None
    if epi != "none":
        bias = _u(n, seed=3, dev=dev)
        kw["bias"] = bias
    rv = res = bl = None
    scale, alpha, per, mod = 1.0, 0.0, 40, 0
    if epi in ("film", "film_mod", "film_res", "short"):
        per, mod = (5 if epi == "short" else 40), (3 if epi == "film_mod" else 0)
        rv = _u(mod if mod else (m + per - 1) // per, n, seed=4, dev=dev)
        kw.update(rowvec=rv, rowvec_rows=per, rowvec_mod=mod)
    if epi in ("parity", "parity_res"):
        per, mod = 1, 2
        rv = _u(2, n, seed=4, dev=dev)
        kw.update(rowvec=rv, rowvec_rows=1, rowvec_mod=2)
    if epi in ("res", "film_res", "blend", "blend_res", "parity_res"):
        res = _u(m, n, seed=5, dtype=dtype, dev=dev)
        kw["residual"] = res
    if epi == "blend":
        bl, alpha, scale = _u(m, n, seed=6, dtype=dtype, dev=dev), 0.3, 0.75
        kw.update(blend=bl, alpha=alpha, acc_scale=scale)
    if epi == "blend_res":
        bl, alpha = res, 0.35
        kw.update(blend=res, alpha=alpha)
    if epi == "fp8":
        kw["out_fp8"] = True
        rtol, atol = 2 ** -4 + 2 * rtol, 2 ** -9 + atol           # (tests/test_ops_gpu.py: one e4m3 rounding on top)
    if epi == "f32out":
        kw["out_f32"] = True
    if epi == "colpad":                                             # column c -> (c // 20) * 24 + c % 20, the gaps stay as they were
        kw.update(out_col_pad=(20, 24), out=torch.zeros((m, n // 20 * 24), dtype=dtype, device=dev))

    def ref(lin):
        v = lin
        if bias is not None:
            v = v + _f(bias)
        v = v * scale
        if rv is not None:
            g = torch.arange(m) // per
            v = v + _f(rv)[g % mod if mod else g]
        if res is not None:
            v = v + _f(res)
        if bl is not None:
            v = alpha * _f(bl) + (1.0 - alpha) * v
        if epi == "fp8":
            v = v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()
        if epi == "colpad":
            v = F.pad(v.view(m, n // 20, 20), (0, 4)).reshape(m, n // 20 * 24)
        return v

    return kw, ref, rtol, atol


def _pre(t, on):
    from this_and_that_vdm_amd.packing import presplit_f32
    return presplit_f32(t) if on else t


def _problem(ops, case, dev):
    """(call: () -> the output of ops.gemm, ref: () -> fp32 reference, hashed: output -> the tensor whose bytes are pinned, rtol, atol)"""
    kind, dtype = case["kind"], DT[case["dt"]]
    pre = case.get("pre", 0)
    hashed = lambda out: out                                                        # noqa: E731
    if kind in ("linear", "sq320"):
        m, n, k0, k1, epi = case["m"], case["n"], case["k0"], case.get("k1", 0), case["epi"]
        n += _wide_n(case, m) if epi not in ("geglu", "colpad") else (_wide_n(case, m) + 79) // 80 * 80
        k = k0 + k1
        w = _u(n, k, seed=2, dtype=dtype, scale=1.7 * k ** -0.5, dev=dev)
        if epi == "inplace":                                                        # strided A, two sources, in place over the residual = blend source
            k1 = 16
            a0, a1 = _u(2 * m, k0, seed=1, dtype=dtype, dev=dev)[0::2], _u(m, k1, seed=7, dtype=dtype, dev=dev)
            w = _u(n, k0 + k1, seed=2, dtype=dtype, scale=1.7 * (k0 + k1) ** -0.5, dev=dev)
            bias, x = _u(n, seed=3, dev=dev), _u(m + 64, n + 16, seed=5, dtype=dtype, dev=dev)
            view = x[32:32 + m, 8:8 + n]
            before = _f(x)
            rtol, atol = TOL[case["dt"]]

            def ref():
                r, xr = before.clone(), before[32:32 + m, 8:8 + n]                  # what lies around the [m, n] window stays as it was
                r[32:32 + m, 8:8 + n] = 0.4 * xr + 0.6 * (torch.cat([_f(a0), _f(a1)], 1) @ _f(w).T + _f(bias) + xr)
                return r
            return (lambda: ops.gemm(a0, w, a1=a1, bias=bias, residual=view, blend=view, alpha=0.4, out=view)), ref, (lambda out: x), rtol, atol
        a0 = _u(m, k0, seed=1, dtype=dtype, dev=dev)
        a1 = _u(m, k1, seed=7, dtype=dtype, dev=dev) if k1 else None
        if epi == "geglu":
            from this_and_that_vdm_amd.packing import pack_geglu
            bias = _u(n, seed=3, dev=dev)
            wp, bp = pack_geglu(w, bias)
            rtol, atol = (5e-3, 5e-3) if dtype == torch.float16 else (TOL[case["dt"]][0], 2 * TOL[case["dt"]][1])      # (tests/test_ops_gpu.py)

            def ref():
                lin = _f(a0) @ _f(w).T + _f(bias)
                return lin[:, :n // 2] * F.gelu(lin[:, n // 2:])
            return (lambda: ops.gemm(a0, wp, bias=bp, geglu=True)), ref, hashed, rtol, atol
        kw, epi_ref, rtol, atol = _epilogue(case, m, n, dtype, dev)
        if case.get("gn"):
            kw["gn"] = (_u(n, seed=11, scale=0.35, dev=dev) + 1, _u(n, seed=12, scale=0.5, dev=dev), 1e-5, True)
        lin = lambda: (torch.cat([_f(a0), _f(a1)], 1) if k1 else _f(a0)) @ _f(w).T     # noqa: E731
        return (lambda: ops.gemm(_pre(a0, pre & 1), _pre(w, pre & 2), a1=a1, stats=case.get("stats", 0), **kw)), (lambda: epi_ref(lin())), hashed, rtol, atol
    if kind in ("ln1", "ln2"):
        from this_and_that_vdm_amd.packing import fold_layernorm, zero_sum_round
        m, n, k = case["m"], case["n"] + _wide_n(case, case["m"]), case["k0"]
        rtol, atol = (2 * t for t in TOL[case["dt"]])                               # (tests/test_ops_gpu.py: folded weights)
        bias = _u(n, seed=3, dev=dev)
        # the LayerNorm rows: sigma 1.5 around means 12 sigma from zero
        rows = lambda r, seed: (_u(r, k, seed=seed, scale=2.6, dev=dev) + 18.0 * (1.0 + 0.1 * _u(r, 1, seed=9, dev=dev))).to(dtype)     # noqa: E731
        g, be = _u(k, seed=7, scale=0.35, dev="cpu") + 1, _u(k, seed=8, scale=0.5, dev="cpu")
        if kind == "ln1":
            a = rows(m, 1)
            wf, bf = fold_layernorm(_u(n, k, seed=2, scale=1.7 * k ** -0.5, dev="cpu"), _f(bias), g, be)
            wq, bf = (zero_sum_round(wf, dtype) if dtype != torch.float32 else wf.float()).to(dev), bf.to(dev)

            def ref():
                x = _f(a)
                return (x @ _f(wq).T) * torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5) + _f(bf)
            return (lambda: ops.gemm(a, _pre(wq, pre & 2), bias=bf, ln_fold=1, ln_eps=1e-5)), ref, hashed, rtol, atol
        # ln2: the rows of W are the LayerNorm inputs (the swapped V^T projection), the rows of A the centred weights
        wt = rows(n, 2)
        af = _u(m, k, seed=1, scale=1.7 * k ** -0.5, dev="cpu")
        af = af - af.mean(1, keepdim=True)
        aq = (zero_sum_round(af, dtype) if dtype != torch.float32 else af.float()).to(dev)

        def ref():
            x = _f(wt)
            return (_f(aq) @ x.T) * torch.rsqrt(x.var(1, unbiased=False) + 1e-5)[None, :] + _f(bias)
        return (lambda: ops.gemm(_pre(aq, pre & 1), wt, bias=bias, ln_fold=2, ln_eps=1e-5)), ref, hashed, rtol, atol
    if kind in ("conv", "m3"):
        from this_and_that_vdm_amd.packing import pack_conv3x3, pack_upsample_phases
        c0, c1, stride, ups = case["c0"], case.get("c1", 0), case.get("stride", 1), case.get("ups", 0)
        nimg, h, wd = (2, 6, 8) if kind == "m3" else (2, 5, 7)
        stride = 2 if kind == "m3" else stride
        if kind == "m3":
            ho, wo = (h + 1 - 3) // 2 + 1, (wd + 1 - 3) // 2 + 1
        elif ups:
            ho, wo = 2 * h, 2 * wd
        else:
            ho, wo = (h + 2 - 3) // stride + 1, (wd + 2 - 3) // stride + 1
        m, c = nimg * ho * wo, c0 + c1
        n = case["n"] + _wide_n(case, nimg * h * wd if ups == 2 else m)
        x0 = _u(nimg * h * wd, c0, seed=1, dtype=dtype, dev=dev)
        x1 = _u(nimg * h * wd, c1, seed=2, dtype=dtype, dev=dev) if c1 else None
        wt = _u(n, c, 3, 3, seed=3, dtype=dtype, scale=1.7 * (9 * c) ** -0.5, dev="cpu")
        wp = (pack_upsample_phases(wt, dtype) if ups == 2 else pack_conv3x3(wt)).to(dev)
        kw, epi_ref, rtol, atol = _epilogue(case, m, n, dtype, dev)

        def ref():
            xin = (torch.cat([_f(x0), _f(x1)], 1) if c1 else _f(x0)).view(nimg, h, wd, c).permute(0, 3, 1, 2)
            if ups == 2:                                                            # on the packed weights the kernel gets: phase (py, px), tap (r, c)
                wph = _f(wp).view(n, 2, 2, 2, 2, c)                                 # reads low-res pixel (y + r - 1 + py, x + c - 1 + px)
                y = torch.zeros(nimg, n, 2 * h, 2 * wd)
                for py in (0, 1):
                    for px in (0, 1):
                        y[:, :, py::2, px::2] = F.conv2d(F.pad(xin, (1 - px, px, 1 - py, py)), wph[:, py, px].permute(0, 3, 1, 2))
            elif kind == "m3":
                y = F.conv2d(F.pad(xin, (0, 1, 0, 1)), wt.float(), None, stride=2)
            else:
                y = F.conv2d(F.interpolate(xin, scale_factor=2, mode="nearest") if ups else xin, wt.float(), None, stride=stride, padding=1)
            return epi_ref(y.permute(0, 2, 3, 1).reshape(m, n))
        return (lambda: ops.gemm(x0, _pre(wp, pre & 2), a1=x1, mode=3 if kind == "m3" else 1, conv=(nimg, h, wd, ho, wo, stride, ups), **kw)), ref, hashed, rtol, atol
    assert kind == "tconv"
    from this_and_that_vdm_amd.packing import pack_tconv3
    b, f, hw, c0, c1 = 2, 3, 40, case["c0"], case.get("c1", 0)
    m, c = b * f * hw, c0 + c1
    n = case["n"] + _wide_n(case, m)
    x0 = _u(m, c0, seed=1, dtype=dtype, dev=dev)
    x1 = _u(m, c1, seed=2, dtype=dtype, dev=dev) if c1 else None
    wt = _u(n, c, 3, 1, 1, seed=3, dtype=dtype, scale=1.7 * (3 * c) ** -0.5, dev="cpu")
    kw, epi_ref, rtol, atol = _epilogue(case, m, n, dtype, dev)

    def ref():
        xin = (torch.cat([_f(x0), _f(x1)], 1) if c1 else _f(x0)).view(b, f, hw, 1, c).permute(0, 4, 1, 2, 3)
        return epi_ref(F.conv3d(xin, wt.float(), None, padding=(1, 0, 0))[..., 0].permute(0, 2, 3, 1).reshape(m, n))
    return (lambda: ops.gemm(x0, _pre(pack_tconv3(wt).to(dev), pre & 2), a1=x1, mode=2, tconv=(f, hw), **kw)), ref, hashed, rtol, atol


@contextlib.contextmanager
def knobs(ops, case):
    """the library's switches of the case, restored on the way out"""
    lib = ops._lib.load()
    split_was, ws_bytes = ops.f32_split(), lib.tt_gemm_ws_bytes
    try:
        ops.set_f32_split(case["dt"] == "split16")
        if DT[case["dt"]] != torch.float32 and case["tile"] >= 0 and not case.get("splitk") and not case.get("nows"):
            lib.tt_gemm_set_tile_override(case["tile"])
        if case.get("wide"):
            lib.tt_gemm_set_wide(2)
        if case["kind"] == "sq320":
            lib.tt_gemm_set_streaming_square(1)
        if case.get("nows"):                                                       # the caller hands over no workspace: the plan falls back to the un-split one
            lib.tt_gemm_ws_bytes = lambda g: 0
        yield lib
    finally:
        lib.tt_gemm_ws_bytes = ws_bytes
        lib.tt_gemm_set_streaming_square(2)
        lib.tt_gemm_set_wide(1)
        lib.tt_gemm_set_tile_override(-1)
        ops.set_f32_split(split_was)


def run_case(ops, case):
    call, ref, hashed, rtol, atol = _problem(ops, case, "cuda")
    with knobs(ops, case):
        ops.PROFILE = []
        try:
            out = call()
            torch.cuda.synchronize()
            name = ops.PROFILE[0][0]
        finally:
            ops.PROFILE = None
    assert name == kernel_of(case), f"the planner moved this case to {name} (expected {kernel_of(case)})"
    extra = []
    if case.get("gn"):                                              # the reduction pass also wrote SiLU(GroupNorm(out)), from the stored values
        gn = getattr(out, "_tt_gn", None)
        assert gn is not None, "no GroupNorm in the reduction pass"
        seg, n = case["stats"], out.shape[1]
        gamma, beta = _u(n, seed=11, scale=0.35) + 1, _u(n, seed=12, scale=0.5)
        x = out.float().view(-1, seg, 32, n // 32)
        mean, var = x.mean((1, 3), keepdim=True), x.var((1, 3), unbiased=False, keepdim=True)
        want = F.silu(((x - mean) * torch.rsqrt(var + 1e-5)).view(-1, n) * gamma + beta)
        torch.testing.assert_close(gn[0].float(), want, rtol=TOL[case["dt"]][0], atol=TOL[case["dt"]][1])
        extra.append(gn[0])
    elif case.get("stats"):
        st = getattr(out, "_tt_stats", None)
        assert st is not None and st[1] == case["srows"], f"no tile sums, or not on tiles of {case['srows']} rows: {st and st[1]}"
        xs, n = out.float(), out.shape[1]
        want = torch.stack([xs.view(-1, st[1], n).sum(1), (xs * xs).view(-1, st[1], n).sum(1)], 1)
        torch.testing.assert_close(st[0], want, rtol=2e-5, atol=2e-4)      # (tests/test_ops_gpu.py's bound for the tile sums)
        extra.append(st[0])
    return hashed(out), extra, ref(), rtol, atol


def plan_case(ops, case):
    """CPU: (rc and cfg[0..6] of tt_gemm_plan, rc and name of tt_gemm_kernel) for the TtGemmArgs ops.gemm builds for the case -- the same
    code as on the GPU with CPU tensors, the launch itself replaced by a stub (the queries look at pointers, never through them)"""
    lib = ops._lib.load()
    seen = []

    def launch(gref, stream):
        g = type(gref._obj)()
        C.memmove(C.byref(g), gref, C.sizeof(g))
        seen.append(g)
        return 0
    saved = ops._p, ops._stream, ops._workspace, lib.tt_gemm
    ops._p = lambda t: None if t is None else t.data_ptr()
    ops._stream = lambda: None
    ops._workspace = lambda nbytes, device: torch.empty(nbytes, dtype=torch.uint8)
    lib.tt_gemm = launch
    try:
        call = _problem(ops, case, "cpu")[0]
        with knobs(ops, case):
            call()
            g, cfg, buf = seen[0], (C.c_int32 * 7)(), C.create_string_buffer(96)
            rc = lib.tt_gemm_plan(C.byref(g), cfg)
            rc_name = lib.tt_gemm_kernel(C.byref(g), buf, len(buf))
    finally:
        ops._p, ops._stream, ops._workspace, lib.tt_gemm = saved
    return [rc] + list(cfg), [rc_name, buf.value.decode()]


def output_hash(out, extra=()):
    """sha256 of the pinned bytes: the stored output (or the buffer it was written into) and the tile sums / normalised copy with it"""
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (out,) + tuple(extra):
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()
