"""The cases of tests/test_groupnorm_bits_gpu.py, shared with tests/golden/make_groupnorm_bits.py (which records their output hashes from
the library of the commit that is the reference).  The GroupNorm kernels of norm.hip are built from shared pieces (gn_source, gn_row_sums,
gn_combine_group32, gn_group_stat, gn_affine8, gn_apply8 / gn_apply_rows), so every case is the smallest shape that reaches
both the unrolled loop and the tail of a loop one of those pieces holds -- the bound tests of tests/test_norm_bounds_gpu.py mostly stay in
the tails at C = 320 -- on every route, in every storage type the route serves, below the conditioning guard (rho = 0) and above it
(rho = 50: every group is recomputed centred, the constant group included), with SiLU off and on.  The derivation stands beside each case.

run_case(ops, case) -> {output name: (sha256 of its bytes, err/bound against the fp64 reference of tests/error_bounds.py, or None for the
fp32 scale / shift tables)}.  It asserts the route of every launch through ops.NORM_TRACE, as tests/test_norm_bounds_gpu.py does, and takes
the launch-geometry replicas (image_adds, grouped_adds, PARTIAL_ADDS), the producers (TILE_CASES, GN_OUT_CASES, produce) and the inputs
(eb.norm_input, eb.ln_input, eb.norm_affine) from there: one definition of each."""
import hashlib

import torch

from tests import error_bounds as eb
from tests.test_norm_bounds_gpu import EPS, GN_OUT_CASES, PARTIAL_ADDS, TILE_CASES, grouped_adds, image_adds, produce, tag, traced

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
ALL, HALF = ("bf16", "f16", "f32"), ("bf16", "f16")
RHOS = (0, 50)                     # below the guard of every route / above it on every route (GN_GUARD_RATIO = 64 is rho = 8, _TILES = 4 is rho = 1.7)

# ---- gn_stats_image_kernel through ops.groupnorm: (c0, c1, h, w), 5 images.  Row lanes rpb = min(1024 / (C / 8), LDS limit, hw).
IMAGE_SHAPES = [(320, 0, 15, 15),          # rpb = 25, hw = 225 = 9 rows per lane: gn_row_sums runs its 8-deep round once, then one tail row, in every
                                           # lane; the 4 apply parts are rows [0, 56), [56, 112), [112, 168), [168, 225): ragged against 25 lanes
                (64, 32, 5, 3),            # cpg = 3: group 21 straddles the two sources (gn_source per vector, gn_centred_group per channel); rpb = 15 = hw: tail only
                (1280, 1280, 4, 7)]        # rpb = 3 (320 vectors per row), 28 rows: 8-deep round once (r + 21 < 28), then the tail
# ---- gn_group_kernel: 9 images (the second round of the XCD mapping holds one image).  gpb = 4 at all three; rlanes = min(512 / nv, hw)
GROUP_SHAPES = [(640, 320, 16, 28),        # 15 vectors, 34 row lanes, 448 rows: 8 x 34 = 272 < 448 and 4 x 34 = 136 < 448: both unrolled loops, both tails;
                                           # slice 5 of 8 (channels 600 .. 719) straddles the sources
                (320, 0, 30, 30),          # 5 vectors, 102 row lanes, 900 rows: 816 < 900, one 8-deep round in every lane, a tail row in 84 of them
                (320, 0, 16, 16)]          # 256 rows, the lower edge of the route: tails only
# ---- gn_partial_kernel + gn_finalize_kernel + gn_apply_kernel, called directly: (c0, c1, h, w), frames per group, images
PARTIAL_SHAPES = [((320, 0, 40, 56), 1, 2),        # 6 row lanes, 48-row chunks: two 4-deep rounds per lane; the last of 47 chunks has 32 rows: one round, then the tail
                  ((320, 0, 9, 11), 4, 8),         # 99 rows: chunks of 48, 48 and 3 rows (tail only, three lanes)
                  ((320, 0, 40, 28), 14, 28),      # 14 frames x 24 chunks = 336 partials per group set > 8 x 32: gn_finalize_kernel's 8-deep loop and its tail
                  ((64, 32, 9, 11), 2, 4)]         # two sources, cpg = 3; 21 row lanes, one 99-row chunk: one 4-deep round (r + 63 < 99), then the tail
# ---- gn_tiles_kernel behind a producer of TILE_CASES: name -> (producer, frames per group, storage types)
TILE_LONG = dict(rows=16384, k=256, n=640, mode=0, hw=256, per_image=True)      # 64 segments of 256 rows; 16-bit: gpb = 4, 10 vectors, parts = 1 and 51 row
#                                                                                 lanes: 4 x 51 = 204 < 256, gn_apply_rows<4> runs its round and its tail
TILES = dict(tiled_linear_fpg1=("tiled_linear", 1, ALL), tiled_linear_fpg4=("tiled_linear", 4, ALL),       # as they stand in TILE_CASES: tail only
             tiled_small_fpg1=("tiled_small", 1, ALL), tiled_small_fpg4=("tiled_small", 4, ALL),           # cpg = 3
             tiled_long=(TILE_LONG, 1, ALL),
             splitk_conv_l3_fpg14=("splitk_conv_l3", 14, HALF))                                            # tile sums of splitk_epilogue_stats_kernel, 392-row segments


def _cases():
    out = []
    for rho in RHOS:
        out += [dict(kind="image", shape=s, dt=dt, rho=rho) for s in IMAGE_SHAPES for dt in ALL]
        out += [dict(kind="image_stats", shape=IMAGE_SHAPES[0], dt=dt, rho=rho) for dt in ALL]      # y == nullptr: scale / shift out, then gn_apply_kernel
        out += [dict(kind="group", shape=s, dt=dt, rho=rho) for s in GROUP_SHAPES for dt in ALL]
        out += [dict(kind="cross", dt=dt, rho=rho) for dt in ALL]
        out += [dict(kind="partial", shape=s, fpg=f, nimg=n, dt=dt, rho=rho) for s, f, n in PARTIAL_SHAPES for dt in ALL]
        out += [dict(kind="tiles", name=name, dt=dt, rho=rho) for name, (_, _, dts) in TILES.items() for dt in dts]
        out += [dict(kind="gn_out", name=name, dt=dt, rho=rho) for name in GN_OUT_CASES for dt in HALF]
        out += [dict(kind="ln", c=c, dt=dt, rho=rho) for c in (64, 320, 1280) for dt in ALL]       # MAXV = 1, 1, 4 ... and 2 below
        out += [dict(kind="ln", c=1024, dt=dt, rho=rho) for dt in ALL]                             # 128 vectors per row: ln_kernel<Tag, 2>
    return out


def case_id(c):
    return "-".join(f"{k}={'x'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in c.items())


CASES = _cases()


def output_hash(out):
    torch.cuda.synchronize()
    return hashlib.sha256(out.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _affine(c, seed):
    gamma, beta = eb.norm_affine(c, seed)
    return gamma.cuda(), beta.cuda()


def _entry(got, bound, dtype):
    return output_hash(got), (eb.ratio(got, bound, dtype) if bound is not None else None)


def _both_silu(ops, res, call, names, bound):
    """y and y_silu of call(silu) -> tensor, each through exactly the launches `names`"""
    for silu in (False, True):
        y, seen = traced(ops, lambda: call(silu))
        assert seen == names, (seen, names)
        res["y_silu" if silu else "y"] = _entry(y, bound(silu), y.dtype)


def run_case(ops, case):
    kind, dtype, rho = case["kind"], DT[case["dt"]], case["rho"]
    t = tag(ops, dtype)
    res = {}
    if kind in ("image", "group"):
        c0, c1, h, w = case["shape"]
        c, hw = c0 + c1, h * w
        nimg = 5 if kind == "image" else 9
        kernel = "gn_stats_image_kernel" if kind == "image" else "gn_group_kernel"
        n_adds = image_adds(c, hw) if kind == "image" else grouped_adds(c, hw, dtype)
        gamma, beta = _affine(c, 7)
        x = eb.norm_input(nimg, hw, c, rho, dtype, 11, device="cuda")
        x0, x1 = x[:, :c0].contiguous(), (x[:, c0:].contiguous() if c1 else None)
        _both_silu(ops, res, lambda silu: ops.groupnorm(x0, x1, nimg, hw, 1, gamma, beta, EPS, silu), [f"{kernel}<{t}>"],
                   lambda silu: eb.groupnorm(x, gamma, beta, EPS, seg_rows=hw, silu=silu, n_adds=n_adds, guard=eb.GN_GUARD_RATIO))
    elif kind == "cross":                                   # test_groupnorm_cross_frame_one_launch's: a video of 14 x 28 = 392 rows is one image of
        c, frames, hw, videos = 1280, 14, 4 * 7, 3          # gn_group_kernel (16-bit: gpb = 2, 10 vectors, 51 row lanes: 8 x 51 = 408 > 392, 4 x 51 = 204 < 392)
        gamma, beta = _affine(c, 9)
        x = eb.norm_input(videos, frames * hw, c, rho, dtype, 13, device="cuda")

        def call(silu):
            keep, ops.GN_CROSS_MAX_ROWS = ops.GN_CROSS_MAX_ROWS, 512
            try:
                return ops.groupnorm(x, None, videos * frames, hw, frames, gamma, beta, EPS, silu)
            finally:
                ops.GN_CROSS_MAX_ROWS = keep
        _both_silu(ops, res, call, [f"gn_group_kernel<{t}>"],
                   lambda silu: eb.groupnorm(x, gamma, beta, EPS, seg_rows=frames * hw, silu=silu, n_adds=grouped_adds(c, frames * hw, dtype),
                                             guard=eb.GN_GUARD_RATIO))
    elif kind in ("partial", "image_stats"):
        c0, c1, h, w = case["shape"]
        c, hw = c0 + c1, h * w
        fpg, nimg = (case["fpg"], case["nimg"]) if kind == "partial" else (1, 5)
        route, n_adds = ("gn_partial_kernel + gn_finalize_kernel", PARTIAL_ADDS) if kind == "partial" else ("gn_stats_image_kernel", image_adds(c, hw))
        gamma, beta = _affine(c, 8)
        x = eb.norm_input(nimg // fpg, fpg * hw, c, rho, dtype, 12, device="cuda")
        x0, x1 = x[:, :c0].contiguous(), (x[:, c0:].contiguous() if c1 else None)
        (sc, sh), seen = traced(ops, lambda: ops.groupnorm_stats(x0, x1, nimg, hw, fpg, gamma, beta, EPS))
        assert seen == [f"{route}<{t}>"], seen
        res["scale"], res["shift"] = _entry(sc, None, None), _entry(sh, None, None)
        _both_silu(ops, res, lambda silu: ops.groupnorm_apply(x0, x1, nimg, hw, sc, sh, silu), [f"gn_apply_kernel<{t}>"],
                   lambda silu: eb.groupnorm(x, gamma, beta, EPS, seg_rows=fpg * hw, silu=silu, n_adds=n_adds, guard=eb.GN_GUARD_RATIO))
    elif kind == "tiles":
        g, fpg, _ = TILES[case["name"]]
        g = TILE_CASES[g] if isinstance(g, str) else g
        n = g["n"]
        if g["mode"] == 0:
            rows = g["rows"]
            hw = g.get("hw") or (rows // 28 if rows % 28 == 0 else rows // 8)          # (test_groupnorm_from_producer_tile_sums's image height)
        else:
            hw = g["h"] * g["w"]
            rows = g["nimg"] * hw
        nimg, seg = rows // hw, fpg * hw
        seg0 = hw if g.get("per_image") else g["frames"] * hw                          # the segment the producer is told about
        gamma, beta = _affine(n, 10)
        assert ops.GN_TILES and ops.GN_TILES_SEG, "the producer hand-off is the default route"
        x = eb.norm_input(rows // seg0, seg0, n, rho, dtype, 14, device="cuda")
        out, name, cfg = produce(ops, g, x, seg0)           # zero weight, x as residual: the stored output is x
        st = getattr(out, "_tt_stats", None)
        assert st is not None and seg % st[1] == 0 and torch.equal(out, x), (case, name, cfg)
        _both_silu(ops, res, lambda silu: ops.groupnorm(out, None, nimg, hw, fpg, gamma, beta, EPS, silu), [f"gn_tiles_kernel<{t}>"],
                   lambda silu: eb.groupnorm(out, gamma, beta, EPS, seg_rows=seg, silu=silu, n_adds=st[1], guard=eb.GN_GUARD_RATIO_TILES))
    elif kind == "gn_out":                                  # splitk_epilogue_gn_kernel: gn_group_stat without the guard, sums in fp64 (n_adds = 0)
        g = GN_OUT_CASES[case["name"]]
        hw, n, fpg, nimg = g["h"] * g["w"], g["n"], g["fpg"], g["nimg"]
        seg = fpg * hw
        gamma, beta = _affine(n, 15)
        assert ops.GN_FUSED
        x = eb.norm_input(nimg // fpg, seg, n, rho, dtype, 16, device="cuda")
        for silu in (False, True):
            out, name, cfg = produce(ops, g, x, seg, gn=(gamma, beta, EPS, silu))
            fz = getattr(out, "_tt_gn", None)
            assert fz is not None and cfg[6] >= 2, f"no split-K reduction pass on this plan ({name}, {cfg})"
            y, seen = traced(ops, lambda: ops.groupnorm(out, None, nimg, hw, fpg, gamma, beta, EPS, silu))
            assert seen == [] and y.data_ptr() == fz[0].data_ptr() and torch.equal(out, x)
            res["y_silu" if silu else "y"] = _entry(y, eb.groupnorm(out, gamma, beta, EPS, seg_rows=seg, silu=silu), dtype)
    else:                                                   # ln_kernel: untouched arithmetic (its instruction stream is the parent's); pins the dtype x MAXV dispatch
        c, rows = case["c"], 37 * 6
        gamma, beta = _affine(c, 17)
        emb = (torch.randn(3, c, generator=torch.Generator().manual_seed(18)) * 0.125).cuda()
        x = eb.ln_input(rows, c, rho, dtype, 19).cuda()
        y, seen = traced(ops, lambda: ops.layernorm(x, gamma, beta, EPS))
        assert seen == [f"ln_kernel<{t}>"], seen
        res["y"] = _entry(y, eb.layernorm(x, gamma, beta, EPS, n_adds=eb.ln_adds(c)), dtype)
        (xs, y2), seen = traced(ops, lambda: ops.layernorm(x, gamma, beta, EPS, rowvec=emb, rows_per_vec=37, nvec=3))
        assert seen == [f"ln_kernel<{t}>"], seen
        res["xsum"] = _entry(xs, None, None)
        res["y_rowvec"] = _entry(y2, eb.layernorm(xs, gamma, beta, EPS, n_adds=eb.ln_adds(c)), dtype)       # normalises the STORED sum
    return res
