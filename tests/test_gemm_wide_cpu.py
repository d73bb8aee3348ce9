"""CPU: the host side of tt_gemm's wide route (operands of 2 GiB and more on windowed descriptors; include/ttvdm.h "Operand sizes").
Fake pointers throughout: every call here either answers from the planner or is refused before a launch.  The refusals are tt_gemm's:
tt_gemm_plan / tt_gemm_ws_bytes / tt_gemm_stats_rows / tt_gemm_gn_fused keep the answers tests/golden/gemm_route_census.json records for
problems of such sizes (they never refused for an operand's size), so a refused problem is told apart by tt_gemm's return code."""
import ctypes as C
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TT_EUNSUPPORTED = -2
G2 = 1 << 31


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    yield lib
    lib.tt_gemm_set_wide(1)
    lib.tt_gemm_set_f32_split(0)


def _es(dtype):
    return 4 if dtype == 2 else 2


def _problem(mode, dtype, *, upsample=0):
    """the small problems of tests/test_gemm_wide_gpu.py with compact strides: (args, input rows)"""
    from this_and_that_vdm_amd._lib import TtGemmArgs
    g = TtGemmArgs()
    g.mode, g.dtype = mode, dtype
    if mode == 0:
        g.m, g.n, g.k0 = 300, 136, 128
        rows, kw = g.m, g.k0
    elif mode == 1:
        g.nimg, g.hin, g.win, g.stride, g.upsample = 24, 4, 6, 1, upsample
        g.hout, g.wout = (8, 12) if upsample else (4, 6)
        g.m, g.n, g.k0 = g.nimg * g.hout * g.wout, 64, 64
        rows, kw = g.nimg * g.hin * g.win, (16 if upsample == 2 else 9) * g.k0
    else:
        g.frames, g.hw = 5, 40
        g.m, g.n, g.k0 = 3 * 5 * 40, 64, 64
        rows, kw = g.m, 3 * g.k0
    g.a0, g.lda0 = 0x10000, g.k0
    g.w, g.ldw = 0x20000, kw
    g.out, g.ldo = 0x30000, g.n
    g.acc_scale = 1.0
    return g, rows


def _stride_past_2g(rows, dtype):
    """smallest row stride (elements, multiple of 8) with which `rows` rows span 2 GiB or more"""
    ld = -(-G2 // ((rows - 1) * _es(dtype)))
    return (ld + 7) // 8 * 8 + 8


def _plan(lib, g):
    cfg = (C.c_int32 * 7)()
    rc = lib.tt_gemm_plan(C.byref(g), cfg)
    return rc, tuple(cfg)


CASES = [(0, 0), (1, 0), (1, 1), (1, 2), (2, 0)]          # (mode, upsample)


# (the phase-packed upsampling conv has a bias-only epilogue: no residual case)
STRIDED = [(m, u, o) for m, u in CASES for o in ("a0", "out", "residual") if not (u == 2 and o == "residual")]


@pytest.mark.parametrize("dtype", [0, 1, 2])
@pytest.mark.parametrize("mode,upsample,operand", STRIDED)
def test_a_strided_operand_of_2_gib_plans_wide_on_the_compact_problems_tile(lib, mode, upsample, operand, dtype):
    lib.tt_gemm_set_wide(1)
    g, rows = _problem(mode, dtype, upsample=upsample)
    rc, compact = _plan(lib, g)
    assert rc == 0 and lib.tt_gemm_is_wide(C.byref(g)) == 0         # a compact problem stays narrow under the default
    if operand == "a0":
        g.lda0 = _stride_past_2g(rows, dtype)
    elif operand == "out":
        g.ldo = _stride_past_2g(g.m, dtype)
    else:
        g.residual, g.ld_res = 0x40000, _stride_past_2g(g.m, dtype)
        rc, compact = _plan(lib, _with_residual(_problem(mode, dtype, upsample=upsample)[0]))
        assert rc == 0
    rc, wide = _plan(lib, g)
    assert rc == 0, lib.tt_last_error()
    assert lib.tt_gemm_is_wide(C.byref(g)) == 1
    assert wide == compact and wide[6] == 1, (wide, compact)
    assert lib.tt_gemm_ws_bytes(C.byref(g)) == 0 and lib.tt_gemm_gn_fused(C.byref(g)) == 0
    c, _ = _problem(mode, dtype, upsample=upsample)                  # the statistics epilogue: the compact problem's answer
    if operand == "residual":
        _with_residual(c)
    assert lib.tt_gemm_stats_rows(C.byref(g)) == lib.tt_gemm_stats_rows(C.byref(c))
    # tt_gemm_set_wide(0): the refusal from before the route existed
    try:
        lib.tt_gemm_set_wide(0)
        assert lib.tt_gemm_is_wide(C.byref(g)) == 0
        assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED
        want = b"tt_gemm: operand larger than 2 GiB (32-bit buffer offsets)" if operand == "a0" else \
            b"tt_gemm: epilogue operand larger than 2 GiB (32-bit buffer offsets)"
        assert lib.tt_last_error() == want
    finally:
        lib.tt_gemm_set_wide(1)


def _with_residual(g):
    g.residual, g.ld_res = 0x40000, g.n
    return g


@pytest.mark.parametrize("dtype,frames,tile", [(0, 8, (128, 128, 64, 2, 4, 2)), (1, 14, (128, 128, 64, 2, 4, 2)), (2, 4, (128, 128, 32, 2, 2, 2))])
def test_the_decoders_launches_at_576x1024_plan_wide(lib, dtype, frames, tile):
    """the third up block's upsampling conv (256 channels out at 576x1024), the 3x3 conv and the frame conv that read its output"""
    from this_and_that_vdm_amd._lib import TtGemmArgs
    lib.tt_gemm_set_wide(1)
    h, w, c = 576, 1024, 256
    for split in ((0, 1) if dtype == 2 else (0,)):
        lib.tt_gemm_set_f32_split(split)
        try:
            up = TtGemmArgs()
            up.mode, up.dtype, up.nimg, up.hin, up.win, up.hout, up.wout, up.stride, up.upsample = 1, dtype, frames, h // 2, w // 2, h, w, 1, 2
            up.m, up.n, up.k0 = frames * h * w, c, c
            up.a0, up.lda0, up.w, up.ldw, up.out, up.ldo, up.acc_scale = 0x10000, c, 0x20000, 16 * c, 0x30000, c, 1.0
            conv = TtGemmArgs()
            conv.mode, conv.dtype, conv.nimg, conv.hin, conv.win, conv.hout, conv.wout, conv.stride = 1, dtype, frames, h, w, h, w, 1
            conv.m, conv.n, conv.k0 = frames * h * w, 128, c
            conv.a0, conv.lda0, conv.w, conv.ldw, conv.out, conv.ldo, conv.acc_scale = 0x10000, c, 0x20000, 9 * c, 0x30000, 128, 1.0
            tconv = TtGemmArgs()
            tconv.mode, tconv.dtype, tconv.frames, tconv.hw = 2, dtype, frames, h * w
            tconv.m, tconv.n, tconv.k0 = frames * h * w, c, c
            tconv.a0, tconv.lda0, tconv.w, tconv.ldw, tconv.out, tconv.ldo, tconv.acc_scale = 0x10000, c, 0x20000, 3 * c, 0x30000, c, 1.0
            tconv.residual = tconv.blend = 0x40000
            tconv.ld_res = tconv.ld_blend = c
            tconv.alpha = 0.25
            short = TtGemmArgs()                                     # the 1 x 1 shortcut: by its shape the persistent kernel's (16-bit)
            short.mode, short.dtype, short.m, short.n, short.k0 = 0, dtype, frames * h * w, 128, c
            short.a0, short.lda0, short.w, short.ldw, short.out, short.ldo, short.acc_scale = 0x10000, c, 0x20000, c, 0x30000, 128, 1.0
            for g in (up, conv, tconv, short):
                rc, cfg = _plan(lib, g)
                assert rc == 0, lib.tt_last_error()
                assert lib.tt_gemm_is_wide(C.byref(g)) == 1 and cfg[:6] == tile and cfg[6] == 1, cfg
        finally:
            lib.tt_gemm_set_f32_split(0)


def test_set_wide_2_takes_what_the_wide_kernels_serve_without_changing_the_plan(lib):
    try:
        for mode, upsample in CASES:
            for dtype in (0, 1, 2):
                g, _ = _problem(mode, dtype, upsample=upsample)
                lib.tt_gemm_set_wide(1)
                rc, narrow = _plan(lib, g)
                assert rc == 0 and lib.tt_gemm_is_wide(C.byref(g)) == 0
                lib.tt_gemm_set_wide(2)
                rc, wide = _plan(lib, g)
                assert rc == 0 and lib.tt_gemm_is_wide(C.byref(g)) == 1 and wide == narrow, (mode, upsample, dtype, wide, narrow)
        # not served: stays narrow (a GEGLU projection; a tile shape without a wide variant; a split-K plan with its workspace)
        lib.tt_gemm_set_wide(2)
        g, _ = _problem(0, 0)
        g.geglu = 1
        assert lib.tt_gemm_is_wide(C.byref(g)) == 0
        g, _ = _problem(0, 0)
        g.m, g.n = 64, 4096                                          # the 64 x 64 tile of the <= 64-row tails
        assert _plan(lib, g)[1][:2] == (64, 64) and lib.tt_gemm_is_wide(C.byref(g)) == 0
        g, _ = _problem(1, 0)
        g.nimg, g.hin, g.win, g.hout, g.wout, g.k0, g.lda0, g.n, g.ldw, g.ldo = 1, 28, 28, 28, 28, 1280, 1280, 1280, 9 * 1280, 1280
        g.m = 784
        need = lib.tt_gemm_ws_bytes(C.byref(g))
        assert need > 0
        g.ws, g.ws_bytes = 0x50000, need
        assert _plan(lib, g)[1][6] > 1 and lib.tt_gemm_is_wide(C.byref(g)) == 0
        assert lib.tt_gemm_set_wide(3) == -1 and lib.tt_gemm_set_wide(-1) == -1
    finally:
        lib.tt_gemm_set_wide(1)


def test_a_window_of_2_gib_is_refused_by_name(lib):
    lib.tt_gemm_set_wide(1)
    g, _ = _problem(0, 0)
    g.lda0 = 1 << 25                                                 # 128 rows of a tile: 127 * 2^25 * 2 bytes = 8.5 GB
    assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED
    msg = lib.tt_last_error().decode()
    assert "window" in msg and "a0" in msg and "128 rows" in msg and str((127 * (1 << 25) + 128) * 2) in msg, msg
    assert lib.tt_gemm_is_wide(C.byref(g)) == 0
    g, _ = _problem(0, 2)
    g.ldo = 1 << 24                                                  # TT_F32: 63 * 2^24 * 4 bytes on the 64 x 64 tile
    assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED
    assert "window" in lib.tt_last_error().decode() and "out" in lib.tt_last_error().decode() and "64 rows" in lib.tt_last_error().decode()
    # mode 1: a tile's window is the images its rows lie in -- seven of these 24-row images for a 128-row tile
    g, rows = _problem(1, 0)
    g.lda0 = 1 << 23
    assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED and "168 rows" in lib.tt_last_error().decode(), lib.tt_last_error()
    # mode 2: the tile's rows and one frame either side
    g, rows = _problem(2, 0)
    g.lda0 = 1 << 23
    assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED and "208 rows" in lib.tt_last_error().decode(), lib.tt_last_error()


def _unserved():
    def a1(g):
        g.a1, g.k1, g.lda1 = 0x60000, 64, 64
        g.ldw += 64
    def geglu(g):
        g.geglu = 1
    def ln_fold(g):
        g.ln_fold, g.ln_eps = 1, 1e-5
    def rowvec(g):
        g.rowvec, g.rowvec_rows, g.ld_rowvec = 0x70000, 100, 136
    def gn_out(g):
        g.gn_out, g.ld_gn, g.gn_gamma, g.gn_beta, g.stats_seg = 0x80000, 136, 0x81000, 0x82000, 100
    def out_fp8(g):
        g.out_fp8 = 1
    def out_col_hw(g):
        g.out_col_hw, g.out_col_hwp = 34, 40
    def presplit(g):
        g.presplit = 2
    return [(a1, "a second source"), (geglu, "geglu"), (ln_fold, "ln_fold"), (rowvec, "rowvec"), (gn_out, "gn_out"),
            (out_fp8, "out_fp8"), (out_col_hw, "out_col_hw"), (presplit, "presplit")]


@pytest.mark.parametrize("setter,name", _unserved(), ids=[n for _, n in _unserved()])
def test_unserved_terms_are_refused_by_name(lib, setter, name):
    lib.tt_gemm_set_wide(1)
    g, rows = _problem(0, 2 if name == "presplit" else 0)
    n0 = g.n
    g.n = 144 if name == "geglu" else n0                             # geglu: n % 16 == 0
    setter(g)
    g.lda0 = _stride_past_2g(rows, g.dtype)
    assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED and name in lib.tt_last_error().decode(), lib.tt_last_error()
    assert lib.tt_gemm_is_wide(C.byref(g)) == 0


def test_an_output_of_2_gib_on_the_persistent_kernels_plan_keeps_that_plan_and_its_refusal(lib):
    lib.tt_gemm_set_wide(1)
    g, _ = _problem(0, 0)
    g.m, g.n, g.k0, g.lda0, g.ldw, g.ldo = 200704, 10240, 320, 320, 320, 10240      # 4.1 GB of output, 31 360 tiles of 256 x 256
    rc, cfg = _plan(lib, g)
    assert rc == 0 and cfg[:6] == (256, 256, 64, 0, 2, 4) and lib.tt_gemm_is_wide(C.byref(g)) == 0
    assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED
    assert lib.tt_last_error() == b"tt_gemm: epilogue operand larger than 2 GiB (32-bit buffer offsets)"


def test_mode_3_and_w_stay_refused(lib):
    from this_and_that_vdm_amd._lib import TtGemmArgs
    lib.tt_gemm_set_wide(1)
    g = TtGemmArgs()
    g.mode, g.dtype, g.nimg, g.hin, g.win, g.hout, g.wout, g.stride = 3, 0, 2, 32, 32, 16, 16, 2
    g.m, g.n, g.k0, g.acc_scale = 2 * 16 * 16, 64, 64, 1.0
    g.a0, g.lda0, g.w, g.ldw, g.out, g.ldo = 0x10000, _stride_past_2g(2 * 32 * 32, 0), 0x20000, 9 * 64, 0x30000, 64
    assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED and "mode 3" in lib.tt_last_error().decode()
    g, _ = _problem(0, 0)
    g.ldw = _stride_past_2g(g.n, 0)                                  # W of 2 GiB or more: the refusal it always had
    assert lib.tt_gemm_is_wide(C.byref(g)) == 0
    assert lib.tt_gemm(C.byref(g), None) == TT_EUNSUPPORTED
    assert lib.tt_last_error() == b"tt_gemm: operand larger than 2 GiB (32-bit buffer offsets)"


def test_abi_is_11_and_header_and_binding_agree_on_the_new_symbols(lib):
    from this_and_that_vdm_amd import _lib, ops
    assert lib.tt_abi_version() == 11
    text = open(os.path.join(REPO, "include", "ttvdm.h")).read()
    assert re.search(r"^int32_t tt_gemm_is_wide\(const TtGemmArgs\* args\);", text, re.M)
    assert re.search(r"^int tt_gemm_set_wide\(int32_t on\);", text, re.M)
    assert _lib.SIGNATURES["tt_gemm_is_wide"] == (C.c_int32, [C.POINTER(_lib.TtGemmArgs)])
    assert _lib.SIGNATURES["tt_gemm_set_wide"] == (C.c_int, [C.c_int32])
    assert callable(ops.set_gemm_wide)
