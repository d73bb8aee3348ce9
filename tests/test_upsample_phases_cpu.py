"""CPU: the phase pack of the nearest-x2 upsampling conv (packing.pack_upsample_phases) and the host side of tt_gemm's
``upsample = 2``: the packing identity in fp64, the one rounding of the stored pack, what tt_gemm_plan / tt_gemm accept and refuse,
and the unchanged ABI."""
import ctypes as C

import pytest
import torch

from tests.upsample_phases_ref import phase_conv, summed_taps, upsample_conv

TT_EINVAL = -1                      # include/ttvdm.h


@pytest.fixture(scope="module")
def lib():
    import os
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("nimg,cin,cout,h,w", [(2, 3, 2, 3, 4), (3, 5, 4, 5, 7), (1, 2, 3, 1, 1)])
def test_packing_identity_fp64(nimg, cin, cout, h, w):
    """four 2 x 2 phase convs on the pre-summed taps == conv3x3(nearest x2), zero padding included (1 x 1 images: every tap but one
    is padding); fp64, so only the order of the additions differs"""
    from this_and_that_vdm_amd.packing import pack_upsample_phases
    g = torch.Generator().manual_seed(7)
    x = torch.randn(nimg, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    wp = pack_upsample_phases(wt, torch.float64)
    assert tuple(wp.shape) == (cout, 16 * cin)
    ref = upsample_conv(x, wt)
    err = (phase_conv(x, wp) - ref).abs().max().item()
    assert err <= 1e-13 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_stored_pack_is_one_rounding_of_the_fp32_sum_of_the_rounded_taps(dtype):
    from this_and_that_vdm_amd.packing import pack_upsample_phases
    g = torch.Generator().manual_seed(8)
    wt = torch.randn(6, 10, 3, 3, generator=g) * torch.exp2(torch.arange(6, dtype=torch.float32) - 3)[:, None, None, None]
    wp = pack_upsample_phases(wt, dtype)
    assert wp.dtype == dtype and wp.is_contiguous()
    want = summed_taps(wt.to(dtype), torch.float32).to(dtype)
    assert torch.equal(wp, want)
    # a single-tap entry (phase (0, 0), tap (0, 0) = 3x3 weight (0, 0)) is the stored weight itself
    assert torch.equal(wp[:, :10], wt.to(dtype)[:, :, 0, 0])


def test_f32_pack_keeps_the_fp32_sum():
    from this_and_that_vdm_amd.packing import pack_upsample_phases
    wt = torch.randn(4, 8, 3, 3, generator=torch.Generator().manual_seed(9))
    assert torch.equal(pack_upsample_phases(wt, torch.float32), summed_taps(wt, torch.float32))


def _args(dtype=0, nimg=28, h=16, w=28, cin=640, cout=640, **kw):
    from this_and_that_vdm_amd import _lib
    g = _lib.TtGemmArgs()
    g.m, g.n, g.k0, g.mode, g.dtype = nimg * 4 * h * w, cout, cin, 1, dtype
    g.nimg, g.hin, g.win, g.hout, g.wout, g.stride, g.upsample = nimg, h, w, 2 * h, 2 * w, 1, 2
    g.lda0, g.ldw, g.ldo = cin, 16 * cin, cout
    g.acc_scale, g.ln_eps = 1.0, 1e-5
    for name, v in kw.items():
        setattr(g, name, v)
    return g


def _plan(lib, g):
    cfg = (C.c_int32 * 7)()
    return lib.tt_gemm_plan(C.byref(g), cfg), list(cfg)


# every combination the route refuses: field values that are valid for upsample = 1 (pointers are fake: nothing is launched)
REFUSED = {
    "a1": dict(a1=256, k1=64, lda1=64), "residual": dict(residual=256, ld_res=640), "blend": dict(blend=256, ld_blend=640, alpha=0.5),
    "rowvec": dict(rowvec=256, rowvec_rows=64, ld_rowvec=640), "stats_out": dict(stats_out=256), "gn_out": dict(gn_out=256, ld_gn=640),
    "geglu": dict(geglu=1), "ln_fold": dict(ln_fold=1), "out_fp8": dict(out_fp8=1), "stride": dict(stride=2),
    "out_f32": dict(out_f32=1), "out_col_hw": dict(out_col_hw=16, out_col_hwp=32), "geometry": dict(hout=16, wout=28, m=28 * 16 * 28),
}


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_plan_accepts_upsample2_on_the_tiled_template_unsplit(lib, dtype):
    # the three UNet levels at 32x56 latents and a tiny problem; a workspace on offer does not make it split
    for (h, w, cin, cout) in [(16, 28, 640, 640), (8, 14, 1280, 1280), (4, 7, 1280, 1280), (1, 1, 64, 128)]:
        g = _args(dtype, h=h, w=w, cin=cin, cout=cout, ws=256, ws_bytes=1 << 30)
        rc, cfg = _plan(lib, g)
        assert rc == 0, lib.tt_last_error()
        assert cfg[3] >= 2 and cfg[1] in (64, 128) and cfg[6] == 1, cfg          # a ring of the tiled template, K not split
        assert lib.tt_gemm_ws_bytes(C.byref(g)) == 0
        assert lib.tt_gemm_stats_rows(C.byref(g)) == 0 and lib.tt_gemm_gn_fused(C.byref(g)) == 0
    # never on the 320-wide kernels, whatever the width
    rc, cfg = _plan(lib, _args(0, h=16, w=28, cin=320, cout=320))
    assert rc == 0 and cfg[1] != 320 and cfg[3] >= 2, cfg


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_plan_and_gemm_refuse_what_the_route_does_not_carry(lib, what):
    g = _args(**REFUSED[what])
    rc, _ = _plan(lib, g)
    assert rc == TT_EINVAL, (what, rc)
    assert b"upsample = 2" in lib.tt_last_error()
    g.a0 = g.w = g.out = 256                       # tt_gemm checks before it resolves a route or launches anything
    assert lib.tt_gemm(C.byref(g), None) == TT_EINVAL, what
    assert b"upsample = 2" in lib.tt_last_error()
    # the same fields with upsample = 1 are a plan of the old route (the refusal is the new value's)
    g.upsample = 1
    if what != "geometry":
        assert _plan(lib, g)[0] == 0, what


def test_upsample1_plan_is_what_it_was(lib):
    """the nine-tap route of the three UNet levels keeps its tiles"""
    g = _args(h=16, w=28, cin=640, cout=640, upsample=1, ldw=9 * 640)
    assert _plan(lib, g) == (0, [128, 128, 64, 2, 4, 2, 1])
    g = _args(h=8, w=14, cin=1280, cout=1280, upsample=1, ldw=9 * 1280)
    assert _plan(lib, g) == (0, [256, 128, 32, 3, 4, 2, 1])


def test_abi_number_and_struct_size_unchanged(lib):
    from this_and_that_vdm_amd import _lib
    assert lib.tt_abi_version() == 11
    assert C.sizeof(_lib.TtGemmArgs) == 320
    assert _lib.TtGemmArgs.upsample.offset == 92 and _lib.TtGemmArgs.upsample.size == 4
