"""Thin torch-tensor front end over the C ABI (include/ttvdm.h).  torch supplies device memory and the
current HIP stream only; every op below is a libttvdm kernel launch and raises if the library is
missing or the tensors are not on a HIP device."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import TT_BF16, TT_F16, TT_F32, TtAttnArgs, TtConvArgs, TtEncAttnArgs, TtGemmArgs, check
from .packing import PreSplitF32


# Optional launch profiler (bench.py): when set to a list, gemm() / conv3x3() / attention() append
# (kernel instance name, algorithmic flops, start event, end event, shape) around their launch on the current stream.  The name is the
# library's own answer (tt_gemm_kernel / tt_conv3x3_kernel / tt_attention_kernel: the selector the launch dispatched on), in the form a
# kernel trace prints, e.g. "gemm_kernel<bf16_tag, 128, 128, 64, 2, 4, 2, 0>".
PROFILE = None


def _prof_begin():
    if PROFILE is None:
        return None
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def _prof_end(start, name, flops, shape=None):
    if start is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        PROFILE.append((name, flops, start, e, shape))


def _kernel_name(query, args) -> str:
    """the answer of a tt_*_kernel query about the launch just made"""
    buf = C.create_string_buffer(96)
    check(query(C.byref(args), buf, len(buf)), query.__name__)
    return buf.value.decode()


# Optional record of the normalisation calls (tests): when set to a list, groupnorm_stats() / groupnorm_apply() / groupnorm() /
# layernorm() / layernorm_block() append the kernel instance of the entry point they called.  It is this front end's record, not an
# observation of a launch: an entry point with one kernel is named outright; for tt_groupnorm_small / tt_groupnorm_stats, which choose
# between kernels, the name is tt_groupnorm_route's answer -- the same host code the launchers decide with.  It tells a test which
# dispatch branch and which route decision a call went through.  Not part of PROFILE: its entries are the MFMA launches bench.py's
# roofline table is built from.
NORM_TRACE = None


def _norm_trace(name: str, dtype) -> None:
    if NORM_TRACE is not None:
        NORM_TRACE.append(f"{name}<{_TAG[_code(dtype)]}>")


_GN_ROUTE = {1: "gn_stats_image_kernel", 2: "gn_group_kernel", 3: "gn_partial_kernel + gn_finalize_kernel"}


# ---- producer -> GroupNorm hand-off (gemm(..., stats=) / gemm(..., gn=) -> groupnorm()).  The producer's per-tile column sums (or the
# tensor its reduction pass already normalised) travel with the OUTPUT TENSOR OBJECT as `_tt_stats` / `_tt_gn`, because producer and
# consumer sit in different modules (a ResBlock's conv feeds the next block's norm).  What makes that safe is the write ledger below:
# every ops.* function that writes a tensor through a raw pointer records a serial number for the tensor's STORAGE, the hand-off stores
# the serial of the launch that produced the sums, and groupnorm() uses them only if no ops.* launch has written that storage since
# (a write through ANY view of the buffer -- gemm(out=view), attention(out=), add_rowvec(out=), add_scaled(out=), nchw_to_tokens(out=) --
# bumps the serial) and the tensor still has the pointer and shape it had then.  Stale sums are ignored (statistics pass), never used.
import itertools

_SERIAL = itertools.count(1)
_LAST_WRITE = {}


# Optional range audit (audit.RangeAudit sets it for the length of a `with` block): every write the ledger records is then followed, on
# the same stream, by a tt_tensor_stats pass over the tensor just written, into the record slot of the call's site.  None (the default):
# one `is None` test per ledger write and nothing else -- no launch, no allocation, the same graph.
AUDIT = None


def _wrote(t: torch.Tensor, op: str = "op") -> int:
    """record a raw-pointer write to (a view of) t's storage by the ops function `op`; returns the write's serial number"""
    n = next(_SERIAL)
    _LAST_WRITE[t.untyped_storage().data_ptr()] = n
    for name in ("_tt_stats", "_tt_gn"):
        if hasattr(t, name):
            delattr(t, name)
    if AUDIT is not None:
        AUDIT.record(t, op)
    return n


def _handoff_valid(t: torch.Tensor, serial: int, ptr: int, shape) -> bool:
    return _LAST_WRITE.get(t.untyped_storage().data_ptr()) == serial and t.data_ptr() == ptr and tuple(t.shape) == shape


_WS = {}
_WS_RETIRED = []          # outgrown buffers stay allocated: a captured hipGraph may still hold their address
WS_FLOOR_BYTES = 64 << 20


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Persistent split-K scratch per (device, stream), grown on demand.  Launches on one stream are ordered, so every
    GEMM on it can share the buffer.  A buffer that has been handed out is NEVER freed: a hipGraph captured earlier keeps
    its raw pointer, so an outgrown buffer is retired (kept alive) instead of dropped."""
    key = (device, torch.cuda.current_stream().cuda_stream)      # per stream: concurrent branches must not share slabs
    buf = _WS.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _WS_RETIRED.append(buf)
        buf = _WS[key] = torch.empty(max(nbytes, WS_FLOOR_BYTES), dtype=torch.uint8, device=device)
    return buf


def _code(dt: torch.dtype) -> int:
    if dt == torch.bfloat16:
        return TT_BF16
    if dt == torch.float16:
        return TT_F16
    if dt == torch.float32:
        return TT_F32          # reference-precision mode (exact-fp32 MFMA): parity runs, not the benchmarked path
    raise RuntimeError(f"libttvdm activations/weights must be bfloat16, float16 or float32, got {dt}")


# TT_F32 products: exact-fp32 MFMA (default) or "split16" -- fp32 operands split on the fly into fp16 hi + lo, three 16-bit MFMAs per
# product block (tt_gemm_set_f32_split, include/ttvdm.h): the mode that meets the north-star tolerance at about a third of the time.
# The library holds the switch (its environment variable is read there, once); this module keeps no copy of it.
def set_f32_split(on: bool) -> None:
    """Process-wide: TT_F32 launches of gemm() use split-fp16 products (True) or the exact-fp32 MFMA (False).  Part of DenoiseLoop's
    graph key, so a captured step is never replayed in the other mode."""
    check(_lib.load().tt_gemm_set_f32_split(int(bool(on))), "tt_gemm_set_f32_split")


def f32_split() -> bool:
    return bool(_lib.load().tt_gemm_get_f32_split())


def set_gemm_wide(on: int) -> None:
    """Process-wide: when gemm() takes tt_gemm's wide route (windowed descriptors for operands of 2 GiB and more): 0 never (such a
    problem is refused), 1 (default) when an operand needs it, 2 whenever the wide kernels can serve the problem (tests, measurements)."""
    check(_lib.load().tt_gemm_set_wide(int(on)), "tt_gemm_set_wide")


WIDE_LAUNCHES = 0          # gemm() launches that ran on the wide route since the process started (tests and tools read the difference)


_TAG = {TT_BF16: "bf16_tag", TT_F16: "f16_tag", TT_F32: "f32_tag"}
FP8 = torch.float8_e4m3fn          # OCP e4m3 (gfx950's fp8; not MI300's fnuz)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libttvdm ops need tensors on the HIP device (no CPU fallback)")
    return t.data_ptr()


def _rows2d(t: torch.Tensor) -> Tuple[int, int]:
    """(row stride, cols) of a 2-D row view whose last dim is contiguous."""
    assert t.dim() == 2 and t.stride(1) == 1, (t.shape, t.stride())
    return t.stride(0), t.shape[1]


def gemm(a0: torch.Tensor, w: torch.Tensor, *, a1: Optional[torch.Tensor] = None, mode: int = 0, conv=None, tconv=None,
         bias=None, acc_scale: float = 1.0, rowvec=None, rowvec_rows: int = 0, rowvec_mod: int = 0, geglu: bool = False, residual=None,
         blend=None, alpha: float = 0.0, out: Optional[torch.Tensor] = None, out_f32: bool = False, m: Optional[int] = None,
         out_col_pad: Optional[Tuple[int, int]] = None, ln_fold: int = 0, ln_eps: float = 1e-5,
         out_fp8: bool = False, stats: int = 0, gn=None) -> torch.Tensor:
    """out[m, n] = epilogue(gather(a0|a1) @ w.T); see TtGemmArgs in include/ttvdm.h.
    stats = S > 0: the output will be read by a GroupNorm whose segments are S rows (h*w for per-image statistics, frames*h*w for the
    temporal ResBlock) -- ask the launch for its per-tile column sums (TtGemmArgs.stats_out).  When the route has a statistics
    epilogue AND S is a whole number of its tiles they are attached to the returned tensor (``out._tt_stats = (buffer, rows per
    tile)``) and groupnorm() normalises in one pass from them; otherwise the launch runs without them (no cost).
    gn = (gamma, beta, eps, silu) next to stats = S: the parameters of THAT GroupNorm.  Where the launch ends in a split-K reduction pass
    (the two coarsest UNet levels) the pass also normalises (TtGemmArgs.gn_out): the result is attached (``out._tt_gn``) and groupnorm()
    with the same parameters returns it without a launch; elsewhere `gn` is ignored and the statistics route above applies.
    conv = (nimg, hin, win, hout, wout, stride, upsample) for mode 1 (3x3, zero padding 1 all round) and mode 3 (3x3, zero padding on the
    bottom / right only: F.pad(x, (0, 1, 0, 1)) + conv(padding=0), the VAE encoder's downsample; upsample 0); tconv = (frames, hw).
    upsample = 2 (mode 1): `w` is the phase pack [n, 16 * k0] of packing.pack_upsample_phases; one source, bias only.
    ln_fold: 1 = rows of a0 / 2 = rows of w are LayerNorm inputs (weights pre-folded by packing.fold_layernorm).
    out_fp8: the output is stored as OCP e4m3 (torch.float8_e4m3fn), the operand format of attention(..., fp8 path)."""
    lib = _lib.load()
    g = TtGemmArgs()
    lda0, k0 = _rows2d(a0)
    g.a0, g.k0, g.lda0 = _p(a0), k0, lda0
    if a1 is not None:
        lda1, k1 = _rows2d(a1)
        g.a1, g.k1, g.lda1 = _p(a1), k1, lda1
    ldw, _ = _rows2d(w)
    n = w.shape[0]
    g.w, g.ldw, g.n = _p(w), ldw, n
    g.mode = mode
    if mode in (1, 3):
        g.nimg, g.hin, g.win, g.hout, g.wout, g.stride, g.upsample = conv
        mm = conv[0] * conv[3] * conv[4]
    elif mode == 2:
        g.frames, g.hw = tconv
        mm = a0.shape[0]
    else:
        mm = a0.shape[0]
    g.m = mm if m is None else m
    g.bias, g.acc_scale = _p(bias), acc_scale
    if rowvec is not None:
        g.rowvec, g.rowvec_rows, g.ld_rowvec, g.rowvec_mod = _p(rowvec), rowvec_rows, rowvec.stride(0), int(rowvec_mod)
        need_rows = rowvec_mod if rowvec_mod > 0 else (((mm if m is None else m) - 1) // rowvec_rows + 1)
        if rowvec.dtype != torch.float32 or rowvec.stride(1) != 1 or rowvec.shape[0] < need_rows or rowvec.shape[1] < n:
            raise RuntimeError(f"gemm: rowvec must be fp32 [>= {need_rows}, >= {n}] with contiguous rows, got {tuple(rowvec.shape)} {rowvec.dtype}")
    g.geglu = int(geglu)
    if residual is not None:
        g.residual, g.ld_res = _p(residual), residual.stride(0)
    if blend is not None:
        g.blend, g.ld_blend, g.alpha = _p(blend), blend.stride(0), alpha
    n_out = n // 2 if geglu else n
    if out is None:
        out = torch.empty((g.m, n_out), dtype=FP8 if out_fp8 else (torch.float32 if out_f32 else a0.dtype), device=a0.device)
    if out_fp8 and out.dtype != FP8:
        raise RuntimeError("out_fp8 needs a torch.float8_e4m3fn output tensor")
    g.out, g.ldo, g.out_f32, g.out_fp8 = _p(out), out.stride(0), int(out_f32), int(out_fp8)
    if out_col_pad is not None:
        g.out_col_hw, g.out_col_hwp = out_col_pad
    g.dtype = _code(a0.dtype)
    g.ln_fold, g.ln_eps = int(ln_fold), float(ln_eps)
    if g.dtype == TT_F32 and lib.tt_gemm_get_f32_split():       # operands packed as fp16 (h, l) pairs (packing.presplit_f32): no conversion in the kernel
        g.presplit = (1 if isinstance(a0, PreSplitF32) else 0) | (2 if isinstance(w, PreSplitF32) else 0)
    elif isinstance(a0, PreSplitF32) or isinstance(w, PreSplitF32):
        raise RuntimeError("gemm: a pre-split operand outside the split16 mode (set_f32_split changed after the weights were packed: "
                           "call prepare() / begin() again)")
    need = lib.tt_gemm_ws_bytes(C.byref(g))
    if need:
        ws = _workspace(need, a0.device)
        g.ws, g.ws_bytes = ws.data_ptr(), ws.numel()
    sbuf = gnbuf = None
    if stats and gn is not None and GN_FUSED:
        g.stats_seg = int(stats)
        if lib.tt_gemm_gn_fused(C.byref(g)):
            gnbuf = torch.empty((g.m, n), dtype=out.dtype, device=a0.device)
            g.gn_out, g.ld_gn, g.gn_gamma, g.gn_beta, g.gn_eps, g.gn_silu = gnbuf.data_ptr(), n, _p(gn[0]), _p(gn[1]), float(gn[2]), int(bool(gn[3]))
    # (only for outputs up to the finest level's size at 256x448: the statistics epilogue costs 1-2.6 us PER TILE of a workgroup, so a
    # launch that walks 3-4 tiles per CU -- 512x896 latents -- pays more than the consumer's saved pass: 107.5 -> 108.5 ms/step, one call)
    if stats and gnbuf is None and GN_TILES and g.m * n <= GN_TILES_MAX_ELEMS:
        g.stats_seg = int(stats) if GN_TILES_SEG else 0        # (lets the split-K routes and the tiled template pick a tile height that divides the segment)
        srows = lib.tt_gemm_stats_rows(C.byref(g))
        if srows > 0 and lib.tt_groupnorm_tiles_supported(int(stats), n, srows, g.dtype):
            sbuf = torch.empty(((g.m + srows - 1) // srows, 2, n), dtype=torch.float32, device=a0.device)
            g.stats_out = sbuf.data_ptr()
    ev = _prof_begin()
    check(lib.tt_gemm(C.byref(g), _stream()), "tt_gemm")
    wide = bool(lib.tt_gemm_is_wide(C.byref(g)))           # (host-only: the resolved route of the launch just made)
    if wide:
        global WIDE_LAUNCHES
        WIDE_LAUNCHES += 1
    serial = _wrote(out, "gemm")                            # `out` was overwritten: sums attached by an earlier launch are dropped
    if gnbuf is not None:
        _wrote(gnbuf, "gemm.gn_out")                        # the normalised copy the reduction pass wrote (a later launch reads it as an activation)
    if sbuf is not None:
        out._tt_stats = (sbuf, srows, serial, out.data_ptr(), tuple(out.shape))
    if gnbuf is not None:
        out._tt_gn = (gnbuf, gn[0].data_ptr(), gn[1].data_ptr(), float(gn[2]), bool(gn[3]), int(stats), serial, out.data_ptr(), tuple(out.shape))
    if ev is not None:
        # (a profiled launch also asks for its plan, as it always has: a caller that wraps lib.tt_gemm_plan -- the `launch` helper of
        # tests/test_error_bounds_gpu.py -- reads the tile of the launch from this call; the record itself takes nothing from it)
        lib.tt_gemm_plan(C.byref(g), (C.c_int32 * 7)())
        taps = 9 if mode in (1, 3) else (3 if mode == 2 else 1)
        if mode == 1 and g.upsample == 2:           # phase-packed upsampling conv: the EXECUTED products, four taps per output pixel
            taps = 4
        _prof_end(ev, _kernel_name(lib.tt_gemm_kernel, g), 2.0 * g.m * n * taps * (g.k0 + g.k1),
                  shape=(mode, g.m, n, taps * (g.k0 + g.k1), int(geglu), int(residual is not None)))
    return out


# ResnetBlock2D routes its 3x3 convs through tt_conv3x3 only when asked to (measured slower than groupnorm_apply + tt_gemm mode 1)
CONV3X3_FUSED = os.environ.get("TT_CONV3X3", "0") == "1"


def conv3x3_supported(h: int, w: int, c0: int, c1: int, n: int, dtype: torch.dtype) -> bool:
    """can tt_conv3x3 (fused GroupNorm + LDS-patch 3x3 conv) serve this problem?  Otherwise: groupnorm_apply + gemm(mode=1)."""
    if dtype not in (torch.bfloat16, torch.float16):
        return False
    return bool(_lib.load().tt_conv3x3_supported(h, w, c0, c1, n, _code(dtype)))


def conv3x3(x0, x1, w, nimg: int, h: int, wd: int, *, gn=None, silu: bool = True, bias=None, rowvec=None, rowvec_rows: int = 0,
            residual=None, out=None):
    """3x3 / stride 1 / pad 1 conv over token-major x0 | x1 with the input's GroupNorm (+SiLU) applied on the fly:
    gn = (scale, shift) fp32 [nimg, C] from groupnorm_stats (None: raw input).  See TtConvArgs in include/ttvdm.h."""
    lib = _lib.load()
    a = TtConvArgs()
    a.x0, a.c0, a.ld0 = _p(x0), x0.shape[1], x0.stride(0)
    if x1 is not None:
        a.x1, a.c1, a.ld1 = _p(x1), x1.shape[1], x1.stride(0)
    n = w.shape[0]
    a.w, a.ldw = _p(w), w.stride(0)
    a.nimg, a.h, a.w_img, a.n = nimg, h, wd, n
    if gn is not None:
        a.gn_scale, a.gn_shift, a.silu = _p(gn[0]), _p(gn[1]), int(silu)
    a.bias = _p(bias)
    if rowvec is not None:
        a.rowvec, a.rowvec_rows, a.ld_rowvec = _p(rowvec), rowvec_rows, rowvec.stride(0)
    if residual is not None:
        a.residual, a.ld_res = _p(residual), residual.stride(0)
    if out is None:
        out = torch.empty((nimg * h * wd, n), dtype=x0.dtype, device=x0.device)
    a.out, a.ldo, a.dtype = _p(out), out.stride(0), _code(x0.dtype)
    ev = _prof_begin()
    check(lib.tt_conv3x3(C.byref(a), _stream()), "tt_conv3x3")
    _wrote(out, "conv3x3")
    if ev is not None:
        k = 9 * (a.c0 + a.c1)
        _prof_end(ev, _kernel_name(lib.tt_conv3x3_kernel, a), 2.0 * nimg * h * wd * n * k, shape=(1, nimg * h * wd, n, k, 0, int(residual is not None)))
    return out


# cross-attention with the query projection computed by the attention kernel itself (tt_attention, TtAttnArgs.qx): on by default,
# TT_ATTN_QPROJ=0 keeps the separate LayerNorm-folded projection GEMM (A/B)
ATTN_QPROJ = os.environ.get("TT_ATTN_QPROJ", "1") != "0"


def attention_qproj_supported(x, head_dim: int, mask: int) -> bool:
    return ATTN_QPROJ and mask != 0 and head_dim == 64 and x.dtype in (torch.float16, torch.bfloat16) and x.shape[-1] % 64 == 0 and \
        x.stride(0) % 8 == 0 and x.stride(1) == 1


def attention(q, k, vt, out, *, nseq, lq, heads, head_dim, mask, lk, k_seq_stride, v_seq_stride, frames=1, ctx_batches=1,
              batch0=0, qx=None, wq=None, bq=None, ln_eps: float = 1e-5, v_rows: bool = False):
    """q [nseq*lq, heads*d] -- or q=None with qx / wq / bq: the kernel computes Q = LN(qx rows) wq^T + bq itself (cross-attention,
    d = 64, 16-bit; wq / bq LayerNorm-folded and row-permuted by packing.permute_q_rows).
    v_rows: `vt` is V itself, [key rows, heads*d] (e.g. a column slice of a fused Q | K | V projection): mask 0, d = 64, 16-bit."""
    lib = _lib.load()
    a = TtAttnArgs()
    if qx is not None:
        # what the C entry point cannot see through raw pointers: element types and the weight's extent (heads * 64 rows of qc)
        if wq.dtype != qx.dtype or bq.dtype != torch.float32 or not bq.is_contiguous() or wq.stride(1) != 1 or \
                tuple(wq.shape) != (heads * head_dim, qx.shape[1]) or bq.numel() != heads * head_dim:
            raise RuntimeError(f"attention: fused query projection needs wq [{heads * head_dim}, {qx.shape[1]}] in {qx.dtype} and a contiguous "
                               f"fp32 bq [{heads * head_dim}]; got wq {tuple(wq.shape)} {wq.dtype}, bq {tuple(bq.shape)} {bq.dtype}")
        a.qx, a.ldqx, a.wq, a.ldwq, a.bq, a.qc, a.ln_eps = _p(qx), qx.stride(0), _p(wq), wq.stride(0), _p(bq), qx.shape[1], float(ln_eps)
        q = qx                                     # dtype / profiling below; a.q stays NULL
    else:
        a.q, a.ldq = _p(q), q.stride(0)
    a.k, a.ldk = _p(k), k.stride(0)
    a.vt, a.ldvt = _p(vt), vt.stride(0)
    a.out, a.ldo = _p(out), out.stride(0)
    a.nseq, a.lq, a.heads, a.head_dim = nseq, lq, heads, head_dim
    a.mask, a.lk, a.k_seq_stride, a.v_seq_stride = mask, lk, k_seq_stride, v_seq_stride
    fp8 = q.dtype == FP8                       # e4m3 operands (gemm(..., out_fp8=True)); the output type names the kernel
    if fp8 and not (k.dtype == FP8 and vt.dtype == FP8):
        raise RuntimeError("fp8 attention needs q, k and vt in torch.float8_e4m3fn")
    a.frames, a.ctx_batches, a.dtype, a.batch0, a.fp8 = frames, ctx_batches, _code(out.dtype if fp8 else q.dtype), batch0, int(fp8)
    a.v_rows = int(bool(v_rows))
    ev = _prof_begin()
    check(lib.tt_attention(C.byref(a), _stream()), "tt_attention")
    _wrote(out, "attention")
    if ev is not None:
        flops = 4.0 * nseq * heads * lq * lk * head_dim + (2.0 * nseq * lq * heads * head_dim * qx.shape[1] if qx is not None else 0.0)
        _prof_end(ev, _kernel_name(lib.tt_attention_kernel, a), flops, shape=("attn", nseq * heads, lq, lk, mask, 0))
    return out


def temporal_attention(qkv, out, *, batch, frames, hw, heads, head_dim):
    lib = _lib.load()
    check(lib.tt_temporal_attention(_p(qkv), qkv.stride(0), _p(out), out.stride(0), batch, frames, hw, heads, head_dim,
                                    _code(qkv.dtype), _stream()), "tt_temporal_attention")
    _wrote(out, "temporal_attention")
    return out


def groupnorm_stats(x0, x1, nimg, hw, frames_per_group, gamma, beta, eps):
    """-> (scale, shift) fp32 [nimg, C] with y = x*scale + shift."""
    lib = _lib.load()
    c0 = x0.shape[-1]
    c1 = 0 if x1 is None else x1.shape[-1]
    c = c0 + c1
    ws_bytes = lib.tt_groupnorm_ws_bytes(nimg, hw, c)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=x0.device)
    scale = torch.empty((nimg, c), dtype=torch.float32, device=x0.device)
    shift = torch.empty_like(scale)
    check(lib.tt_groupnorm_stats(_p(x0), c0, _p(x1), c1, nimg, hw, frames_per_group, _p(gamma), _p(beta), eps,
                                 _p(scale), _p(shift), _p(ws), ws_bytes, _code(x0.dtype), _stream()), "tt_groupnorm_stats")
    if NORM_TRACE is not None:
        _norm_trace(_GN_ROUTE[lib.tt_groupnorm_route(hw, c, _code(x0.dtype), frames_per_group, 0)], x0.dtype)
    return scale, shift


def groupnorm_apply(x0, x1, nimg, hw, scale, shift, silu: bool, out=None):
    lib = _lib.load()
    c0 = x0.shape[-1]
    c1 = 0 if x1 is None else x1.shape[-1]
    if out is None:
        out = torch.empty((nimg * hw, c0 + c1), dtype=x0.dtype, device=x0.device)
    check(lib.tt_groupnorm_apply(_p(x0), c0, _p(x1), c1, nimg, hw, _p(scale), _p(shift), int(silu), _p(out), out.stride(0),
                                 _code(x0.dtype), _stream()), "tt_groupnorm_apply")
    _norm_trace("gn_apply_kernel", x0.dtype)
    _wrote(out, "groupnorm_apply")
    return out


GN_SMALL = os.environ.get("TT_GN_SMALL", "1") != "0"      # A/B switch for the one-launch GroupNorm
# cross-frame statistics (TemporalResnetBlock: one GroupNorm per video over frames x h x w): the frames of a video are contiguous
# rows, so a video is one "image" of frames * hw rows for the one-launch kernel (a launch then has batch x 16 working blocks).
# OFF by default (0 rows): one launch instead of three (-44 launches per step at the coarsest level, 14 x 28 = 392 rows per video),
# but the step is not faster -- 30.40 / 30.42 ms without, 30.46 / 30.47 with a bound of 512 rows, 30.62 / 30.60 with 2048 (one
# gpurun call, interleaved): the three short launches hide behind the other branch.  TT_GN_CROSS_ROWS=512 enables it (A/B, tests).
GN_CROSS_MAX_ROWS = int(os.environ.get("TT_GN_CROSS_ROWS", "0"))


# GroupNorm from the producer's tile sums (tt_gemm stats_out -> tt_groupnorm_tiles): on by default, TT_GN_TILES=0 keeps every
# GroupNorm on the statistics-pass kernels (A/B)
GN_TILES = os.environ.get("TT_GN_TILES", "1") != "0"
GN_TILES_SEG = os.environ.get("TT_GN_TILES_SEG", "1") != "0"       # ... also on the split-K routes (coarse levels) and with per-wave-row sums of the tiled template (A/B)
GN_FUSED = os.environ.get("TT_GN_FUSED", "1") != "0"        # GroupNorm inside the split-K reduction pass (TtGemmArgs.gn_out), A/B
GN_TILES_MAX_ELEMS = int(os.environ.get("TT_GN_TILES_MAX_ELEMS", str(17 << 20)))
# (the "apply-only consumer" timing experiment of round 5 -- groupnorm() with scale 1 / shift 0, wrong numbers -- lives in
# tools/gn_emulate.py as a monkeypatch now: a leaked TT_GN_EMULATE=1 can no longer corrupt every GroupNorm silently)
if os.environ.get("TT_GN_EMULATE", "0") == "1":
    raise RuntimeError("TT_GN_EMULATE is no longer read by the library (it produced wrong numbers by design): use tools/gn_emulate.py")


def groupnorm(x0, x1, nimg, hw, frames_per_group, gamma, beta, eps, silu: bool):
    """act(group_norm(x0 | x1)) -> new tensor.  Small per-image problems take ONE launch (tt_groupnorm_small), everything else
    tt_groupnorm_stats + tt_groupnorm_apply."""
    lib = _lib.load()
    c0 = x0.shape[-1]
    c1 = 0 if x1 is None else x1.shape[-1]
    fz = getattr(x0, "_tt_gn", None) if x1 is None else None
    if fz is not None and fz[1:6] == (gamma.data_ptr(), beta.data_ptr(), float(eps), bool(silu), frames_per_group * hw) and \
            _handoff_valid(x0, *fz[6:]):
        return fz[0]                                         # the producer's reduction pass already normalised (gemm(..., gn=))
    st = getattr(x0, "_tt_stats", None) if (GN_TILES and x1 is None) else None
    if st is not None and not _handoff_valid(x0, *st[2:]):
        st = None                                            # something wrote the buffer after the producer: statistics pass instead
    if st is not None and nimg % frames_per_group == 0 and x0.is_contiguous() and st[0].shape[2] == c0 and \
            lib.tt_groupnorm_tiles_supported(frames_per_group * hw, c0, st[1], _code(x0.dtype)):
        # the producer of x0 left per-tile column sums: one pass over x0, one launch, per-image and cross-frame statistics alike
        out = torch.empty((nimg * hw, c0), dtype=x0.dtype, device=x0.device)
        check(lib.tt_groupnorm_tiles(_p(x0), c0, _p(st[0]), st[1], nimg // frames_per_group, frames_per_group * hw, _p(gamma), _p(beta), eps,
                                     int(silu), _p(out), out.stride(0), _code(x0.dtype), _stream()), "tt_groupnorm_tiles")
        _norm_trace("gn_tiles_kernel", x0.dtype)
        _wrote(out, "groupnorm")
        return out
    if GN_SMALL and frames_per_group > 1 and nimg % frames_per_group == 0 and frames_per_group * hw <= GN_CROSS_MAX_ROWS and \
            lib.tt_groupnorm_small_supported(frames_per_group * hw, c0 + c1, _code(x0.dtype)):
        nimg, hw, frames_per_group = nimg // frames_per_group, frames_per_group * hw, 1
    if GN_SMALL and frames_per_group == 1 and lib.tt_groupnorm_small_supported(hw, c0 + c1, _code(x0.dtype)):
        out = torch.empty((nimg * hw, c0 + c1), dtype=x0.dtype, device=x0.device)
        check(lib.tt_groupnorm_small(_p(x0), c0, _p(x1), c1, nimg, hw, _p(gamma), _p(beta), eps, int(silu), _p(out), out.stride(0),
                                     _code(x0.dtype), _stream()), "tt_groupnorm_small")
        if NORM_TRACE is not None:
            _norm_trace(_GN_ROUTE[lib.tt_groupnorm_route(hw, c0 + c1, _code(x0.dtype), 1, 1)], x0.dtype)
        _wrote(out, "groupnorm")
        return out
    sc, sh = groupnorm_stats(x0, x1, nimg, hw, frames_per_group, gamma, beta, eps)
    return groupnorm_apply(x0, x1, nimg, hw, sc, sh, silu)


def layernorm(x, gamma, beta, eps=1e-5, rowvec=None, rows_per_vec=0, nvec=0):
    """-> y, or (x + rowvec, y) when a row vector is fused in."""
    lib = _lib.load()
    rows, c = x.shape
    y = torch.empty((rows, c), dtype=x.dtype, device=x.device)
    xs = torch.empty((rows, c), dtype=x.dtype, device=x.device) if rowvec is not None else None
    if xs is not None:
        assert x.stride(0) == c
    check(lib.tt_layernorm(_p(x), x.stride(0), rows, c, _p(gamma), _p(beta), eps, _p(rowvec), rows_per_vec, nvec, _p(xs),
                           _p(y), y.stride(0), _code(x.dtype), _stream()), "tt_layernorm")
    _norm_trace("ln_kernel", x.dtype)
    if xs is not None:
        _wrote(xs, "layernorm.sum")
    _wrote(y, "layernorm")
    return (xs, y) if xs is not None else y


def add_rowvec(x, rowvec, rows_per_vec: int, nvec: int, out=None):
    """y[r] = x[r] + rowvec[(r // rows_per_vec) % nvec]  (frame-position embedding, transformer_temporal.py:358-359).
    ``out`` may be ``x`` itself (in place) and both may be strided row views."""
    lib = _lib.load()
    rows, c = x.shape
    assert x.stride(1) == 1 and rowvec.dtype == torch.float32 and rowvec.stride(1) == 1
    y = torch.empty((rows, c), dtype=x.dtype, device=x.device) if out is None else out
    assert y.shape == x.shape and y.stride(1) == 1 and y.dtype == x.dtype
    check(lib.tt_add_rowvec(_p(x), x.stride(0), rows, c, _p(rowvec), rowvec.stride(0), rows_per_vec, nvec, _p(y), y.stride(0),
                            _code(x.dtype), _stream()), "tt_add_rowvec")
    _wrote(y, "add_rowvec")
    return y


def softmax_rows(x, dtype, cols: Optional[int] = None, out=None):
    """row softmax of fp32 scores x[:, :cols] -> `dtype`, columns cols..out.shape[1] zeroed (padding for a following GEMM).
    Contract of tt_softmax_rows: the kernel reads whole float4 quads up to round_up(cols, 8), so the score rows must be
    at least that long in memory (x.stride(0) >= round_up(cols, 8); the values beyond `cols` are ignored) and the output
    has round_up(cols, 8) or more columns."""
    lib = _lib.load()
    assert x.dtype == torch.float32 and x.stride(1) == 1
    rows = x.shape[0]
    cols = x.shape[1] if cols is None else cols
    cols_pad = (cols + 7) // 8 * 8
    if x.stride(0) < cols_pad:
        raise ValueError(f"softmax_rows: score rows of {cols} columns need a row stride >= {cols_pad} floats (got {x.stride(0)}): "
                         "allocate the score buffer with its column count rounded up to 8")
    if out is None:
        out = torch.empty((rows, cols_pad), dtype=dtype, device=x.device)
    if out.shape[1] < cols_pad:
        raise ValueError(f"softmax_rows: output needs >= {cols_pad} columns, got {out.shape[1]}")
    check(lib.tt_softmax_rows(_p(x), x.stride(0), rows, cols, _p(out), out.stride(0), out.shape[1], _code(dtype), _stream()),
          "tt_softmax_rows")
    _wrote(out, "softmax_rows")
    return out


def small_linear(x, w, bias=None, act_in=False, act_out=False, out=None, accumulate=False):
    lib = _lib.load()
    rows, k = x.shape
    n = w.shape[0]
    if out is None:
        out = torch.empty((rows, n), dtype=torch.float32, device=x.device)
    assert x.dtype == torch.float32 and out.dtype == torch.float32
    check(lib.tt_small_linear(_p(x), x.stride(0), rows, k, _p(w), w.stride(0), n, _p(bias), int(act_in), int(act_out),
                              int(accumulate), _p(out), out.stride(0), _code(w.dtype), _stream()), "tt_small_linear")
    _wrote(out, "small_linear")
    return out


def timestep_embedding(t, dim):
    lib = _lib.load()
    assert t.dtype == torch.float32 and t.dim() == 1
    out = torch.empty((t.shape[0], dim), dtype=torch.float32, device=t.device)
    check(lib.tt_timestep_embedding(_p(t), t.shape[0], dim, _p(out), out.stride(0), _stream()), "tt_timestep_embedding")
    _wrote(out, "timestep_embedding")
    return out


def prep_model_input(latents, image_latents, cond, sigmas, step, batch, frames, h, w, cpad, dtype):
    lib = _lib.load()
    x = torch.empty((batch * frames * h * w, cpad), dtype=dtype, device=latents.device)
    check(lib.tt_prep_model_input(_p(latents), _p(image_latents), _p(cond), _p(sigmas), step, batch, frames, h, w, cpad,
                                  _p(x), _code(dtype), _stream()), "tt_prep_model_input")
    _wrote(x, "prep_model_input")
    return x


def cfg_euler_step(eps, latents, guidance, sigmas, step, batch, frames, h, w, image_guidance_scale=None):
    """batch 1 (no CFG), 2 (uncond, cond) or 3 (use_instructpix2pix: first-frame, cond, uncond + image_guidance_scale)."""
    lib = _lib.load()
    if batch == 3:
        if image_guidance_scale is None or guidance is None:
            raise ValueError("a CFG batch of 3 needs guidance and image_guidance_scale")
        check(lib.tt_cfg3_euler_step(_p(eps), eps.stride(0), _p(latents), _p(guidance), float(image_guidance_scale), _p(sigmas),
                                     step, frames, h, w, _stream()), "tt_cfg3_euler_step")
        _wrote(latents, "cfg_euler_step")
        return latents
    check(lib.tt_cfg_euler_step(_p(eps), eps.stride(0), _p(latents), _p(guidance), _p(sigmas), step, batch, frames, h, w,
                                _stream()), "tt_cfg_euler_step")
    _wrote(latents, "cfg_euler_step")
    return latents


def prep_model_input_requests(latents, image_latents, cond, sigmas, step, requests, cfg, frames, h, w, cpad, dtype):
    """R requests in one launch: latents fp32 [R,F,4,h,w], image_latents fp32 [R*C,F,4,h,w] in the reference's (CFG-major) order,
    cond None, fp32 [F,4,h,w] (shared by all requests) or [R,F,4,h,w] -> token rows [R*C*F*h*w, cpad], batch element c * R + r."""
    lib = _lib.load()
    per_request = 0
    if cond is not None:
        if cond.numel() not in (frames * 4 * h * w, requests * frames * 4 * h * w):
            raise ValueError(f"prep_model_input_requests: cond holds {cond.numel()} elements, expected [F,4,h,w] or [R,F,4,h,w] "
                             f"with R = {requests}, F = {frames}, h = {h}, w = {w}")
        per_request = int(requests > 1 and cond.numel() == requests * frames * 4 * h * w)
    x = torch.empty((requests * cfg * frames * h * w, cpad), dtype=dtype, device=latents.device)
    check(lib.tt_prep_model_input_requests(_p(latents), _p(image_latents), _p(cond), per_request, _p(sigmas), step, requests, cfg,
                                           frames, h, w, cpad, _p(x), _code(dtype), _stream()), "tt_prep_model_input_requests")
    _wrote(x, "prep_model_input")
    return x


def cfg_euler_step_requests(eps, latents, guidance, sigmas, step, requests, cfg, frames, h, w, image_guidance_scale=None):
    """R requests in one launch: eps fp32 token rows of batch element c * R + r, latents fp32 [R,F,4,h,w] (updated in place),
    guidance None (cfg 1), fp32 [F] / [1,F] for all requests or [R,F]; cfg 3 is use_instructpix2pix and needs image_guidance_scale."""
    lib = _lib.load()
    if cfg == 3 and (image_guidance_scale is None or guidance is None):
        raise ValueError("a CFG batch of 3 needs guidance and image_guidance_scale")
    per_request = 0
    if guidance is not None:
        if guidance.numel() not in (frames, requests * frames):
            raise ValueError(f"cfg_euler_step_requests: guidance holds {guidance.numel()} values, expected [1,F] or [R,F] with "
                             f"R = {requests}, F = {frames}")
        per_request = int(requests > 1 and guidance.numel() == requests * frames)
    check(lib.tt_cfg_euler_step_requests(_p(eps), eps.stride(0), _p(latents), _p(guidance), per_request,
                                         float(image_guidance_scale) if cfg == 3 else 0.0, _p(sigmas), step, requests, cfg, frames, h, w,
                                         _stream()), "tt_cfg_euler_step_requests")
    _wrote(latents, "cfg_euler_step")
    return latents


def cfg_multistep_step_requests(eps, latents, x0_hist, guidance, sigmas, step, coef, requests, cfg, frames, h, w,
                                image_guidance_scale=None):
    """The DPM-Solver++ 2M step (include/ttvdm.h) for R >= 1 requests in one launch: cfg_euler_step_requests' operands plus x0_hist
    fp32 [R,F,4,h,w] (the previous step's data prediction: read when this step's coefficient is not 0, always rewritten) and coef, one
    fp32 on the device.  Updates latents and x0_hist in place."""
    lib = _lib.load()
    if cfg == 3 and (image_guidance_scale is None or guidance is None):
        raise ValueError("a CFG batch of 3 needs guidance and image_guidance_scale")
    if x0_hist.numel() != latents.numel() or x0_hist.dtype != torch.float32 or latents.numel() != requests * frames * 4 * h * w:
        raise ValueError(f"cfg_multistep_step_requests: latents hold {latents.numel()} and x0_hist {x0_hist.numel()} ({x0_hist.dtype}) "
                         f"elements, expected fp32 [R,F,4,h,w] each with R = {requests}, F = {frames}, h = {h}, w = {w}")
    if coef.numel() != 1 or coef.dtype != torch.float32:
        raise ValueError(f"cfg_multistep_step_requests: coef holds {coef.numel()} values ({coef.dtype}), expected one fp32 (this step's c)")
    per_request = 0
    if guidance is not None:
        if guidance.numel() not in (frames, requests * frames):
            raise ValueError(f"cfg_multistep_step_requests: guidance holds {guidance.numel()} values, expected [1,F] or [R,F] with "
                             f"R = {requests}, F = {frames}")
        per_request = int(requests > 1 and guidance.numel() == requests * frames)
    check(lib.tt_cfg_multistep_step_requests(_p(eps), eps.stride(0), _p(latents), _p(x0_hist), _p(guidance), per_request,
                                             float(image_guidance_scale) if cfg == 3 else 0.0, _p(sigmas), step, _p(coef), requests, cfg,
                                             frames, h, w, _stream()), "tt_cfg_multistep_step_requests")
    _wrote(latents, "cfg_multistep_step")
    _wrote(x0_hist, "cfg_multistep_x0")
    return latents


def nchw_to_tokens(src, dtype, ld=None, out=None):
    """[N,C,H,W] contiguous (fp32 or `dtype`) -> token-major `dtype` [N*H*W, ld>=C] (extra columns zero), or into
    ``out`` (a [N*H*W, C] column window of a wider token buffer)."""
    lib = _lib.load()
    n, c, h, w = src.shape
    src = src.contiguous()
    if src.dtype not in (torch.float32, dtype):
        src = src.float()
    if out is None:
        ld = c if ld is None else ld
        out = (torch.zeros if ld != c else torch.empty)((n * h * w, ld), dtype=dtype, device=src.device)
    assert out.dtype == dtype and out.stride(1) == 1
    check(lib.tt_nchw_to_tokens(_p(src), int(src.dtype == torch.float32), n, c, h * w, _p(out), out.stride(0), _code(dtype),
                                _stream()), "tt_nchw_to_tokens")
    _wrote(out, "nchw_to_tokens")
    return out


def tokens_to_nchw(src, n, c, h, w, out_dtype):
    lib = _lib.load()
    src_f32 = src.dtype == torch.float32
    # `dtype` names the 16-bit side of the conversion; fp32 -> fp32 (eps of the UNet, TT_F32 tokens) has none and passes TT_F32
    tok_dtype = out_dtype if src_f32 and out_dtype != torch.float32 else (src.dtype if not src_f32 else torch.float32)
    dst_f32 = out_dtype == torch.float32
    if not dst_f32 and not src_f32:
        assert out_dtype == src.dtype
    dst = torch.empty((n, c, h, w), dtype=out_dtype, device=src.device)
    check(lib.tt_tokens_to_nchw(_p(src), int(src_f32), src.stride(0), n, c, h * w, _p(dst), int(dst_f32), _code(tok_dtype),
                                _stream()), "tt_tokens_to_nchw")
    _wrote(dst, "tokens_to_nchw")
    return dst


def add_scaled(a, b, scale=1.0, out=None):
    lib = _lib.load()
    assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape
    if out is None:
        out = torch.empty_like(a)
    check(lib.tt_add_scaled(_p(a), _p(b), scale, _p(out), a.numel(), _code(a.dtype), _stream()), "tt_add_scaled")
    _wrote(out, "add_scaled")
    return out


# ---- the CLIP encoders (this_and_that_vdm_amd/clip.py)
def encoder_attention(q, k, v, out, *, nseq, l, heads, head_dim, causal=False, k_seq_stride=None, v_seq_stride=None):
    """softmax(q k^T / sqrt(d) [+ causal]) v per (sequence, head), l queries = l keys, head_dim 64 or 80 (tt_encoder_attention).
    q [nseq*l, heads*d]; k [rows, heads*d], key j of sequence s in row s*k_seq_stride + j (default l).  16-bit storage: v like k (V itself,
    e.g. q / k / v = the three column slices of a fused projection); fp32 storage: v is V TRANSPOSED, [heads*d, columns], key j of
    sequence s in column s*v_seq_stride + j (gemm(..., out_col_pad=(l, v_seq_stride)), v_seq_stride a multiple of 4)."""
    lib = _lib.load()
    if not (q.dtype == k.dtype == v.dtype == out.dtype):
        raise RuntimeError("encoder_attention: q, k, v and out must share one dtype")
    for t in (q, k, v, out):
        assert t.dim() == 2 and t.stride(1) == 1, (t.shape, t.stride())
    a = TtEncAttnArgs()
    a.q, a.ldq, a.k, a.ldk = _p(q), q.stride(0), _p(k), k.stride(0)
    a.v, a.ldv, a.out, a.ldo = _p(v), v.stride(0), _p(out), out.stride(0)
    a.nseq, a.l, a.heads, a.head_dim, a.causal = nseq, l, heads, head_dim, int(bool(causal))
    a.k_seq_stride = l if k_seq_stride is None else k_seq_stride
    a.v_seq_stride = l if v_seq_stride is None else v_seq_stride
    a.dtype = _code(q.dtype)
    ev = _prof_begin()
    check(lib.tt_encoder_attention(C.byref(a), _stream()), "tt_encoder_attention")
    _wrote(out, "encoder_attention")
    if ev is not None:
        _prof_end(ev, f"enc_attn_kernel<{_TAG[a.dtype]}, {head_dim}, {'true' if causal else 'false'}>",
                  4.0 * nseq * heads * l * l * head_dim * (0.5 if causal else 1.0), shape=("attn", nseq * heads, l, l, int(bool(causal)), 0))
    return out


ACTS = {"gelu": 0, "quick_gelu": 1}


def act_rows(x, act: str = "gelu", out=None):
    """y = act(x) over a [rows, c] row view (strides allowed; out=x: in place).  act: "gelu" (exact erf) or "quick_gelu"."""
    lib = _lib.load()
    if act not in ACTS:
        raise RuntimeError(f"act_rows: unknown activation {act!r} (one of {sorted(ACTS)})")
    assert x.dim() == 2 and x.stride(1) == 1, (x.shape, x.stride())
    y = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device) if out is None else out
    assert y.shape == x.shape and y.stride(1) == 1 and y.dtype == x.dtype
    check(lib.tt_act_rows(_p(x), x.stride(0), x.shape[0], x.shape[1], ACTS[act], _p(y), y.stride(0), _code(x.dtype), _stream()), "tt_act_rows")
    _wrote(y, "act_rows")
    return y


def patch_tokens(src, patch: int, dtype, kpad=None):
    """[N, C, H, W] (fp32 or `dtype`) -> [N*(H/p)*(W/p), kpad] rows of `dtype`, k = (c, ky, kx), zero tail (kpad = C*p*p rounded up to 8)."""
    lib = _lib.load()
    n, c, h, w = src.shape
    src = src.contiguous()
    if src.dtype not in (torch.float32, dtype):
        src = src.float()
    kk = c * patch * patch
    kpad = (kk + 7) // 8 * 8 if kpad is None else kpad
    if h % patch or w % patch:
        raise RuntimeError(f"patch_tokens: image {h}x{w} is not a whole number of {patch}x{patch} patches")
    out = torch.empty((n * (h // patch) * (w // patch), kpad), dtype=dtype, device=src.device)
    check(lib.tt_patch_tokens(_p(src), int(src.dtype == torch.float32), n, c, h, w, patch, _p(out), out.stride(0), kpad, _code(dtype),
                              _stream()), "tt_patch_tokens")
    _wrote(out, "patch_tokens")
    return out


def embed_rows(table, pos, *, ids=None, cls=None, l: int, out=None):
    """Text (ids int64 [rows]): out[r] = table[ids[r]] + pos[r % l].  Vision (cls [c], table = patch rows [N*(l-1), c]):
    out[r] = (class row | patch row) + pos[r % l], rows = N*l."""
    lib = _lib.load()
    assert table.dim() == 2 and table.stride(1) == 1 and pos.dim() == 2 and pos.stride(1) == 1 and pos.dtype == table.dtype
    c = table.shape[1]
    if pos.shape[0] < l or pos.shape[1] != c:
        raise RuntimeError(f"embed_rows: position table {tuple(pos.shape)} does not cover {l} positions of width {c}")
    if (ids is None) == (cls is None):
        raise RuntimeError("embed_rows: pass ids (text) or cls (vision)")
    if ids is not None:
        if ids.dtype != torch.int64 or not ids.is_contiguous():
            raise RuntimeError("embed_rows: ids must be a contiguous int64 tensor")
        rows, mode = ids.numel(), 0
    else:
        assert cls.dtype == table.dtype and cls.is_contiguous() and cls.numel() == c
        if l < 2 or table.shape[0] % (l - 1):
            raise RuntimeError(f"embed_rows: {table.shape[0]} patch rows are not a whole number of images of {l - 1} patches")
        rows, mode = table.shape[0] // (l - 1) * l, 1
    if out is None:
        out = torch.empty((rows, c), dtype=table.dtype, device=table.device)
    assert out.shape == (rows, c) and out.stride(1) == 1 and out.dtype == table.dtype
    check(lib.tt_embed_rows(mode, _p(ids), _p(table), table.stride(0), table.shape[0], _p(cls), _p(pos), pos.stride(0), rows, l, c,
                            _p(out), out.stride(0), _code(table.dtype), _stream()), "tt_embed_rows")
    _wrote(out, "embed_rows")
    return out


# ---- the request path around the models (svd/pipeline_stable_video_diffusion_controlnet.py: encode_clip, decode_latents + tensor2vid)
def clip_image(src, size, mean, std, dtype):
    """CLIP image preprocessing on the device (tt_clip_image): ``pipeline_utils.resize_with_antialiasing(x * 2 - 1, size)`` -> ``(. + 1) / 2``
    -> ``(. - mean) / std`` in fp32.  src: uint8 [N, H, W, 3] (or [H, W, 3]; x = u / 255) or float32 [N, 3, H, W] in [0, 1].
    -> [N, 3, size[0], size[1]] in `dtype`."""
    lib = _lib.load()
    _p(src)
    if src.dtype == torch.uint8:
        src = src[None] if src.dim() == 3 else src
        if src.dim() != 4 or src.shape[-1] != 3:
            raise RuntimeError(f"clip_image: a uint8 source is [N, H, W, 3], got {tuple(src.shape)}")
        kind, (n, h, w) = 0, src.shape[:3]
    elif src.dtype == torch.float32:
        if src.dim() != 4 or src.shape[1] != 3:
            raise RuntimeError(f"clip_image: a float32 source is [N, 3, H, W], got {tuple(src.shape)}")
        kind, n, (h, w) = 1, src.shape[0], src.shape[2:]
    else:
        raise RuntimeError(f"clip_image: the source must be uint8 (NHWC) or float32 (NCHW), got {src.dtype}")
    if len(mean) != 3 or len(std) != 3:
        raise RuntimeError("clip_image: mean and std hold one value per RGB channel")
    src = src.contiguous()
    oh, ow = int(size[0]), int(size[1])
    out = torch.empty((n, 3, oh, ow), dtype=dtype, device=src.device)
    need = lib.tt_clip_image_ws_bytes(n, h, w)
    ws = _workspace(need, src.device)
    check(lib.tt_clip_image(_p(src), kind, n, h, w, oh, ow, *[float(v) for v in mean], *[float(v) for v in std], _p(out), _code(dtype),
                            _p(ws), need, _stream()), "tt_clip_image")
    _wrote(out, "clip_image")
    return out


def layernorm_block(x, rows: int, eps: float = 1e-5, out=None):
    """LayerNorm without affine parameters over each [rows, c] block of the row view x [nb * rows, c] (tt_layernorm_block): the
    ``nn.LayerNorm((rows, c))`` encode_clip builds afresh for the use_text context.  ``out`` may be ``x`` (in place) or a row view with
    x's row stride."""
    lib = _lib.load()
    _p(x)
    assert x.dim() == 2 and x.stride(1) == 1, (x.shape, x.stride())
    if rows <= 0 or x.shape[0] % rows:
        raise RuntimeError(f"layernorm_block: {x.shape[0]} rows are not a whole number of blocks of {rows}")
    y = torch.empty_strided(tuple(x.shape), tuple(x.stride()), dtype=x.dtype, device=x.device) if out is None else out
    if y.shape != x.shape or y.stride() != x.stride() or y.dtype != x.dtype:
        raise RuntimeError("layernorm_block: out must have x's shape, strides and dtype")
    check(lib.tt_layernorm_block(_p(x), x.stride(0), x.shape[0] // rows, rows, x.shape[1], float(eps), _p(y), _code(x.dtype), _stream()),
          "tt_layernorm_block")
    _norm_trace("ln_block_kernel", x.dtype)
    _wrote(y, "layernorm_block")
    return y


def frames_out(x, kind: int):
    """Decoder output [N, C, H, W] (C <= 4, bf16 / fp16 / fp32) -> NHWC frames as the caller receives them (tt_frames_out):
    kind 0 float32 ``clamp(x / 2 + 0.5, 0, 1)`` (output_type "np"), kind 1 uint8 ``rint(that * 255)`` ("pil") -- bit for bit what
    ``VaeImageProcessor.postprocess`` / ``numpy_to_pil`` compute."""
    lib = _lib.load()
    _p(x)
    if kind not in (0, 1):
        raise RuntimeError(f"frames_out: kind {kind!r} (0 float32, 1 uint8)")
    assert x.dim() == 4, x.shape
    x = x.contiguous()
    n, ch, h, w = x.shape
    out = torch.empty((n, h, w, ch), dtype=torch.float32 if kind == 0 else torch.uint8, device=x.device)
    check(lib.tt_frames_out(_p(x), _code(x.dtype), n, ch, h, w, kind, _p(out), _stream()), "tt_frames_out")
    _wrote(out, "frames_out")
    return out


def gesture_maps(records, nmaps: int, frames: int, org_hw, out_hw, dilate: bool, flip: bool, dtype, device, out=None):
    """Gesture frames rasterised on the device from the annotated points (tt_gesture_maps): `records` is a sequence of up to 64
    ``(map, frame, x, y, first)`` integer tuples as ``gesture_map.point_records`` builds them -- the point (x horizontal, y vertical, in
    pixels of the ``org_hw`` image) decides frame `frame` of map `map`, the last record of a (map, frame) wins, unnamed frames are zeros.
    -> [nmaps, frames, 3, out_hw[0], out_hw[1]] in `dtype`, every element written by the call.  No host array is built and nothing is
    copied to the device: the records travel as kernel arguments.  ``out``: a contiguous tensor of that shape and dtype to write instead of a new one."""
    lib = _lib.load()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("libttvdm ops need tensors on the HIP device (no CPU fallback)")
    lim = 1 << 31
    recs = (_lib.TtGesturePoint * max(len(records), 1))()
    for i, rec in enumerate(records):
        m, f, x, y, first = (int(v) for v in rec)
        # a centre beyond int32 is outside every image the library serves: clamping it keeps the (empty) box empty
        recs[i] = _lib.TtGesturePoint(m, f, max(-lim, min(lim - 1, x)), max(-lim, min(lim - 1, y)), first)
    n, (oh, ow) = len(records), (int(out_hw[0]), int(out_hw[1]))
    with torch.cuda.device(device):
        shape = (int(nmaps), int(frames), 3, oh, ow)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=device)
        elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
            raise RuntimeError(f"gesture_maps: out must be a contiguous {dtype} tensor of shape {shape}")
        need = lib.tt_gesture_maps_ws_bytes(n, oh, ow)
        ws = _workspace(need, out.device) if need else None
        check(lib.tt_gesture_maps(recs if n else None, n, int(nmaps), int(frames), int(org_hw[0]), int(org_hw[1]), oh, ow, int(dilate), int(flip),
                                  _p(out), _code(dtype), _p(ws), need, _stream()), "tt_gesture_maps")
    _wrote(out, "gesture_maps")
    return out


# ---- the request image: PIL's 8-bit resize and the VAE input computed from it (tt_resample_coeffs / tt_resize_u8 / tt_vae_image)
RESAMPLE = {"lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}          # PIL.Image.Resampling's codes
_RESAMPLE_TABLES = {}          # (in, out, filter, device) -> (device table, ksize), least recently used first
RESAMPLE_TABLES_MAX = 64       # a few KiB each; a caller whose image sizes keep changing rebuilds tables instead of piling them up


def _resample_code(resample) -> int:
    code = RESAMPLE.get(resample.lower()) if isinstance(resample, str) else resample
    if isinstance(code, bool) or not isinstance(code, int) or code not in RESAMPLE.values():
        raise RuntimeError(f"resample {resample!r}: one of {sorted(RESAMPLE)} (or PIL's code of one of them)")
    return code


def resample_coeffs(in_size: int, out_size: int, resample="lanczos"):
    """The tables PIL's 8-bit resampler builds for one axis (tt_resample_coeffs; host only, no device): ``(ksize, bounds, kk)`` with
    bounds int32 [out_size, 2] = (first source index, taps) and kk int32 [out_size, ksize], the taps in 2^-22 fixed point."""
    import numpy as np
    lib = _lib.load()
    code, ksize = _resample_code(resample), C.c_int32(0)
    check(lib.tt_resample_coeffs(int(in_size), int(out_size), code, C.byref(ksize), None, None), "tt_resample_coeffs")
    bounds, kk = np.empty((int(out_size), 2), np.int32), np.empty((int(out_size), ksize.value), np.int32)
    i32p = C.POINTER(C.c_int32)
    check(lib.tt_resample_coeffs(int(in_size), int(out_size), code, C.byref(ksize), bounds.ctypes.data_as(i32p), kk.ctypes.data_as(i32p)),
          "tt_resample_coeffs")
    return ksize.value, bounds, kk


def _resample_table(in_size: int, out_size: int, code: int, device):
    """(device table, ksize) of one axis in the layout the kernels read (include/ttvdm.h: [out] first, [out] taps, [ksize][out] kk),
    (None, 0) for an axis that keeps its size.  Built and uploaded once per (in, out, filter, device); the RESAMPLE_TABLES_MAX most
    recently used are kept."""
    if in_size == out_size:
        return None, 0
    key = (int(in_size), int(out_size), code, torch.device(device))
    hit = _RESAMPLE_TABLES.pop(key, None)
    if hit is None:
        import numpy as np
        ksize, bounds, kk = resample_coeffs(in_size, out_size, code)
        hit = (torch.from_numpy(np.ascontiguousarray(np.concatenate([bounds.T, kk.T], 0))).to(device), ksize)
    _RESAMPLE_TABLES[key] = hit                       # (re)inserted last: the most recently used
    while len(_RESAMPLE_TABLES) > RESAMPLE_TABLES_MAX:
        # dropped, not retired like a workspace: the launches already on the stream keep the memory alive (the caching allocator reuses
        # a block in stream order); a captured graph must hold its own reference to the tables it replays
        del _RESAMPLE_TABLES[next(iter(_RESAMPLE_TABLES))]
    return hit


def _resample_args(name, src, size, resample):
    _p(src)
    if src.dtype != torch.uint8 or src.dim() not in (3, 4) or src.shape[-1] != 3:
        raise RuntimeError(f"{name}: the source is uint8 [N, H, W, 3] (or [H, W, 3]), got {src.dtype} {tuple(src.shape)}")
    src = (src[None] if src.dim() == 3 else src).contiguous()
    n, h, w = src.shape[:3]
    oh, ow = int(size[0]), int(size[1])
    if min(n, h, w, oh, ow) <= 0:
        raise RuntimeError(f"{name}: {n} image(s) of {h} x {w} -> {oh} x {ow}, every size must be positive")
    code = _resample_code(resample)
    tx, kx = _resample_table(w, ow, code, src.device)
    ty, ky = _resample_table(h, oh, code, src.device)
    return src, (n, h, w, oh, ow), (tx, kx, ty, ky)             # the tensors, not their addresses: the caller holds them across its launch


def resize_u8(src, size, resample="lanczos"):
    """``PIL.Image.resize((size[1], size[0]), resample)`` of RGB images on the device, byte for byte (tt_resize_u8): src uint8
    [N, H, W, 3] (or [H, W, 3]) -> uint8 [N, size[0], size[1], 3].  resample: "box", "bilinear", "hamming", "bicubic" or "lanczos"."""
    lib = _lib.load()
    src, dims, tabs = _resample_args("resize_u8", src, size, resample)
    out = torch.empty((dims[0], dims[3], dims[4], 3), dtype=torch.uint8, device=src.device)
    need = lib.tt_resize_u8_ws_bytes(*dims)
    ws = _workspace(need, src.device) if need else None
    tx, kx, ty, ky = tabs
    check(lib.tt_resize_u8(_p(src), *dims, _p(tx), kx, _p(ty), ky, _p(out), _p(ws), need, _stream()), "tt_resize_u8")
    _wrote(out, "resize_u8")
    return out


def vae_image(src, size, noise, noise_aug_strength, dtype, videos_per_image: int = 1, resample="lanczos"):
    """The VAE input of a request from its uint8 pixels (tt_vae_image): PIL's resize to `size`, ``2 * (u / 255) - 1``, each image
    repeated for its ``videos_per_image`` requests, ``+ noise_aug_strength * noise`` and the cast to `dtype` -- what
    ``VaeImageProcessor.preprocess``, ``repeat_interleave``, the noise augmentation and ``.to(dtype)`` compute, bit for bit.
    src uint8 [N, H, W, 3] (or [H, W, 3]); noise float32 [N * videos_per_image, 3, size[0], size[1]] on the device, or None.
    -> [N * videos_per_image, 3, size[0], size[1]] in `dtype`."""
    lib = _lib.load()
    src, dims, tabs = _resample_args("vae_image", src, size, resample)
    nvid = int(videos_per_image)
    if nvid < 1:
        raise RuntimeError(f"vae_image: {videos_per_image} videos per image")
    shape = (dims[0] * nvid, 3, dims[3], dims[4])
    if noise is not None:
        _p(noise)
        if noise.dtype != torch.float32 or tuple(noise.shape) != shape or noise.device != src.device:
            raise RuntimeError(f"vae_image: noise must be float32 {shape} on {src.device}, got {noise.dtype} {tuple(noise.shape)} on {noise.device}")
        noise = noise.contiguous()
    out = torch.empty(shape, dtype=dtype, device=src.device)
    need = lib.tt_vae_image_ws_bytes(*dims)
    ws = _workspace(need, src.device) if need else None
    tx, kx, ty, ky = tabs
    check(lib.tt_vae_image(_p(src), *dims, _p(tx), kx, _p(ty), ky, _p(noise), float(noise_aug_strength), nvid, _p(out), _code(dtype), _p(ws), need, _stream()),
          "tt_vae_image")
    _wrote(out, "vae_image")
    return out


# ---- the range audit's instrument (tt_tensor_stats; audit.py decodes the records and names the sites)
STATS_BYTES = C.sizeof(_lib.TtTensorStats)
# |x| >= 448: e4m3 saturates (on an e4m3 tensor: values sitting at the clip); >= 65520: rounds to inf in fp16; >= 65520 * 2^8: split16's
# high term h = fp16(x 2^-8) overflows; the fourth is free (default 2^15: within one binade of fp16's largest value)
STATS_THRESHOLDS = (448.0, 65520.0, 16773120.0, 32768.0)


def _stats_code(dt: torch.dtype) -> int:
    if dt == FP8:
        return _lib.TT_FP8_E4M3
    if dt in (torch.bfloat16, torch.float16, torch.float32):
        return _code(dt)
    raise RuntimeError(f"tensor_stats: bfloat16, float16, float32 or float8_e4m3fn, got {dt}")


def _rows_view(x: torch.Tensor):
    """(rows, cols, row stride) of x read as a row-strided 2-D tensor: the last dimension contiguous, the leading ones collapsing to
    one row stride; raises for any other layout."""
    dims = [(n, st) for n, st in zip(x.shape, x.stride()) if n != 1]
    if x.numel() == 0:
        return 0, 0, 0
    if not dims:
        return 1, 1, 1
    cols, st = dims[-1]
    if st != 1:
        raise RuntimeError(f"tensor_stats: the last dimension must be contiguous (shape {tuple(x.shape)}, strides {tuple(x.stride())})")
    lead = dims[:-1]
    if not lead:
        return 1, cols, cols
    for (_, s0), (n1, s1) in zip(lead[:-1], lead[1:]):
        if s0 != s1 * n1:
            raise RuntimeError(f"tensor_stats: the leading dimensions must collapse to one row stride (shape {tuple(x.shape)}, strides "
                               f"{tuple(x.stride())})")
    rows = 1
    for n, _ in lead:
        rows *= n
    ld = lead[-1][1]
    if ld < cols:
        raise RuntimeError(f"tensor_stats: rows overlap (shape {tuple(x.shape)}, strides {tuple(x.stride())})")
    if cols >= 1 << 31:
        raise RuntimeError(f"tensor_stats: {cols} columns; reshape the tensor to rows of fewer than 2^31 elements")
    return rows, cols, ld


def tensor_stats_launch(dtype: torch.dtype):
    """(most workgroups of a launch, lanes per workgroup, elements per 16-byte load of `dtype`): the constants tt_tensor_stats launches with"""
    g, b, e = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(_lib.load().tt_tensor_stats_launch(_stats_code(dtype), C.byref(g), C.byref(b), C.byref(e)), "tt_tensor_stats_launch")
    return g.value, b.value, e.value


def tensor_stats(x: torch.Tensor, *, thresholds=None, out: Optional[torch.Tensor] = None, slot: int = 0, accumulate: bool = False):
    """One pass over x (bf16 / fp16 / fp32 / float8_e4m3fn; last dimension contiguous, leading dimensions collapsing to one row stride)
    -> the TtTensorStats record (include/ttvdm.h) as a uint8 device tensor of STATS_BYTES bytes: record `slot` of ``out`` (a uint8 buffer
    of whole records) or a new one.  thresholds: four fp32 values for n_ge (default STATS_THRESHOLDS).  accumulate: merge into the record
    already there.  Asynchronous and capturable; ``audit.decode`` turns records into Python objects after one device-to-host copy."""
    lib = _lib.load()
    _p(x)
    rows, cols, ld = _rows_view(x)
    code = _stats_code(x.dtype)
    thr = thresholds if isinstance(thresholds, C.Array) else (C.c_float * 4)(*(STATS_THRESHOLDS if thresholds is None else thresholds))
    if len(thr) != 4:
        raise RuntimeError("tensor_stats: four thresholds")
    if out is None:
        if accumulate:
            raise RuntimeError("tensor_stats: accumulate needs the record to merge into (out=)")
        out = torch.empty(STATS_BYTES, dtype=torch.uint8, device=x.device)
        slot = 0
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.device != x.device or slot < 0 or (slot + 1) * STATS_BYTES > out.numel():
        raise RuntimeError(f"tensor_stats: out must be a contiguous uint8 tensor on {x.device} holding record {slot} ({STATS_BYTES} bytes each)")
    need = lib.tt_tensor_stats_ws_bytes(rows, cols, code)
    ws = _workspace(need, x.device) if need else None
    check(lib.tt_tensor_stats(x.data_ptr() if rows else None, ld, rows, cols, code, thr, out.data_ptr() + slot * STATS_BYTES, _p(ws), need,
                              int(bool(accumulate)), _stream()), "tt_tensor_stats")
    return out[slot * STATS_BYTES:(slot + 1) * STATS_BYTES]


# ---- two videos compared on the device (tt_frame_metrics / tt_frames_pool2; metrics.py turns the records into PSNR / SSIM / MS-SSIM)
METRICS_BYTES = C.sizeof(_lib.TtFrameMetricsRecord)


def _frames_kind(x: torch.Tensor, what: str) -> int:
    if x.dtype == torch.uint8:
        return 1
    if x.dtype == torch.float32:
        return 0
    raise RuntimeError(f"{what}: uint8 or float32 NHWC frames, got {x.dtype}")


def frame_metrics_window():
    """the 11 fp64 weights of the SSIM window as the kernel uses them (Gaussian, sigma 1.5, normalised)"""
    g = (C.c_double * 11)()
    check(_lib.load().tt_frame_metrics_window(g), "tt_frame_metrics_window")
    return list(g)


def frame_metrics_launch(dtype: torch.dtype):
    """(windows per tile edge, lanes per workgroup, elements per 16-byte load of `dtype`): the constants tt_frame_metrics launches with"""
    kind = 1 if dtype == torch.uint8 else 0
    t, b, e = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    check(_lib.load().tt_frame_metrics_launch(kind, C.byref(t), C.byref(b), C.byref(e)), "tt_frame_metrics_launch")
    return t.value, b.value, e.value


def frame_metrics(a: torch.Tensor, b: torch.Tensor, data_range=None, sse_only: bool = False, out: Optional[torch.Tensor] = None):
    """Frames a and b, [N, H, W, C] contiguous NHWC (C <= 4), both uint8 or both float32 (what ``frames_out`` writes) -> N
    TtFrameMetricsRecord records (include/ttvdm.h) as a uint8 device tensor [N, METRICS_BYTES]: per frame and channel the sum of squared
    differences and the sums of ssim and cs over the (H - 10) (W - 10) windows of the 11-tap Gaussian, all in fp64.  data_range: the L of
    C1 = (0.01 L)^2, C2 = (0.03 L)^2 (default 255 for uint8, 1 for float32).  sse_only: no window work (frames below 11 x 11 are
    served).  ``out``: a contiguous uint8 tensor of N records to write instead of a new one.  Asynchronous on the current stream and
    capturable; ``metrics.compare_frames`` reads the records after one device-to-host copy."""
    lib = _lib.load()
    _p(a), _p(b)
    kind = _frames_kind(a, "frame_metrics")
    if a.dim() != 4 or a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
        raise RuntimeError(f"frame_metrics: two [N, H, W, C] tensors of one shape, dtype and device, got {tuple(a.shape)} {a.dtype} and "
                           f"{tuple(b.shape)} {b.dtype}")
    if not (a.is_contiguous() and b.is_contiguous()):
        raise RuntimeError("frame_metrics: contiguous NHWC frames")
    n, h, w, ch = a.shape
    if data_range is None:
        data_range = 255.0 if kind else 1.0
    flags = _lib.TT_METRICS_SSE_ONLY if sse_only else 0
    if out is None:
        out = torch.empty((n, METRICS_BYTES), dtype=torch.uint8, device=a.device)
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.device != a.device or out.numel() != n * METRICS_BYTES:
        raise RuntimeError(f"frame_metrics: out must be a contiguous uint8 tensor on {a.device} of {n} records ({METRICS_BYTES} bytes each)")
    need = lib.tt_frame_metrics_ws_bytes(n, h, w, flags)
    ws = _workspace(need, a.device) if need else None
    check(lib.tt_frame_metrics(_p(a), _p(b), kind, n, h, w, ch, float(data_range), flags, _p(out), _p(ws), need, _stream()), "tt_frame_metrics")
    _wrote(out, "frame_metrics")
    return out.view(n, METRICS_BYTES)


def frames_pool2(x: torch.Tensor):
    """[N, H, W, C] uint8 or float32 NHWC frames (H, W even) -> float32 [N, H / 2, W / 2, C], the 2 x 2 mean
    ``0.25f * ((x00 + x01) + (x10 + x11))`` in fp32: one level of the MS-SSIM pyramid (tt_frames_pool2)."""
    lib = _lib.load()
    _p(x)
    kind = _frames_kind(x, "frames_pool2")
    if x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError(f"frames_pool2: contiguous [N, H, W, C] frames, got {tuple(x.shape)}")
    n, h, w, ch = x.shape
    out = torch.empty((n, h // 2, w // 2, ch), dtype=torch.float32, device=x.device)
    check(lib.tt_frames_pool2(_p(x), kind, n, h, w, ch, _p(out), _stream()), "tt_frames_pool2")
    _wrote(out, "frames_pool2")
    return out


# ---- the GIF export's device half (tt_color_hist / tt_palette_map; export.py drives them and holds the host half)
COLOR_BINS = _lib.TT_GIF_BINS


def _rgb_frames(x: torch.Tensor, what: str):
    _p(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
        raise RuntimeError(f"{what}: contiguous uint8 [N, H, W, 3] frames, got {tuple(x.shape)} {x.dtype}")
    return x.shape


def color_hist(frames: torch.Tensor, per_frame: bool = True, out: Optional[torch.Tensor] = None):
    """uint8 NHWC frames [N, H, W, 3] -> int32 device tensor [N or 1, 32768, 4]: per bin ``r5 << 10 | g5 << 5 | b5`` (the top five bits
    of each channel) the pixels it holds and the sums of their full 8-bit R, G and B (the bits are uint32: TtColorBin, include/ttvdm.h).
    ``per_frame=False``: one histogram over all frames.  Exact integers; the same bits every call.  Asynchronous on the current stream."""
    lib = _lib.load()
    n, h, w, ch = _rgb_frames(frames, "color_hist")
    nhist = n if per_frame else 1
    if out is None:
        out = torch.empty((nhist, COLOR_BINS, 4), dtype=torch.int32, device=frames.device)
    if out.dtype != torch.int32 or not out.is_contiguous() or out.device != frames.device or tuple(out.shape) != (nhist, COLOR_BINS, 4):
        raise RuntimeError(f"color_hist: out must be a contiguous int32 tensor [{nhist}, {COLOR_BINS}, 4] on {frames.device}")
    check(lib.tt_color_hist(_p(frames), n, h, w, ch, nhist, _p(out), _stream()), "tt_color_hist")
    _wrote(out, "color_hist")
    return out


def palette_map(frames: torch.Tensor, palettes: torch.Tensor, ncolors, stats: bool = False):
    """uint8 NHWC frames [N, H, W, 3], device palettes uint8 [N or 1, 256, 3] and ``ncolors`` (host integers, one per palette, 1 .. 256)
    -> (indices uint8 [N, H, W], sse int64 [N], stats): every pixel's nearest entry among the first ``ncolors`` of its frame's palette
    (squared RGB distance, the lowest index on a tie), per frame the exact sum of those squared distances, and with ``stats=True`` an
    int32 tensor [N or 1, 256, 4] of (pixels, sum R, sum G, sum B) per entry (uint32 bits), else None -- all on the device (tt_palette_map)."""
    lib = _lib.load()
    n, h, w, ch = _rgb_frames(frames, "palette_map")
    _p(palettes)
    if palettes.dtype != torch.uint8 or palettes.dim() != 3 or tuple(palettes.shape[1:]) != (256, 3) or not palettes.is_contiguous() \
            or palettes.device != frames.device:
        raise RuntimeError(f"palette_map: palettes must be a contiguous uint8 tensor [N or 1, 256, 3] on {frames.device}, got "
                           f"{tuple(palettes.shape)} {palettes.dtype}")
    npal = palettes.shape[0]
    counts = [int(c) for c in ncolors]
    if len(counts) != npal:
        raise RuntimeError(f"palette_map: {len(counts)} ncolors for {npal} palettes")
    nc = (C.c_int32 * npal)(*counts)
    indices = torch.empty((n, h, w), dtype=torch.uint8, device=frames.device)
    sse = torch.empty((n,), dtype=torch.int64, device=frames.device)
    rec = torch.empty((npal, 256, 4), dtype=torch.int32, device=frames.device) if stats else None
    check(lib.tt_palette_map(_p(frames), n, h, w, ch, _p(palettes), npal, nc, _p(indices), _p(sse), _p(rec), _stream()), "tt_palette_map")
    _wrote(indices, "palette_map")
    return indices, sse, rec


def gif_lzw(indices: torch.Tensor, min_code_size, segment: Optional[int] = None):
    """Device uint8 indices [N, H, W] or [N, npix] and ``min_code_size`` (an int, or one per frame: a sequence or an int32 device tensor
    [N]) -> (data uint8 [N, bound], lengths int32 [N], status int32 [N]), all on the device: frame f's finished GIF image data -- the
    min-code-size byte, the sub-blocks, the terminator -- is ``data[f, :lengths[f]]``, coded in independent segments of ``segment`` pixels
    (None: the built default, TT_LZW_SEGMENT; with ``segment >= npix`` the bytes are tt_gif_lzw's).  ``status[f]`` is 0, or says that the
    frame held an index that does not fit its min_code_size (1) or a min_code_size outside 2 .. 8 (2): its stream is then meaningless.
    Bytes behind a frame's length are not written (tt_gif_lzw_frames).  Asynchronous on the current stream."""
    lib = _lib.load()
    _p(indices)
    if indices.dtype != torch.uint8 or indices.dim() not in (2, 3) or not indices.is_contiguous() or indices.numel() == 0:
        raise RuntimeError(f"gif_lzw: contiguous uint8 indices [N, H, W] or [N, npix], got {tuple(indices.shape)} {indices.dtype}")
    n, npix = indices.shape[0], indices[0].numel()
    seg = 0 if segment is None else int(segment)
    if segment is not None and not 1 <= seg <= _lib.TT_LZW_SEGMENT_MAX:
        raise RuntimeError(f"gif_lzw: segment = {segment!r} (1 to {_lib.TT_LZW_SEGMENT_MAX}, or None for the default {_lib.TT_LZW_SEGMENT})")
    if torch.is_tensor(min_code_size):
        mcs = min_code_size
        _p(mcs)
        if mcs.dtype != torch.int32 or mcs.dim() != 1 or mcs.numel() not in (1, n) or not mcs.is_contiguous() or mcs.device != indices.device:
            raise RuntimeError(f"gif_lzw: min_code_size must be a contiguous int32 tensor [1 or {n}] on {indices.device}, got "
                               f"{tuple(mcs.shape)} {mcs.dtype}")
    else:
        values = [int(min_code_size)] if isinstance(min_code_size, int) else [int(v) for v in min_code_size]
        if len(values) not in (1, n):
            raise RuntimeError(f"gif_lzw: {len(values)} min_code_size values for {n} frames (one, or one per frame)")
        mcs = torch.tensor(values, dtype=torch.int32).to(indices.device)
    bound = lib.tt_gif_lzw_frames_bound(npix, seg)
    ws_bytes = lib.tt_gif_lzw_frames_ws_bytes(n, npix, seg)
    data = torch.empty((n, max(int(bound), 16)), dtype=torch.uint8, device=indices.device)
    lengths = torch.empty((n,), dtype=torch.int32, device=indices.device)
    status = torch.empty((n,), dtype=torch.int32, device=indices.device)
    ws = torch.empty((max(int(ws_bytes), 16),), dtype=torch.uint8, device=indices.device)
    check(lib.tt_gif_lzw_frames(_p(indices), n, npix, _p(mcs), mcs.numel(), seg, _p(data), data.numel(), _p(lengths), _p(status), _p(ws), ws.numel(),
                                _stream()), "tt_gif_lzw_frames")
    for t in (data, lengths, status):
        _wrote(t, "gif_lzw")
    return data, lengths, status


# ---- the PNG export's device half (tt_png_filter / tt_png_tokens / tt_png_emit; export.py drives them and holds the host half)
PNG_FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}


def _png_shape(shape, what: str):
    h, w, ch = (int(v) for v in shape)
    if h <= 0 or w <= 0 or not 1 <= ch <= 4:
        raise RuntimeError(f"{what}: shape (h, w, ch) with 1 to 4 channels, got {tuple(shape)}")
    return h, w, ch


def _png_filtered(filtered: torch.Tensor, shape, what: str):
    lib = _lib.load()
    h, w, ch = _png_shape(shape, what)
    _p(filtered)
    stride = lib.tt_png_frame_stride(h, w, ch)
    if filtered.dtype != torch.uint8 or filtered.dim() != 2 or filtered.shape[1] != stride or not filtered.is_contiguous() or filtered.shape[0] < 1:
        raise RuntimeError(f"{what}: filtered must be a contiguous uint8 tensor [N, {stride}] (png_filter's), got {tuple(filtered.shape)} {filtered.dtype}")
    return lib, filtered.shape[0], h, w, ch, lib.tt_png_stripes(h, w, ch)


def png_filter(frames: torch.Tensor, filter=5):
    """uint8 NHWC frames [N, H, W, C], C 1 .. 4 -> uint8 device tensor [N, stride]: per frame the PNG-filtered stream of H (1 + W C) bytes,
    every row its filter-type byte and its filtered bytes; stride rounds that up to 16 and the padding is not written.  ``filter``: 0 .. 4
    (none, sub, up, average, paeth on every row), 5 (per row the type with the least sum of |signed byte|, the lowest on a tie), or one
    of those names (tt_png_filter).  Asynchronous on the current stream."""
    lib = _lib.load()
    _p(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or not frames.is_contiguous():
        raise RuntimeError(f"png_filter: contiguous uint8 [N, H, W, C] frames, got {tuple(frames.shape)} {frames.dtype}")
    kind = PNG_FILTERS.get(filter, filter)
    if not isinstance(kind, int) or isinstance(kind, bool) or not 0 <= kind <= 5:
        raise RuntimeError(f"png_filter: filter {filter!r} (0 to 5, or one of {sorted(PNG_FILTERS)})")
    n, h, w, ch = frames.shape
    _png_shape((h, w, ch), "png_filter")
    out = torch.empty((n, lib.tt_png_frame_stride(h, w, ch)), dtype=torch.uint8, device=frames.device)
    check(lib.tt_png_filter(_p(frames), n, h, w, ch, kind, _p(out), _stream()), "tt_png_filter")
    _wrote(out, "png_filter")
    return out


def png_tokens(filtered: torch.Tensor, shape):
    """``png_filter``'s output for frames of ``shape`` (h, w, ch) -> int32 device tensor [N stripes, 288] (uint32 bits): per 32 KiB stripe
    of every frame's stream the counts of the 286 literal/length symbols its run tokens use and its Adler-32 pair (tt_png_tokens)."""
    lib, n, h, w, ch, stripes = _png_filtered(filtered, shape, "png_tokens")
    rec = torch.empty((n * stripes, _lib.TT_PNG_RECORD_WORDS), dtype=torch.int32, device=filtered.device)
    check(lib.tt_png_tokens(_p(filtered), n, h, w, ch, _p(rec), _stream()), "tt_png_tokens")
    _wrote(rec, "png_tokens")
    return rec


def png_emit(filtered: torch.Tensor, shape, tables: torch.Tensor, headers: torch.Tensor, out_bytes: int):
    """``png_filter``'s output, and per stripe the code table with its byte offset [N stripes, 288] and the block header [N stripes, 72]
    (int32 device tensors holding what tt_png_plan made) -> uint8 device tensor [out_bytes]: every stripe's DEFLATE block followed by an
    empty stored block, at its offset (tt_png_emit)."""
    lib, n, h, w, ch, stripes = _png_filtered(filtered, shape, "png_emit")
    for t, words, name in ((tables, _lib.TT_PNG_TABLE_WORDS, "tables"), (headers, _lib.TT_PNG_HEADER_WORDS, "headers")):
        _p(t)
        if t.dtype != torch.int32 or tuple(t.shape) != (n * stripes, words) or not t.is_contiguous() or t.device != filtered.device:
            raise RuntimeError(f"png_emit: {name} must be a contiguous int32 tensor [{n * stripes}, {words}] on {filtered.device}, got "
                               f"{tuple(t.shape)} {t.dtype}")
    out = torch.empty((int(out_bytes),), dtype=torch.uint8, device=filtered.device)
    check(lib.tt_png_emit(_p(filtered), n, h, w, ch, _p(tables), _p(headers), _p(out), int(out_bytes), out.numel(), _stream()), "tt_png_emit")
    _wrote(out, "png_emit")
    return out


# ---- the JPEG export's device half (tt_jpeg_coeffs / tt_jpeg_scan; export.py drives them and holds the tables and the file layer)
JPEG_SUBSAMPLING = {"4:4:4": _lib.TT_JPEG_444, "4:2:0": _lib.TT_JPEG_420}


def _jpeg_shape(shape, subsampling, what: str):
    h, w, ch = (int(v) for v in shape)
    if h <= 0 or w <= 0 or ch not in (1, 3):
        raise RuntimeError(f"{what}: shape (h, w, ch) with 1 (grey) or 3 (RGB) channels -- JPEG has no alpha --, got {tuple(shape)}")
    sub = JPEG_SUBSAMPLING.get(subsampling, subsampling)
    if isinstance(sub, bool) or sub not in (_lib.TT_JPEG_444, _lib.TT_JPEG_420):
        raise RuntimeError(f"{what}: subsampling {subsampling!r} (one of {sorted(JPEG_SUBSAMPLING)}, or 0 / 2)")
    return h, w, ch, sub


def jpeg_coeffs(frames: torch.Tensor, quality: int = 75, subsampling="4:2:0", counts: bool = True):
    """uint8 NHWC frames [N, H, W, C], C 1 or 3 -> (int16 device tensor [N, blocks, 64]: every 8 x 8 block's quantised DCT coefficients
    in zig-zag order, blocks in scan order with the 4:2:0 dummy blocks; int32 device tensor [N, 4, 256] (uint32 bits) of the frames'
    symbol counts -- DC luminance, AC luminance, DC chrominance, AC chrominance -- or None with ``counts=False``) (tt_jpeg_coeffs).
    Asynchronous on the current stream."""
    lib = _lib.load()
    _p(frames)
    if frames.dtype != torch.uint8 or frames.dim() != 4 or not frames.is_contiguous() or frames.shape[0] < 1:
        raise RuntimeError(f"jpeg_coeffs: contiguous uint8 [N, H, W, C] frames, got {tuple(frames.shape)} {frames.dtype}")
    n = frames.shape[0]
    h, w, ch, sub = _jpeg_shape(frames.shape[1:], subsampling, "jpeg_coeffs")
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise RuntimeError(f"jpeg_coeffs: quality {quality!r} (an integer, 1 to 100)")
    coeffs = torch.empty((n, lib.tt_jpeg_blocks(h, w, ch, sub), 64), dtype=torch.int16, device=frames.device)
    cnt = torch.empty((n, 4, _lib.TT_JPEG_TABLE_WORDS), dtype=torch.int32, device=frames.device) if counts else None
    check(lib.tt_jpeg_coeffs(_p(frames), n, h, w, ch, quality, sub, _p(coeffs), _p(cnt), _stream()), "tt_jpeg_coeffs")
    _wrote(coeffs, "jpeg_coeffs")
    if cnt is not None:
        _wrote(cnt, "jpeg_coeffs")
    return coeffs, cnt


def _jpeg_restart(restart_interval, what: str) -> int:
    if isinstance(restart_interval, bool) or not isinstance(restart_interval, int) or not 0 <= restart_interval <= 65535:
        raise RuntimeError(f"{what}: restart_interval {restart_interval!r} (an integer: 0 for none, to 65535 MCUs)")
    return restart_interval


def jpeg_counts_restart(coeffs: torch.Tensor, shape, subsampling, restart_interval: int) -> torch.Tensor:
    """``jpeg_coeffs``' coefficients -> int32 device tensor [N, 4, 256] (uint32 bits): the frames' symbol counts with the DC predictors
    reset every ``restart_interval`` MCUs (tt_jpeg_counts_restart); 0 gives ``jpeg_coeffs``' own counts."""
    lib = _lib.load()
    h, w, ch, sub = _jpeg_shape(shape, subsampling, "jpeg_counts_restart")
    ri = _jpeg_restart(restart_interval, "jpeg_counts_restart")
    _p(coeffs)
    blocks = lib.tt_jpeg_blocks(h, w, ch, sub)
    if coeffs.dtype != torch.int16 or coeffs.dim() != 3 or tuple(coeffs.shape[1:]) != (blocks, 64) or not coeffs.is_contiguous() or coeffs.shape[0] < 1:
        raise RuntimeError(f"jpeg_counts_restart: coeffs must be a contiguous int16 tensor [N, {blocks}, 64] (jpeg_coeffs'), got {tuple(coeffs.shape)} {coeffs.dtype}")
    n = coeffs.shape[0]
    cnt = torch.empty((n, 4, _lib.TT_JPEG_TABLE_WORDS), dtype=torch.int32, device=coeffs.device)
    check(lib.tt_jpeg_counts_restart(_p(coeffs), n, h, w, ch, sub, ri, _p(cnt), _stream()), "tt_jpeg_counts_restart")
    _wrote(cnt, "jpeg_counts_restart")
    return cnt


def jpeg_scan(coeffs: torch.Tensor, shape, subsampling, tables: torch.Tensor, restart_interval: int = 0):
    """``jpeg_coeffs``' coefficients for frames of ``shape`` (h, w, ch) and code tables [1 or N, 4, 256] (int32 device tensor: per symbol
    code | length << 16, what export.jpeg_standard_tables / jpeg_optimized_tables make) -> (uint8 device tensor [N, stride]: every
    frame's finished, byte-stuffed scan; int32 device tensor [N]: its length; bytes behind it are not written) (tt_jpeg_scan).  With
    ``restart_interval`` > 0 the scan carries a restart marker every that many MCUs (tt_jpeg_scan_restart; the stride grows by them)."""
    lib = _lib.load()
    h, w, ch, sub = _jpeg_shape(shape, subsampling, "jpeg_scan")
    ri = _jpeg_restart(restart_interval, "jpeg_scan")
    _p(coeffs)
    blocks = lib.tt_jpeg_blocks(h, w, ch, sub)
    if coeffs.dtype != torch.int16 or coeffs.dim() != 3 or tuple(coeffs.shape[1:]) != (blocks, 64) or not coeffs.is_contiguous() or coeffs.shape[0] < 1:
        raise RuntimeError(f"jpeg_scan: coeffs must be a contiguous int16 tensor [N, {blocks}, 64] (jpeg_coeffs'), got {tuple(coeffs.shape)} {coeffs.dtype}")
    n = coeffs.shape[0]
    _p(tables)
    if tables.dtype != torch.int32 or tables.dim() != 3 or tuple(tables.shape[1:]) != (4, _lib.TT_JPEG_TABLE_WORDS) or tables.shape[0] not in (1, n) \
            or not tables.is_contiguous() or tables.device != coeffs.device:
        raise RuntimeError(f"jpeg_scan: tables must be a contiguous int32 tensor [1 or {n}, 4, {_lib.TT_JPEG_TABLE_WORDS}] on {coeffs.device}, got "
                           f"{tuple(tables.shape)} {tables.dtype}")
    stride = lib.tt_jpeg_scan_bound_restart(h, w, ch, sub, ri) if ri else lib.tt_jpeg_scan_bound(h, w, ch, sub)
    out = torch.empty((n, stride), dtype=torch.uint8, device=coeffs.device)
    lengths = torch.empty((n,), dtype=torch.int32, device=coeffs.device)
    if ri:
        ws = torch.empty((lib.tt_jpeg_scan_restart_ws_bytes(n, h, w, ch, sub, ri),), dtype=torch.uint8, device=coeffs.device)
        check(lib.tt_jpeg_scan_restart(_p(coeffs), n, h, w, ch, sub, ri, _p(tables), tables.shape[0], _p(out), out.numel(), _p(lengths), _p(ws), ws.numel(),
                                       _stream()), "tt_jpeg_scan_restart")
    else:
        ws = torch.empty((lib.tt_jpeg_scan_ws_bytes(n, h, w, ch, sub),), dtype=torch.uint8, device=coeffs.device)
        check(lib.tt_jpeg_scan(_p(coeffs), n, h, w, ch, sub, _p(tables), tables.shape[0], _p(out), out.numel(), _p(lengths), _p(ws), ws.numel(), _stream()),
              "tt_jpeg_scan")
    _wrote(out, "jpeg_scan")
    _wrote(lengths, "jpeg_scan")
    return out, lengths


# ---- the JPEG import's device half (tt_jpeg_entropy / tt_jpeg_pixels; ingest.py parses the files and builds the tables)
def jpeg_entropy(scans: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, max_bytes: int, shape, subsampling, tables: torch.Tensor):
    """Byte-stuffed scans -> (int16 device tensor [N, blocks, 64]: ``jpeg_coeffs``' layout; int32 device tensor [N]: every frame's status
    bits, 0 for a clean decode) (tt_jpeg_entropy).  ``scans``: uint8 device tensor holding frame f's scan at byte ``offsets[f]`` (int64
    device tensor [N]; any layout, ``jpeg_scan``'s [N, stride] rows among them) with ``lengths[f]`` bytes (int32 device tensor [N]);
    ``max_bytes``: a host integer no length exceeds; ``tables``: int32 device tensor [1 or N, 1028] of decode-table sets
    (ingest.jpeg_decode_set).  Asynchronous on the current stream."""
    lib = _lib.load()
    h, w, ch, sub = _jpeg_shape(shape, subsampling, "jpeg_entropy")
    for t in (scans, offsets, lengths, tables):
        _p(t)
    if scans.dtype != torch.uint8 or not scans.is_contiguous() or scans.numel() < 1:
        raise RuntimeError(f"jpeg_entropy: scans must be a contiguous uint8 tensor, got {tuple(scans.shape)} {scans.dtype}")
    n = offsets.numel()
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or n < 1 or not offsets.is_contiguous() or lengths.dtype != torch.int32 \
            or tuple(lengths.shape) != (n,) or not lengths.is_contiguous():
        raise RuntimeError(f"jpeg_entropy: offsets int64 [N] and lengths int32 [N], got {tuple(offsets.shape)} {offsets.dtype} and "
                           f"{tuple(lengths.shape)} {lengths.dtype}")
    if tables.dtype != torch.int32 or tables.dim() != 2 or tables.shape[1] != _lib.TT_JPEG_DECODE_SET_WORDS or tables.shape[0] not in (1, n) \
            or not tables.is_contiguous():
        raise RuntimeError(f"jpeg_entropy: tables must be a contiguous int32 tensor [1 or {n}, {_lib.TT_JPEG_DECODE_SET_WORDS}], got "
                           f"{tuple(tables.shape)} {tables.dtype}")
    if any(t.device != scans.device for t in (offsets, lengths, tables)):
        raise RuntimeError("jpeg_entropy: scans, offsets, lengths and tables must be on one device")
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 1:
        raise RuntimeError(f"jpeg_entropy: max_bytes {max_bytes!r} (a positive integer)")
    coeffs = torch.empty((n, lib.tt_jpeg_blocks(h, w, ch, sub), 64), dtype=torch.int16, device=scans.device)
    status = torch.empty((n,), dtype=torch.int32, device=scans.device)
    ws = torch.empty((max(lib.tt_jpeg_entropy_ws_bytes(n, max_bytes), 16),), dtype=torch.uint8, device=scans.device)
    check(lib.tt_jpeg_entropy(_p(scans), scans.numel(), _p(offsets), _p(lengths), max_bytes, n, h, w, ch, sub, _p(tables), tables.shape[0], _p(coeffs),
                              _p(status), _p(ws), ws.numel(), _stream()), "tt_jpeg_entropy")
    _wrote(coeffs, "jpeg_entropy")
    _wrote(status, "jpeg_entropy")
    return coeffs, status


def jpeg_entropy_spans(scans: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, span_frame: torch.Tensor, span_first: torch.Tensor,
                       span_blocks: torch.Tensor, max_bytes: int, frames: int, shape, subsampling, tables: torch.Tensor):
    """``jpeg_entropy`` per SPAN -- the stretch of a scan between two restart markers -- instead of per frame: one workgroup a span
    (tt_jpeg_entropy_spans).  Span s is ``offsets[s]`` / ``lengths[s]`` of ``scans`` (int64 / int32 device tensors [S]), belongs to frame
    ``span_frame[s]`` and holds ``span_blocks[s]`` blocks from block ``span_first[s]`` of it (int32 device tensors [S]); ``max_bytes``: a
    host integer no span's length exceeds; ``frames``: N; ``tables``: int32 [1 or N, 1028].  -> (coeffs int16 [N, blocks, 64], status int32
    [N], per FRAME).  At most 65535 spans a call."""
    lib = _lib.load()
    h, w, ch, sub = _jpeg_shape(shape, subsampling, "jpeg_entropy_spans")
    for t in (scans, offsets, lengths, span_frame, span_first, span_blocks, tables):
        _p(t)
    if scans.dtype != torch.uint8 or not scans.is_contiguous() or scans.numel() < 1:
        raise RuntimeError(f"jpeg_entropy_spans: scans must be a contiguous uint8 tensor, got {tuple(scans.shape)} {scans.dtype}")
    s = offsets.numel()
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or s < 1 or not offsets.is_contiguous():
        raise RuntimeError(f"jpeg_entropy_spans: offsets int64 [S], got {tuple(offsets.shape)} {offsets.dtype}")
    for name, t in (("lengths", lengths), ("span_frame", span_frame), ("span_first", span_first), ("span_blocks", span_blocks)):
        if t.dtype != torch.int32 or tuple(t.shape) != (s,) or not t.is_contiguous():
            raise RuntimeError(f"jpeg_entropy_spans: {name} int32 [{s}], got {tuple(t.shape)} {t.dtype}")
    if s > _lib.TT_JPEG_MAX_SPANS:
        raise RuntimeError(f"jpeg_entropy_spans: {s} spans in one call (at most {_lib.TT_JPEG_MAX_SPANS})")
    n = frames
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise RuntimeError(f"jpeg_entropy_spans: frames {frames!r} (a positive integer)")
    if tables.dtype != torch.int32 or tables.dim() != 2 or tables.shape[1] != _lib.TT_JPEG_DECODE_SET_WORDS or tables.shape[0] not in (1, n) \
            or not tables.is_contiguous():
        raise RuntimeError(f"jpeg_entropy_spans: tables must be a contiguous int32 tensor [1 or {n}, {_lib.TT_JPEG_DECODE_SET_WORDS}], got "
                           f"{tuple(tables.shape)} {tables.dtype}")
    if any(t.device != scans.device for t in (offsets, lengths, span_frame, span_first, span_blocks, tables)):
        raise RuntimeError("jpeg_entropy_spans: scans, the span arrays and tables must be on one device")
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 1:
        raise RuntimeError(f"jpeg_entropy_spans: max_bytes {max_bytes!r} (a positive integer)")
    coeffs = torch.empty((n, lib.tt_jpeg_blocks(h, w, ch, sub), 64), dtype=torch.int16, device=scans.device)
    status = torch.empty((n,), dtype=torch.int32, device=scans.device)
    ws = torch.empty((max(lib.tt_jpeg_entropy_ws_bytes(s, max_bytes), 16),), dtype=torch.uint8, device=scans.device)
    check(lib.tt_jpeg_entropy_spans(_p(scans), scans.numel(), _p(offsets), _p(lengths), _p(span_frame), _p(span_first), _p(span_blocks), max_bytes, s, n, h, w,
                                    ch, sub, _p(tables), tables.shape[0], _p(coeffs), _p(status), _p(ws), ws.numel(), _stream()), "tt_jpeg_entropy_spans")
    _wrote(coeffs, "jpeg_entropy_spans")
    _wrote(status, "jpeg_entropy_spans")
    return coeffs, status


def jpeg_entropy_progressive(scans: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, desc: torch.Tensor, tables: torch.Tensor, max_bytes: int,
                             frames: int, shape, subsampling):
    """The scans of N progressive frames -> (coeffs int16 [N, blocks, 64], status int32 [N]) as ``jpeg_entropy`` gives them
    (tt_jpeg_entropy_progressive).  Item f S + s is scan s of frame f, S = the most scans a frame of the call has: ``offsets`` / ``lengths``
    (int64 / int32 device tensors [N S]) place its stuffed segment in ``scans``; ``desc`` int32 [N S, 8] = component mask, Ss, Se, Ah, Al,
    0, 0, 0 (mask 0: the frame has no scan s); ``tables`` int32 [N S, 3, 256]: a DC-first scan's DC table of component c at [c], an AC
    scan's table at [0] (ingest.jpeg_decode_table).  ``max_bytes``: a host integer no length exceeds.  Asynchronous on the current stream."""
    lib = _lib.load()
    h, w, ch, sub = _jpeg_shape(shape, subsampling, "jpeg_entropy_progressive")
    for t in (scans, offsets, lengths, desc, tables):
        _p(t)
    if scans.dtype != torch.uint8 or not scans.is_contiguous() or scans.numel() < 1:
        raise RuntimeError(f"jpeg_entropy_progressive: scans must be a contiguous uint8 tensor, got {tuple(scans.shape)} {scans.dtype}")
    n = frames
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise RuntimeError(f"jpeg_entropy_progressive: frames {frames!r} (a positive integer)")
    items = offsets.numel()
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or items < 1 or items % n or not offsets.is_contiguous():
        raise RuntimeError(f"jpeg_entropy_progressive: offsets int64 [{n} x scans], got {tuple(offsets.shape)} {offsets.dtype}")
    nscans = items // n
    if nscans > _lib.TT_JPEG_MAX_SCANS or items > _lib.TT_JPEG_MAX_ITEMS:
        raise RuntimeError(f"jpeg_entropy_progressive: {n} frames of {nscans} scans (at most {_lib.TT_JPEG_MAX_SCANS} scans a frame, {_lib.TT_JPEG_MAX_ITEMS} in all)")
    if lengths.dtype != torch.int32 or tuple(lengths.shape) != (items,) or not lengths.is_contiguous():
        raise RuntimeError(f"jpeg_entropy_progressive: lengths int32 [{items}], got {tuple(lengths.shape)} {lengths.dtype}")
    if desc.dtype != torch.int32 or tuple(desc.shape) != (items, _lib.TT_JPEG_SCAN_WORDS) or not desc.is_contiguous():
        raise RuntimeError(f"jpeg_entropy_progressive: desc int32 [{items}, {_lib.TT_JPEG_SCAN_WORDS}], got {tuple(desc.shape)} {desc.dtype}")
    if tables.dtype != torch.int32 or tuple(tables.shape) != (items, 3, _lib.TT_JPEG_DECODE_WORDS) or not tables.is_contiguous():
        raise RuntimeError(f"jpeg_entropy_progressive: tables int32 [{items}, 3, {_lib.TT_JPEG_DECODE_WORDS}], got {tuple(tables.shape)} {tables.dtype}")
    if any(t.device != scans.device for t in (offsets, lengths, desc, tables)):
        raise RuntimeError("jpeg_entropy_progressive: scans, offsets, lengths, desc and tables must be on one device")
    if isinstance(max_bytes, bool) or not isinstance(max_bytes, int) or max_bytes < 1:
        raise RuntimeError(f"jpeg_entropy_progressive: max_bytes {max_bytes!r} (a positive integer)")
    coeffs = torch.empty((n, lib.tt_jpeg_blocks(h, w, ch, sub), 64), dtype=torch.int16, device=scans.device)
    status = torch.empty((n,), dtype=torch.int32, device=scans.device)
    ws = torch.empty((max(lib.tt_jpeg_entropy_progressive_ws_bytes(n, nscans, max_bytes, h, w, ch, sub), 16),), dtype=torch.uint8, device=scans.device)
    check(lib.tt_jpeg_entropy_progressive(_p(scans), scans.numel(), _p(offsets), _p(lengths), _p(desc), _p(tables), max_bytes, n, nscans, h, w, ch, sub,
                                          _p(coeffs), _p(status), _p(ws), ws.numel(), _stream()), "tt_jpeg_entropy_progressive")
    _wrote(coeffs, "jpeg_entropy_progressive")
    _wrote(status, "jpeg_entropy_progressive")
    return coeffs, status


def jpeg_pixels(coeffs: torch.Tensor, shape, subsampling, quant: torch.Tensor) -> torch.Tensor:
    """``jpeg_entropy``'s (or ``jpeg_coeffs``') coefficients of frames of ``shape`` (h, w, ch) and quantiser tables [1 or N, 3, 64] (uint8
    device tensor: per component, natural order) -> uint8 device tensor [N, h, w, ch]: dequantised, inverse DCT, 4:2:0 chroma upsampled,
    converted to RGB -- libjpeg's decoded pixels (tt_jpeg_pixels).  Asynchronous on the current stream."""
    lib = _lib.load()
    h, w, ch, sub = _jpeg_shape(shape, subsampling, "jpeg_pixels")
    _p(coeffs)
    blocks = lib.tt_jpeg_blocks(h, w, ch, sub)
    if coeffs.dtype != torch.int16 or coeffs.dim() != 3 or tuple(coeffs.shape[1:]) != (blocks, 64) or not coeffs.is_contiguous() or coeffs.shape[0] < 1:
        raise RuntimeError(f"jpeg_pixels: coeffs must be a contiguous int16 tensor [N, {blocks}, 64], got {tuple(coeffs.shape)} {coeffs.dtype}")
    n = coeffs.shape[0]
    _p(quant)
    if quant.dtype != torch.uint8 or quant.dim() != 3 or tuple(quant.shape[1:]) != (3, 64) or quant.shape[0] not in (1, n) or not quant.is_contiguous() \
            or quant.device != coeffs.device:
        raise RuntimeError(f"jpeg_pixels: quant must be a contiguous uint8 tensor [1 or {n}, 3, 64] on {coeffs.device}, got {tuple(quant.shape)} {quant.dtype}")
    frames = torch.empty((n, h, w, ch), dtype=torch.uint8, device=coeffs.device)
    check(lib.tt_jpeg_pixels(_p(coeffs), n, h, w, ch, sub, _p(quant), quant.shape[0], _p(frames), _stream()), "tt_jpeg_pixels")
    _wrote(frames, "jpeg_pixels")
    return frames


# ---- the GIF import's device half (tt_gif_decode_indices / tt_gif_compose; ingest.py parses the file and builds the tables)
def gif_indices(data: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, npix: torch.Tensor, min_code_size: torch.Tensor, rows: torch.Tensor,
                map_offsets: torch.Tensor, maps_bytes: int):
    """The LZW bytes of N images -> (uint8 device tensor [maps_bytes]: image f's w h indices in raster order, interlace undone, at
    ``map_offsets[f]``; int32 device tensor [N]: every image's status bits, 0 for a clean decode) (tt_gif_decode_indices).  ``data``: uint8
    device tensor holding image f's bytes at ``offsets[f]`` (int64 [N]) with ``lengths[f]`` bytes; ``npix[f]`` = w h; ``min_code_size[f]``;
    ``rows[f]``: the height of an interlaced image, else 0 (int32 device tensors [N]); ``map_offsets``: int64 [N]; ``maps_bytes``: a host
    integer.  Asynchronous on the current stream."""
    lib = _lib.load()
    for t in (data, offsets, lengths, npix, min_code_size, rows, map_offsets):
        _p(t)
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous() or data.numel() < 1:
        raise RuntimeError(f"gif_indices: data must be a contiguous uint8 tensor [bytes], got {tuple(data.shape)} {data.dtype}")
    n = offsets.numel()
    for name, t, dt in (("offsets", offsets, torch.int64), ("map_offsets", map_offsets, torch.int64), ("lengths", lengths, torch.int32), ("npix", npix, torch.int32),
                        ("min_code_size", min_code_size, torch.int32), ("rows", rows, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (n,) or n < 1 or not t.is_contiguous() or t.device != data.device:
            raise RuntimeError(f"gif_indices: {name} must be a contiguous {dt} tensor [{n}] on {data.device}, got {tuple(t.shape)} {t.dtype}")
    if isinstance(maps_bytes, bool) or not isinstance(maps_bytes, int) or maps_bytes < 1:
        raise RuntimeError(f"gif_indices: maps_bytes {maps_bytes!r} (a positive integer)")
    maps = torch.empty((maps_bytes,), dtype=torch.uint8, device=data.device)
    status = torch.empty((n,), dtype=torch.int32, device=data.device)
    ws = torch.empty((max(lib.tt_gif_decode_ws_bytes(n, data.numel()), 16),), dtype=torch.uint8, device=data.device)
    check(lib.tt_gif_decode_indices(_p(data), data.numel(), _p(offsets), _p(lengths), _p(npix), _p(min_code_size), _p(rows), _p(map_offsets), n, _p(maps),
                                    maps_bytes, _p(status), _p(ws), ws.numel(), _stream()), "tt_gif_decode_indices")
    _wrote(maps, "gif_indices")
    _wrote(status, "gif_indices")
    return maps, status


def gif_compose(maps: torch.Tensor, table: torch.Tensor, palettes: torch.Tensor, size, initial: int) -> torch.Tensor:
    """``gif_indices``' maps, ``table`` (uint8 device tensor [N, 40]: the bytes of N TtGifComposeFrame rows) and ``palettes`` (uint8 device
    tensor [N, 256, 3]) drawn onto a canvas of ``size`` (height, width) that starts as the colour ``initial`` (0x00BBGGRR) -> uint8 device
    tensor [N, height, width, 3]: the canvas after every frame (tt_gif_compose).  Asynchronous on the current stream."""
    lib = _lib.load()
    for t in (maps, table, palettes):
        _p(t)
    if maps.dtype != torch.uint8 or maps.dim() != 1 or not maps.is_contiguous() or maps.numel() < 1:
        raise RuntimeError(f"gif_compose: maps must be a contiguous uint8 tensor [bytes], got {tuple(maps.shape)} {maps.dtype}")
    rowsize = C.sizeof(_lib.TtGifComposeFrame)
    if table.dtype != torch.uint8 or table.dim() != 2 or table.shape[1] != rowsize or table.shape[0] < 1 or not table.is_contiguous():
        raise RuntimeError(f"gif_compose: table must be a contiguous uint8 tensor [N, {rowsize}], got {tuple(table.shape)} {table.dtype}")
    n = table.shape[0]
    if palettes.dtype != torch.uint8 or tuple(palettes.shape) != (n, 256, 3) or not palettes.is_contiguous():
        raise RuntimeError(f"gif_compose: palettes must be a contiguous uint8 tensor [{n}, 256, 3], got {tuple(palettes.shape)} {palettes.dtype}")
    if table.device != maps.device or palettes.device != maps.device:
        raise RuntimeError("gif_compose: maps, table and palettes must be on one device")
    height, width = (int(v) for v in size)
    if height < 1 or width < 1:
        raise RuntimeError(f"gif_compose: size {size!r} (height, width; positive)")
    out = torch.empty((n, height, width, 3), dtype=torch.uint8, device=maps.device)
    check(lib.tt_gif_compose(_p(maps), maps.numel(), _p(table), _p(palettes), n, height, width, int(initial) & 0xffffff, _p(out), _stream()), "tt_gif_compose")
    _wrote(out, "gif_compose")
    return out


# ---- the PNG import's device half (tt_png_inflate / tt_png_unfilter; ingest.py parses the files)
def png_inflate(data: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, expected: torch.Tensor, out_offsets: torch.Tensor, max_out: int, out_bytes: int):
    """N zlib streams -> (uint8 device tensor [out_bytes]: stream f's ``expected[f]`` bytes at ``out_offsets[f]``; int32 device tensor [N]: every
    stream's status bits, 0 for a clean decode) (tt_png_inflate; a general inflate that knows nothing of PNG).  ``data``: uint8 device tensor
    holding stream f at ``offsets[f]`` (int64 [N]) with ``lengths[f]`` bytes (int32 [N]); ``expected``: int32 [N], none above the host integer
    ``max_out``; ``out_offsets``: int64 [N]; ``out_bytes``: a host integer.  Bytes of ``out`` that belong to no stream are not written.
    Asynchronous on the current stream."""
    lib = _lib.load()
    for t in (data, offsets, lengths, expected, out_offsets):
        _p(t)
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous() or data.numel() < 1:
        raise RuntimeError(f"png_inflate: data must be a contiguous uint8 tensor [bytes], got {tuple(data.shape)} {data.dtype}")
    n = offsets.numel()
    for name, t, dt in (("offsets", offsets, torch.int64), ("out_offsets", out_offsets, torch.int64), ("lengths", lengths, torch.int32), ("expected", expected, torch.int32)):
        if t.dtype != dt or tuple(t.shape) != (n,) or n < 1 or not t.is_contiguous() or t.device != data.device:
            raise RuntimeError(f"png_inflate: {name} must be a contiguous {dt} tensor [{n}] on {data.device}, got {tuple(t.shape)} {t.dtype}")
    for name, v in (("max_out", max_out), ("out_bytes", out_bytes)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise RuntimeError(f"png_inflate: {name} {v!r} (a positive integer)")
    out = torch.empty((out_bytes,), dtype=torch.uint8, device=data.device)
    status = torch.empty((n,), dtype=torch.int32, device=data.device)
    ws = torch.empty((max(lib.tt_png_decode_ws_bytes(n, out_bytes, max_out), 16),), dtype=torch.uint8, device=data.device)
    check(lib.tt_png_inflate(_p(data), data.numel(), _p(offsets), _p(lengths), _p(expected), _p(out_offsets), n, max_out, _p(out), out_bytes, _p(status), _p(ws),
                             ws.numel(), _stream()), "tt_png_inflate")
    _wrote(out, "png_inflate")
    _wrote(status, "png_inflate")
    return out, status


def png_unfilter(filtered: torch.Tensor, shape):
    """``png_filter``'s layout (uint8 device tensor [N, stride]) for frames of ``shape`` (h, w, ch) -> (uint8 device tensor [N, h, w, ch]: the
    pixels, the exact inverse of ``png_filter``; int32 device tensor [N]: bit 0 where a row's filter type is above 4) (tt_png_unfilter).
    Asynchronous on the current stream."""
    lib, n, h, w, ch, _ = _png_filtered(filtered, shape, "png_unfilter")
    out = torch.empty((n, h, w, ch), dtype=torch.uint8, device=filtered.device)
    status = torch.empty((n,), dtype=torch.int32, device=filtered.device)
    check(lib.tt_png_unfilter(_p(filtered), n, h, w, ch, _p(out), _p(status), _stream()), "tt_png_unfilter")
    _wrote(out, "png_unfilter")
    _wrote(status, "png_unfilter")
    return out, status
