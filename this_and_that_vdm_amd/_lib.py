"""ctypes binding of libttvdm.so (include/ttvdm.h).  The product path has NO fallback: if the
library is missing or a call fails, a RuntimeError is raised."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("TT_LIBTTVDM") or os.path.join(CSRC, "libttvdm.so")      # TT_LIBTTVDM: A/B builds of the same ABI

TT_BF16, TT_F16, TT_F32 = 0, 1, 2
TT_FP8_E4M3 = 3          # tt_tensor_stats only (OCP e4m3 bytes, what gemm(out_fp8=True) writes)


class TtGemmArgs(C.Structure):
    _fields_ = [
        ("a0", C.c_void_p), ("a1", C.c_void_p), ("k0", C.c_int32), ("k1", C.c_int32),
        ("lda0", C.c_int64), ("lda1", C.c_int64), ("w", C.c_void_p), ("ldw", C.c_int64),
        ("m", C.c_int32), ("n", C.c_int32), ("mode", C.c_int32),
        ("nimg", C.c_int32), ("hin", C.c_int32), ("win", C.c_int32), ("hout", C.c_int32), ("wout", C.c_int32),
        ("stride", C.c_int32), ("upsample", C.c_int32), ("frames", C.c_int32), ("hw", C.c_int32),
        ("bias", C.c_void_p), ("acc_scale", C.c_float),
        ("rowvec", C.c_void_p), ("rowvec_rows", C.c_int32), ("ld_rowvec", C.c_int64),
        ("geglu", C.c_int32), ("residual", C.c_void_p), ("ld_res", C.c_int64),
        ("blend", C.c_void_p), ("ld_blend", C.c_int64), ("alpha", C.c_float),
        ("out", C.c_void_p), ("ldo", C.c_int64), ("out_f32", C.c_int32),
        ("out_col_hw", C.c_int32), ("out_col_hwp", C.c_int32), ("dtype", C.c_int32),
        ("ws", C.c_void_p), ("ws_bytes", C.c_int64),
        ("ln_fold", C.c_int32), ("ln_eps", C.c_float), ("out_fp8", C.c_int32),
        ("rowvec_mod", C.c_int32),          # ABI 7: periodic row vector
        ("stats_out", C.c_void_p),          # ABI 8: per (row tile, column) sum / sum of squares of the stored output
        ("stats_seg", C.c_int32),           # ... rows of the consumer's GroupNorm segment (hint for the statistics tile height)
        ("gn_out", C.c_void_p), ("ld_gn", C.c_int64), ("gn_gamma", C.c_void_p), ("gn_beta", C.c_void_p),      # ABI 9: GroupNorm in the split-K reduction
        ("gn_eps", C.c_float), ("gn_silu", C.c_int32),
        ("presplit", C.c_int32),            # ABI 11: bit 0 a0 / a1, bit 1 w hold pre-split fp16 pairs (TT_F32 split16 mode)
    ]


class TtAttnArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("ldq", C.c_int64), ("k", C.c_void_p), ("ldk", C.c_int64),
        ("vt", C.c_void_p), ("ldvt", C.c_int64), ("out", C.c_void_p), ("ldo", C.c_int64),
        ("nseq", C.c_int32), ("lq", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
        ("mask", C.c_int32), ("lk", C.c_int32), ("k_seq_stride", C.c_int32), ("v_seq_stride", C.c_int32),
        ("frames", C.c_int32), ("ctx_batches", C.c_int32), ("dtype", C.c_int32), ("batch0", C.c_int32), ("fp8", C.c_int32),
        # ABI 6: fused query projection of the cross-attention (qx != NULL: Q = LN(qx rows) wq^T + bq computed by the kernel)
        ("qx", C.c_void_p), ("ldqx", C.c_int64), ("wq", C.c_void_p), ("ldwq", C.c_int64), ("bq", C.c_void_p),
        ("qc", C.c_int32), ("ln_eps", C.c_float),
        ("v_rows", C.c_int32),              # ABI 10: `vt` is V itself, [key rows, ldvt]
    ]


class TtConvArgs(C.Structure):
    _fields_ = [
        ("x0", C.c_void_p), ("x1", C.c_void_p), ("c0", C.c_int32), ("c1", C.c_int32), ("ld0", C.c_int64), ("ld1", C.c_int64),
        ("w", C.c_void_p), ("ldw", C.c_int64),
        ("nimg", C.c_int32), ("h", C.c_int32), ("w_img", C.c_int32), ("n", C.c_int32),
        ("gn_scale", C.c_void_p), ("gn_shift", C.c_void_p), ("silu", C.c_int32),
        ("bias", C.c_void_p),
        ("rowvec", C.c_void_p), ("rowvec_rows", C.c_int32), ("ld_rowvec", C.c_int64),
        ("residual", C.c_void_p), ("ld_res", C.c_int64),
        ("out", C.c_void_p), ("ldo", C.c_int64),
        ("dtype", C.c_int32),
    ]


class TtGesturePoint(C.Structure):
    _fields_ = [("map", C.c_int32), ("frame", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("first", C.c_int32)]


class TtEncAttnArgs(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("ldq", C.c_int64), ("k", C.c_void_p), ("ldk", C.c_int64),
        ("v", C.c_void_p), ("ldv", C.c_int64), ("out", C.c_void_p), ("ldo", C.c_int64),
        ("nseq", C.c_int32), ("l", C.c_int32), ("heads", C.c_int32), ("head_dim", C.c_int32),
        ("causal", C.c_int32), ("k_seq_stride", C.c_int32), ("v_seq_stride", C.c_int32), ("dtype", C.c_int32),
    ]


class TtTensorStats(C.Structure):
    """The device record of tt_tensor_stats: 616 bytes, the field order and offsets of include/ttvdm.h."""
    _fields_ = [
        ("count", C.c_uint64), ("n_nan", C.c_uint64), ("n_pinf", C.c_uint64), ("n_ninf", C.c_uint64), ("n_zero", C.c_uint64),
        ("n_ge", C.c_uint64 * 4),
        ("hist", C.c_uint64 * 64),
        ("sum", C.c_double), ("sum_sq", C.c_double),
        ("max_abs", C.c_float), ("min_abs_nonzero", C.c_float), ("max_val", C.c_float), ("min_val", C.c_float),
    ]


class TtFrameMetricsRecord(C.Structure):
    """The device record of tt_frame_metrics, one per frame: 104 bytes, the field order and offsets of include/ttvdm.h."""
    _fields_ = [("sse", C.c_double * 4), ("ssim_sum", C.c_double * 4), ("cs_sum", C.c_double * 4), ("count", C.c_int64)]


TT_METRICS_SSE_ONLY = 1


class TtColorBin(C.Structure):
    """One histogram bin or palette entry of the GIF export (tt_color_hist / tt_palette_map): 16 bytes, pixels and channel sums."""
    _fields_ = [("count", C.c_uint32), ("sum_r", C.c_uint32), ("sum_g", C.c_uint32), ("sum_b", C.c_uint32)]


TT_GIF_BINS = 32768
TT_LZW_SEGMENT, TT_LZW_SEGMENT_MAX = 16384, 65536
TT_GIF_LZW_STATUS = {1: "an index that does not fit min_code_size", 2: "a min_code_size outside 2 .. 8"}
TT_PNG_STRIPE, TT_PNG_SYMS, TT_PNG_RECORD_WORDS, TT_PNG_TABLE_WORDS, TT_PNG_HEADER_WORDS = 32768, 286, 288, 288, 72
TT_JPEG_444, TT_JPEG_420, TT_JPEG_TABLE_WORDS, TT_JPEG_COUNT_WORDS = 0, 2, 256, 1024
TT_JPEG_CHUNK, TT_JPEG_DECODE_WORDS, TT_JPEG_DECODE_SET_WORDS = 4096, 256, 1028
TT_JPEG_MAX_SPANS = 65535
TT_JPEG_MAX_SCANS, TT_JPEG_SCAN_WORDS, TT_JPEG_MAX_ITEMS = 256, 8, 65535
TT_JPEG_STATUS = {1: "a marker inside the scan", 2: "an invalid Huffman code", 4: "the wrong number of blocks", 8: "bits left over behind the last block",
                  16: "a scan outside the buffer"}


TT_GIF_DEC_STATUS = {1: "an invalid LZW code", 2: "fewer pixels than the rectangle holds", 4: "a data span or an index map outside the buffers"}
TT_GIF_DEC_CHUNK, TT_GIF_MAX_FRAMES, TT_GIF_MAX_PIXELS = 16384, 65535, 16843009


class TtGifHeader(C.Structure):
    """What tt_gif_parse reads of the logical screen: the field order of include/ttvdm.h."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("background", C.c_int32), ("loop", C.c_int32),
                ("global_colors", C.c_int32), ("frames", C.c_int32), ("version", C.c_int32), ("reserved", C.c_int32), ("data_bytes", C.c_int64)]


class TtGifFrame(C.Structure):
    """One image of a GIF file as tt_gif_parse reads it (824 bytes): the field order of include/ttvdm.h."""
    _fields_ = [("left", C.c_int32), ("top", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("interlace", C.c_int32), ("transparent", C.c_int32), ("disposal", C.c_int32), ("delay", C.c_int32),
                ("min_code_size", C.c_int32), ("local_colors", C.c_int32), ("data_offset", C.c_int64), ("data_bytes", C.c_int64),
                ("palette", (C.c_uint8 * 3) * 256)]


class TtGifComposeFrame(C.Structure):
    """One row of tt_gif_compose's device table (40 bytes): the field order of include/ttvdm.h."""
    _fields_ = [("left", C.c_int32), ("top", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("transparent", C.c_int32), ("disposal", C.c_int32),
                ("fill", C.c_uint32), ("reserved", C.c_int32), ("map_offset", C.c_int64)]


TT_INFLATE_STATUS = {1: "a bad zlib header, a reserved block type or a stored block whose lengths disagree", 2: "an invalid set of code lengths or an invalid code",
                     4: "a distance that reaches before the first byte", 8: "fewer bytes than the image holds", 16: "more bytes than the image holds",
                     32: "an Adler-32 mismatch", 64: "a stream outside the buffers"}
TT_PNG_UNFILTER_STATUS = {1: "a filter type above 4"}
TT_INFLATE_CHUNK, TT_INFLATE_MAX_STREAMS, TT_PNG_UNFILTER_BAND = 4096, 65535, 256


class TtPngHeader(C.Structure):
    """What tt_png_parse reads of a PNG file: the field order of include/ttvdm.h."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32), ("bit_depth", C.c_int32), ("color_type", C.c_int32), ("interlace", C.c_int32),
                ("spans", C.c_int32), ("frames", C.c_int32), ("plays", C.c_int32), ("announced", C.c_int32), ("default_is_frame", C.c_int32), ("reserved", C.c_int32),
                ("idat_offset", C.c_int64), ("idat_bytes", C.c_int64), ("data_bytes", C.c_int64)]


class TtPngSpan(C.Structure):
    """One IDAT / fdAT payload as tt_png_parse reads it (24 bytes): the field order of include/ttvdm.h."""
    _fields_ = [("file_offset", C.c_int64), ("bytes", C.c_int64), ("frame", C.c_int32), ("reserved", C.c_int32)]


class TtPngFrame(C.Structure):
    """One fcTL of an animated PNG as tt_png_parse reads it (56 bytes): the field order of include/ttvdm.h."""
    _fields_ = [("sequence", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("delay_num", C.c_int32),
                ("delay_den", C.c_int32), ("dispose", C.c_int32), ("blend", C.c_int32), ("spans", C.c_int32), ("data_offset", C.c_int64), ("data_bytes", C.c_int64)]


class TtJpegHeader(C.Structure):
    """What tt_jpeg_parse reads from one baseline JPEG file: the field order of include/ttvdm.h."""
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("ch", C.c_int32), ("subsampling", C.c_int32),
                ("scan_offset", C.c_int64), ("scan_bytes", C.c_int64),
                ("dc_table", C.c_int32 * 3), ("ac_table", C.c_int32 * 3),
                ("quant", (C.c_uint8 * 64) * 3), ("bits", (C.c_uint8 * 16) * 4), ("huffval", (C.c_uint8 * 256) * 4)]


class TtJpegScan(C.Structure):
    """One scan of a progressive JPEG file as tt_jpeg_parse_progressive reads it (856 bytes): the field order of include/ttvdm.h."""
    _fields_ = [("comps", C.c_int32), ("ss", C.c_int32), ("se", C.c_int32), ("ah", C.c_int32), ("al", C.c_int32), ("reserved", C.c_int32),
                ("offset", C.c_int64), ("bytes", C.c_int64), ("bits", (C.c_uint8 * 16) * 3), ("huffval", (C.c_uint8 * 256) * 3)]


class TtJpegProgressiveHeader(C.Structure):
    """What tt_jpeg_parse_progressive reads of the frame: the field order of include/ttvdm.h."""
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("ch", C.c_int32), ("subsampling", C.c_int32), ("nscans", C.c_int32), ("reserved", C.c_int32),
                ("quant", (C.c_uint8 * 64) * 3)]


_i32, _i64, _f32, _vp, _sz = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t

# name -> (restype, argtypes): every symbol include/ttvdm.h declares
SIGNATURES = {
    "tt_abi_version": (C.c_int, []),
    "tt_target_arch": (C.c_char_p, []),
    "tt_last_error": (C.c_char_p, []),
    "tt_gemm": (C.c_int, [C.POINTER(TtGemmArgs), _vp]),
    "tt_gemm_set_streaming_square": (C.c_int, [C.c_int32]),
    "tt_gemm_set_big_tile": (C.c_int, [C.c_int32]),
    "tt_gemm_set_f32_split": (C.c_int, [C.c_int32]),
    "tt_gemm_plan": (C.c_int, [C.POINTER(TtGemmArgs), C.POINTER(C.c_int32)]),
    "tt_gemm_set_tile_override": (C.c_int, [_i32]),
    "tt_gemm_ws_bytes": (_sz, [C.POINTER(TtGemmArgs)]),
    # the wide route for operands of 2 GiB and more (additive; the ABI version is unchanged)
    "tt_gemm_is_wide": (C.c_int32, [C.POINTER(TtGemmArgs)]),
    "tt_gemm_set_wide": (C.c_int, [C.c_int32]),
    # the kernel instance a launch runs, by name, and the split16 mode in force (host-only, additive; the ABI version is unchanged)
    "tt_gemm_kernel": (C.c_int, [C.POINTER(TtGemmArgs), C.c_char_p, _i32]),
    "tt_conv3x3_kernel": (C.c_int, [C.POINTER(TtConvArgs), C.c_char_p, _i32]),
    "tt_attention_kernel": (C.c_int, [C.POINTER(TtAttnArgs), C.c_char_p, _i32]),
    "tt_gemm_get_f32_split": (C.c_int32, []),
    "tt_attention": (C.c_int, [C.POINTER(TtAttnArgs), _vp]),
    "tt_conv3x3_supported": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "tt_conv3x3": (C.c_int, [C.POINTER(TtConvArgs), _vp]),
    "tt_temporal_attention": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "tt_groupnorm_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "tt_groupnorm_small_supported": (C.c_int, [_i32, _i32, _i32]),
    "tt_groupnorm_route": (C.c_int, [_i32, _i32, _i32, _i32, _i32]),
    "tt_groupnorm_small": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _f32, _i32, _vp, _i64, _i32, _vp]),
    "tt_groupnorm_stats": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _f32, _vp, _vp, _vp, _sz, _i32, _vp]),
    "tt_groupnorm_apply": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i64, _i32, _vp]),
    "tt_groupnorm_tiles_supported": (C.c_int, [_i32, _i32, _i32, _i32]),
    "tt_groupnorm_tiles": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _f32, _i32, _vp, _i64, _i32, _vp]),
    "tt_gemm_stats_rows": (C.c_int32, [C.POINTER(TtGemmArgs)]),
    "tt_gemm_gn_fused": (C.c_int32, [C.POINTER(TtGemmArgs)]),
    "tt_layernorm": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _f32, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _vp]),
    "tt_zero_sum_round": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "tt_small_linear": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "tt_timestep_embedding": (C.c_int, [_vp, _i32, _i32, _vp, _i64, _vp]),
    "tt_prep_model_input": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "tt_cfg_euler_step": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "tt_cfg3_euler_step": (C.c_int, [_vp, _i32, _vp, _vp, C.c_float, _vp, _i32, _i32, _i32, _i32, _vp]),
    # the R-request forms of the loop glue (additive; the ABI version is unchanged)
    "tt_prep_model_input_requests": (C.c_int, [_vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "tt_cfg_euler_step_requests": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _f32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    # the DPM-Solver++ 2M step on the same glue (additive; the ABI version is unchanged)
    "tt_cfg_multistep_step_requests": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i32, _f32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "tt_nchw_to_tokens": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "tt_tokens_to_nchw": (C.c_int, [_vp, _i32, _i64, _i32, _i32, _i32, _vp, _i32, _i32, _vp]),
    "tt_add_scaled": (C.c_int, [_vp, _vp, _f32, _vp, _i64, _i32, _vp]),
    "tt_add_rowvec": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp]),
    "tt_softmax_rows": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _i64, _i32, _i32, _vp]),
    # the CLIP encoders (additive; the ABI version is unchanged)
    "tt_encoder_attention": (C.c_int, [C.POINTER(TtEncAttnArgs), _vp]),
    "tt_act_rows": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    "tt_patch_tokens": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _vp]),
    "tt_embed_rows": (C.c_int, [_i32, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _i64, _i32, _vp]),
    # the request path around the models: CLIP preprocessing, context LayerNorm, frame export (additive as well)
    "tt_clip_image_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "tt_clip_image": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _f32, _f32, _vp, _i32, _vp, _sz, _vp]),
    "tt_layernorm_block": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _f32, _vp, _i32, _vp]),
    "tt_frames_out": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    # gesture maps rasterised from the annotated points (additive as well)
    "tt_gesture_maps_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "tt_gesture_maps": (C.c_int, [C.POINTER(TtGesturePoint), _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _sz, _vp]),
    # PIL's 8-bit resize and the VAE input computed from it (additive as well); tt_resample_coeffs is host-only
    "tt_resample_coeffs": (C.c_int, [_i32, _i32, _i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tt_resize_u8_ws_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "tt_resize_u8": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    "tt_vae_image_ws_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "tt_vae_image": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _f32, _i32, _vp, _i32, _vp, _sz, _vp]),
    # the range audit's one-pass tensor statistics (additive as well)
    "tt_tensor_stats_ws_bytes": (_i64, [_i64, _i32, _i32]),
    "tt_tensor_stats_launch": (C.c_int, [_i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tt_tensor_stats": (C.c_int, [_vp, _i64, _i64, _i32, _i32, C.POINTER(C.c_float), _vp, _vp, _i64, _i32, _vp]),
    # two videos compared on the device: the sums behind PSNR / SSIM per frame, and the MS-SSIM pyramid's 2 x 2 mean (additive as well)
    "tt_frame_metrics_window": (C.c_int, [C.POINTER(C.c_double)]),
    "tt_frame_metrics_launch": (C.c_int, [_i32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tt_frame_metrics_ws_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "tt_frame_metrics": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, C.c_double, _i32, _vp, _vp, _i64, _vp]),
    "tt_frames_pool2": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    # the GIF export: colour histograms and the palette map on the device, median cut and LZW on the host (additive as well)
    "tt_color_hist": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "tt_palette_map": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp]),
    "tt_palette_median_cut": (C.c_int, [_vp, _i32, _vp, C.POINTER(C.c_int32), _vp]),
    "tt_gif_lzw_bound": (_i64, [_i64]),
    "tt_gif_lzw": (C.c_int, [_vp, _i64, _i32, _vp, _i64, C.POINTER(C.c_int64)]),
    # ... and the LZW stage on the device, in independent segments (additive as well)
    "tt_gif_lzw_frames_bound": (_i64, [_i64, _i32]),
    "tt_gif_lzw_frames_ws_bytes": (_i64, [_i32, _i64, _i32]),
    "tt_gif_lzw_frames": (C.c_int, [_vp, _i32, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp]),
    # the PNG export: filter, tokens and emit on the device, code lengths and block headers on the host (additive as well)
    "tt_png_stream_bytes": (_i64, [_i32, _i32, _i32]),
    "tt_png_frame_stride": (_i64, [_i32, _i32, _i32]),
    "tt_png_stripes": (_i64, [_i32, _i32, _i32]),
    "tt_png_filter": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "tt_png_tokens": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "tt_png_emit": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _i64, _vp]),
    "tt_png_code_lengths": (C.c_int, [_vp, _i32, _i32, _vp]),
    "tt_png_block_header": (C.c_int, [_vp, _vp, _vp, _i32, C.POINTER(C.c_int64)]),
    "tt_png_plan": (C.c_int, [_vp, _i64, _vp, _vp, C.POINTER(C.c_int64)]),
    # the JPEG export: coefficients and the stuffed scan on the device, quantiser and Huffman tables on the host (additive as well)
    "tt_jpeg_blocks": (_i64, [_i32, _i32, _i32, _i32]),
    "tt_jpeg_scan_bound": (_i64, [_i32, _i32, _i32, _i32]),
    "tt_jpeg_scan_ws_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "tt_jpeg_quant_tables": (C.c_int, [_i32, _vp]),
    "tt_jpeg_standard_table": (C.c_int, [_i32, _vp, _vp, C.POINTER(C.c_int32), _vp]),
    "tt_jpeg_optimized_table": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_int32), _vp]),
    "tt_jpeg_coeffs": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "tt_jpeg_scan": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp, _vp, _i64, _vp]),
    # ... with restart intervals (additive as well)
    "tt_jpeg_scan_bound_restart": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "tt_jpeg_scan_restart_ws_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "tt_jpeg_counts_restart": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "tt_jpeg_scan_restart": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp, _vp, _i64, _vp]),
    # the JPEG import: header and decode tables on the host, unstuffing, entropy decode and reconstruction on the device (additive as well)
    "tt_jpeg_parse": (C.c_int, [_vp, _i64, C.POINTER(TtJpegHeader)]),
    "tt_jpeg_decode_table": (C.c_int, [_vp, _vp, _vp]),
    "tt_jpeg_sequence_bits": (_i64, []),
    "tt_jpeg_entropy_ws_bytes": (_i64, [_i32, _i64]),
    "tt_jpeg_entropy": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    "tt_jpeg_pixels": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp]),
    # ... with restart intervals: the scan's spans on the host, one workgroup per span on the device (additive as well)
    "tt_jpeg_parse_spans": (C.c_int, [_vp, _i64, C.POINTER(TtJpegHeader), C.POINTER(C.c_int32), _vp, _vp, _i64, C.POINTER(C.c_int64)]),
    "tt_jpeg_entropy_spans": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i64, _vp]),
    # ... progressive files: every scan's place and tables on the host, the scans applied round by round on the device (additive as well)
    "tt_jpeg_parse_progressive": (C.c_int, [_vp, _i64, C.POINTER(TtJpegProgressiveHeader), _vp, _i64, C.POINTER(C.c_int64)]),
    "tt_jpeg_entropy_progressive_ws_bytes": (_i64, [_i32, _i32, _i64, _i32, _i32, _i32, _i32]),
    "tt_jpeg_entropy_progressive": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    # the GIF import: the container on the host, LZW, interlace and composition on the device (additive as well)
    "tt_gif_parse": (C.c_int, [_vp, _i64, C.POINTER(TtGifHeader), _vp, _i64, _vp, _i64]),
    "tt_gif_decode_ws_bytes": (_i64, [_i32, _i64]),
    "tt_gif_decode_indices": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _vp, _i64, _vp]),
    "tt_gif_compose": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _i32, _i32, C.c_uint32, _vp, _vp]),
    # the PNG import: the container on the host, a general zlib inflate and the inverse row filters on the device (additive as well)
    "tt_png_parse": (C.c_int, [_vp, _i64, C.POINTER(TtPngHeader), _vp, _i64, _vp, _i64, _vp, _i64]),
    "tt_png_decode_ws_bytes": (_i64, [_i32, _i64, _i64]),
    "tt_png_inflate": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "tt_png_unfilter": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
}

_lib = None


def build(verbose: bool = False) -> str:
    """Compile libttvdm.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-C", CSRC, "-j4"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"building libttvdm.so failed:\n{r.stdout[-4000:]}\n{r.stderr[-4000:]}")
    if verbose:
        print(r.stdout[-2000:])
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: run `make -C {CSRC}` (or __graft_entry__.build()). "
                           "There is no CPU/PyTorch fallback for the denoise path.")
    # torch first: its wheel bundles its own HIP runtime (libamdhip64).  If libttvdm.so is dlopen'ed before torch, the system
    # runtime it links against is the one that initialises, torch then brings a second copy, and kernels launched through this
    # library fail with "no ROCm-capable device is detected" (seen with build() + smoke() in one process).  With torch loaded
    # first the library's DT_NEEDED entry resolves to the runtime that owns torch's streams and allocations.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here == ABI mismatch with include/ttvdm.h
        fn.restype, fn.argtypes = res, args
    if lib.tt_abi_version() != 11:
        raise RuntimeError("libttvdm.so ABI version mismatch")
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        msg = load().tt_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({code}): {msg}")
