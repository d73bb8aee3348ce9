/*
 * ttvdm.h -- C ABI of libttvdm.so: the MI355X (gfx950) kernels behind the SVD denoise hot path
 * of Kiteretsu77/This_and_That_VDM.
 *
 * The reference has NO native boundary for this path: it is eager PyTorch calling stock
 * Conv2d/Conv3d/Linear/GroupNorm/LayerNorm/SDPA through diffusers==0.25.1.  The
 * entry points below are therefore the operators that path lowers to; each cites
 * the reference site(s) whose work it replaces.  Citations are relative to /root/reference.
 *
 * Conventions
 *   - plain C: pointers + sizes only.  Every pointer is a DEVICE pointer unless marked host.
 *   - no ownership transfer, no allocation, no host sync inside: stream-ordered and stateless,
 *     hence safe to capture in a hipGraph and thread-safe per stream.
 *   - return 0 on success, a negative TT_E* code otherwise (never throws).
 *   - activations are token-major ("NHWC"): [frames*batch, h*w, C], C contiguous.
 *   - `dtype` selects the storage type of activations/weights: TT_BF16 or TT_F16; all
 *     accumulation, norm statistics, softmax and small vectors (bias, FiLM rows) are fp32.
 *     TT_F32 is the reference-precision mode: the SAME kernels instantiated on fp32 storage with the
 *     exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32, 1/16 of the bf16 rate).  It exists so the
 *     whole launch sequence can be checked against the fp32 CPU reference at rtol 1e-3 / atol 1e-4
 *     (16-bit operand rounding alone exceeds that); it is not the benchmarked path.
 */
#ifndef TTVDM_H
#define TTVDM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tt_stream_t; /* hipStream_t */

enum { TT_BF16 = 0, TT_F16 = 1, TT_F32 = 2 };
enum { TT_OK = 0, TT_EINVAL = -1, TT_EUNSUPPORTED = -2, TT_ELAUNCH = -3 };

/* library/ABI version and target arch string ("gfx950"). */
int tt_abi_version(void);
const char* tt_target_arch(void);
/* text of the last error on the calling thread (host pointer, valid until the next call). */
const char* tt_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * tt_gemm: out = epilogue( gather(A) x W^T ).  One kernel family for every dense contraction:
 *   mode 0  Linear            nn.Linear sites: transformer_temporal.py:326,373 (proj_in/out) and the
 *                             diffusers Attention/FeedForward linears built at :240-261; 1x1 convs:
 *                             ResnetBlock2D.conv_shortcut, temporal_controlnet.py:614-622 zero-convs.
 *   mode 1  Conv2d 3x3 pad 1  ResnetBlock2D.conv1/conv2 (unet_3d_blocks.py:2094 etc.),
 *                             Downsample2D stride 2 (:2117-2123), Upsample2D nearest x2 + conv
 *                             (:2223,2332; the upsample is an index map, never materialised),
 *                             conv_in / conv_in_concat / conv_out
 *                             (unet_spatio_temporal_condition.py:455,528; temporal_controlnet.py:580).
 *   mode 2  Conv3d (3,1,1)    TemporalResnetBlock.conv1/conv2 (diffusers; reached from
 *                             unet_3d_blocks.py:1891-2316): 3 taps along the frame axis.
 *   mode 3  Conv2d 3x3,       the VAE encoder's Downsample2D(use_conv=True, padding=0) (diffusers; reached from
 *           zero padding      vae.encode, svd/pipeline_stable_video_diffusion_controlnet.py:200,652):
 *           left 0 / right 1  F.pad(x, (0,1,0,1)) + conv(stride, padding=0) in one launch.  Output (y, x), tap (ky, kx)
 *           top 0 / bottom 1  reads input pixel (y*stride + ky, x*stride + kx); pixels with index >= hin / win read as zero.
 *                             Same fields and weight layout as mode 1 (nimg, hin, win, hout, wout, stride); upsample
 *                             must be 0 (TT_EINVAL).  Built only for the tile configurations the planner gives mode-3
 *                             problems: a tile override (tt_gemm_set_tile_override / TT_GEMM_CFG) naming another
 *                             configuration makes tt_gemm / tt_gemm_plan return TT_EUNSUPPORTED for mode 3.
 * W is [n, taps*(k0+k1)] row-major with k index (tap, source, channel); two sources implement
 * torch.cat([h, skip], dim=1) (unet_3d_blocks.py:2242,2352) without a concat buffer.
 * upsample (mode 1): 0 none; 1 nearest x2 as an index map of the 9-tap gather (hout = 2 hin, wout = 2 win); 2 the same conv on
 * PHASE-PACKED weights, W [n, 16*k0] with k index (phase py*2+px, tap r*2+c, channel): output pixel (Y, X) of phase (Y & 1, X & 1)
 * sees 2 x 2 distinct input pixels, so its nine taps collapse onto four -- tap (r, c) reads input pixel (Y/2 + r - 1 + py,
 * X/2 + c - 1 + px) and carries the sum of the 3x3 weights whose rows {0},{1,2} (py = 0) / {0,1},{2} (py = 1) and columns (same rule)
 * fall on it (packing.pack_upsample_phases).  4/9 of the products of upsample = 1, one launch, same m / geometry fields / output
 * layout.  Served by the tiled template only, with one source and a bias-only epilogue: a1 / k1, residual, blend, rowvec, stats_out,
 * gn_out, geglu, ln_fold, out_fp8, out_f32, out_col_hw or stride != 1 make tt_gemm and tt_gemm_plan return TT_EINVAL; never split
 * along K (tt_gemm_ws_bytes = 0, tt_gemm_stats_rows = 0).
 * Epilogue, in this order (every term optional):
 *   acc *= 1/sigma of the LayerNorm-folded operand row (ln_fold, below)
 *   v = (acc + bias[n]) * acc_scale + rowvec[m / rowvec_rows][n]        (row index taken modulo rowvec_mod when that is > 0)
 *   geglu: v = v_value * gelu_erf(v_gate)      (W rows pre-interleaved in 16-row groups: 8 value, 8 gate)
 *   v += residual[m][n];  v = alpha*blend[m][n] + (1-alpha)*v   (AlphaBlender, video branch)
 * `out` may alias `residual` (same pointer and stride: in-place update of the hidden states -- every element's residual is
 * read by the lane that writes it, in the tile kernels and in the split-K reduction); it must not alias a0 / a1 / blend.
 * Operand sizes.  Every kernel of the family indexes an operand with 32-bit byte offsets from its base, so a problem whose a0, a1,
 * out, residual and blend each span less than 2 GiB (first byte to the end of the last row, strides included) runs on any route.  A
 * problem in which one of them spans 2 GiB or more runs on the WIDE route: the tiled template's windowed variant, in which every
 * workgroup rebases its descriptors once per tile onto the first row the tile can touch (64-bit arithmetic) and the lanes' offsets
 * count from there.  Same tile, K order and epilogue arithmetic as the narrow route -- bit-equal results on the same values --,
 * never split along K.  It serves modes 0 / 1 / 2 (upsample 0 / 1 / 2 included) with one source and the bias / acc_scale /
 * residual (also aliasing out) / blend / out_f32 epilogue terms and stats_out on bf16, fp16 and TT_F32 storage (exact and split16
 * products).  TT_EUNSUPPORTED, with a message that names the cause, for: a second source, geglu, ln_fold, rowvec, gn_out, out_fp8,
 * out_col_hw, presplit or mode 3 on such a problem; W of 2 GiB or more; and a problem in which the window of ONE tile would itself
 * reach 2 GiB (mode 0: the tile's 64 / 128 rows of a0; mode 1: the images its output rows lie in; mode 2: its rows and one frame
 * either side; out / residual / blend: the tile's rows) -- e.g. mode 0 on 16-bit storage with lda0 = 2^25.  The ~302 MB frames of
 * the temporal VAE decoder at 576x1024 (svd/pipeline_stable_video_diffusion_controlnet.py:257-283) are what it is for.
 * ---------------------------------------------------------------------------------------------- */
typedef struct TtGemmArgs {
  const void* a0; const void* a1;      /* activation sources; a1 NULL if k1 == 0 */
  int32_t k0, k1;                      /* channels per tap taken from a0 / a1 (multiples of 8) */
  int64_t lda0, lda1;                  /* row strides, elements */
  const void* w; int64_t ldw;          /* [n, taps*(k0+k1)] */
  int32_t m, n;                        /* n multiple of 4 */
  int32_t mode;                        /* 0 linear, 1 conv3x3, 2 tconv3, 3 conv3x3 padded bottom / right only */
  int32_t nimg, hin, win, hout, wout, stride, upsample;   /* modes 1 and 3 (hin/win = stored input size); upsample 0 / 1 / 2: above */
  int32_t frames, hw;                  /* mode 2: row = (b*frames + f)*hw + p */
  const float* bias;
  float acc_scale;
  const float* rowvec; int32_t rowvec_rows; int64_t ld_rowvec;
  int32_t geglu;
  const void* residual; int64_t ld_res;
  const void* blend; int64_t ld_blend; float alpha;
  void* out; int64_t ldo; int32_t out_f32;
  int32_t out_col_hw, out_col_hwp;     /* if hw>0: column c -> (c/hw)*hwp + c%hw (padded V^T sequences) */
  int32_t dtype;
  void* ws; int64_t ws_bytes;          /* optional caller-owned scratch for split-K (tt_gemm_ws_bytes); NULL = never split */
  /* Fused LayerNorm of one operand (nn.LayerNorm sites inside Basic/TemporalBasicTransformerBlock, reached from
   * transformer_temporal.py:342-365; mode 0, k1 == 0, k0 = the LayerNorm width):
   *   ln_fold 1   acc[m][n] is multiplied by 1/sqrt(var(a0 row m) + ln_eps)      -> out = LN(A) W^T
   *   ln_fold 2   acc[m][n] is multiplied by 1/sqrt(var(w  row n) + ln_eps)      -> out = A LN(W)^T  (swapped V^T projection)
   * before bias / acc_scale / the other epilogue terms.  The statistics are taken inside the K loop from the operand
   * fragments themselves (no separate pass).  The CALLER folds the affine part: the un-normalised operand is multiplied by
   * (weight * gamma), centred over k so that each weight row sums to zero (then x W^T == (x - mean) W^T), and beta
   * enters through `bias` (this_and_that_vdm_amd/packing.py:fold_layernorm). */
  int32_t ln_fold; float ln_eps;
  /* out_fp8 != 0: `out` receives OCP e4m3 bytes (row stride ldo BYTES, saturating conversion) instead of 16-bit values:
   * the Q | K and V^T operands of tt_attention's fp8 path (BASELINE config 5).  Plain mode-0 linears only (ln_fold and
   * out_col_hw are allowed; no geglu / residual / blend / rowvec / out_f32); dtype stays the 16-bit type of a0 / w. */
  int32_t out_fp8;
  /* ABI 7.  rowvec_mod > 0: row m takes rowvec[(m / rowvec_rows) % rowvec_mod] -- a PERIODIC row vector.  rowvec_rows = 1,
   * rowvec_mod = 2 gives even and odd rows their own vector: the temporal transformer block's output projection serves the rows of
   * both context classes (quirk Q3 pairs query pixel p with context p mod 2; the class whose context is all zeros also receives the
   * cross-attention's to_out bias, transformer_temporal.py:342-365 via TemporalBasicTransformerBlock) in ONE launch instead of one
   * launch per class on strided row views.  0: the plain form above. */
  int32_t rowvec_mod;
  /* ABI 8.  stats_out != NULL: beside its output the kernel writes, per row tile of R = tt_gemm_stats_rows(args) output rows and per
   * column, the sum and the sum of squares of the values it STORES (after rounding to the storage type):
   *     stats_out[(t * 2 + 0) * n + c] = sum_{r in tile t} out[r][c]        stats_out[(t * 2 + 1) * n + c] = sum of squares
   * fp32, [ceil(m / R)][2][n] floats, no atomics (fixed summation order: bit-reproducible).  This is the producer half of GroupNorm
   * (nn.GroupNorm(32) in ResnetBlock2D / TemporalResnetBlock / TransformerSpatioTemporalModel.norm -- unet_3d_blocks.py:1891-2316,
   * transformer_temporal.py:323-326): the tensor a GroupNorm reads is the output of a conv / Linear launch, whose epilogue has every
   * value in registers; tt_groupnorm_tiles turns the tile sums into the normalised tensor in ONE pass over it, without a
   * statistics pass.  Only routes and shapes for which tt_gemm_stats_rows(args) > 0 (TT_EUNSUPPORTED otherwise). */
  float* stats_out;
  /* rows of the consumer's GroupNorm segment (one image: h*w; the frames of a video: frames*h*w), a hint that lets the route pick a
   * statistics tile height R that divides it: the split-K routes (coarse UNet levels; the sums are taken by the reduction kernel, any
   * height works) use the largest divisor of stats_seg up to 128; the tiled template falls back from its tile height (128) to the
   * 32 / 64 rows of one wave row when only that divides stats_seg (448-row images, 1568-row videos).  0: the route's tile height. */
  int32_t stats_seg;
  /* ABI 9.  gn_out != NULL: the launch ALSO writes act(GroupNorm_32(out)) to gn_out (same storage type, row stride ld_gn elements), with
   * statistics per segment of stats_seg output rows (one image, or the frames of a video), gamma / beta fp32 [n], SiLU when gn_silu != 0
   * -- the GroupNorm that reads this launch's output (ResnetBlock2D.norm2 after conv1, TemporalResnetBlock.norm1 / norm2 --
   * unet_3d_blocks.py:1891-2316 via diffusers ResnetBlock2D / TemporalResnetBlock).  Only where the launch ends in the split-K
   * reduction pass anyway (the two coarsest UNet levels: 784 / 3136 rows), which then owns a whole (segment, group) per block: it sums
   * the fp32 slabs, applies the epilogue, stores `out`, and normalises the stored values from registers -- one launch instead of the
   * reduction plus a GroupNorm launch.  tt_gemm_gn_fused(args) != 0 says whether `args` qualifies (TT_EUNSUPPORTED otherwise);
   * exclusive with stats_out. */
  void* gn_out; int64_t ld_gn;
  const float* gn_gamma; const float* gn_beta;
  float gn_eps; int32_t gn_silu;
  /* ABI 11.  TT_F32 with tt_gemm_set_f32_split(1) only: an operand that is a constant of the request (packed weights) may be handed over
   * PRE-SPLIT, so the kernel does not convert it again in every launch: bit 0 = a0 / a1, bit 1 = w.  A pre-split matrix has the shape,
   * strides and element size of the fp32 matrix it replaces; every aligned group of 4 consecutive k-elements (16 bytes) holds the eight
   * fp16 values  h0 h1 h2 h3 l0 l1 l2 l3  with  h = fp16(x 2^-8), l = fp16((x - 2^8 h) 2^3)  of its four fp32 values
   * (this_and_that_vdm_amd/packing.py:presplit_f32).  Not together with the LayerNorm statistics of that operand (ln_fold 1 with
   * bit 0, ln_fold 2 with bit 1).  0 = plain fp32 operands. */
  int32_t presplit;
} TtGemmArgs;
int tt_gemm(const TtGemmArgs* args, tt_stream_t stream);
/* 1 if tt_gemm serves `args` with gn_out (a split-K plan, 16-bit storage, stats_seg rows per segment dividing m and short enough for one
 * block -- up to 816 rows at 1280 channels, 1632 at 640 --, n / 32 channels per group a multiple of 4, plain row-major 16-bit output), else 0.
 * Host-only; set ws / ws_bytes as for tt_gemm. */
int32_t tt_gemm_gn_fused(const TtGemmArgs* args);
/* rows per statistics tile R if tt_gemm can serve `args` with stats_out (see stats_seg; m must be a multiple of R -- on the tiled
 * template a ragged last tile is fine, its rows beyond m add nothing); 0: this problem's route has no statistics epilogue (GEGLU,
 * fp8 / fp32 / transposed outputs, the persistent kernels, a split-K route without stats_seg) -- leave stats_out NULL.  Host-only;
 * call with ws / ws_bytes set as for tt_gemm (the plan depends on them). */
int32_t tt_gemm_stats_rows(const TtGemmArgs* args);
/* which tile configuration tt_gemm will use for this problem: cfg[0..6] = BM, BN, BK, ring stages, waves along M,
 * waves along N, split-K factor (stages = 0: not the tiled template).  Host-only, no launch. */
int tt_gemm_plan(const TtGemmArgs* args, int32_t cfg[7]);
/* The kernel instance tt_gemm launches for this problem (additive entry points, like tt_conv3x3_kernel and tt_attention_kernel below; the
 * ABI version is unchanged): its name is written to name[0..cap), NUL-terminated.  The name is the kernel's demangled symbol without return
 * type, parameter list and namespace qualifiers, EVERY template argument written out -- the form a kernel trace prints:
 *   gemm_kernel<bf16_tag, 128, 128, 64, 2, 4, 2, 0>    the tiled template: tag, the tile (cfg[0..5] of tt_gemm_plan) and the variant --
 *                                                      0..5 (gather modes 0 / 1 / 2, LayerNorm folded over the rows of A / of W, mode 3)
 *                                                      + 8 split16 + 16 / + 32 pre-split W / A + 64 the wide route
 *   gemm_pp_kernel<f16_tag, 1, 0>                      the persistent kernel: tag, LayerNorm fold, GEGLU
 *   gemm_w320_kernel / gemm_w320h_kernel<tag, 0, 1>    the big-tile kernels: tag, gather mode, LayerNorm fold
 *   sq320_kernel<bf16_tag, true, true>                 the streaming kernel: tag, residual, row vector
 * It comes from the selector the launch itself dispatches on, so it names what runs.  A problem launched in two parts (persistent kernel +
 * tail) gives the head's kernel, as tt_gemm_plan gives the head's tile; a split-K plan gives the main kernel, not the reduction pass.
 * Host-only, no launch, no device: set ws / ws_bytes as for tt_gemm (the plan depends on them).  Returns what tt_gemm_plan returns for a
 * problem it refuses, and TT_EINVAL when the name does not fit `cap` bytes (64 hold every name). */
int tt_gemm_kernel(const TtGemmArgs* args, char* name, int32_t cap);
/* bytes of fp32 scratch tt_gemm would like for this problem (0 = no split-K planned).  Problems with few output
 * tiles and a long K (convs at the coarsest UNet levels) are split over K; the slabs are summed in a fixed order,
 * so results stay bit-reproducible.  Without (enough) workspace the un-split plan runs instead. */
size_t tt_gemm_ws_bytes(const TtGemmArgs* args);
/* tuning knob: force tile configuration `cfg` (index into the table in gemm.hip) for every tt_gemm call of this
 * process; -1 restores the built-in heuristic.  Also settable by the TT_GEMM_CFG environment variable. */
int tt_gemm_set_tile_override(int32_t cfg);
/* tuning knob: route the 320 x 320 linears with m >= 4096 (mode 0, one source, bias / residual / self-blend epilogue) to
 * the persistent W-in-registers streaming kernel: 0 never, 1 always, 2 (the default) from 131 072 rows on -- 64x112 latents, where the
 * big-tile kernel walks 3.06 rounds of tiles; at 32x56 it is faster alone and slower inside the step.  Also TT_GEMM_SQ320=0|1|2. */
int tt_gemm_set_streaming_square(int32_t on);
/* tuning knob for the N = 320 t big-tile kernels (gemm_w320.hip), for A/B measurements and tests; also TT_GEMM_W320=0|1|2|3|4:
 *   0  keep these problems on the tiled kernels;
 *   1  (default) problems with >= 180 row tiles of 256 (the finest UNet level: ResnetBlock2D / temporal convs, shortcuts, proj_in/out,
 *      to_out, FF2, LayerNorm-folded Q projections -- svd/diffusion_arch/unet_3d_blocks.py:2094,2212,2311,
 *      svd/diffusion_arch/transformer_temporal.py:323-376) go to the 256 x 320 kernel; conv3x3 problems with fewer rows but >= 180
 *      tiles of 128 rows (the second level at 32x56 latents) to its 128 x 320 variant (measured: +9..16 % on those convs, nothing
 *      on the linears / temporal convs of that level, which therefore stay on the tiled kernels); long-K problems of the two
 *      coarsest levels (FF2 at 3136 rows, conv3x3 at 3136 / 784 rows: 100 / 28 tiles of 128 x 320) go to the variant with the K
 *      loop split over 2..16 workgroups per tile (fp32 slabs in the tt_gemm_ws_bytes workspace, summed in a fixed order);
 *   2  the 256 x 320 kernel only;    3  the 128 x 320 variant for every gather mode (its linear / temporal-conv / LayerNorm paths);
 *   4  as 1 without the split-K route. */
int tt_gemm_set_big_tile(int32_t on);
/* ABI 11 (round 6).  How TT_F32 launches of tt_gemm form their products (process-wide; also TT_F32_SPLIT=0|1 in the environment):
 *   0  (default) exact-fp32 MFMA, v_mfma_f32_32x32x2_f32: bitwise an fmaf chain in k order, 157 TFLOP/s peak;
 *   1  "split16": every fp32 operand x is split on the fly into two fp16 parts on different binary scales, h = fp16(x 2^-8) and
 *      l = fp16((x - 2^8 h) 2^3), and a b ~ 2^16 a_h b_h + 2^5 (a_h b_l + a_l b_h) runs as three v_mfma_f32_32x32x16_f16 into two fp32
 *      accumulators -- max(2^-22 |x|, 2^-28) per operand, operands up to |x| < 2^24 (beyond that the hi part overflows to inf),
 *      3 x 8 passes per 32 x 32 x 16 block instead of 8 x 16.  Storage, epilogues,
 *      LayerNorm statistics and accumulation stay fp32; the mode meets the north-star tolerance (rtol 1e-3 / atol 1e-4 against the
 *      reference's CPU fp32 forward, svd/unet_spatio_temporal_condition.py:363-536) at about half of the exact mode's step time.
 *      tt_attention on fp32 storage (head_dim 64) follows the same switch; few-tile long-K problems take a split-K plan in this mode
 *      (fp32 slabs in the tt_gemm_ws_bytes workspace, summed in a fixed order). */
int tt_gemm_set_f32_split(int32_t on);
/* the mode in force: 0 or 1, from TT_F32_SPLIT (any value atoi reads as non-zero) or the last tt_gemm_set_f32_split.  Host-only (additive). */
int32_t tt_gemm_get_f32_split(void);
/* The wide route (see "Operand sizes" above; additive entry points, the ABI version is unchanged).
 * tt_gemm_is_wide: 1 if tt_gemm would run `args` on the wide route, else 0 (also for problems it refuses).  Host-only. */
int32_t tt_gemm_is_wide(const TtGemmArgs* args);
/* When tt_gemm takes the wide route (process-wide; also TT_GEMM_WIDE=0|1|2 in the environment):
 *   0  never: a problem with an operand of 2 GiB or more is refused (TT_EUNSUPPORTED "operand larger than 2 GiB"), for A/B runs;
 *   1  (default) when an operand needs it;
 *   2  for every problem the wide variant can serve without changing its plan (tiled template, un-split, a tile shape whose wide
 *      variant is built): tests and measurements of the wide kernels against the narrow ones on the same problem. */
int tt_gemm_set_wide(int32_t on);

/* ------------------------------------------------------------------------------------------------
 * tt_conv3x3: Conv2d 3x3 / stride 1 / pad 1 with the GroupNorm (+SiLU) of its INPUT fused in -- the ResnetBlock2D convs
 * (norm1 -> SiLU -> conv1 (+ time-embedding FiLM), norm2 -> SiLU -> conv2 (+ shortcut); reached from
 * unet_3d_blocks.py:1891-2316) without a normalised copy of the activation and with the input staged in LDS as a spatial
 * patch with halo, read 9 times (once per tap) from there:
 *   out[p][n] = bias[n] + rowvec[p / rowvec_rows][n] + residual[p][n] + sum_{tap,c} act(x[p+tap][c]) W[n][(tap, c)]
 *   act(v) = silu?(v * gn_scale[image][c] + gn_shift[image][c])     (gn_* = outputs of tt_groupnorm_stats; NULL: identity)
 * Halo pixels outside the image contribute exact zeros (zero padding of the ACTIVATED tensor, as in the reference).
 * x0 | x1: token-major sources (virtual channel concat, c0 and c1 multiples of 64); W as for tt_gemm mode 1.
 * Serves the image sizes tt_conv3x3_supported() accepts (h x w tiled by 16x8, 8x16 or 8x14 rectangles); everything else
 * (stride 2, upsampling, tiny images, TT_F32) stays on tt_groupnorm_apply + tt_gemm mode 1.
 * ---------------------------------------------------------------------------------------------- */
typedef struct TtConvArgs {
  const void* x0; const void* x1; int32_t c0, c1; int64_t ld0, ld1;
  const void* w; int64_t ldw;                 /* [n, 9*(c0+c1)], k index (tap, source, channel) */
  int32_t nimg, h, w_img, n;
  const float* gn_scale; const float* gn_shift; int32_t silu;     /* fp32 [nimg, c0+c1] each, or both NULL */
  const float* bias;
  const float* rowvec; int32_t rowvec_rows; int64_t ld_rowvec;
  const void* residual; int64_t ld_res;
  void* out; int64_t ldo;
  int32_t dtype;                              /* TT_BF16 or TT_F16 */
} TtConvArgs;
int tt_conv3x3_supported(int32_t h, int32_t w, int32_t c0, int32_t c1, int32_t n, int32_t dtype);
int tt_conv3x3(const TtConvArgs* args, tt_stream_t stream);
/* the instance tt_conv3x3 launches, conv_patch_kernel<tag, TH, TW, BN> (pixel tile, output columns per block), in the form and with the
 * return codes of tt_gemm_kernel: what tt_conv3x3 itself returns for arguments it refuses (the operand pointers are checked, not read). */
int tt_conv3x3_kernel(const TtConvArgs* args, char* name, int32_t cap);

/* ------------------------------------------------------------------------------------------------
 * tt_attention: softmax(Q K^T / sqrt(d)) V with online softmax on MFMA tiles; replaces
 * F.scaled_dot_product_attention inside diffusers AttnProcessor2_0 for
 *   mask 0  spatial self-attention            (BasicTransformerBlock.attn1; transformer_temporal.py:353)
 *   mask 1  spatial cross-attention, S<=pad   (attn2; context of batch n/frames)
 *   mask 2  temporal cross-attention          (TemporalBasicTransformerBlock.attn2, :361-365) with the
 *           reference's (hw,B)-flattened context pairing reproduced: query (b,p) sees context
 *           (b*hw + p) % ctx_batches  (transformer_temporal.py:316-319).
 * q [nseq*lq, ldq] (+ head*d), k [rows, ldk] (+ head*d), vt = V transposed [heads*d, ldvt].
 * ---------------------------------------------------------------------------------------------- */
typedef struct TtAttnArgs {
  const void* q; int64_t ldq;
  const void* k; int64_t ldk;
  const void* vt; int64_t ldvt;
  void* out; int64_t ldo;
  int32_t nseq, lq, heads, head_dim;   /* head_dim 64 or 128 */
  int32_t mask;                        /* 0,1,2 as above */
  int32_t lk;                          /* valid keys per sequence/context */
  int32_t k_seq_stride, v_seq_stride;  /* rows of k / columns of vt per sequence (mask 0) or per context (1,2) */
  /* Finite values between lk and the stride never contribute: the rows of k and the columns of vt (v_rows: the rows of V) in
   * [lk, stride) of a sequence / context may hold anything finite -- their probability is an exact zero, on every route (fp8, v_rows and
   * the fused query projection included).  tests/test_attention_closed_forms_gpu.py runs every route with that padding poisoned. */
  int32_t frames, ctx_batches;         /* masks 1,2 */
  int32_t dtype;
  int32_t batch0;                      /* masks 1,2: batch index of sequence 0 (a launch may cover a sub-range of the batch) */
  /* fp8 != 0 (mask 0 only): q, k, vt hold OCP e4m3 bytes (strides in bytes = elements; written by tt_gemm out_fp8),
   * QK^T and PV run on v_mfma_scale_f32_32x32x64_f8f6f4 (unit block scales) with P = 8 * exp2(s c - m) converted to e4m3, m a
   * lazily updated reference that keeps P inside e4m3's range (the factor cancels against the row sum); softmax statistics
   * and the output accumulation stay fp32, `out` is `dtype` (16-bit).  Scales are 1: the
   * operands are LayerNorm-ed projections, far inside e4m3's +-448.  Its tolerance is e4m3's (3 mantissa bits), see
   * tests/test_ops_gpu.py::test_attention_fp8. */
  int32_t fp8;
  /* Fused query projection (ABI 6; masks 1 / 2, head_dim 64, 16-bit dtype): when qx != NULL, `q` is ignored (may be NULL) and every
   * block computes its own queries  Q = LN(x rows) Wq^T + bq  in front of the key loop -- the nn.Linear to_q of the cross-attention
   * (BasicTransformerBlock.attn2 / TemporalBasicTransformerBlock.attn2, reached from transformer_temporal.py:353-365) and the
   * LayerNorm in front of it, without a Q tensor or a launch of their own.  qx [nseq*lq rows, ldqx] holds the UN-normalised hidden
   * states (rows addressed like q: query r of sequence s is row s*lq + r), qc = the LayerNorm width = columns of wq.
   * wq [heads*64, ldwq] and bq [heads*64] are the LayerNorm-folded projection (packing.fold_layernorm) with bits 2 and 3 of the
   * row index swapped inside every group of 16 rows (packing.permute_q_rows): the projection's MFMA accumulators then ARE the
   * Q^T operand fragments of the score product.  qx and wq hold elements of `dtype`, bq is fp32; all three start on 16-byte
   * boundaries (TT_EINVAL otherwise), wq spans heads*64 rows of qc elements. */
  const void* qx; int64_t ldqx;
  const void* wq; int64_t ldwq;
  const float* bq;
  int32_t qc; float ln_eps;
  /* ABI 10.  v_rows != 0 (mask 0, head_dim 64, 16-bit dtype): `vt` holds V ITSELF -- [key rows, ldvt] (+ head*d), rows addressed like k
   * (sequence s starts at row s * v_seq_stride) -- as it leaves a fused Q | K | V projection (nn.Linear to_q / to_k / to_v of
   * BasicTransformerBlock.attn1 in ONE tt_gemm launch; transformer_temporal.py:353 via diffusers Attention): no V^T projection launch.
   * The kernel transposes on the way out of LDS (ds_read_b64_tr_b16). */
  int32_t v_rows;
} TtAttnArgs;
int tt_attention(const TtAttnArgs* args, tt_stream_t stream);
/* the instance tt_attention launches, in the form and with the return codes of tt_gemm_kernel (tt_attention's own for arguments it refuses;
 * the operand pointers are checked, not read): attn_kernel<tag, head_dim, mask, fused query projection, v_rows, split16>,
 * attn_pipe_kernel<tag> (v_rows with two or more whole tiles of 64 keys) or attn8_kernel<tag, head_dim> (fp8). */
int tt_attention_kernel(const TtAttnArgs* args, char* name, int32_t cap);

/* temporal self-attention over the frame axis (seq = frames <= 32), one 16/32-lane group per
 * (batch, pixel, head); replaces TemporalBasicTransformerBlock.attn1 incl. its two
 * [(B F),hw,C] <-> [(B hw),F,C] permute copies (diffusers; reached from transformer_temporal.py:361).
 * qkv [batch*frames*hw, ldqkv] holds Q | K | V at column offsets 0, C, 2C; columns from 3C up to ldqkv are never read. */
int tt_temporal_attention(const void* qkv, int64_t ldqkv, void* out, int64_t ldo, int32_t batch, int32_t frames,
                          int32_t hw, int32_t heads, int32_t head_dim, int32_t dtype, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GroupNorm(32 groups) split in statistics -> affine (+SiLU); nn.GroupNorm sites: ResnetBlock2D /
 * TemporalResnetBlock norm1/norm2, transformer_temporal.py:234,323, unet...:244,526.
 * `frames_per_group` = 1 for per-image statistics, = F for the temporal block (stats over F*h*w).
 * Two sources = virtual channel concat.  ws must hold tt_groupnorm_ws_bytes().
 * tt_groupnorm_stats writes per-(image, channel) scale/shift fp32 [nimg, C] each:
 *     y = x*scale + shift  ==  (x-mean)*rstd*gamma + beta
 * ---------------------------------------------------------------------------------------------- */
size_t tt_groupnorm_ws_bytes(int32_t nimg, int32_t hw, int32_t c);
int tt_groupnorm_stats(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t nimg, int32_t hw,
                       int32_t frames_per_group, const float* gamma, const float* beta, float eps,
                       float* scale, float* shift, void* ws, size_t ws_bytes, int32_t dtype, tt_stream_t stream);
/* GroupNorm(32) (+SiLU) of x [nseg * seg_rows, c] from the tile sums its producer left (TtGemmArgs.stats_out, stat_rows = the
 * tt_gemm_stats_rows of that launch): ONE pass over x, one launch, for per-image statistics (seg_rows = h*w) and for the cross-frame
 * statistics of TemporalResnetBlock (seg_rows = frames*h*w) alike.  seg_rows must be a multiple of stat_rows (a segment is a whole
 * number of statistics tiles): tt_groupnorm_tiles_supported.  Replaces the statistics pass of tt_groupnorm_small / tt_groupnorm_stats
 * for nn.GroupNorm sites whose input is the direct output of one tt_gemm launch (unet_3d_blocks.py:1891-2316). */
int tt_groupnorm_tiles_supported(int32_t seg_rows, int32_t c, int32_t stat_rows, int32_t dtype);
int tt_groupnorm_tiles(const void* x, int32_t c, const float* stats, int32_t stat_rows, int32_t nseg, int32_t seg_rows,
                       const float* gamma, const float* beta, float eps, int32_t silu, void* y, int64_t ldy, int32_t dtype,
                       tt_stream_t stream);
/* y[n,p,0:c0+c1] = act(x*scale+shift), act = SiLU if silu else identity; y has row stride ldy (>= c0+c1,
 * extra columns untouched). */
int tt_groupnorm_apply(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t nimg, int32_t hw,
                       const float* scale, const float* shift, int32_t silu, void* y, int64_t ldy,
                       int32_t dtype, tt_stream_t stream);

/* Statistics + apply in ONE launch for per-image GroupNorm (frames_per_group = 1): y = act(group_norm(x0 | x1)), no workspace, no
 * scale/shift arrays.  Images of 256 to 4096 rows: one block per (image, slice of consecutive groups) -- a group's statistics need only
 * its own channels, so blocks never exchange anything and x is read from HBM once (the apply pass re-reads the slice from L2).
 * Smaller images (at most 640 KiB per image: the 8x14 / 4x7 levels at 256x448): one block per image and row part, each recomputing
 * the image's statistics.  Same result as tt_groupnorm_stats + tt_groupnorm_apply up to fp32 summation order; bit-reproducible.
 * ResnetBlock2D norm1 / norm2 (diffusers resnet.py), TransformerSpatioTemporalModel.norm (transformer_temporal.py:323),
 * conv_norm_out (unet...:526). */
int tt_groupnorm_small_supported(int32_t hw, int32_t c, int32_t dtype);
/* Which kernels a GroupNorm of hw rows x c channels per image runs (host only; the launchers take their decisions from the same code).
 * one_launch != 0: tt_groupnorm_small -- TT_GN_ROUTE_GROUPED (gn_group_kernel, one block per image and group slice), TT_GN_ROUTE_IMAGE
 * (gn_stats_image_kernel, one block per image and row part) or 0 (not served: frames_per_group must be 1).  one_launch == 0:
 * tt_groupnorm_stats -- TT_GN_ROUTE_IMAGE (gn_stats_image_kernel writes scale / shift) or TT_GN_ROUTE_PARTIAL (gn_partial_kernel +
 * gn_finalize_kernel).  0 for channel counts no GroupNorm entry point accepts.  For launch traces and tests. */
#define TT_GN_ROUTE_IMAGE 1
#define TT_GN_ROUTE_GROUPED 2
#define TT_GN_ROUTE_PARTIAL 3
int tt_groupnorm_route(int32_t hw, int32_t c, int32_t dtype, int32_t frames_per_group, int32_t one_launch);
int tt_groupnorm_small(const void* x0, int32_t c0, const void* x1, int32_t c1, int32_t nimg, int32_t hw,
                       const float* gamma, const float* beta, float eps, int32_t silu, void* y, int64_t ldy,
                       int32_t dtype, tt_stream_t stream);

/* LayerNorm over the last dim (eps, affine); nn.LayerNorm inside Basic/TemporalBasicTransformerBlock.
 * Optional fused frame-position embedding (transformer_temporal.py:358-359): when rowvec != NULL,
 * x' = x + rowvec[(row / rows_per_vec) % nvec] is written to xsum_out and normalised. */
int tt_layernorm(const void* x, int64_t ldx, int32_t rows, int32_t c, const float* gamma, const float* beta,
                 float eps, const float* rowvec, int32_t rows_per_vec, int32_t nvec, void* xsum_out,
                 void* y, int64_t ldy, int32_t dtype, tt_stream_t stream);

/* Weight packing on the device (packing.zero_sum_round; the LayerNorm-folded projections of Basic / TemporalBasicTransformerBlock reached
 * from transformer_temporal.py:342-365): rounds the rows of w (fp32 [n, k], each summing to ~0) to the 16-bit `dtype` such that every ROUNDED
 * row sums to exactly zero -- binade by binade from `hi` down to max(lo, hi - 48) (the largest / smallest binade exponent of the rounded
 * non-zero values of the whole matrix), up to round(|row sum| / ulp) elements of a binade move by one ulp.  One block per row; the result is
 * bit-identical to the host implementation.  k <= 16384. */
int tt_zero_sum_round(const float* w, int64_t ldw, int32_t n, int32_t k, int32_t hi, int32_t lo, void* out, int64_t ldo,
                      int32_t dtype, tt_stream_t stream);
/* ------------------------------------------------------------------------------------------------
 * small dense layers on <=32 rows, fp32 activations (time / add / FiLM / frame-position MLPs:
 * unet...:416-432, ResnetBlock2D.time_emb_proj, transformer_temporal.py:338):
 *   y[r][n] = act_out( sum_k act_in(x[r][k]) * W[n][k] + bias[n] ),  act: 0 none, 1 SiLU.
 * W is `dtype`, x/y/bias fp32.  accumulate != 0 adds into y.  k % 8 == 0 and k <= 8192 (the activated rows of x are staged
 * in LDS four at a time: 4 x k fp32; TT_EUNSUPPORTED beyond -- the path's widest MLP input is 1280).
 * x and w are read in 16-byte vectors: TT_EINVAL when either does not start on a 16-byte boundary, when ldx or ldw is below k or
 * ldy below n (with more than one row / column behind the stride).
 * ---------------------------------------------------------------------------------------------- */
int tt_small_linear(const float* x, int64_t ldx, int32_t rows, int32_t k, const void* w, int64_t ldw, int32_t n,
                    const float* bias, int32_t act_in, int32_t act_out, int32_t accumulate, float* y, int64_t ldy,
                    int32_t dtype, tt_stream_t stream);
/* diffusers Timesteps(dim, flip_sin_to_cos=True, shift=0): out[r] = [cos(t_r*f_i) | sin(t_r*f_i)], fp32.
 * `t` device fp32 [rows].  TT_EINVAL: ldo < dim (more than one row), rows * dim / 2 beyond 32 bits (the kernel's element index). */
int tt_timestep_embedding(const float* t, int32_t rows, int32_t dim, float* out, int64_t ldo, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * denoise-loop glue (pipeline_stable_video_diffusion_controlnet.py:630-635,704-709):
 * tt_prep_model_input: x[b,f,p,0:4] = latents[f,:,p] * c_in (CFG: same latents for every b),
 *   x[...,4:8] = image_latents[b,f,:,p], x[...,8:12] = cond[f,:,p] (if cond), rest of cpad zero.
 *   latents/image_latents/cond are fp32 NCHW-per-frame as the pipeline holds them.
 * tt_cfg_euler_step: eps[b,f,p,0:4] fp32 token-major (conv_out) ->
 *   v = u + g_f*(c-u);  x0 = v*(-s/sqrt(s^2+1)) + x/(s^2+1);  x += (x-x0)/s*(s_next-s)   (in place, fp32)
 * tt_cfg3_euler_step: the use_instructpix2pix variant (:698-702), eps batch of 3 in the reference's order
 *   (first-frame e1, cond c, uncond u):  v = u + g_f*(c-u) + image_guidance_scale*(c-e1), then the same Euler update.
 * sigma scalars live on the device (sigmas[step], sigmas[step+1]) so a captured graph can be replayed
 * for every step.  TT_EINVAL (all three): h or w <= 0, h * w beyond 32 bits (the kernels hold the pixel count in an int).
 * ---------------------------------------------------------------------------------------------- */
int tt_prep_model_input(const float* latents, const float* image_latents, const float* cond, const float* sigmas,
                        int32_t step, int32_t batch, int32_t frames, int32_t h, int32_t w, int32_t cpad,
                        void* x, int32_t dtype, tt_stream_t stream);
int tt_cfg_euler_step(const float* eps, int32_t ld_eps, float* latents, const float* guidance, const float* sigmas,
                      int32_t step, int32_t batch, int32_t frames, int32_t h, int32_t w, tt_stream_t stream);
int tt_cfg3_euler_step(const float* eps, int32_t ld_eps, float* latents, const float* guidance, float image_guidance_scale,
                       const float* sigmas, int32_t step, int32_t frames, int32_t h, int32_t w, tt_stream_t stream);

/* The same glue for R independent requests in one launch (additive: the ABI version is unchanged).  The reference's __call__ takes a
 * list of images and num_videos_per_prompt > 1 (pipeline_stable_video_diffusion_controlnet.py:392, :520-605) and runs the loop body
 * (:630-635 prep, :698-709 CFG + scheduler.step) on the joint batch; here every request is computed as a call of its own would.
 * Batch order is CFG-major, b = c * requests + r, c in [0, cfg): what torch.cat([neg, cond]) (:185, :211)
 * gives for batched tensors, so image_latents [R*C,F,4,h,w] is taken as the reference holds it.
 * tt_prep_model_input_requests: x[b,f,p,0:4] = latents[r,f,:,p] * c_in, x[...,4:8] = image_latents[b,f,:,p],
 *   x[...,8:12] = cond[f,:,p] (cond_per_request 0: one [F,4,h,w] for all requests, reference :660) or cond[r,f,:,p]
 *   (cond_per_request 1: [R,F,4,h,w]); cond NULL: 8 channels.  x [R*C*F*h*w, cpad] token rows in `dtype`.
 * tt_cfg_euler_step_requests: eps [R*C*F*h*w, ld_eps] fp32 token rows in the same order; cfg 1 (no CFG; guidance may be NULL),
 *   2 (uncond, cond) or 3 (first-frame, cond, uncond + image_guidance_scale, :698-702); guidance fp32 [F] for all requests
 *   (guidance_per_request 0) or [R,F] (1); latents fp32 [R,F,4,h,w] updated in place by the v-prediction Euler step.  All requests
 *   share sigmas[step], sigmas[step+1].
 * Element indices are 64-bit throughout.  TT_EINVAL: a null operand, requests / frames / h / w <= 0, cfg outside 1..3, cpad < 8 (12
 * with cond) or not a multiple of 8, a flag that is not 0 / 1, ld_eps < 4, cfg 3 without guidance, a bad dtype. */
int tt_prep_model_input_requests(const float* latents, const float* image_latents, const float* cond, int32_t cond_per_request,
                                 const float* sigmas, int32_t step, int32_t requests, int32_t cfg, int32_t frames, int32_t h,
                                 int32_t w, int32_t cpad, void* x, int32_t dtype, tt_stream_t stream);
int tt_cfg_euler_step_requests(const float* eps, int64_t ld_eps, float* latents, const float* guidance, int32_t guidance_per_request,
                               float image_guidance_scale, const float* sigmas, int32_t step, int32_t requests, int32_t cfg,
                               int32_t frames, int32_t h, int32_t w, tt_stream_t stream);

/* A second sampler on the same glue (additive: the ABI version is unchanged): DPM-Solver++ multistep, second order ("2M"; Lu, Zhou,
 * Bao, Chen, Li, Zhu, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", 2022, the multistep
 * second-order data-prediction update) in the sigma parametrisation alpha = 1, lambda = -ln sigma.  One network evaluation per step,
 * like Euler; the only state is the previous step's data prediction x0.
 * Schedule and coefficients (host; svd/scheduling_dpmsolver_multistep.py): the schedule is EulerDiscreteScheduler.set_timesteps' --
 *   the same fp32 sigmas (N values and a final 0), timesteps 0.25 ln sigma, init_noise_sigma, scale_model_input.  For step i with
 *   1 <= i <= N-2:  h_i = ln(sigma_i / sigma_{i+1}),  c_i = h_i / (2 h_{i-1}),  computed in fp64 from the fp32 sigmas and rounded to
 *   fp32.  c_0 = 0 (no history yet); c_{N-1} = 0 (sigma_N = 0, h infinite: diffusers' final_sigmas_type "zero" makes the last step
 *   first order).  solver_order 1: every c_i = 0.  N = 1 and N = 2 run first order throughout.
 * Per latent element, fp32, every product and sum rounded on its own (contraction off), in the statement order of
 * tt_cfg_euler_step_requests:
 *     v    = CFG combination of eps                       the three cases and statements of tt_cfg_euler_step_requests
 *     x0   = v * c_out + x * c_skip                       c_out = -s / sqrtf(s*s + 1), c_skip = 1 / (s*s + 1), s = sigmas[step]
 *     D    = (c != 0) ? x0 + c * (x0 - hist) : x0         a branch, not a multiply: hist is NOT read when c == 0
 *     hist = x0                                           always stored
 *     x    = x + (x - D) / s * (s_next - s)               s_next = sigmas[step + 1]
 * which is  x' = (s'/s) x + (1 - s'/s) [(1 + 1/(2r)) x0 - (1/(2r)) x0_prev],  r = h_{i-1} / h_i:  diffusers' "dpmsolver++" /
 * "midpoint" second-order update.  With c == 0 it is tt_cfg_euler_step_requests statement for statement, bit for bit.
 * tt_cfg_multistep_step_requests: eps, latents, guidance, the batch order and cfg 1 / 2 / 3 as tt_cfg_euler_step_requests (requests >=
 *   1); x0_hist fp32 [R,F,4,h,w], laid out like latents; coef: device, one fp32, the c of this step.  coef and sigmas are read on the
 *   device, so one captured graph serves every step.  Element indices are 64-bit.  TT_EINVAL (tt_last_error has the text; nothing is
 *   launched): a null eps / latents / x0_hist / sigmas / coef, and every refusal of tt_cfg_euler_step_requests. */
int tt_cfg_multistep_step_requests(const float* eps, int64_t ld_eps, float* latents, float* x0_hist, const float* guidance,
                                   int32_t guidance_per_request, float image_guidance_scale, const float* sigmas, int32_t step,
                                   const float* coef /* device, one fp32: c of this step */, int32_t requests, int32_t cfg,
                                   int32_t frames, int32_t h, int32_t w, tt_stream_t stream);

/* layout plumbing at the drop-in boundary: NCHW (any float dtype code below) <-> token-major.
 * src_kind/dst_kind: 0 = dtype (bf16/f16), 1 = fp32. */
int tt_nchw_to_tokens(const void* src, int32_t src_f32, int32_t nimg, int32_t c, int32_t hw, void* dst, int64_t ld_dst,
                      int32_t dtype, tt_stream_t stream);
int tt_tokens_to_nchw(const void* src, int32_t src_f32, int64_t ld_src, int32_t nimg, int32_t c, int32_t hw, void* dst,
                      int32_t dst_f32, int32_t dtype, tt_stream_t stream);
/* y = a + b*scale (dtype, elementwise, n multiple of 8): ControlNet residual add, unet...:485-491,501-502.
 * a, b and y are accessed in 16-byte vectors: TT_EINVAL when one does not start on a 16-byte boundary. */
int tt_add_scaled(const void* a, const void* b, float scale, void* y, int64_t n, int32_t dtype, tt_stream_t stream);
/* y[r][c] = x[r][c] + rowvec[(r / rows_per_vec) % nvec][c]: the frame-position embedding added to the hidden states before
 * the temporal transformer block (transformer_temporal.py:358-359; the block's norm_in is folded into its first GEMM).
 * x, y `dtype` [rows, c] (c multiple of 8), rowvec fp32 [nvec, c].  TT_EINVAL: x, y or rowvec off a 16-byte boundary (vector accesses);
 * ldx or ldy below c with more than one row, ld_rowvec below c with more than one vector. */
int tt_add_rowvec(const void* x, int64_t ldx, int32_t rows, int32_t c, const float* rowvec, int64_t ld_rowvec,
                  int32_t rows_per_vec, int32_t nvec, void* y, int64_t ldy, int32_t dtype, tt_stream_t stream);

/* y[r, 0:cols] = softmax(x[r, 0:cols]) over fp32 scores, y[r, cols:cols_pad] = 0; y in `dtype` storage.  The attention of the
 * temporal VAE decoder's mid block (one head of 512 channels over h*w tokens per frame: diffusers
 * autoencoder_kl_temporal_decoder.py MidBlockTemporalDecoder, reached from
 * svd/pipeline_stable_video_diffusion_controlnet.py:257-283) runs as  scores = tt_gemm(Q, K, out_f32)  ->  tt_softmax_rows
 * ->  tt_gemm(P, V^T): head_dim 512 is outside tt_attention's 64 / 128.  Rows are read as float4 and written four elements at a time:
 * TT_EINVAL when x is off a 16-byte boundary or y off a boundary of four of its elements (8 bytes for the 16-bit types, 16 for fp32). */
int tt_softmax_rows(const float* x, int64_t ldx, int32_t rows, int32_t cols, void* y, int64_t ldy, int32_t cols_pad,
                    int32_t dtype, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The CLIP encoders behind encode_clip (svd/pipeline_stable_video_diffusion_controlnet.py:130-185): the image encoder
 * CLIPVisionModelWithProjection (loaded at test_code/inference.py:325; ViT-H/14: width 1280, 16 heads of 80, 257 tokens) and the
 * text encoder CLIPTextModel (test_code/inference.py:348; SD-2.1: width 1024, 16 heads of 64, 77 tokens, causal), chosen per
 * checkpoint by train_code/train_svd.py:214-231.  Their Linear layers and LayerNorms are tt_gemm / tt_layernorm; the entry points
 * below are what those do not cover.  Additive: the ABI version is unchanged.
 *
 * tt_encoder_attention: self-attention  softmax(Q K^T / sqrt(d) [+ causal]) V  per (sequence, head) with lq == lk == l, any l >= 1,
 * head_dim 64 or 80 (CLIPAttention; transformers modeling_clip.py, reached from encode_clip :130-185).
 *   q   [nseq * l, ldq]  (+ head * d): query r of sequence s is row s * l + r
 *   k   [rows, ldk]      (+ head * d): key j of sequence s is row s * k_seq_stride + j
 *   v   TT_BF16 / TT_F16: V itself, [rows, ldv] (+ head * d), rows addressed like k with v_seq_stride -- q, k and v are then the three
 *                         column slices of one fused [nseq * l, 3 C] projection output; the kernel transposes on the way out of LDS.
 *       TT_F32:           V TRANSPOSED, [heads * d, ldv]: key j of sequence s is column s * v_seq_stride + j (written by tt_gemm with
 *                         out_col_hw = l, out_col_hwp = v_seq_stride, a multiple of 4; fp32 storage has no transposing LDS read).
 *   out [nseq * l, ldo]  (+ head * d)
 * causal != 0: key j > query r scores -inf (CLIPTextModel's mask); key tiles wholly past a block's last query are skipped.
 * Keys >= l of a sequence (a stride larger than l) never contribute: their probability is an exact zero (finite values assumed).
 * head_dim 80 runs as a head padded to 128 columns in LDS: chunks beyond the head's 80 elements read as zeros through the buffer
 * descriptor (never from the next head), the scale is 1/sqrt(80), 80 columns are stored.  TT_F32 always multiplies with the
 * exact-fp32 MFMA (tt_gemm_set_f32_split does not change this kernel).
 * ---------------------------------------------------------------------------------------------- */
typedef struct TtEncAttnArgs {
  const void* q; int64_t ldq;
  const void* k; int64_t ldk;
  const void* v; int64_t ldv;
  void* out; int64_t ldo;
  int32_t nseq, l, heads, head_dim;    /* head_dim 64 or 80 */
  int32_t causal;                      /* 0 / 1 */
  int32_t k_seq_stride, v_seq_stride;  /* rows of k (and of v, 16-bit) / columns of v (TT_F32) per sequence, >= l */
  int32_t dtype;
} TtEncAttnArgs;
int tt_encoder_attention(const TtEncAttnArgs* args, tt_stream_t stream);

/* y[r][0:c] = act(x[r][0:c]) over `dtype` rows with strides (c, ldx, ldy multiples of 8); y may be x (in place).
 *   act 0  exact-erf GELU            (hidden_act "gelu": CLIP ViT-H and SD-2.1's text encoder; CLIPMLP between fc1 and fc2)
 *   act 1  x * sigmoid(1.702 x)      ("quick_gelu": OpenAI CLIP checkpoints)
 * encode_clip, svd/pipeline_stable_video_diffusion_controlnet.py:130-185. */
int tt_act_rows(const void* x, int64_t ldx, int32_t rows, int32_t c, int32_t act, void* y, int64_t ldy, int32_t dtype,
                tt_stream_t stream);

/* NCHW image -> patch token rows for CLIPVisionEmbeddings.patch_embedding (Conv2d(3, C, p, stride p, bias=False); the
 * CLIPVisionModelWithProjection of test_code/inference.py:325):  dst[(n, py, px)][k] = src[n][c][py*p + ky][px*p + kx],
 * k = (c, ky, kx) as patch_embedding.weight.flatten(1) orders it, columns ch*p*p .. kpad zero-filled (kpad a multiple of 8,
 * >= ch*p*p, <= ld_dst).  The conv is then one mode-0 tt_gemm against the weight packed to kpad columns.
 * src fp32 (src_f32 != 0) or `dtype`, contiguous [nimg, ch, h, w], h and w multiples of p. */
int tt_patch_tokens(const void* src, int32_t src_f32, int32_t nimg, int32_t ch, int32_t h, int32_t w, int32_t p, void* dst,
                    int64_t ld_dst, int32_t kpad, int32_t dtype, tt_stream_t stream);

/* The embedding rows of the two encoders (CLIPTextEmbeddings / CLIPVisionEmbeddings; encode_clip :130-185), `dtype` tables,
 * c a multiple of 8, out [rows, ldo]:
 *   mode 0 (text)    out[r] = table[ids[r]] + pos[r % l]                      ids int64 [rows], each in [0, table_rows)
 *                    (an id outside the table leaves a row of zeros + pos: no out-of-range read)
 *   mode 1 (vision)  out[r] = (r % l == 0 ? cls : patches[(r / l) * (l - 1) + r % l - 1]) + pos[r % l]
 *                    table = patch rows [rows / l * (l - 1), ld_table], cls = the class embedding [c], ids unused. */
int tt_embed_rows(int32_t mode, const int64_t* ids, const void* table, int64_t ld_table, int32_t table_rows, const void* cls,
                  const void* pos, int64_t ld_pos, int32_t rows, int32_t l, int32_t c, void* out, int64_t ldo, int32_t dtype,
                  tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The request path around the models: what encode_clip does to the image before the CLIP vision model and to the context after the
 * text encoder, and what decode_latents / tensor2vid do to the decoder's output (svd/pipeline_stable_video_diffusion_controlnet.py).
 * Additive: the ABI version is unchanged.
 *
 * tt_clip_image: the preprocessing in front of CLIPVisionModelWithProjection -- _resize_with_antialiasing (:741-767) as encode_clip
 * calls it (:130-185: image * 2 - 1, resize to out_h x out_w, (image + 1) / 2) and the feature extractor's per-channel
 * normalisation (:145-152).  All arithmetic fp32:
 *   src      src_kind 0: uint8 [nimg, h, w, 3] (what np.asarray of a PIL RGB image holds), x = u / 255;
 *            src_kind 1: fp32 [nimg, 3, h, w] in [0, 1]
 *   v = 2 x - 1
 *   per axis: f = in / out, sigma = max((f - 1) / 2, 1e-3), k = int(max(4 sigma, 3)) made odd; taps exp(-t^2 / (2 sigma^2)) for
 *            t = -(k / 2) .. k / 2, normalised to sum 1 (formed on the host in fp64, rounded to fp32)
 *   blur     along x, then along y, each with reflect padding (no edge repeat)
 *   resample bicubic, align_corners = True (source position o (in - 1) / (out - 1)), A = -0.75, the four tap indices clamped to the image
 *   dst[n][c] = ((v + 1) / 2 - mean_c) / std_c   in `dtype` (TT_BF16 / TT_F16 / TT_F32), contiguous [nimg, 3, out_h, out_w]
 * THREE launches (blur x: src -> ws, blur y: ws -> ws, resample + normalise: ws -> dst); ws holds two fp32 copies of the image planes,
 * tt_clip_image_ws_bytes(nimg, h, w) bytes, 16-byte aligned.  Refused: TT_EINVAL for a null operand, a bad src_kind / dtype, an empty
 * image, out_h or out_w < 2 (align_corners divides by out - 1), a std <= 0, a reflect pad k / 2 that reaches the image size (h or
 * w <= k / 2: torch refuses it too), a workspace that is too small or misaligned; TT_EUNSUPPORTED for more than 63 taps on an axis (63
 * covers in / out <= 32.5, e.g. a 3500-pixel side -> 224). */
size_t tt_clip_image_ws_bytes(int32_t nimg, int32_t h, int32_t w);
int tt_clip_image(const void* src, int32_t src_kind, int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w,
                  float mean0, float mean1, float mean2, float std0, float std1, float std2, void* dst, int32_t dtype,
                  void* ws, size_t ws_bytes, tt_stream_t stream);

/* LayerNorm without affine parameters over a whole [rows, c] block per batch element: the nn.LayerNorm((78, 1024)) that encode_clip
 * constructs afresh (weight 1, bias 0) for the text + image context of use_text requests (:172):
 *   y[b] = (x[b] - mean_b) * rsqrt(var_b + eps),  mean_b / var_b (biased) over all rows * c elements of batch element b.
 * x and y are [nb * rows, ldx] in `dtype` with the same row stride (c, ldx multiples of 8, ldx >= c; columns c .. ldx are neither
 * read nor written); y may be x.  Statistics: the mean first (fp32 sums of x - x[b][0][0] per thread, fp64 across threads), then the sum
 * of squares centred on it -- never E[x^2] - E[x]^2.  One 256-thread block per batch element, one launch. */
int tt_layernorm_block(const void* x, int64_t ldx, int32_t nb, int32_t rows, int32_t c, float eps, void* y, int32_t dtype,
                       tt_stream_t stream);

/* Decoder output -> what the caller receives: decode_latents' permute + float (:257-283) and tensor2vid / VaeImageProcessor.postprocess
 * (image / 2 + 0.5, clamp to [0, 1], NCHW -> NHWC; for "pil" numpy_to_pil's (image * 255).round().astype(uint8)).
 *   src  [n, ch, h, w] in src_dtype (TT_BF16 / TT_F16 / TT_F32), 1 <= ch <= 4 (TT_EUNSUPPORTED beyond)
 *   dst  [n, h, w, ch]:  kind 0  fp32   f = clamp(x * 0.5 + 0.5, 0, 1)
 *                        kind 1  uint8  rint(f * 255), round-half-to-even
 * Bit-exact with the torch / numpy statements on the fp32 value of x: x * 0.5 is exact, so the addition is the only rounding, and
 * f * 255 is one fp32 product.  A NaN is not part of the contract: the kernel writes 0 (kind 0: +0.0f) where torch writes NaN.
 * One launch. */
int tt_frames_out(const void* src, int32_t src_dtype, int32_t n, int32_t ch, int32_t h, int32_t w, int32_t kind, void* dst,
                  tt_stream_t stream);

/* tt_gesture_maps: the "this"/"that" conditioning frames of a request, rasterised from the annotated points themselves -- the
 * reference's get_thisthat_sam (data_loader/video_this_that_dataset.py:28-130, blur kernel utils/optical_flow_utils.py:197-219) as
 * this_and_that_vdm_amd/gesture_map.py restates it.  The reference draws a 21 x 21 square on a white canvas of the ORIGINAL image
 * size, blurs it (filter2D, 99 Gaussian taps, BORDER_REFLECT_101), resizes it (INTER_CUBIC) and divides by 255.  The canvas is
 * 255 - (255 - colour) box with box an outer product of two 1-D indicators, and blur and resize are separable with rows that sum
 * to 1, so every frame is rank 1:  1 - d_c ry[y] rx[x]  with two short profiles per point.
 *
 *   points   HOST pointer: npoints <= 64 records, copied into kernel arguments before the call returns (no device copy of them)
 *            {map, frame, x, y, first}: the point (x horizontal, y vertical, original-image pixels, may lie outside the image)
 *            decides frame `frame` of map `map`; first != 0 marks the "this" point (red), the others are green.
 *            The LAST record of the list with a given (map, frame) wins; a frame no record names is all zeros.
 *   per axis of original length n, centre c, output length n_out:
 *     box      b[i] = 1 for max(0, c - 10) <= i < min(n, c + 11), else 0 (may be empty: the frame is then all ones)
 *     blur     g[i] = sum_{t < T} k[t] b[r101(i + t - T / 2)];  r101(j): 0 if n == 1, else p = 2 (n - 1), j = |j| mod p, p - j if j >= n
 *              dilate = 1: T = 99, k[t] ~ exp(-x^2 / 200), x = -49 .. 49, normalised to sum 1 (host, fp64); dilate = 0: T = 1, k = [1]
 *     resize   s = (o + 0.5) (n / n_out) - 0.5, base = floor(s), t = s - base; Keys weights (A = -0.75) far(t + 1), near(t),
 *              near(1 - t), far(2 - t) on g[clamp(base - 1 + tap, 0, n - 1)]; no antialiasing, no clamping of the result
 *     flip = 1 mirrors the horizontal profile: rx[o] <- rx[out_w - 1 - o]
 *   dst[m][f][c][y][x] = 1 - d_c ry[y] rx[x], planes in the reference's B, G, R order: d = (1, 1, 0) for a first record, (1, 0, 1)
 *            otherwise.  Contiguous [nmaps, frames, 3, out_h, out_w] in `dtype` (TT_F32 / TT_F16 / TT_BF16); EVERY element is
 *            written by the call, the exact zeros of unnamed frames included.
 * The profiles are accumulated in fp64; ry[y] rx[x] is the fp64 product rounded once to fp32, the subtraction is fp32, and a 16-bit
 * dtype stores the round-to-nearest-even of that fp32 value.  Stores are 16-byte vectors over the flat output whatever out_w is;
 * only the last total % (16 / element size) elements leave one by one.
 * TWO launches (profiles -> ws, store stream ws -> dst), no host array, no copy, no synchronisation: the call can be captured.
 * ws: tt_gesture_maps_ws_bytes(npoints, out_h, out_w) bytes on a 16-byte boundary (0 bytes, and ws may be NULL, for npoints == 0).
 * Refused before the first HIP call.  TT_EINVAL: null dst; null points with npoints > 0; nmaps / frames / out_h / out_w / org_h /
 * org_w <= 0; npoints < 0; a record's map or frame out of range; first, dilate or flip other than 0 / 1; a bad dtype; dst off a
 * 16-byte boundary; a workspace that is missing, too small or misaligned.  TT_EUNSUPPORTED: more than 64 points; an original axis
 * longer than TT_GESTURE_MAX_AXIS; an output beyond the kernel's 32-bit per-frame indices (3 out_h out_w > 2^31 - 4096,
 * nmaps frames >= 2^31, or more than 2^31 - 1 blocks of 256 16-byte stores). */
#define TT_GESTURE_MAX_POINTS 64
#define TT_GESTURE_MAX_AXIS (1 << 24)      /* original height / width: 2 (n - 1) and i + 98 stay far inside int32 */
typedef struct TtGesturePoint { int32_t map, frame, x, y, first; } TtGesturePoint;
size_t tt_gesture_maps_ws_bytes(int32_t npoints, int32_t out_h, int32_t out_w);
int tt_gesture_maps(const TtGesturePoint* points /* host */, int32_t npoints, int32_t nmaps, int32_t frames, int32_t org_h,
                    int32_t org_w, int32_t out_h, int32_t out_w, int32_t dilate, int32_t flip, void* dst, int32_t dtype, void* ws,
                    size_t ws_bytes, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The request image itself: PIL's 8-bit resize (Image.resize on an RGB image; what VaeImageProcessor.preprocess does with LANCZOS,
 * svd/pipeline_stable_video_diffusion_controlnet.py:530, and what the reference's callers do with BICUBIC before the pipeline,
 * test_code/inference.py:83,198, app.py:278) and the VAE input that follows it (:530-532).  The resampler is integer arithmetic on
 * tables the host forms in fp64, so the result equals Pillow's byte for byte.  Additive: the ABI version is unchanged.
 *
 * tt_resample_coeffs (HOST only, no HIP call): the tables of one axis, Pillow's precompute_coeffs + normalize_coeffs_8bpc, in fp64
 * with libm, in this order:
 *   scale = in / out, fs = max(scale, 1), ss = 1 / fs, support = S fs, ksize = 2 ceil(support) + 1
 *   per output o:  c = (o + 0.5) scale,  xmin = max((int)(c - support + 0.5), 0),  n = min((int)(c + support + 0.5), in) - xmin
 *                  w[x] = f((x + xmin - c + 0.5) ss) for x < n, ww their sum in index order, w[x] /= ww when ww != 0
 *                  kk[o][x] = (int)(w[x] 2^22 + 0.5) for w[x] >= 0, (int)(w[x] 2^22 - 0.5) otherwise (truncating); 0 for n <= x < ksize
 *                  bounds[o] = (xmin, n)
 *   filter (PIL's codes)  TT_RESAMPLE_BOX 4       S = 0.5  1 on (-0.5, 0.5]
 *                         TT_RESAMPLE_BILINEAR 2  S = 1    1 - |x|
 *                         TT_RESAMPLE_HAMMING 5   S = 1    sinc(x) (0.54f + 0.46f cos(pi x)), 1 at 0: the two constants are fp32 values
 *                         TT_RESAMPLE_BICUBIC 3   S = 2    Keys, a = -0.5
 *                         TT_RESAMPLE_LANCZOS 1   S = 3    sinc(x) sinc(x / 3) on [-3, 3)
 * *ksize is always written; bounds [2 out] and kk [out ksize] are written when both are non-null (both null: ksize only).
 * Refused: TT_EINVAL for a null ksize, one null buffer of the two, in_size or out_size <= 0, an unknown filter; TT_EUNSUPPORTED for
 * a size above TT_RESAMPLE_MAX_AXIS.
 *
 * DEVICE table of one axis, int32 [(2 + ksize) out], tap-major so that neighbouring outputs read neighbouring words:
 *   tab[o] = xmin, tab[out + o] = n, tab[(2 + t) out + o] = kk[o][t].  NULL for an axis whose size does not change.
 *
 * The two passes (Pillow's ImagingResampleHorizontal_8bpc, then ImagingResampleVertical_8bpc), each skipped when its size is
 * unchanged:  acc = 1 << 21 (int32);  acc += pixel kk[t] for t < n;  byte = clamp(acc >> 22 (arithmetic), 0, 255).
 * The intermediate [nimg, h, out_w, 3] is uint8, as in PIL.  The kernels clamp xmin to [0, in - 1] and n to [0, min(ksize, in - xmin)],
 * so no table makes them read outside the source or the table.
 *
 * tt_resize_u8:  src uint8 [nimg, h, w, 3] -> dst uint8 [nimg, out_h, out_w, 3].  Both sizes unchanged: one device-to-device copy on the stream.
 * tt_vae_image:  the same pixels through the epilogue of the LAST pass (the only launch when neither size changes), for request r of
 *   image r / nvid, r < nimg nvid:   x = u / 255.0f;  v = 2 x - 1;  y = v + na noise[r]   (noise NULL: y = v, na ignored)
 *   every operation rounded to fp32 on its own (no contraction), then ONE round-to-nearest-even to `dtype`;
 *   dst contiguous [nimg nvid, 3, out_h, out_w] in `dtype`, noise fp32 of the same shape -- image_processor.preprocess, the
 *   repeat_interleave of the videos of an image, + noise_aug_strength * randn and .to(vae.dtype) in one store.
 * AT MOST TWO launches.  ws holds the intermediate: tt_*_ws_bytes() = nimg h out_w 3 bytes when both sizes change, else 0 (ws may
 * then be NULL); 16-byte aligned.
 * Refused before the first HIP call.  TT_EINVAL: null src / dst; nimg, a size or nvid <= 0; a table that is NULL for an axis that
 * changes, or given for one that does not; ksize < 1 for a given table; a bad dtype; dst (uint8) off a 4-byte boundary, dst / noise
 * (tt_vae_image) off their element size, a table off a 4-byte boundary; a workspace that is missing, too small or misaligned.
 * TT_EUNSUPPORTED: a size above TT_RESAMPLE_MAX_AXIS, or more elements than one grid covers. */
#define TT_RESAMPLE_MAX_AXIS (1 << 20)
enum { TT_RESAMPLE_LANCZOS = 1, TT_RESAMPLE_BILINEAR = 2, TT_RESAMPLE_BICUBIC = 3, TT_RESAMPLE_BOX = 4, TT_RESAMPLE_HAMMING = 5 };
int tt_resample_coeffs(int32_t in_size, int32_t out_size, int32_t filter, int32_t* ksize /* host */, int32_t* bounds /* host [2 out] */,
                       int32_t* kk /* host [out ksize] */);
size_t tt_resize_u8_ws_bytes(int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w);
int tt_resize_u8(const void* src, int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w, const int32_t* tab_x,
                 int32_t ksize_x, const int32_t* tab_y, int32_t ksize_y, void* dst, void* ws, size_t ws_bytes, tt_stream_t stream);
size_t tt_vae_image_ws_bytes(int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w);
int tt_vae_image(const void* src, int32_t nimg, int32_t h, int32_t w, int32_t out_h, int32_t out_w, const int32_t* tab_x,
                 int32_t ksize_x, const int32_t* tab_y, int32_t ksize_y, const float* noise, float na, int32_t nvid, void* dst,
                 int32_t dtype, void* ws, size_t ws_bytes, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * tt_tensor_stats: the range audit's instrument -- ONE pass over a row-strided 2-D tensor x [rows, cols] (row stride ldx elements,
 * columns cols..ldx-1 of a row are never read) fills a fixed-size DEVICE record with exact integer counts and bit-exact extrema.
 * Nothing in the denoise path calls it unless an audit is active (this_and_that_vdm_amd/audit.py).  Additive: the ABI version is
 * unchanged.
 *
 * dtype: TT_BF16, TT_F16, TT_F32 or TT_FP8_E4M3 (OCP e4m3 bytes, what tt_gemm's out_fp8 writes: no infinities, S.1111.111 is NaN).
 * Every value is widened to fp32 first (exact for all four) and classified on the fp32 bit pattern u, a = u & 0x7fffffff:
 *   NaN a > 0x7f800000, +-inf a == 0x7f800000 (by sign), zero a == 0 (both signs), everything else "finite non-zero".
 *
 * TtTensorStats -- 616 bytes, every field naturally aligned, no padding (byte offsets in brackets):
 *   [  0] uint64 count             rows * cols
 *   [  8] uint64 n_nan   [ 16] n_pinf   [ 24] n_ninf   [ 32] n_zero
 *   [ 40] uint64 n_ge[4]           finite values with |x| >= thr[i] (thr: four fp32 thresholds, >= 0, not NaN; +inf never counts)
 *   [ 72] uint64 hist[64]          finite non-zero values by biased fp32 exponent E = a >> 23: bin = clamp(E - 127 + 40, 0, 63), i.e. bin b
 *                                  holds [2^(b-40), 2^(b-39)); fp32 subnormals (E = 0) and everything below 2^-40 land in bin 0
 *   [584] double sum               over finite values, fp64
 *   [592] double sum_sq            over finite values, fp64 (the square of an fp32 value is exact in fp64)
 *   [600] float  max_abs           over finite non-zero values; 0 when there are none
 *   [604] float  min_abs_nonzero   over finite non-zero values; +inf when there are none
 *   [608] float  max_val           over finite values (zeros included); -inf when there are none
 *   [612] float  min_val           over finite values; +inf when there are none
 * max_val / min_val order the bit patterns (-0 below +0), so every field but sum / sum_sq is independent of the summation order, and
 * the launch order is fixed: the same input gives a byte-identical record every time.
 *
 * Launches: workgroups of TT_STATS_BLOCK lanes walk the tensor grid-strided (at most TT_STATS_MAX_GRID of them; 16-byte loads when
 * x, ldx and cols allow -- a contiguous tensor, ldx == cols, is walked as one flat run with a scalar tail -- else one element per
 * lane and trip), each writes its partial record to ws, and a second one-workgroup launch merges the partials into rec in a fixed
 * order (eight runs of consecutive partials, each run in index order, then the runs in order).  A tensor that one workgroup covers takes one launch and no workspace.  No atomics on global memory, no flags or counters
 * between workgroups.  No allocation and no synchronisation: capturable.
 * accumulate != 0 merges into the record already at rec (counts, histogram and sums add, extrema combine) -- a replayed graph
 * accumulates over steps; accumulate == 0 overwrites it.  rows == 0 or cols == 0: the empty record (accumulate: rec unchanged, no
 * launch at all).
 * ws: tt_tensor_stats_ws_bytes(rows, cols, dtype) bytes (0 for a one-workgroup tensor: ws may then be NULL), 8-byte aligned.
 * tt_tensor_stats_launch reports (TT_STATS_MAX_GRID, TT_STATS_BLOCK, elements per 16-byte load of `dtype`) for tests and tools.
 * TT_EINVAL: null x (non-empty tensor) / thr / rec; rows or cols < 0; ldx < cols with more than one row; a bad dtype; a threshold
 * that is negative or NaN; x off its element size, rec or ws off an 8-byte boundary; a workspace that is missing or too small. */
enum { TT_FP8_E4M3 = 3 };               /* tt_tensor_stats only: the other entry points name fp8 operands by their own switches */
#define TT_STATS_BLOCK 256
#define TT_STATS_MAX_GRID 1024
typedef struct TtTensorStats {
  uint64_t count, n_nan, n_pinf, n_ninf, n_zero;
  uint64_t n_ge[4];
  uint64_t hist[64];
  double sum, sum_sq;
  float max_abs, min_abs_nonzero, max_val, min_val;
} TtTensorStats;
int64_t tt_tensor_stats_ws_bytes(int64_t rows, int32_t cols, int32_t dtype);
int tt_tensor_stats_launch(int32_t dtype, int32_t* max_grid /* host */, int32_t* block /* host */, int32_t* elems_per_load /* host */);
int tt_tensor_stats(const void* x, int64_t ldx, int64_t rows, int32_t cols, int32_t dtype, const float* thr /* host [4] */,
                    TtTensorStats* rec, void* ws, int64_t ws_bytes, int32_t accumulate, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * tt_frame_metrics: how far two videos are from each other, frame by frame -- the sums behind MSE / PSNR and SSIM (Wang, Bovik,
 * Sheikh, Simoncelli 2004, as skimage, torchmetrics and pytorch-msssim compute it) of frames a and b that are on the device
 * already, e.g. from tt_frames_out.  Additive: the ABI version is unchanged.
 *
 *   a, b   [n, h, w, ch] contiguous NHWC, 1 <= ch <= 4, both of `kind`: 1 uint8, 0 fp32 (tt_frames_out's codes); aligned to their
 *          element, nothing more: a pointer offset by whole frames is served like any other
 *   rec    n records on the DEVICE, one per frame, 8-byte aligned.  TtFrameMetricsRecord -- 104 bytes, no padding:
 *            [ 0] double sse[4]       per channel c:  sum over the frame of (a - b)^2
 *            [32] double ssim_sum[4]  per channel:  sum over the windows of ssim
 *            [64] double cs_sum[4]    per channel:  sum over the windows of cs
 *            [96] int64  count        windows per channel, (h - 10) (w - 10); 0 with TT_METRICS_SSE_ONLY
 *          SUMS, not means: the host divides.  Channels ch .. 3 hold 0.
 *   sse    uint8: integer differences, squares and sums; the record holds the exact integer (below 2^53 for any frame of fewer than
 *          2^37 pixels, so the fp64 is exact).  fp32: d = (double)a - (double)b, d d and the sums in fp64.
 *   window g[k] = exp(-(k - 5)^2 / 4.5) / S for k = 0 .. 10, S their sum in index order: the 11-tap Gaussian of sigma 1.5, normalised,
 *          separable, in fp64 (tt_frame_metrics_window copies the 11 doubles the kernel uses to the caller).
 *          G*x at window (y, x), "valid" windows only (0 <= y < h - 10, 0 <= x < w - 10), no padding:
 *            row[r][x] = g[0] v[r][x] + g[1] v[r][x + 1] + .. + g[10] v[r][x + 10]         (left to right, starting from the first product)
 *            (G*v)[y][x] = g[0] row[y][x] + .. + g[10] row[y + 10][x]                       (likewise)
 *          for v = a, b, a a, a b, b b (the products formed in fp64 per pixel).
 *   ssim   C1 = (0.01 L)^2, C2 = (0.03 L)^2, L = data_range (255 for uint8 frames, 1 for fp32 frames in [0, 1]: always passed)
 *            mu_a = G*a, mu_b = G*b;  maa = mu_a mu_a, mbb = mu_b mu_b, mab = mu_a mu_b
 *            s_aa = G*(a a) - maa,  s_bb = G*(b b) - mbb,  s_ab = G*(a b) - mab
 *            cs   = (2 s_ab + C2) / ((s_aa + s_bb) + C2)
 *            ssim = ((2 mab + C1) / ((maa + mbb) + C1)) cs
 *          ALL of it in fp64, every operation rounded on its own (no contraction): with fp32 moments the cancellation in
 *          G*(x x) - mu^2 costs up to 5.5e-4 per window on a bright flat region (x x reaches 65 025, C2 is 58.5).  Identical frames
 *          give cs == ssim == 1.0 in every window, hence ssim_sum == count exactly.
 *   flags  TT_METRICS_SSE_ONLY: sse only -- no window work, ssim_sum = cs_sum = 0, count = 0, and frames smaller than 11 x 11 are served.
 *
 * Launches: TWO.  One workgroup of TT_METRICS_BLOCK lanes per (frame, tile of TT_METRICS_TILE x TT_METRICS_TILE windows), all
 * channels of the tile: the tile's pixels with their 10-pixel halo of both operands go to LDS (16-byte loads along the contiguous
 * w ch axis wherever an aligned 16 bytes lies inside the tile's row, single elements at its ends), then per channel a horizontal and
 * a vertical pass in fp64.  A pixel's squared difference is counted by the tile that holds it among its first TT_METRICS_TILE rows and
 * columns (the last tile of an axis: to the frame's edge).  Each workgroup sums in a fixed shape and writes 12 doubles to ws; the
 * second launch (one workgroup per frame) adds the tiles' partial sums IN TILE ORDER.  No atomics, no flags between workgroups:
 * the same call on the same inputs gives the same bits every time, and a frame's record does not depend on the other frames of the
 * call.  Element indices are 64-bit.  No allocation, no synchronisation: capturable.
 * ws: tt_frame_metrics_ws_bytes(n, h, w, flags) bytes, 8-byte aligned (0 for arguments tt_frame_metrics refuses).
 * tt_frame_metrics_launch reports (TT_METRICS_TILE, TT_METRICS_BLOCK, elements per 16-byte load of `kind`) for tests and tools.
 * Refused before the first HIP call.  TT_EINVAL: null a / b / rec; n <= 0; h or w <= 0; ch outside 1 .. 4; an unknown kind; unknown
 * flag bits; h < 11 or w < 11 without TT_METRICS_SSE_ONLY; data_range <= 0 or not finite; a / b off their element size, rec or ws off
 * an 8-byte boundary; a workspace that is missing or too small.  TT_EUNSUPPORTED: more than 2^31 - 1 tiles in one call.
 *
 * tt_frames_pool2: one level of the MS-SSIM pyramid (Wang, Simoncelli, Bovik 2003), the 2 x 2 mean:
 *   src [n, h, w, ch] (kind 1 uint8 / 0 fp32) -> dst fp32 [n, h / 2, w / 2, ch],
 *   dst[f][y][x][c] = 0.25f * ((x00 + x01) + (x10 + x11)) in fp32, in that order (xij = src[f][2 y + i][2 x + j][c]).
 * For frames that began as uint8, four levels are exact: every value stays a multiple of 2^-8 below 2^8.  One launch.
 * TT_EINVAL: null src / dst; n, h or w <= 0; h or w odd; ch outside 1 .. 4; an unknown kind; fp32 src or dst off a 4-byte boundary. */
#define TT_METRICS_WIN 11
#define TT_METRICS_TILE 16
#define TT_METRICS_BLOCK 256
#define TT_METRICS_SSE_ONLY 1
typedef struct TtFrameMetricsRecord {
  double sse[4], ssim_sum[4], cs_sum[4];
  int64_t count;
} TtFrameMetricsRecord;
int tt_frame_metrics_window(double* g /* host [TT_METRICS_WIN] */);
int tt_frame_metrics_launch(int32_t kind, int32_t* tile /* host */, int32_t* block /* host */, int32_t* elems_per_load /* host */);
int64_t tt_frame_metrics_ws_bytes(int32_t n, int32_t h, int32_t w, int32_t flags);
int tt_frame_metrics(const void* a, const void* b, int32_t kind, int32_t n, int32_t h, int32_t w, int32_t ch, double data_range,
                     int32_t flags, TtFrameMetricsRecord* rec, void* ws, int64_t ws_bytes, tt_stream_t stream);
int tt_frames_pool2(const void* src, int32_t kind, int32_t n, int32_t h, int32_t w, int32_t ch, float* dst, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GIF export: a video's frames quantised to 256-colour palettes with the per-pixel work on the device (this_and_that_vdm_amd/export.py
 * drives it).  Two kernels (tt_color_hist, tt_palette_map) and two host routines (tt_palette_median_cut, tt_gif_lzw; plain C++, they
 * touch no device).  Integers only, everywhere: every call gives the same bits.  Additive: the ABI version is unchanged.
 *
 * TtColorBin -- 16 bytes: uint32 count, sum_r, sum_g, sum_b: how many pixels a bin (or a palette entry) holds and the sums of their
 * FULL 8-bit channel values.  A sum is at most 255 count, so all four fit while count <= TT_GIF_MAX_PIXELS = (2^32 - 1) / 255 =
 * 16 843 009 pixels per histogram (14 frames of 576 x 1024 are 8.3 M); more than that is refused, never wrapped.
 *
 * tt_color_hist: frames [n, h, w, 3] uint8 NHWC on the device -> nhist histograms of TT_GIF_BINS = 32 768 TtColorBin each on the
 * device, nhist == n (one per frame) or nhist == 1 (one over all frames).  A pixel (r, g, b) belongs to
 *   bin = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)
 * and adds (1, r, g, b) to it.  The call zeroes hist first (a memset on the stream), then ONE launch: a workgroup of TT_GIF_BLOCK lanes
 * walks a contiguous run of one histogram's pixels, 16 pixels (three aligned 16-byte loads) per lane and trip with single pixels at the
 * run's two ends, and adds into a PRIVATE table in LDS of TT_GIF_HIST_SLOTS slots {bin, count, sum_r, sum_g, sum_b}: a pixel's slot is a
 * hash of its bin, claimed by compare-and-swap on the slot's bin word; a pixel whose slot another bin holds adds to hist directly.  At
 * the end of its run the workgroup adds its occupied slots to hist.  All adds are integer atomics (LDS, then global): they commute, so
 * which pixels took which way changes no bit.  (All 32 768 bins private would take 512 KB of LDS against the CU's 160 KB; counts alone
 * 128 KB.  A natural frame fills a few hundred bins; a frame of ONE colour sends every pixel of a workgroup to one LDS word -- 64 adds
 * of one wave instruction serialise in the LDS, not in the L2 -- and the workgroup's whole run reaches hist as four global adds.)
 * TT_EINVAL: null frames / hist; n, h or w <= 0; ch != 3; nhist neither n nor 1; hist off a 16-byte boundary.  TT_EUNSUPPORTED: more
 * than TT_GIF_MAX_PIXELS pixels per histogram; more than 65 535 histograms.
 *
 * tt_palette_map: frames as above, palettes [npal, 256, 3] uint8 on the device (npal == n: frame f uses palette f; npal == 1: all
 * frames use the one), ncolors [npal] on the HOST, each 1 .. 256 -> indices [n, h, w] uint8 on the device,
 *   index = the k in 0 .. ncolors - 1 that minimises (r - R_k)^2 + (g - G_k)^2 + (b - B_k)^2, the LOWEST such k on a tie
 * (entries ncolors .. 255 are never read as candidates); sse [n] uint64 on the device, per frame the sum of that minimum over its
 * pixels; and, when stats is not NULL, stats [npal, 256] TtColorBin on the device: per palette and entry (count, sum_r, sum_g, sum_b) of
 * the pixels assigned to it (entries >= ncolors hold zeros) -- the input of a Lloyd step.  The call zeroes sse and stats, then ONE launch
 * for all frames: grid (runs of a frame, n); every lane keeps 4 pixels in registers and walks the palette ONCE for them; the palette
 * is the same for every lane of a workgroup, so its dwords are read through uniform (scalar) loads, four entries per three dwords, and
 * unpacked on the scalar unit; ncolors travel as kernel arguments (hence at most TT_GIF_MAX_PALETTES palettes).  Per-entry sums go to a
 * 4 KB table in LDS and from there to stats, the squared error through a wave and workgroup reduction to one global add per workgroup;
 * integer atomics throughout.
 * TT_EINVAL: null frames / palettes / ncolors / indices / sse; n, h or w <= 0; ch != 3; npal neither n nor 1; an ncolors outside
 * 1 .. 256; palettes off a 4-byte, sse off an 8-byte, stats off a 16-byte boundary.  TT_EUNSUPPORTED: more than TT_GIF_MAX_PALETTES
 * palettes, more than 65 535 frames, or (with stats) more than TT_GIF_MAX_PIXELS pixels per palette.
 * Both are refused before the first HIP call; no allocation, no synchronisation.
 *
 * tt_palette_median_cut (host): one histogram (TT_GIF_BINS TtColorBin, host memory) -> at most `colors` (1 .. 256) palette entries.
 * A bin's coordinates are (r5, g5, b5) = (bin >> 10, (bin >> 5) & 31, bin & 31); a bin is occupied when its count is not 0.
 *   A box is a set of occupied bins; its count is the sum of theirs.  Box 0 holds all occupied bins.
 *   While there are fewer than `colors` boxes and some box holds more than one occupied bin:
 *     1. take the box with the largest count among those that hold more than one bin; on a tie the one created first (lowest index);
 *     2. the axis: the largest extent, max - min coordinate over the box's bins; ties go to R, then G, then B;
 *     3. t = the smallest coordinate on that axis for which 2 * (count of the box's pixels at coordinates <= t) >= the box's count;
 *     4. if t is the box's maximum coordinate on the axis, t = the next lower coordinate that one of the box's bins has;
 *     5. bins with coordinate <= t stay in the box (it keeps its index), the others become a new box with the next index.
 *   Entry k, per channel: (2 sum + count) / (2 count), integer division, over box k -- the mean of the box's PIXELS rounded half up,
 *   not a bin centre.  Hence a frame whose colours fall one per bin into at most `colors` bins is reproduced exactly.
 * palette: host [256][3], entries ncolors_out .. 255 are written as zeros.  bin_box (may be NULL): host [TT_GIF_BINS], the box index
 * of every occupied bin, -1 for the others.  TT_EINVAL: a null pointer, colors outside 1 .. 256, a histogram without a pixel.
 *
 * tt_gif_lzw (host): indices [npix] (each below 2^min_code_size; min_code_size 2 .. 8) -> the image data of one GIF frame (GIF89a,
 * appendix F): the min-code-size byte, data sub-blocks of at most 255 bytes, the block terminator 0.  Codes are packed from the least
 * significant bit.  The stream starts with a clear code; the width starts at min_code_size + 1 and grows to 12 as the table does (one
 * bit more from the code after the entry 2^width was made); when the table is full (entry 4095 made) the next code is followed by a
 * clear code and the table and width start over; the end-of-information code closes the stream.  out holds cap bytes:
 * tt_gif_lzw_bound is enough for any input of npix indices (12 bits per index and per clear code, at most one clear code per 2048
 * indices, plus the sub-block framing); nbytes_out receives the bytes written.  TT_EINVAL: a null pointer, npix <= 0, min_code_size
 * outside 2 .. 8, an index that does not fit it, cap too small (nothing beyond out[cap - 1] is ever written). */
#define TT_GIF_BINS 32768
#define TT_GIF_MAX_PIXELS 16843009
#define TT_GIF_MAX_PALETTES 1024
#define TT_GIF_BLOCK 256
#define TT_GIF_HIST_SLOTS 2048
typedef struct TtColorBin {
  uint32_t count, sum_r, sum_g, sum_b;
} TtColorBin;
int tt_color_hist(const void* frames, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t nhist, TtColorBin* hist, tt_stream_t stream);
int tt_palette_map(const void* frames, int32_t n, int32_t h, int32_t w, int32_t ch, const void* palettes, int32_t npal,
                   const int32_t* ncolors /* host [npal] */, uint8_t* indices, uint64_t* sse, TtColorBin* stats, tt_stream_t stream);
int tt_palette_median_cut(const TtColorBin* hist /* host */, int32_t colors, uint8_t* palette /* host [256][3] */,
                          int32_t* ncolors_out /* host */, int32_t* bin_box /* host [TT_GIF_BINS] or NULL */);
int64_t tt_gif_lzw_bound(int64_t npix);
int tt_gif_lzw(const uint8_t* indices /* host */, int64_t npix, int32_t min_code_size, uint8_t* out /* host */, int64_t cap,
               int64_t* nbytes_out /* host */);

/* ------------------------------------------------------------------------------------------------
 * GIF LZW on the device: tt_gif_lzw_frames writes the image data of every frame of a video from index maps that are already on the
 * device (tt_palette_map's), coding each frame in independent SEGMENTS.  LZW is sequential only within one dictionary; a clear code
 * starts a new one, and a stream may hold as many clear codes as it likes -- so a frame cut into segments, each with its own
 * dictionary, is ordinary GIF, and the segments are coded side by side.  Opt-in (this_and_that_vdm_amd/export.py: lzw="device");
 * tt_gif_lzw is untouched.  Integers only: the same bytes every call.  Additive: the ABI version is unchanged.
 *
 * The format:
 * 1. A frame's npix indices, in raster order, are cut into segments of `segment` pixels; the last may be shorter.  `segment` is 1 ..
 *    TT_LZW_SEGMENT_MAX; segment = 0 selects TT_LZW_SEGMENT, the built default.
 * 2. The frame's code stream is: clear, codes of segment 0, clear, codes of segment 1, ..., clear, codes of the last segment,
 *    end-of-information.
 * 3. The codes of a segment are exactly what tt_gif_lzw writes for those pixels alone, between its leading clear code and its
 *    end-of-information code: table and width start fresh (width min_code_size + 1, next entry 2^min_code_size + 2); matching is
 *    greedy longest-match; when entry 4095 has been made, the next code is followed by a clear code and the table starts over.
 * 4. The clear (or end-of-information) code that closes a segment is written at the width in force after the segment's last code --
 *    one more when that code made entry 2^width, the rule tt_gif_lzw applies to its end-of-information code.  (A code's width is thus
 *    a function of its place r behind the last clear code alone: min(12, bit length of 2^min_code_size + 1 + r).)
 * 5. Codes are packed from the least significant bit; the last byte is padded with zeros.
 * 6. The image data of a frame: the min-code-size byte; sub-blocks of 255 bytes, then one shorter sub-block if bytes remain (no empty
 *    sub-block when the data is a multiple of 255); the terminator 0.  Data byte k lies at 2 + k + k / 255.
 * 7. The stream is a function of (indices, min_code_size, segment) only; the hash function and probing are free, because greedy LZW
 *    has one answer.
 * 8. Hence with segment >= npix the image data equals tt_gif_lzw's byte for byte.
 *
 * tt_gif_lzw_frames_bound(npix, segment): a frame's stride in out, a multiple of 16, enough for any indices (12 bits per index, per
 * clear code of a full table, per closing code of a segment and for the first clear code, plus the framing); 0 for arguments the
 * entry point refuses.  tt_gif_lzw_frames_ws_bytes(n, npix, segment): the workspace (per segment its code count, its bit offset and
 * its codes as uint16); 0 likewise.
 *
 * tt_gif_lzw_frames: indices [n][npix] uint8 and min_code_size [nmcs] int32 on the device (nmcs == 1: one value for all frames;
 * nmcs == n: one per frame) -> frame f's finished image data at out + f * bound, its byte count in lengths[f], and status[f]: 0, or
 * TT_GIF_LZW_STATUS_INDEX (an index does not fit the frame's min_code_size) | TT_GIF_LZW_STATUS_MCS (a min_code_size outside 2 .. 8).
 * The kernels clamp both, so whatever the data hold nothing is written outside out[f * bound, (f + 1) * bound) and ws; a frame with a
 * non-zero status has a meaningless stream, its neighbours are unaffected.  Bytes of out behind a frame's length are not written.
 * Four launches on the stream and a memset of status; no workgroup waits on another, no host readback in between, and every loop's
 * trip count is known before it starts:
 *   codes   -- grid (segments, n), one wave per segment: all lanes stage the segment's indices in LDS (4 KiB at a time) and clear the
 *              string table (8192 slots of key << 12 | code, 32 KiB, never more than half full); the walk through the pixels is one
 *              dependent chain of LDS probes, run by every lane alike on wave-uniform (scalar) values; lane 0 stores the 16-bit codes
 *              and the segment's code count; at a full table every lane clears;
 *   offsets -- grid (n): a segment's bit length is a closed form of its code count (rule 4); an exclusive scan over the frame's
 *              segments gives their bit offsets, the frame's data bytes and lengths[f];
 *   fill    -- the frame's bytes 0 .. length - 1 zeroed, with the min-code-size byte, the sub-blocks' length bytes and the terminator;
 *   pack    -- per tile of 2048 codes: every code ORed into LDS at its bit offset (a closed form of its ordinal), the tile's bytes
 *              ORed into the frame at their framed places (atomic OR of aligned words: neighbouring tiles share bytes at their ends).
 * TT_EINVAL: a null pointer; n or npix <= 0; nmcs neither 1 nor n; segment < 0 or above TT_LZW_SEGMENT_MAX; out or ws off a 16-byte,
 * lengths, status or min_code_size off a 4-byte boundary; cap < n * bound ("cap too small"); ws_bytes below
 * tt_gif_lzw_frames_ws_bytes ("ws too small").  TT_EUNSUPPORTED: more than 65 535 frames; a frame's stride of 2^29 bytes or more (bit
 * offsets inside a frame are 32-bit); 2^31 codes or more in the workspace (code offsets are 32-bit).  All are refused before the
 * first HIP call; no allocation, no synchronisation. */
#define TT_LZW_SEGMENT 16384
#define TT_LZW_SEGMENT_MAX 65536
#define TT_GIF_LZW_STATUS_INDEX 1
#define TT_GIF_LZW_STATUS_MCS 2
int64_t tt_gif_lzw_frames_bound(int64_t npix, int32_t segment);
int64_t tt_gif_lzw_frames_ws_bytes(int32_t n, int64_t npix, int32_t segment);
int tt_gif_lzw_frames(const uint8_t* indices /* device [n][npix] */, int32_t n, int64_t npix,
                      const int32_t* min_code_size /* device [nmcs], nmcs 1 or n */, int32_t nmcs, int32_t segment, uint8_t* out, int64_t cap,
                      uint32_t* lengths /* device [n] */, uint32_t* status /* device [n] */, void* ws, int64_t ws_bytes, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PNG export: frames written as standard 8-bit PNG files whose row filter, tokens and Huffman-coded bits are made on the device
 * (this_and_that_vdm_amd/export.py drives it).  Three kernels (tt_png_filter, tt_png_tokens, tt_png_emit) and three host routines
 * (tt_png_code_lengths, tt_png_block_header, tt_png_plan; plain C++, they touch no device).  Integers only: the same frames give the
 * same bytes every time.  Additive: the ABI version is unchanged.  The filtered bytes never leave the device; the host sees 1152 bytes
 * of counts per stripe and the finished compressed stream.
 *
 * 1. Filter -- tt_png_filter: frames [n, h, w, ch] uint8 NHWC on the device, ch 1 .. 4 (PNG colour types 0, 4, 2, 6; bpp = ch) ->
 *    per frame the FILTERED STREAM of tt_png_stream_bytes = h (1 + w ch) bytes: every row is its filter-type byte followed by its
 *    w ch filtered bytes.  With x the byte, a the byte bpp to its left, b the byte above, c the byte above a (zeros left of the first
 *    pixel and above the first row), all mod 256:  type 0: x;  1: x - a;  2: x - b;  3: x - ((a + b) >> 1);  4: x - paeth(a, b, c),
 *    paeth: p = a + b - c, pa = |p - a|, pb = |p - b|, pc = |p - c|; a if pa <= pb and pa <= pc, else b if pb <= pc, else c.
 *    filter = 0 .. 4: that type on every row.  filter = 5 (TT_PNG_ADAPTIVE): per row the type with the smallest sum over the row's
 *    filtered bytes v of (v < 128 ? v : 256 - v); the LOWEST type on a tie.  A row needs the raw row above it only: one workgroup of
 *    TT_PNG_FILTER_BLOCK lanes per row, ONE launch for all frames.  Frame f's stream starts at byte f tt_png_frame_stride (the stream
 *    bytes rounded up to 16) of `filtered`; the padding is never read as data.
 *    TT_EINVAL: null frames / filtered; n, h or w <= 0; ch outside 1 .. 4; filter outside 0 .. 5; filtered off a 16-byte boundary.
 *    TT_EUNSUPPORTED: a stream of 2^31 bytes or more; more rows than one grid covers (n h > 2^31 - 1).
 *
 * 2. Stripes: a frame's filtered stream is cut into stripes of TT_PNG_STRIPE = 32 768 bytes (the last may be shorter), by bytes and
 *    not by rows; tt_png_stripes = ceil(stream bytes / TT_PNG_STRIPE) per frame.  No token crosses a stripe boundary, and every
 *    stripe is one DEFLATE block with its own codes that starts and ends on a byte, so stripes are coded independently.
 *
 * 3. Tokens -- tt_png_tokens (zlib's Z_RLE idea as a closed rule): inside a stripe, a maximal run of L equal bytes becomes one
 *    literal, then (L - 1) / 258 matches of (length 258, distance 1); with r = (L - 1) mod 258, one match (length r, distance 1)
 *    follows if r >= 3, else r literals.  No other match is made.  One workgroup of TT_PNG_BLOCK lanes per stripe, every lane holding
 *    32 consecutive bytes in registers; where the run through a lane's first byte starts and where the run through its last byte ends
 *    come from two workgroup scans (a running maximum of run starts forward, a running minimum backward); with them every byte
 *    position knows its run and so whether a token starts at it.  Per stripe one RECORD of TT_PNG_RECORD_WORDS = 288 uint32 (1152
 *    bytes): the counts of the 286 literal/length symbols (symbol 256, end of block, counts 1; length m is symbol 254 + m for m <= 10,
 *    285 for 258, else 265 + 4 (k - 1) + (((m - 3) >> k) & 3) with k = floor(log2(m - 3)) - 2 extra bits holding (m - 3) mod 2^k), then
 *    the stripe's Adler-32 pair s1, s2 mod 65 521 started from (1, 0): s1 = 1 + sum b_i, s2 = len + sum (len - i) b_i.  A lane's
 *    32 terms are below 2^29; it reduces mod 65 521 before the workgroup sum (1024 x 65 521), so nothing wraps.  ONE launch for all frames.
 *    TT_EINVAL: null filtered / records; n, h or w <= 0; ch outside 1 .. 4; filtered or records off a 16-byte boundary.
 *
 * 4. Code lengths -- tt_png_code_lengths (host): counts[nsym] -> lengths[nsym] (0 for a count of 0) that minimise sum count length
 *    subject to length <= limit and Kraft sum <= 1 -- package-merge.  Leaves are the used symbols in ascending (count, symbol).
 *    List 1 is the leaves; list l + 1 is the leaves merged with the packages of list l (items 2k and 2k + 1 added, an odd last item
 *    dropped), by ascending weight, a LEAF BEFORE A PACKAGE of equal weight, cut to 2 u - 2 items (u used symbols).  The first
 *    2 u - 2 items of list `limit` are taken; taking a package takes its two items of the list before.  A symbol's length is the
 *    number of lists in which its leaf is taken (in each list the taken leaves are a prefix of the leaf order, so of two symbols with
 *    equal counts the lower one never gets the shorter code).  One used symbol gets length 1; with two or more the Kraft sum is
 *    exactly 1.  limit is 15 for the literal/length code, 7 for the code-length code.  The distance code is not computed: it is
 *    always symbol 0 alone with length 1 (RFC 1951 3.2.7: "one distance code of one bit"), every match's distance is the bit 0.
 *    Codes are canonical (RFC 1951 3.2.2) and go into the stream from their most significant bit.
 *    TT_EINVAL: null pointer; nsym outside 1 .. 286; limit outside 1 .. 15 or 2^limit below the used symbols; no used symbol.
 *
 * 5. Block header -- tt_png_block_header (host): counts[286] and lengths[286] -> the dynamic-block header of the stripe, LSB first:
 *    BFINAL 0, BTYPE 2, HLIT = max(257, last used symbol + 1) - 257, HDIST - 1 = 0, HCLEN - 4, the code-length code's lengths (3 bits
 *    each, in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, up to the last used one, at least 4), then the HLIT + 257
 *    literal/length lengths followed by the one distance length 1, as ONE sequence coded greedily from the left: a maximal run of R
 *    equal values v.  v = 0: while R >= 11, symbol 18 with min(R, 138) (7 extra bits: that - 11); then symbol 17 with R (3 extra bits:
 *    R - 3) if R >= 3, else R symbols 0.  v > 0: symbol v once; then while R >= 3 of what is left, symbol 16 with min(R, 6) (2 extra
 *    bits: that - 3); then what is left as symbols v.  The code-length code's lengths are tt_png_code_lengths(limit 7) of those
 *    symbols' counts.  header[0] receives the header's bits, header[1 ..] the bits packed from the least significant bit of each
 *    uint32 (zeros behind the last); the header is at most 17 + 57 + 287 x 7 = 2083 bits, TT_PNG_HEADER_WORDS = 72 words hold it.
 *    stripe_bits_out receives the exact size of the stripe's block: header + sum count length + sum count (extra bits of the length
 *    symbol) + matches (one distance bit each) -- the end-of-block code is in the counts -- + the 3 header bits of the empty stored
 *    block that follows.  The stripe takes ceil(stripe_bits / 8) + 4 bytes.
 *    TT_EINVAL: null pointer; cap_words < TT_PNG_HEADER_WORDS ("cap too small"); a length above 15; a used symbol (or symbol 256)
 *    without a length; lengths whose Kraft sum exceeds 1.
 *    tt_png_plan (host) does 4 and 5 for every record of a call: records [nstripes][288] as tt_png_tokens wrote them -> tables
 *    [nstripes][TT_PNG_TABLE_WORDS = 288] (entry s < 286: the canonical code of symbol s with its bits REVERSED, so that it is ORed in
 *    LSB first, | length << 16; words 286 / 287: the low / high half of the stripe's byte offset in the output), headers
 *    [nstripes][TT_PNG_HEADER_WORDS], and the total bytes of all stripes, each starting where the one before ends.
 *
 * 6. Emit -- tt_png_emit: per stripe, at its byte offset: the header bits; every token's code in order -- a literal's code; a match's
 *    length code, its extra bits, then the distance bit 0: at most 15 + 5 + 1 bits --; the end-of-block code; an empty stored block
 *    (bits 000, zeros up to the byte, 00 00 FF FF), so that the next stripe starts on a byte.  One workgroup per stripe; a token's
 *    bit position is the header's bits plus a workgroup scan of the lanes' token bits.  Bits are assembled in LDS in chunks of
 *    TT_PNG_CHUNK = 16 384 bytes laid over the OUTPUT's 16-byte grid: a lane shifts its tokens into a 64-bit accumulator and ORs every
 *    finished 32-bit word in (integer atomic OR: its first and last word are shared with its neighbours); a chunk then leaves through
 *    16-byte vector stores, except the 16-byte units a stripe shares with its neighbours, whose bytes of this stripe are written one
 *    by one.  No byte at or beyond out_bytes is written whatever the tables hold.
 *    TT_EINVAL: null filtered / tables / headers / out; n, h or w <= 0; ch outside 1 .. 4; filtered, tables, headers or out off a
 *    16-byte boundary; out_bytes <= 0; cap < out_bytes ("cap too small").
 *    All three kernels are refused before the first HIP call; no allocation, no synchronisation.
 *
 * 7. Stream and file (export.py): a frame's zlib stream is 78 01, its stripes, 01 00 00 FF FF (the final, empty stored block), then
 *    the Adler-32 of the whole filtered stream big-endian, combined from the stripes' pairs as zlib's adler32_combine does.
 *    Worst case: no code is longer than a flat one of 8 and 9 bits, so a stripe takes at most 9/8 of its bytes + 272; on uniform noise
 *    the stream is about 1 % above the raw bytes (there is no stored-block fallback). */
#define TT_PNG_STRIPE 32768
#define TT_PNG_BLOCK 1024
#define TT_PNG_FILTER_BLOCK 256
#define TT_PNG_ADAPTIVE 5
#define TT_PNG_SYMS 286
#define TT_PNG_RECORD_WORDS 288
#define TT_PNG_TABLE_WORDS 288
#define TT_PNG_HEADER_WORDS 72
#define TT_PNG_CHUNK 16384
int64_t tt_png_stream_bytes(int32_t h, int32_t w, int32_t ch);     /* h (1 + w ch); 0 for arguments tt_png_filter refuses */
int64_t tt_png_frame_stride(int32_t h, int32_t w, int32_t ch);     /* ... rounded up to 16 */
int64_t tt_png_stripes(int32_t h, int32_t w, int32_t ch);          /* stripes per frame */
int tt_png_filter(const void* frames, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t filter, uint8_t* filtered, tt_stream_t stream);
int tt_png_tokens(const uint8_t* filtered, int32_t n, int32_t h, int32_t w, int32_t ch, uint32_t* records, tt_stream_t stream);
int tt_png_emit(const uint8_t* filtered, int32_t n, int32_t h, int32_t w, int32_t ch, const uint32_t* tables, const uint32_t* headers,
                uint8_t* out, int64_t out_bytes, int64_t cap, tt_stream_t stream);
int tt_png_code_lengths(const uint32_t* counts /* host */, int32_t nsym, int32_t limit, uint8_t* lengths /* host */);
int tt_png_block_header(const uint32_t* counts /* host [286] */, const uint8_t* lengths /* host [286] */,
                        uint32_t* header /* host [cap_words] */, int32_t cap_words, int64_t* stripe_bits_out /* host */);
int tt_png_plan(const uint32_t* records /* host */, int64_t nstripes, uint32_t* tables /* host */, uint32_t* headers /* host */,
                int64_t* total_bytes_out /* host */);

/* ------------------------------------------------------------------------------------------------
 * JPEG export: frames written as baseline JPEG files (and as a Motion-JPEG AVI) whose colour conversion, chroma downsampling, DCT,
 * quantiser, Huffman-coded bits and byte stuffing are made on the device (this_and_that_vdm_amd/export.py drives it).  Two device
 * entry points (tt_jpeg_coeffs, tt_jpeg_scan) and three host routines (tt_jpeg_quant_tables, tt_jpeg_standard_table,
 * tt_jpeg_optimized_table; plain C++, they touch no device).  Baseline JPEG as libjpeg writes it is integers from end to end: the same
 * frames give the same bytes every time, and with the standard tables the scan equals libjpeg's ("islow" DCT) byte for byte.
 * Additive: the ABI version is unchanged.  Only the finished scans and their lengths (and, for optimized tables, 4 KiB of counts per
 * frame) reach the host.  Restart intervals are rule 6a.  Not here: progressive and arithmetic coding, 4:2:2, EXIF / ICC, CMYK, 12-bit
 * samples, trellis quantisation.
 *
 * Input: frames [n, h, w, ch] uint8 NHWC on the device, ch 1 (grey) or 3 (RGB).  subsampling: TT_JPEG_444 (0) or TT_JPEG_420 (2);
 * a grey frame has one component and ignores it.
 *
 * 1. Quantiser tables -- tt_jpeg_quant_tables (host): the Annex K luminance and chrominance tables scaled as jpeg_set_quality does:
 *    s = 5000 / quality (integer division) for quality < 50, else 200 - 2 quality; every entry is clamp((base s + 50) / 100, 1, 255).
 *    tables receives [2][64] bytes in natural (row-major) order.  TT_EINVAL: null tables; quality outside 1 .. 100.
 * 2. Colour (16-bit fixed point, arithmetic shifts; grey input is Y as it stands):
 *    Y = (19595 R + 38470 G + 7471 B + 32768) >> 16;  Cb = (-11059 R - 21709 G + 32768 B + 128 65536 + 32767) >> 16;
 *    Cr = (32768 R - 27439 G - 5329 B + 128 65536 + 32767) >> 16.
 * 3. Geometry.  4:4:4 and grey: every component is padded to whole 8 x 8 blocks by repeating its last column and row; an MCU is one
 *    block of each component, MCUs left to right, top to bottom.  4:2:0: an MCU is 16 x 16 pixels; Y is padded by edge replication to
 *    ceil(h / 8) 8 x ceil(w / 8) 8; the full-resolution Cb / Cr planes are edge-replicated to 2 ceil(h / 2) rows and 16 x (chroma
 *    blocks per row) columns, every chroma sample is (a + b + c + d + bias) >> 2 over its 2 x 2 cell with bias 1 on even and 2 on odd
 *    output columns, and the DOWNSAMPLED plane is then edge-replicated downwards to whole blocks.  An MCU is Y top-left, top-right,
 *    bottom-left, bottom-right, Cb, Cr.  A Y block of an MCU beyond ceil(w / 8) block columns or ceil(h / 8) block rows is a dummy
 *    block: its AC coefficients are zero and its DC is the DC of the block coded just before it in that MCU; it is coded like any other.
 *    tt_jpeg_blocks: the blocks of one frame's scan, dummies included.
 * 4. Transform: samples minus 128 through the jfdctint ("islow") forward DCT in 32-bit integers -- rows first (PASS1_BITS = 2), then
 *    columns, CONST_BITS = 13, rounding right shifts, multipliers 2446 3196 4433 6270 7373 9633 12299 15137 16069 16819 20995 25172 --;
 *    the output is scaled by 8.
 * 5. Quantiser: with d the DCT output and Q = 8 x the table entry, the coefficient is sign(d) ((|d| + (Q >> 1)) / Q), integer
 *    division (the kernel divides; no reciprocal).
 *    tt_jpeg_coeffs does 2 - 5 in ONE launch for all frames: a workgroup takes one MCU row down and 256 pixels across, reads every
 *    pixel once, converts it (and sums the 4:2:0 cells) into LDS, then one lane per block transforms 8 x 8 samples held in registers
 *    and stores the block's 64 int16 in ZIG-ZAG order: coeffs [n][tt_jpeg_blocks][64], blocks in scan order.  With counts != NULL a
 *    second launch counts every frame's symbols (rule 6): counts [n][TT_JPEG_COUNT_WORDS = 4 x 256] uint32 -- DC luminance, AC
 *    luminance, DC chrominance, AC chrominance, indexed by symbol.
 *    TT_EINVAL: null frames / coeffs; n, h or w <= 0; ch not 1 or 3; quality outside 1 .. 100; subsampling not 0 or 2; coeffs or
 *    counts off a 16-byte boundary.  TT_EUNSUPPORTED: a frame of 2^31 bytes or more; a scan bound of 2^31 bytes or more; n > 65535.
 * 6. Entropy coding: baseline sequential Huffman, one interleaved scan, no restart markers (6a adds them).  DC: the difference to the previous
 *    block of the same component in scan order (0 before the first), as its size category (the bits of |diff|) and that many
 *    magnitude bits (diff, or diff - 1 when negative, low bits).  AC: over zig-zag 1 .. 63, symbol (run of zeros << 4 | size) with the
 *    magnitude bits; 0xF0 stands for 16 zeros; 0x00 (EOB) only when the block ends in zeros.  Codes go MSB first, a 0x00 follows
 *    every 0xFF byte, the last byte is filled with one-bits.
 * 6a. Restart intervals, as libjpeg writes them (restart_interval = Ri MCUs, 1 .. 65535; 0: none, rule 6 as it stands).  The scan is cut
 *    into ceil(MCUs / Ri) intervals of Ri MCUs (the last may be shorter).  (i) The DC predictor of every component is 0 at the first MCU
 *    of an interval.  (ii) Behind the last block of every interval but the frame's last the byte is filled with one-bits; a filled byte
 *    that comes out as 0xFF IS stuffed; then FF D0 + (k mod 8) follows for the k-th marker (k from 0), NOT stuffed.  (iii) No marker
 *    stands behind the last interval, also when the MCU count is a multiple of Ri: ceil(MCUs / Ri) - 1 markers; Ri >= MCUs writes none.
 *    (iv) The file carries FF DD 00 04 Ri directly before SOS (rule 8).  (v) The symbol counts of an optimized table are taken with the
 *    same predictor resets: tt_jpeg_counts_restart recounts tt_jpeg_coeffs' coefficients (counts zeroed, one launch).
 *    tt_jpeg_scan_restart is tt_jpeg_scan with the interval; tt_jpeg_scan IS its restart_interval = 0: the same kernels.  The offsets
 *    scan, still one workgroup per frame, then takes per interval the bits its pad and marker add (pad to a byte + 16) and scans those;
 *    the lane of an interval's last block writes pad and marker and sets the bit of the marker's FF byte in a per-frame bitmap of the
 *    unstuffed bytes (one more memset); the stuffing passes skip the bytes whose bit is set -- a marker is known by its POSITION, never
 *    by its value: a data FF followed by D0 .. D7 is legal in the unstuffed stream.  No host round trip with standard tables.
 *    tt_jpeg_scan_bound_restart: tt_jpeg_scan_bound plus, per marker, pad 1 + marker 2 bytes, the pad doubled when stuffed (4), taken as
 *    6 so that half the bound still holds the unstuffed stream; rounded up to 16; 0 for refused arguments; restart_interval 0 gives
 *    tt_jpeg_scan_bound.  It is the frame stride of out; ws: tt_jpeg_scan_restart_ws_bytes.  TT_EINVAL as tt_jpeg_scan, and
 *    restart_interval outside 0 .. 65535.
 * 7. Huffman tables.  A table is BITS[16] (codes per length), HUFFVAL (symbols by ascending code) and, for the device, 256 uint32:
 *    per symbol its canonical code (T.81 Annex C) | length << 16.  tt_jpeg_standard_table (host): `which` 0 .. 3 (DC luminance, AC
 *    luminance, DC chrominance, AC chrominance) -> the Annex K.3 table.  tt_jpeg_optimized_table (host): counts[256] -> the table of
 *    tt_png_code_lengths (limit 15) over 257 symbols -- entry 0 a reserved symbol of count 1, entries 1 .. 256 the counts --: first in
 *    the package-merge's leaf order, the reserved symbol gets a longest code, and, placed last among the codes of that length, the
 *    code of one-bits only, which therefore no real symbol has (T.81 Annex K.2); it is then dropped.  HUFFVAL is by (length, symbol).
 *    TT_EINVAL: null pointer; which outside 0 .. 3.
 *    tt_jpeg_scan: coeffs and tables [ntables][4][256] (ntables 1: one set for all frames; n: one per frame) -> every frame's finished,
 *    stuffed scan at byte f tt_jpeg_scan_bound of out, and its length in lengths[f] (device uint32); bytes at or beyond the length are
 *    not written.  Six launches and one memset for all frames, no host round trip: the bits of every block (one lane per block), an
 *    exclusive scan over each frame's blocks (one workgroup per frame), the bits ORed MSB first into the zeroed unstuffed stream (a
 *    lane's first and last 32-bit word are shared with its neighbours: integer atomic OR; the words between are stored), then per
 *    TT_JPEG_CHUNK = 4096 bytes the count of 0xFF bytes, a scan of those counts, and the scatter with a 0x00 behind every 0xFF.
 *    tt_jpeg_scan_bound: a block takes at most TT_JPEG_BLOCK_BITS = 64 x (16 + 11) bits, doubled for stuffing, plus the padded byte,
 *    rounded up to 16.  ws: tt_jpeg_scan_ws_bytes of device scratch.  Whatever the tables hold, nothing is written outside out and ws.
 *    TT_EINVAL: null coeffs / tables / out / lengths / ws; n, h or w <= 0; ch not 1 or 3; subsampling not 0 or 2; ntables not 1 or n;
 *    coeffs, tables, out or ws off a 16-byte boundary; cap < n tt_jpeg_scan_bound ("cap too small"); ws_bytes too small.
 *    TT_EUNSUPPORTED: as for tt_jpeg_coeffs.  Both entry points refuse before the first HIP call; no allocation, no synchronisation.
 * 8. File (export.py): SOI; APP0 JFIF 1.01, units 0, density 1 x 1; one DQT marker per table (8-bit, zig-zag order); SOF0 (sampling
 *    2 x 2 for Y in 4:2:0, else 1 x 1); one DHT marker per table; with a restart interval DRI (FF DD 00 04 Ri); SOS; the scan; EOI. */
#define TT_JPEG_444 0
#define TT_JPEG_420 2
#define TT_JPEG_TABLE_WORDS 256
#define TT_JPEG_COUNT_WORDS 1024
#define TT_JPEG_BLOCK_BITS 1728
#define TT_JPEG_CHUNK 4096
int64_t tt_jpeg_blocks(int32_t h, int32_t w, int32_t ch, int32_t subsampling);          /* 0 for arguments tt_jpeg_coeffs refuses */
int64_t tt_jpeg_scan_bound(int32_t h, int32_t w, int32_t ch, int32_t subsampling);      /* a frame's stride in tt_jpeg_scan's out */
int64_t tt_jpeg_scan_ws_bytes(int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling);
int tt_jpeg_quant_tables(int32_t quality, uint8_t* tables /* host [2][64] */);
int tt_jpeg_standard_table(int32_t which, uint8_t* bits /* host [16] */, uint8_t* huffval /* host [256] */, int32_t* nvals /* host */,
                           uint32_t* codes /* host [256] */);
int tt_jpeg_optimized_table(const uint32_t* counts /* host [256] */, uint8_t* bits /* host [16] */, uint8_t* huffval /* host [256] */,
                            int32_t* nvals /* host */, uint32_t* codes /* host [256] */);
int tt_jpeg_coeffs(const void* frames, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t quality, int32_t subsampling, int16_t* coeffs,
                   uint32_t* counts /* or NULL */, tt_stream_t stream);
int tt_jpeg_scan(const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, const uint32_t* tables,
                 int32_t ntables, uint8_t* out, int64_t cap, uint32_t* lengths, void* ws, int64_t ws_bytes, tt_stream_t stream);
/* rule 6a: restart intervals (additive; restart_interval 0 is the entry points above) */
int64_t tt_jpeg_scan_bound_restart(int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t restart_interval);
int64_t tt_jpeg_scan_restart_ws_bytes(int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t restart_interval);
int tt_jpeg_counts_restart(const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t restart_interval,
                           uint32_t* counts, tt_stream_t stream);
int tt_jpeg_scan_restart(const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, int32_t restart_interval,
                         const uint32_t* tables, int32_t ntables, uint8_t* out, int64_t cap, uint32_t* lengths, void* ws, int64_t ws_bytes,
                         tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * JPEG import: baseline JPEG files decoded on the device to uint8 [n, h, w, ch] NHWC frames, byte for byte what libjpeg ("islow"
 * inverse DCT, fancy upsampling; Pillow's decoder) gives (this_and_that_vdm_amd/ingest.py drives it).  Only the compressed bytes cross
 * to the device.  Two host routines (tt_jpeg_parse, tt_jpeg_decode_table; plain C++, they touch no device), two device entry points
 * (tt_jpeg_entropy, tt_jpeg_pixels) and two size queries.  Integers from end to end: equality is the bound.  Additive: the ABI version
 * is unchanged.  Accepted: SOF0, 8-bit samples, one interleaved scan, one component (any sampling factor, taken as 1 x 1) or three
 * (YCbCr, sampling 1x1 / 1x1 / 1x1 or 2x2 / 1x1 / 1x1), 8-bit DQT, up to two DC and two AC Huffman tables, any component -> table map;
 * APPn and COM segments are skipped; restart intervals through tt_jpeg_parse_spans / tt_jpeg_entropy_spans (rules 1a, 4a);
 * progressive (SOF2) files through tt_jpeg_parse_progressive / tt_jpeg_entropy_progressive (rules 1b, 4b, behind the prototypes).  Not here:
 * arithmetic and 12-bit files, several scans in a baseline file, 4:2:2, CMYK / Adobe files, EXIF orientation (not applied).  Coefficients whose inverse DCT leaves 0 .. 255 clamp to 0 / 255; libjpeg's range-limit
 * table wraps there, so such crafted files are not held to it.
 *
 * 1. Parse -- tt_jpeg_parse (host): one file -> TtJpegHeader: the geometry, the subsampling, the byte range of the entropy-coded
 *    segment (behind the SOS header, before EOI), per component its quantiser table in natural (row-major) order and its DC / AC table
 *    index (0 or 1), and BITS / HUFFVAL of the tables DC 0, AC 0, DC 1, AC 1 (zeros for a table the file neither defines nor uses).
 *    TT_EINVAL: null pointer; size <= 0; no SOI; a segment or the file ends early ("ends before"); no EOI behind the scan.
 *    TT_EUNSUPPORTED, each by name: SOF1 / SOF2 and the other frame types ("progressive", "arithmetic", "extended sequential");
 *    12-bit samples; a non-zero DRI ("restart"); a second SOS ("several scans"); sampling other than the above ("sampling"); 16-bit
 *    DQT; four components or an Adobe APP14 segment; a table a component names but no DQT / DHT defines ("missing"); a Huffman table
 *    index above 1; a scan that does not hold every component in order or has Ss / Se / Ah / Al other than 0 / 63 / 0 / 0.
 * 1a. Parse with restart intervals -- tt_jpeg_parse_spans (host): accepts what tt_jpeg_parse accepts, plus DRI segments (the last one
 *    counts) and the RSTn markers inside the scan; tt_jpeg_parse itself keeps refusing both.  -> the header (scan_offset / scan_bytes:
 *    the whole entropy-coded segment, markers included), *restart_interval = Ri (0: none) and the scan's SPANS: per interval its byte
 *    offset in the file and its stuffed length, markers excluded; *nspans = markers + 1.  span_offsets / span_lengths NULL (both): only
 *    the count is taken; else span_cap >= *nspans entries are filled.  A file without DRI (or with DRI 0) gives ONE span, equal to
 *    tt_jpeg_parse's scan range.  Rule 1's refusals come with rule 1's texts, "tt_jpeg_parse: ..." included.  TT_EINVAL, each by name: a marker RSTm where RST(k mod 8) is due for the k-th ("is due"); a marker
 *    count other than ceil(MCUs / Ri) - 1 ("restart markers where"); a marker in a file with no DRI segment or with DRI 0 ("in a file");
 *    two DRI segments that disagree ("disagree"); span_cap too small; null restart_interval / nspans.
 * 2. Decode tables -- tt_jpeg_decode_table (host): BITS / HUFFVAL -> TT_JPEG_DECODE_WORDS = 256 uint32 the kernel reads: words 0 ..
 *    127: 256 uint16 indexed by the next 8 bits, length << 8 | symbol for a code of at most 8 bits, else 0; words 128 + l, l = 1 .. 16:
 *    the largest code of length l as int32, -1 for none (T.81 F.2.2.3 MAXCODE); words 145 + l: (index into HUFFVAL of the first code of
 *    length l) - (that code) as int32; words 192 .. 255: HUFFVAL, 256 bytes.  The kernel masks every index it forms with 255: whatever
 *    the words hold, nothing outside them is read.  TT_EINVAL: null pointer; a BITS that oversubscribes the code space; more than 256
 *    codes.  A frame's table set is TT_JPEG_DECODE_SET_WORDS = 4 x 256 + 4 words: the tables DC 0, AC 0, DC 1, AC 1, then one word whose
 *    bit 2 c is the DC and bit 2 c + 1 the AC table index of component c, then three zero words.
 * 3. Unstuff (device): per frame the 0x00 behind every 0xFF is dropped -- per TT_JPEG_CHUNK of the stuffed bytes the count of such
 *    pairs (a pair may straddle two chunks: the byte before a chunk is read with it), a scan of the counts, a gather.  An 0xFF followed
 *    by anything else, or ending the scan, sets TT_JPEG_STATUS_MARKER.
 * 4. Entropy decode (device), self-synchronising.  The plain stream of L bits is cut into subsequences of S = TT_JPEG_SUBSEQ_BITS bits,
 *    one lane each; 256 lanes, one workgroup, take a sequence of tt_jpeg_sequence_bits = 256 S bits.  A lane's state is (p, m, z): bit
 *    position, block within the MCU, zig-zag index.  f_i(entry) decodes the whole symbols (code and magnitude bits, T.81 F.2.2) that
 *    start in [max(entry p, i S), (i + 1) S) and gives the exit state and the blocks completed.  Pass 0: x_i = f_i((i S, 0, 0)), lane 0
 *    from the true state; pass k: x_i = f_i(x_{i-1}) where the entry changed.  After k passes the first k + 1 lanes are exact, so at
 *    most 255 further passes run, fewer when a pass changes nothing (a workgroup-uniform exit).  ONE workgroup walks the sequences of a
 *    frame in order, the true state carried from one to the next; frames run side by side.  No workgroup waits on another; every loop's
 *    bound is computed before it starts (sequences: ceil(L / 256 S); passes: 256; symbols of a lane: S); no host readback.  Outcomes
 *    under a speculative state: a bit pattern that is no code, with 16 or more bits left: one bit is skipped; a run that passes index
 *    63: the block ends; a symbol that would read beyond L (or no code within the bits left): the lane stops, and every lane behind it
 *    passes its entry state on.  A magnitude's size is the symbol's low 4 bits.  Lanes write nothing until the states are final; then
 *    an exclusive scan of the block counts gives every lane its first block, and a last pass from the true entries writes the DC
 *    differences and AC values into the zero-filled coeffs [n][tt_jpeg_blocks][64] int16, zig-zag, scan order, dummy blocks included --
 *    tt_jpeg_coeffs' layout -- guarded by block < tt_jpeg_blocks.  On that true path an invalid code, a DC size above 11 or a run
 *    beyond 63 sets TT_JPEG_STATUS_CODE.  A prefix sum per component over the DC differences (int32, stored as int16) makes them
 *    absolute.  TT_JPEG_STATUS_BLOCKS: blocks found != tt_jpeg_blocks.  TT_JPEG_STATUS_TAIL: what is left of the stream is not fewer than
 *    8 one-bits.  TT_JPEG_STATUS_SPAN: offset / length outside scans or above max_bytes (the frame is taken as empty).  A frame whose
 *    status is not 0 is corrupt or truncated; its coefficients mean nothing.
 *    tt_jpeg_entropy: scans (device bytes, scans_bytes of them), frame f's stuffed scan at offsets[f] with lengths[f] bytes (device
 *    int64 / uint32), max_bytes >= every length (it sizes grids and ws), tables [ntables][TT_JPEG_DECODE_SET_WORDS] (ntables 1 or n) ->
 *    coeffs and status [n] (device uint32).  ws: tt_jpeg_entropy_ws_bytes(n, max_bytes).  Two memsets and five launches.
 *    TT_EINVAL: null pointer; n, h, w, max_bytes or scans_bytes <= 0; ch not 1 or 3; subsampling not 0 or 2; ntables not 1 or n;
 *    tables, coeffs or ws off a 16-byte boundary; offsets off 8, lengths or status off 4; ws_bytes too small.  TT_EUNSUPPORTED: as
 *    tt_jpeg_coeffs; max_bytes of 2^28 or more.
 * 4a. Spans -- tt_jpeg_entropy_spans (device): rules 3 and 4 per SPAN instead of per frame.  Behind a restart marker the stream is at a
 *    byte, block 0 of an MCU begins and the DC predictors are zero: every span starts from the true state (0, 0, 0) and needs nobody
 *    else's result.  ONE workgroup per span: a clip of F frames with one interval per MCU row runs F x (MCU rows) workgroups where
 *    tt_jpeg_entropy runs F.  Span s is offsets[s] / lengths[s] of scans, belongs to frame span_frame[s] (int32) and holds
 *    span_blocks[s] blocks from block span_first[s] of that frame (uint32; all device arrays of nspans entries); max_bytes >= every
 *    span's length; ws: tt_jpeg_entropy_ws_bytes(nspans, max_bytes).  The span's values go to its blocks of the frame's coeffs, guarded
 *    by block < span_blocks[s]; the DC prefix sum restarts at every span.  status stays per FRAME [n]: a span whose block count is wrong
 *    sets its frame's TT_JPEG_STATUS_BLOCKS, one whose tail is wrong TT_JPEG_STATUS_TAIL, and so on; a span whose frame, first block or
 *    count lies outside its frame is taken as empty and sets TT_JPEG_STATUS_SPAN (its frame index is clamped into 0 .. n - 1).  Every
 *    property of rule 4 stays: no workgroup waits on another, every loop's bound is computed before it, lanes write nothing until the
 *    states are final, every index is masked or guarded.  tt_jpeg_entropy IS the case "one span per frame, whole": the same kernels.
 *    nspans <= TT_JPEG_MAX_SPANS = 65535 (a grid dimension): more is TT_EUNSUPPORTED ("spans"), refused before any HIP call.
 *    TT_EINVAL as tt_jpeg_entropy, and null or misaligned span arrays, nspans <= 0.
 * 5. Reconstruct -- tt_jpeg_pixels (device), one launch: per block coef x Q, then jidctint: columns first, then rows, 32-bit integers.
 *    Even part: z1 = (in2 + in6) 4433, tmp2 = z1 - in6 15137, tmp3 = z1 + in2 6270, tmp0 = (in0 + in4) << 13, tmp1 = (in0 - in4) << 13;
 *    odd part: the multipliers 2446 16819 25172 12299 7373 20995 16069 3196 9633 of the export's rule 4 in jidctint's order; descale
 *    (round half up, arithmetic shift) by 11 after the columns and 18 after the rows; + 128; clamp to 0 .. 255.  Grey: that, cropped.
 *    4:2:0: the chroma planes of hc x wc = ceil(h / 2) x ceil(w / 2) REAL samples are upsampled: v[2r] = 3 s[r] + s[max(r - 1, 0)],
 *    v[2r + 1] = 3 s[r] + s[min(r + 1, hc - 1)], out[2c] = (3 v[c] + v[max(c - 1, 0)] + 8) >> 4, out[2c + 1] = (3 v[c] + v[min(c + 1,
 *    wc - 1)] + 7) >> 4 -- the clamps act at the real size, not at the padded plane --; with wc <= 2 every chroma sample is repeated
 *    2 x 2 instead, as libjpeg does.  Colour: R = Y + ((91881 (Cr - 128) + 32768) >> 16), G = Y + ((-22554 (Cb - 128) - 46802 (Cr -
 *    128) + 32768) >> 16), B = Y + ((116130 (Cb - 128) + 32768) >> 16), clamped.  Dummy blocks are dropped.
 *    quant: device bytes [ntables][3][64], per component, natural order.  TT_EINVAL / TT_EUNSUPPORTED as tt_jpeg_coeffs, and ntables.
 * 6. Output: frames uint8 [n, h, w, ch]; nothing is written outside it.
 *    Every entry point refuses before the first HIP call; no allocation, no synchronisation. */
#define TT_JPEG_DECODE_WORDS 256
#define TT_JPEG_DECODE_SET_WORDS 1028
#ifndef TT_JPEG_SUBSEQ_BITS
#define TT_JPEG_SUBSEQ_BITS 1024                /* a build flag may try another S (a multiple of 32, 64 or more) */
#endif
#define TT_JPEG_STATUS_MARKER 1u
#define TT_JPEG_STATUS_CODE 2u
#define TT_JPEG_STATUS_BLOCKS 4u
#define TT_JPEG_STATUS_TAIL 8u
#define TT_JPEG_STATUS_SPAN 16u
#define TT_JPEG_MAX_SPANS 65535
typedef struct {
  int32_t h, w, ch, subsampling;
  int64_t scan_offset, scan_bytes;
  int32_t dc_table[3], ac_table[3];
  uint8_t quant[3][64];
  uint8_t bits[4][16];
  uint8_t huffval[4][256];
} TtJpegHeader;
int tt_jpeg_parse(const uint8_t* data /* host */, int64_t size, TtJpegHeader* header /* host */);
int tt_jpeg_decode_table(const uint8_t* bits /* host [16] */, const uint8_t* huffval /* host [256] */, uint32_t* table /* host [256] */);
int64_t tt_jpeg_sequence_bits(void);
int64_t tt_jpeg_entropy_ws_bytes(int32_t n, int64_t max_bytes);                          /* 0 for arguments tt_jpeg_entropy refuses */
int tt_jpeg_entropy(const uint8_t* scans, int64_t scans_bytes, const int64_t* offsets, const uint32_t* lengths, int64_t max_bytes, int32_t n,
                    int32_t h, int32_t w, int32_t ch, int32_t subsampling, const uint32_t* tables, int32_t ntables, int16_t* coeffs,
                    uint32_t* status, void* ws, int64_t ws_bytes, tt_stream_t stream);
int tt_jpeg_pixels(const int16_t* coeffs, int32_t n, int32_t h, int32_t w, int32_t ch, int32_t subsampling, const uint8_t* quant,
                   int32_t ntables, void* frames, tt_stream_t stream);
/* rules 1a and 4a: restart intervals (additive) */
int tt_jpeg_parse_spans(const uint8_t* data /* host */, int64_t size, TtJpegHeader* header /* host */, int32_t* restart_interval /* host */,
                        int64_t* span_offsets /* host [span_cap] or NULL */, int64_t* span_lengths /* host [span_cap] or NULL */, int64_t span_cap,
                        int64_t* nspans /* host */);
int tt_jpeg_entropy_spans(const uint8_t* scans, int64_t scans_bytes, const int64_t* offsets, const uint32_t* lengths, const int32_t* span_frame,
                          const uint32_t* span_first, const uint32_t* span_blocks, int64_t max_bytes, int32_t nspans, int32_t n, int32_t h, int32_t w,
                          int32_t ch, int32_t subsampling, const uint32_t* tables, int32_t ntables, int16_t* coeffs, uint32_t* status, void* ws,
                          int64_t ws_bytes, tt_stream_t stream);
/* Progressive files (SOF2; additive: tt_jpeg_parse and tt_jpeg_parse_spans keep refusing them, and a baseline file takes the launches
 * above).  A progressive file ends where a baseline one does: every scan is absorbed into the coefficient layout of rule 4, then rule 5
 * (tt_jpeg_pixels) runs unchanged.  Equal to libjpeg for every file whose progression is COMPLETE (below).
 * 1b. Parse -- tt_jpeg_parse_progressive (host): one file -> TtJpegProgressiveHeader (geometry, subsampling, per component its quantiser
 *    table in natural order, the scan count) and per scan a TtJpegScan: `comps` (bit c: component c of the frame is in the scan), Ss, Se,
 *    Ah, Al, the byte offset and stuffed length of its entropy-coded segment, and BITS / HUFFVAL of the tables in force AT THAT SOS (DHT
 *    segments between scans redefine the slots 0 .. 3 of either class, so the tables are snapshotted per scan): a DC-first scan (Ss = 0,
 *    Ah = 0) has component c's DC table at [c], an AC scan its one AC table at [0], a DC-refine scan none (zeros).  Two calls, as
 *    tt_jpeg_parse_spans: scans == NULL counts (*nscans); else scan_cap >= *nscans entries are filled.
 *    Validation (T.81 G.1.1.1.1, libjpeg's progression bookkeeping), TT_EINVAL, each by name: Ss = 0 with Se != 0 ("a DC scan with Se");
 *    Ss > 0 with more than one component ("an AC scan of"); Se < Ss or Se > 63 ("band"); Al > 13 ("Al ="); Ah != 0 on a coefficient's
 *    first visit, or on a later one Ah != the coefficient's previous Al or Al != Ah - 1 ("successive approximation"); an AC scan of a
 *    component before its DC-first scan ("before its DC"); a DC scan holding some but not all components, or not in frame order
 *    ("component subset"); a scan naming a component the frame does not have, or twice.
 *    TT_EUNSUPPORTED, each by name: what tt_jpeg_parse refuses other than SOF2 and several scans (12-bit, arithmetic, four components /
 *    Adobe, 16-bit DQT, other sampling, missing tables); a non-zero DRI ("restart intervals in a progressive file"); a DQT behind the
 *    first SOS ("a DQT behind"); more than TT_JPEG_MAX_SCANS = 256 scans; a baseline SOF0 file ("tt_jpeg_parse_spans" decodes it); and an
 *    INCOMPLETE PROGRESSION: at EOI every coefficient 0 .. 63 of every component must have reached Al = 0 ("incomplete progression").
 *    libjpeg smooths the blocks of files that stop earlier (jdcoefct.c, smoothing_ok), so their pixels are not the inverse DCT of their
 *    coefficients; they are refused, not decoded differently.  Every loop advances through the file.
 * 4b. Entropy decode of progressive scans -- tt_jpeg_entropy_progressive (device).  ITEMS are (frame, scan) pairs: item f nscans + s is
 *    scan s of frame f; offsets / lengths [n nscans] place its stuffed segment in `scans`; desc [n nscans][TT_JPEG_SCAN_WORDS = 8]
 *    uint32 = comps, Ss, Se, Ah, Al, 0, 0, 0 (comps = 0: the frame has no scan s); tables [n nscans][3][TT_JPEG_DECODE_WORDS] as rule
 *    1b lays them out.  All items are unstuffed at once by rule 3's three kernels; coeffs and status are zero-filled; then nscans ROUNDS
 *    follow, one launch each, grid (n): round s applies scan s of every frame that has one, ONE workgroup of 256 lanes per frame, the
 *    scan's kind read from desc.  Frames with different scan scripts share a call; stream order is the scan-to-scan dependency.
 *    Block map.  An interleaved scan (all components) walks the MCUs: its k-th block is block k of the layout.  A single-component scan
 *    walks the component's ceil(ceil(w Hi / Hmax) / 8) x ceil(ceil(h Vi / Vmax) / 8) REAL blocks in raster order: 4:2:0 Y block (by, bx)
 *    is block (by & 1) 2 + (bx & 1) of MCU (by / 2, bx / 2); a chroma block or a 4:4:4 block k is block k of its component in MCU k;
 *    grey: block k.  Dummy blocks keep zero AC (and the DC the interleaved DC scans give them).
 *    DC first (Ss = 0, Ah = 0): rule 4's lanes and passes with the state (p, block within the MCU); a symbol is a DC size code and its
 *    magnitude bits; the differences are written through the block map, then prefix-summed per component over the scan's own block order
 *    in int32 and stored as pred << Al.
 *    AC first (Ss > 0, Ah = 0): rule 4's lanes and passes with the state (p, z), z in Ss .. Se.  A symbol RS is as in baseline except
 *    S = 0, R < 15: EOBn, a run of (1 << R) + receive(R) blocks that end here, this one included: the lane's blocks-completed count
 *    advances by the run (saturating at 2^22 a lane, 2^31 a scan), so the exclusive scan that gives every lane its first block works
 *    unchanged.  Values are stored as value << Al; a run that passes Se ends the block and sets TT_JPEG_STATUS_CODE on the true path.
 *    DC refine (Ss = 0, Ah > 0): no Huffman code: bit k of the plain stream belongs to the scan's k-th block; one lane per block does
 *    coef |= bit << Al.  A stream shorter than the block count sets TT_JPEG_STATUS_BLOCKS.
 *    AC refine (Ss > 0, Ah > 0; T.81 G.1.2.3, libjpeg's decode_mcu_AC_refine), p1 = 1 << Al.  A code with S = 1 reads a sign bit for a new
 *    coefficient +-p1; S = 0, R = 15 skips 16 zero-history coefficients; S = 0, R < 15 starts an EOB run of (1 << R) + receive(R) blocks;
 *    S > 1 sets TT_JPEG_STATUS_CODE (and is taken as 1).  While R zero-history coefficients are skipped, every already-nonzero
 *    coefficient passed takes one correction bit: if it is 1 and (coef & p1) == 0, coef += coef >= 0 ? p1 : -p1; the blocks of an EOB
 *    run still take correction bits for the nonzero coefficients of their band.  The bits a block takes depend on which coefficients
 *    were nonzero BEFORE the scan, so a lane that guesses its block cannot resynchronise.  Instead of lanes and passes:
 *      masks  -- every lane takes blocks of the scan and stores per block a 64-bit mask of its nonzero coefficients inside Ss .. Se;
 *      walk   -- ONE lane walks the stream from the true state (0, block 0, Ss, no run).  It never reads a coefficient or a correction
 *                bit: a code moves z to the (R + 1)-th zero bit of the mask at or behind z and p by the code, the sign bit and the
 *                popcount of the mask bits passed; an EOB run moves p by a popcount a block.  It stores, per block, the bit position its
 *                first code (or, inside a run, its first correction bit) has, and a flag "inside a run".  The stream (a window of
 *                tt_jpeg_sequence_bits + 64 bits) and the masks (1024 a time) are staged in LDS by all lanes; the stages are bounded by
 *                L / (sequence bits - 31) + blocks / 1024 + 2, a stage's steps by sequence bits + 1024: every step takes a bit or a block;
 *      replay -- every lane takes blocks: from its block's recorded position it decodes the block's codes and correction bits again,
 *                now with the coefficients, and writes only that block.
 *    The serial chain is thus bit-position arithmetic alone, one table lookup, one or two popcounts a code; what it replaces is a pass
 *    per lane, each a full decode.  The walk stops at the first bit pattern that is no code (TT_JPEG_STATUS_CODE) or symbol that would
 *    read beyond L; blocks it did not reach are not touched and set TT_JPEG_STATUS_BLOCKS.
 *    All kinds: TT_JPEG_STATUS_TAIL as in rule 4; a descriptor whose numbers no scan has (an AC scan with several components or Se < Ss)
 *    sets TT_JPEG_STATUS_SPAN and is skipped; Ss, Se are held to 0 .. 63, Al to 0 .. 13.  No workgroup waits on another; every loop's
 *    bound is computed before it starts; every table and buffer index is masked or guarded; no host readback; status stays one word per
 *    frame with rule 4's bits.  Two memsets, one fill, three unstuffing launches, nscans round launches.
 *    ws: tt_jpeg_entropy_progressive_ws_bytes: tt_jpeg_entropy_ws_bytes(n nscans, max_bytes), then per item its frame (int32), then per
 *    frame tt_jpeg_blocks masks (uint64) and positions (uint32).
 *    TT_EINVAL: null pointer; n, nscans, h, w, max_bytes or scans_bytes <= 0; ch, subsampling as tt_jpeg_entropy; tables, coeffs, ws or
 *    desc off a 16-byte boundary; offsets off 8, lengths or status off 4; ws_bytes too small.  TT_EUNSUPPORTED: as tt_jpeg_coeffs;
 *    max_bytes of 2^28 or more; nscans above TT_JPEG_MAX_SCANS; n nscans above 65535 (a grid dimension).  Refused before any HIP call. */
#define TT_JPEG_MAX_SCANS 256
#define TT_JPEG_SCAN_WORDS 8
typedef struct {
  int32_t comps, ss, se, ah, al, reserved;
  int64_t offset, bytes;
  uint8_t bits[3][16];
  uint8_t huffval[3][256];
} TtJpegScan;
typedef struct {
  int32_t h, w, ch, subsampling, nscans, reserved;
  uint8_t quant[3][64];
} TtJpegProgressiveHeader;
int tt_jpeg_parse_progressive(const uint8_t* data /* host */, int64_t size, TtJpegProgressiveHeader* header /* host */,
                              TtJpegScan* scans /* host [scan_cap] or NULL */, int64_t scan_cap, int64_t* nscans /* host */);
int64_t tt_jpeg_entropy_progressive_ws_bytes(int32_t n, int32_t nscans, int64_t max_bytes, int32_t h, int32_t w, int32_t ch,
                                             int32_t subsampling);                       /* 0 for arguments the entry point refuses */
int tt_jpeg_entropy_progressive(const uint8_t* scans, int64_t scans_bytes, const int64_t* offsets, const uint32_t* lengths, const uint32_t* desc,
                                const uint32_t* tables, int64_t max_bytes, int32_t n, int32_t nscans, int32_t h, int32_t w, int32_t ch,
                                int32_t subsampling, int16_t* coeffs, uint32_t* status, void* ws, int64_t ws_bytes, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GIF import: an animated GIF decoded on the device to uint8 [F, H, W, 3] RGB frames, each the canvas a viewer shows after drawing
 * that frame (this_and_that_vdm_amd/ingest.py drives it: decode_gif / read_gif).  Only the compressed bytes cross to the device.  One
 * host routine (tt_gif_parse; plain C++, it touches no device), two device entry points (tt_gif_decode_indices, tt_gif_compose) and one
 * size query.  Integers only: the same bytes on every call and every stream.  Additive: the ABI version is unchanged.
 *
 * 1. Container -- tt_gif_parse (host).  GIF87a and GIF89a.  The logical screen W x H, the global colour table and the background
 *    index; per image its rectangle (left, top, w, h), the interlace flag, its local colour table, and from the graphic control
 *    extension before it the transparent index (-1: none), the disposal bits 0 .. 7 and the delay in 1/100 s (an image without one: -1,
 *    0, 0); the loop count of the NETSCAPE2.0 block (-1: no such block).  Comment, plain-text and other application extensions are
 *    skipped.  An image's data sub-blocks (any length 1 .. 255 each) are walked here and their payload is copied contiguously into
 *    `upload`: frame f's LZW bytes are upload[data_offset, data_offset + data_bytes).  A frame's palette is its local table, else the
 *    global one, padded with zeros to 256 entries.  A missing trailer behind a complete image is accepted.
 *    Two calls, as tt_jpeg_parse_spans: frames == NULL and upload == NULL count (header->frames, header->data_bytes); else
 *    frame_cap >= header->frames entries and upload_cap >= header->data_bytes bytes are filled, and nothing beyond either is written.
 *    TT_EINVAL, the text names the cause and the frame: null data / header; size <= 0; a bad signature ("signature"); a file that
 *    ends inside a header, table, extension or sub-block ("ends inside"); no image at all ("no image"); a rectangle of zero size ("zero
 *    size") or one that leaves the logical screen ("leaves the logical screen"; Pillow grows the canvas, this library refuses); an
 *    image with neither a local nor a global table ("no colour table"); a minimum code size outside 2 .. 8 ("minimum code size"); an
 *    unknown block ("unknown block"); frames without upload or the reverse ("go together"); frame_cap or upload_cap too small.
 *    TT_EUNSUPPORTED: more than 65 535 frames; a frame with 2^29 data bytes or more; a canvas above TT_GIF_MAX_PIXELS.
 *    Every loop of the parser advances through the file: its trips are bounded by the file's size.
 * 2. LZW (device).  A frame's stream starts with an empty table whether or not its first code is a clear code.  With C = 2^mcs (the
 *    clear code), C + 1 (end of information) and E0 = C + 2, between two clear codes:
 *    a. the code at place r (0, 1, ... behind the clear code) is min(12, bit length of C + 1 + r) bits wide ("GIF LZW on the device",
 *       rule 4) -- 12 once the table is full; codes are packed from the least significant bit;
 *    b. it is valid if it is below C (a pixel), or if it is E0 + k with k <= min(r - 1, 4095 - E0); k = r - 1 names the entry being
 *       made; the code at place 0 must be below C.  An INVALID code is read as the pixel 0;
 *    c. entry E0 + k is the string of the code at place k plus the first pixel of the string at place k + 1; it is made only while
 *       E0 + k <= 4095.  Behind a full table the codes stay 12 bits wide and make no entries (deferred clear) until a clear code comes;
 *    d. the stream ends at the end-of-information code, at the first code that does not lie whole inside the data, or at the end of
 *       the data.  Pixels beyond w h are ignored; pixels the stream does not reach are index 0.
 * 3. Status, one word per frame, each bit marks only its own frame: TT_GIF_DEC_STATUS_CODE: an invalid code whose string would start
 *    before pixel w h; TT_GIF_DEC_STATUS_SHORT: fewer than w h pixels; TT_GIF_DEC_STATUS_SPAN: an offset, length, pixel count or map
 *    offset outside the uploaded bytes or the index maps (the frame is taken as empty and nothing of it is written).
 * 4. Interlace: the rows of an interlaced image arrive in the four passes 0, 8, ... / 4, 12, ... / 2, 6, ... / 1, 3, ... and go to their
 *    real rows; the index maps are in raster order.
 * 5. Composition.  The canvas before frame 0 is, everywhere, frame 0's palette entry at frame 0's transparent index, entry 0 if it has
 *    none.  Before frame f >= 1 is drawn, the disposal of frame f - 1 is applied to frame f - 1's rectangle: 2: filled with B(f - 1),
 *    frame f - 1's palette at its transparent index if it has one, else at the logical screen's background index; 3: what the rectangle
 *    held before frame f - 1 was drawn is put back; any other value: left.  Drawing: every pixel of the rectangle whose index is not
 *    the frame's transparent index becomes the frame's palette entry.  Frame f of the output is the canvas after frame f is drawn.
 *    This equals Pillow (Image.open, seek(f), convert("RGB")) except in two patterns where Pillow departs from GIF89a, and the library
 *    follows the rule above in both: (a) frame 0 has disposal 3 and no transparent index: Pillow leaves frame 0 in place; (b) a frame
 *    has disposal 0 and the nearest earlier frame with non-zero bits has 2 or 3: Pillow keeps applying the earlier method.
 *
 * tt_gif_decode_indices: data (device, data_bytes of them) holds frame f's LZW bytes at offsets[f] (int64) with lengths[f] bytes; npix[f]
 * = w h; min_code_size[f]; rows[f] = the image's height when it is interlaced, else 0; map_offsets[f] (int64): where in maps (device,
 * maps_bytes of them) the frame's w h indices go -- all device arrays of n entries -> maps and status [n].  Values the arrays hold
 * are clamped or checked by the kernels: whatever they and the data hold, nothing is written outside maps, status and ws.  A memset of
 * maps and of status, then four launches; no workgroup waits on another, no readback sizes a grid, and every loop's trip count is
 * bounded before it starts (by the data length, the segment's code count, 4096, 12 or n):
 *   clears  -- grid (n), one workgroup per frame follows the chain of clear codes: from a clear code the place of every later code is a
 *              closed form (rule 2a), so the lanes extract a batch of codes a round and take the first clear code, end code or end of
 *              data; the SEGMENT between two clear codes (its first bit, its code count) is recorded when it holds a code;
 *   lengths -- workgroups stride over a frame's segments through the device-side count.  Per segment: parent(r) = code - E0 for the
 *              places r < 4096; a binary-lifting table of 12 levels x 4096 x 2 bytes = 96 KiB in LDS, built in 11 doubling rounds; from
 *              it every place's string length and first pixel in 12 lookups; then the length of every code of the segment, summed;
 *   offsets -- grid (n): a scan over the frame's segments gives each its first pixel (clipped to w h), sets SHORT, and cuts the
 *              segments' pixels into chunks of TT_GIF_DEC_CHUNK for the last launch;
 *   pixels  -- workgroups stride over a frame's chunks.  The segment's tables are rebuilt as above; its codes are walked in tiles of
 *              1024 with a scan of their lengths; every lane takes a pixel of the chunk, finds its code by a binary search of the tile
 *              (10 steps) and the pixel by walking depth - place ancestors up in at most 12 lookups: the dependent work per pixel does
 *              not grow with its string's length.  The index is stored at its raster (rule 4) place, guarded by w h.
 * The workspace is a derived bound: a segment that holds a code costs its closing code too, at least 2 (mcs + 1) >= 6 bits, so a frame
 * of b bytes has at most 8 b / 6 + 1 of them; tt_gif_decode_ws_bytes(n, data_bytes) holds 8 data_bytes / 6 + n segment records and n
 * frame records (0 for arguments the entry point refuses).
 * TT_EINVAL: a null pointer; n <= 0, data_bytes <= 0 or maps_bytes <= 0; offsets or map_offsets off an 8-byte, the other arrays and
 * status off a 4-byte, ws off a 16-byte boundary; ws_bytes too small ("ws too small").  TT_EUNSUPPORTED: more than 65 535 frames;
 * data_bytes of 2^29 or more (bit offsets are 32-bit); maps_bytes of 2^31 or more.
 *
 * tt_gif_compose: maps as above, table [n] TtGifComposeFrame and palettes [n][256][3] on the device, the initial colour 0x00BBGGRR ->
 * out uint8 [n, height, width, 3].  One launch, one lane per canvas pixel: it walks f = 0 .. n - 1 with the running colour and the
 * colour saved before the last draw (rule 5), reads each frame's map once and writes each output byte once.  A table entry whose
 * rectangle leaves the canvas or whose map leaves maps draws nothing.  TT_EINVAL: a null pointer; n, width, height or maps_bytes <= 0;
 * table off an 8-byte boundary.  TT_EUNSUPPORTED: more than 65 535 frames; a canvas above TT_GIF_MAX_PIXELS.
 * Every entry point refuses before the first HIP call; no allocation, no synchronisation. */
#define TT_GIF_DEC_STATUS_CODE 1u
#define TT_GIF_DEC_STATUS_SHORT 2u
#define TT_GIF_DEC_STATUS_SPAN 4u
#define TT_GIF_DEC_CHUNK 16384
#define TT_GIF_MAX_FRAMES 65535
typedef struct TtGifHeader {
  int32_t width, height, background, loop;         /* loop: -1 without a NETSCAPE2.0 block */
  int32_t global_colors, frames, version;           /* version: 87 or 89 */
  int32_t reserved;
  int64_t data_bytes;                               /* the LZW bytes of all frames, end to end */
} TtGifHeader;
typedef struct TtGifFrame {
  int32_t left, top, w, h;
  int32_t interlace, transparent, disposal, delay;  /* transparent: -1 for none; delay in 1/100 s */
  int32_t min_code_size, local_colors;              /* local_colors: 0 when the frame uses the global table */
  int64_t data_offset, data_bytes;                  /* in upload */
  uint8_t palette[256][3];
} TtGifFrame;
typedef struct TtGifComposeFrame {
  int32_t left, top, w, h, transparent, disposal;   /* transparent: -1 for none */
  uint32_t fill;                                     /* B of rule 5, 0x00BBGGRR */
  int32_t reserved;
  int64_t map_offset;
} TtGifComposeFrame;
int tt_gif_parse(const uint8_t* data /* host */, int64_t size, TtGifHeader* header /* host */, TtGifFrame* frames /* host [frame_cap] or NULL */,
                 int64_t frame_cap, uint8_t* upload /* host [upload_cap] or NULL */, int64_t upload_cap);
int64_t tt_gif_decode_ws_bytes(int32_t n, int64_t data_bytes);
int tt_gif_decode_indices(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const uint32_t* lengths, const uint32_t* npix,
                          const int32_t* min_code_size, const int32_t* rows, const int64_t* map_offsets, int32_t n, uint8_t* maps,
                          int64_t maps_bytes, uint32_t* status, void* ws, int64_t ws_bytes, tt_stream_t stream);
int tt_gif_compose(const uint8_t* maps, int64_t maps_bytes, const TtGifComposeFrame* table, const uint8_t* palettes, int32_t n, int32_t height,
                   int32_t width, uint32_t initial, uint8_t* out, tt_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PNG import: 8-bit PNG files decoded on the device to uint8 [F, H, W, ch] NHWC frames, byte for byte what Pillow's Image.open holds
 * (this_and_that_vdm_amd/ingest.py drives it: decode_png / read_pngs / read_apng).  Only the compressed bytes cross to the device.  One
 * host routine (tt_png_parse; plain C++, it touches no device), two device entry points (tt_png_inflate, tt_png_unfilter) and one size
 * query.  Integers only: the same bytes on every call and every stream.  Additive: the ABI version is unchanged.
 *
 * 1. Container -- tt_png_parse (host).  The signature, then chunks (length, type, payload, CRC) up to IEND.  IHDR must come first and
 *    its CRC-32 is verified; the CRCs of all other chunks are NOT (Pillow does not verify IDAT's either; the data's integrity is held
 *    by the Adler-32, rule 4).  Accepted: bit depth 8, colour types 0 / 4 / 2 / 6 (channels 1 / 2 / 3 / 4), not interlaced; any number
 *    of IDAT chunks of any length, zero included, one behind the other; ancillary chunks are skipped, tRNS and PLTE (a suggested palette)
 *    included.  Animated files: acTL (plays, announced frames), every fcTL (sequence, width, height, x, y, delay, dispose, blend) and
 *    the fdAT chunks behind it (their payload without the 4-byte sequence number); an fcTL before the IDAT makes the default image
 *    frame 0.  The payloads are copied contiguously into `upload` in file order: the default image's zlib stream is upload[idat_offset,
 *    idat_offset + idat_bytes), frame f's is upload[data_offset, data_offset + data_bytes).  spans[s] names chunk s's payload in the
 *    file and its frame (-1: the IDAT of a default image that is no frame).
 *    Two calls, as tt_gif_parse: spans, frames and upload all NULL count (header->spans, header->frames, header->data_bytes); else
 *    span_cap >= header->spans, frame_cap >= header->frames entries and upload_cap >= header->data_bytes bytes are filled, and nothing
 *    beyond them is written (frames may be NULL when header->frames is 0).
 *    TT_EINVAL, the text names the cause: null data / header; size <= 0; a bad signature ("signature"); a file that ends inside a
 *    chunk or before IEND ("ends inside"); no IHDR first ("IHDR"); an IHDR of another length or with a bad CRC ("CRC"); zero size
 *    ("zero size"); no IDAT ("no IDAT"); IDAT chunks with other chunks between them ("apart"); an unknown critical chunk ("unknown
 *    critical chunk"); a zlib stream of fewer than 2 bytes or whose header is not method 8 ("method 8"), names a window above 32 KiB
 *    ("window"), has a preset dictionary ("preset dictionary") or fails its check bits ("check bits"), the default image's and every
 *    frame's; an fcTL or acTL of the wrong length, an fdAT before any fcTL or shorter than 4 bytes; outputs that do not go together
 *    or caps too small.  TT_EUNSUPPORTED: bit depths 1 / 2 / 4 / 16 ("bit depth"); palette files ("colour type 3"); Adam7
 *    ("interlaced"); a compression or filter method other than 0; a stream of 2^29 bytes or more; more than 65 535 frames.
 *    Every loop of the parser advances through the file: its trips are bounded by the file's size.
 * 2. Inflate -- tt_png_inflate (device): n zlib streams (RFC 1950 / 1951), stream f at data[offsets[f], + lengths[f]), with the number
 *    of bytes each must give, expected[f] <= max_out -> those bytes at out[out_offsets[f] ...] and status[n].  It knows nothing of PNG.
 *    For a PNG, expected = tt_png_stream_bytes, out_offsets[f] = f tt_png_frame_stride: the layout tt_png_filter writes.  Every window
 *    size, stored, fixed and dynamic blocks in any order.  Bytes the stream does not reach are 0; bytes beyond expected are dropped.
 *    A memset of status, then 3 + ceil(log2(max_out)) launches:
 *      tokens -- grid (n), one workgroup of 1024 lanes per stream walks its blocks in order.  A stored block is a byte-aligned copy by
 *                all lanes.  A dynamic block's code lengths are read by one lane (at most 320 symbols) into canonical codes in LDS
 *                (counts per length and symbols by code, decoded length by length in at most 15 steps); the fixed block's codes are
 *                built the same way from its constant lengths.  The block's symbols are decoded in windows of 16 KiB staged in LDS:
 *                lane i starts at bit 128 i of the window, decodes the tokens that START in its 128 bits and records where it leaves
 *                them; then every lane takes its neighbour's exit as its start and decodes again if that moved, until nothing moves
 *                (lane k is right from round k on: at most 1024 rounds, a handful on real data, because a Huffman stream decoded
 *                from a wrong bit falls into step).  The state a lane inherits is the one bit position.  The first lane that meets
 *                the end of block (or an error, or the end of the data) ends the window; a scan of the lanes' byte counts places
 *                every token, and the lanes decode once more to write the SOURCE WORD of every byte: a literal (bit 31 set, the byte
 *                below) or the index in `out` of the byte it copies, its own position less the distance;
 *      jumps  -- ceil(log2(max_out)) launches of src[i] <- src[src[i]] over every byte that is not yet a literal: a byte's chain of
 *                copies is shorter than max_out, and after round k a word is a literal or names a byte 2^k copies back or more.  A
 *                constant stream (one chain as long as the stream) takes the same rounds as noise;
 *      bytes  -- per chunk of TT_INFLATE_CHUNK bytes: the literals leave as bytes, and the chunk's Adler-32 pair (sum b, sum (L - i) b);
 *      adler  -- grid (n): s1 = 1 + sum of the chunks' first sums, s2 = expected + sum of (second sum + bytes behind the chunk x first
 *                sum), mod 65 521, against the stream's big-endian trailer.
 *    No workgroup waits on another, no readback sizes a grid, every loop's trip count is bounded before it starts (by the stream's
 *    bits, 1024, 320, 258, 15 or the chunk count), and the dependent work per output byte grows neither with its chain of copies nor
 *    with the length of its Huffman stream.
 * 3. Status of tt_png_inflate, one word per stream, each bit marks only its own stream:
 *    TT_INFLATE_STATUS_BLOCK: a zlib header rule 1 names as refused, a reserved block type, or a stored LEN / NLEN mismatch;
 *    TT_INFLATE_STATUS_CODE: more than 286 / 30 codes, an over-subscribed or incomplete set of code lengths (incomplete is allowed for
 *      a literal/length or distance set whose longest code is 1 bit, as zlib allows it), a repeat with nothing before it or past the
 *      last length, no end-of-block code, bits that are no code of the set, the symbols 286 / 287 or the distance symbols 30 / 31;
 *    TT_INFLATE_STATUS_DIST: a distance that reaches before the stream's first byte (the bytes are 0 and the decode goes on);
 *    TT_INFLATE_STATUS_SHORT: fewer bytes than expected -- also where a BLOCK or CODE error or the end of the data stops the stream;
 *    TT_INFLATE_STATUS_LONG: more bytes than expected;
 *    TT_INFLATE_STATUS_ADLER: the stream ended with its final block and exactly the expected bytes, and its trailer is missing or is
 *      not the Adler-32 of those bytes;
 *    TT_INFLATE_STATUS_SPAN: offsets / lengths outside data, expected above max_out, or out_offsets / expected outside out (the
 *      stream is taken as empty and nothing of it is written).
 *    Whatever the data and the arrays hold, nothing is written outside out, status and ws.
 * 4. Unfilter -- tt_png_unfilter (device): filtered streams in tt_png_filter's layout -> pixels [n, h, w, ch]; the exact inverse of
 *    tt_png_filter for all five types (x = v + a; + b; + ((a + b) >> 1), the 9-bit sum floored; + paeth(a, b, c) with the tie order
 *    a, b, c), mod 256.  A pixel needs its left, upper and upper-left neighbours, so the anti-diagonals x + y = t are independent:
 *    one launch, grid (bands of TT_PNG_UNFILTER_BAND rows, n), a lane per row, step t handles x = t - row with all channels of the
 *    pixel, the upper pixel handed down through LDS.  A band whose first row is of type 0 or 1 needs nothing of the row above: its
 *    workgroup starts there and runs on through the following bands up to the next such band.  Status bit
 *    TT_PNG_UNFILTER_STATUS_TYPE: a filter-type byte above 4 (the row is read as type 0).
 *
 * The workspace grows with the OUTPUT, which the host knows exactly, not with the compressed size: tt_png_decode_ws_bytes(n,
 * out_bytes, max_out) = n records of 32 bytes + 4 out_bytes (a source word per byte of out) + 8 n ceil(max_out / TT_INFLATE_CHUNK) (a
 * pair per chunk), each part rounded up to 16; 0 for arguments the entry point refuses.
 * TT_EINVAL: a null pointer; n, data_bytes, out_bytes or max_out <= 0; max_out above out_bytes; offsets or out_offsets off an 8-byte,
 * lengths, expected and status off a 4-byte, ws (and tt_png_unfilter's filtered) off a 16-byte boundary; ws_bytes too small ("ws too
 * small"); tt_png_unfilter: n, h or w <= 0, ch outside 1 .. 4.  TT_EUNSUPPORTED: more than 65 535 streams; data_bytes of 2^29 or more
 * (bit offsets are 32-bit); out_bytes of 2^31 or more (a source word's index is 31-bit).
 * Every entry point refuses before the first HIP call; no allocation, no synchronisation. */
#define TT_INFLATE_STATUS_BLOCK 1u
#define TT_INFLATE_STATUS_CODE 2u
#define TT_INFLATE_STATUS_DIST 4u
#define TT_INFLATE_STATUS_SHORT 8u
#define TT_INFLATE_STATUS_LONG 16u
#define TT_INFLATE_STATUS_ADLER 32u
#define TT_INFLATE_STATUS_SPAN 64u
#define TT_PNG_UNFILTER_STATUS_TYPE 1u
#define TT_INFLATE_CHUNK 4096
#define TT_INFLATE_MAX_STREAMS 65535
#define TT_PNG_UNFILTER_BAND 256
typedef struct TtPngHeader {
  int32_t width, height, channels, bit_depth, color_type, interlace;
  int32_t spans, frames;                            /* IDAT + fdAT chunks; fcTL chunks (0: not animated) */
  int32_t plays, announced;                         /* acTL's num_plays and num_frames; -1, 0 without acTL */
  int32_t default_is_frame, reserved;               /* an fcTL stands before the IDAT */
  int64_t idat_offset, idat_bytes, data_bytes;      /* in upload; data_bytes: all payloads, end to end */
} TtPngHeader;
typedef struct TtPngSpan {
  int64_t file_offset, bytes;                       /* the payload in the file (an fdAT's without its sequence number) */
  int32_t frame, reserved;                          /* -1: the IDAT of a default image that is no frame */
} TtPngSpan;
typedef struct TtPngFrame {
  int32_t sequence, width, height, x, y, delay_num, delay_den, dispose, blend, spans;
  int64_t data_offset, data_bytes;                  /* in upload */
} TtPngFrame;
int tt_png_parse(const uint8_t* data /* host */, int64_t size, TtPngHeader* header /* host */, TtPngSpan* spans /* host [span_cap] or NULL */,
                 int64_t span_cap, TtPngFrame* frames /* host [frame_cap] or NULL */, int64_t frame_cap, uint8_t* upload /* host [upload_cap] or NULL */,
                 int64_t upload_cap);
int64_t tt_png_decode_ws_bytes(int32_t n, int64_t out_bytes, int64_t max_out);
int tt_png_inflate(const uint8_t* data, int64_t data_bytes, const int64_t* offsets, const uint32_t* lengths, const uint32_t* expected,
                   const int64_t* out_offsets, int32_t n, int64_t max_out, uint8_t* out, int64_t out_bytes, uint32_t* status, void* ws,
                   int64_t ws_bytes, tt_stream_t stream);
int tt_png_unfilter(const uint8_t* filtered, int32_t n, int32_t h, int32_t w, int32_t ch, uint8_t* out, uint32_t* status, tt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TTVDM_H */
