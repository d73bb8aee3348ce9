// tt_attention: flash-style attention on gfx950 MFMA; tt_temporal_attention: frame-axis attention.
//
// tt_attention -- per (q-block of 128 rows, head, sequence): 4 waves x 32 query rows.
//   S^T = K Q^T  (v_mfma 32x32x16, K tile rows as the MFMA "A" operand, Q^T held in registers as "B"),
//   so every lane owns ONE query column and 16 keys of each 32-key block: the softmax row reductions
//   are in-register plus a single lane^32 exchange, and P (converted in-register) is already the "B"
//   operand of  O^T += V^T P^T.  V is consumed TRANSPOSED from memory (vt = [heads*d, keys], written
//   by the V projection GEMM with swapped operands), so both tiles are plain K-contiguous rows staged by
//   the same LDS-DMA + swizzle as the GEMM.  K tile rows are permuted on the READ side (pi below) so
//   that accumulator register r of a lane is key 16*(lane>>5)+r: P needs no data movement at all.
//   Online softmax in fp32 with exp2; masked keys get -inf, running max starts at -1e30 (no NaN).
#include <stdlib.h>
#include <type_traits>
#include "common.h"

#ifndef TT_ATTN_PIPE_SGB
#define TT_ATTN_PIPE_SGB 1
#endif

namespace {

struct AttnP {
  const char* q; long ldq;
  const char* k; long ldk;
  const char* vt; long ldvt;
  char* out; long ldo;
  int nseq, lq, heads;
  int mask, lk, k_seq_stride, v_seq_stride, frames, ctx_batches, batch0;
  int k_rows_total;     // rows of k that exist
  long vt_cols_total;   // columns of vt that exist
  unsigned k_bytes, vt_bytes;   // extents for the buffer descriptors
  float scale_log2e;
  // fused query projection (cross-attention, round 4): Q = LN(x) Wq^T + bq computed by the block itself (QP instances)
  const char* qx; long ldqx; const char* wq; long ldwq; const float* bq; int qc; float ln_eps;
  unsigned qx_bytes, wq_bytes;
  int v_rows;           // TtAttnArgs.v_rows: `vt` holds V itself, [key rows, ldvt] like k (VR instances)
};

constexpr int QB = 128;   // queries per block
constexpr int KB = 64;    // keys per tile

// raw v_exp_f32: inputs here are <= 0 or -inf (exp2(-inf) = 0), no denormal/range fix-ups needed
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// XCD-aware block order (cdna guide T1, bijective form): the dispatcher places linear block b on XCD b % 8; remap so that each
// XCD runs a CONTIGUOUS range of logical blocks, x fastest -- the query blocks of one (head, sequence) then share an XCD and its
// L2 keeps their K / V^T (every query block streams all of them) instead of all eight L2s fetching a copy through the fabric.
struct Bid3 { int x, y, z; };
// HEADFAST (the fused-query cross-attention, whose large operand is the block's x rows, not the 78-token context): heads fastest, so the
// heads of one query block run on one XCD next to each other and its L2 serves the x tile to all but the first (TT_ATTN_QP_HEADFAST=0: A/B build)
#ifndef TT_ATTN_QP_HEADFAST
#define TT_ATTN_QP_HEADFAST 1
#endif
template <bool HEADFAST = false>
__device__ __forceinline__ Bid3 xcd_remap3() {
  const int gx = gridDim.x, gy = gridDim.y;
  const int nwg = gx * gy * (int)gridDim.z;
  int bid = (int)blockIdx.x + gx * ((int)blockIdx.y + gy * (int)blockIdx.z);
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  Bid3 o;
  if constexpr (HEADFAST) {
    o.y = bid % gy;
    const int t = bid / gy;
    o.x = t % gx;
    o.z = t / gx;
  } else {
    o.x = bid % gx;
    const int t = bid / gx;
    o.y = t % gy;
    o.z = t / gy;
  }
  return o;
}

// ---------------------------------------------------------------------------------------------
// The pieces attn_kernel, attn_pipe_kernel and attn8_kernel share: one copy each, force-inlined.  The three kernels run the same
// algorithm on the same lane layout (lane = one query, half hi, 16 keys of each 32-key block), so whatever does not depend on the
// operand format or on the order of a tile's raw reads and waits lives here.

// K-tile row read by MFMA row i = l31 so that accumulator reg r <-> key 16*hi + r  (see header)
__device__ __forceinline__ int key_perm(int l31) { return 16 * ((l31 >> 2) & 1) + (l31 & 3) + 4 * (l31 >> 3); }

// Q^T fragments straight from global (QES bytes per stored element): lane (query row qrow, half hi) holds the 16-byte chunks 2 n + hi
// of its head's D elements; rows beyond lq read as zeros
template <int QES, int D>
__device__ __forceinline__ void load_q_frags(const AttnP& p, int seq, int head, int qrow, bool qok, int hi, uint4 (&qf)[D * QES / 32]) {
  const char* qp = p.q + (((long)seq * p.lq + (qok ? qrow : 0)) * p.ldq + head * D) * QES;
#pragma unroll
  for (int n = 0; n < D * QES / 32; ++n) qf[n] = qok ? *(const uint4*)(qp + (n * 2 + hi) * 16) : make_uint4(0, 0, 0, 0);
}

// VR operand layout: the two per-lane addresses of the transposing reads (tile half `half` of a fragment's 8 keys); see attn_kernel's header
__device__ __forceinline__ void vr_read_addrs(int lane, unsigned lds_base, unsigned (&out)[2]) {
  const int gi = lane & 15, gg = lane >> 4, r2 = gi >> 2;
  const int base = ((gg & 1) * 2 + ((gi & 3) >> 1)) ^ ((gi >> 3) & 1);
#pragma unroll
  for (int half = 0; half < 2; ++half)
    out[half] = lds_base + (gg >> 1) * 2048 + r2 * 128 + half * 512 + ((base ^ (half << 1)) << 4) + (gi & 1) * 8;
}

// K / V^T staging by buffer_load ... lds (EB bytes per element: 1 = e4m3, 2, 4): per-lane 32-bit byte offsets computed once, the tile
// position is a scalar offset, out-of-range rows/columns land beyond num_records and read as zeros (same scheme as gemm.hip).
// A stage of the ring is the K tile ([64 keys][D], 16-byte chunks swizzled per row) followed by the V^T tile ([D][64 keys]; VR: V itself,
// rows = keys like the K tile).
// DH < D (tt_encoder_attention, head dimension 80 staged as 128 columns): the head holds DH elements in memory; the chunks / V^T rows of
// the tile beyond them are requested past num_records, i.e. land as zeros -- never as the next head's data.
template <int EB, int D, bool VR, int DH = D>
struct KvStage {
  static constexpr int EPC = 16 / EB;                                   // elements per 16-byte chunk
  static constexpr int KCPR = D / EPC, VCPR = VR ? D / EPC : KB / EPC;  // 16-B chunks per K-tile row (row = key, D elements) / per V^T-tile row (row = d, 64 keys; VR: row = key)
  static_assert(DH <= D && DH % EPC == 0, "whole chunks of the head");
  static constexpr int K_BYTES = KB * D * EB, V_BYTES = D * KB * EB, STAGE = K_BYTES + V_BYTES;
  static constexpr int KPT = (KB * KCPR) / 256, VPT = ((VR ? KB : D) * VCPR) / 256;  // chunks per thread (both tiles hold KB * D elements)
  static_assert(KPT * 4096 == K_BYTES && VPT * 4096 == V_BYTES, "the staged pieces cover each tile exactly");
  static constexpr int INV = (int)0x80000000;
  static_assert(KPT >= 1 && VPT >= 1, "tile smaller than the block");
  const AttnP& p;
  char* const ring;                                                     // this wave's first piece of stage 0
  const __amdgpu_buffer_rsrc_t rk, rv;
  int kvo[KPT], kr[KPT], vvo[VPT], vc[VPT];
  const int k_rows_left;                                                // rows of K that exist from kbase on
  const long v_cols_left;
  __device__ __forceinline__ KvStage(const AttnP& p_, char* smem, int tid, int wid, int head, int kbase, int vbase)
      : p(p_), ring(smem + wid * 1024),
        rk(__builtin_amdgcn_make_buffer_rsrc((void*)p_.k, 0, p_.k_bytes, 0x00020000)),
        rv(__builtin_amdgcn_make_buffer_rsrc((void*)p_.vt, 0, p_.vt_bytes, 0x00020000)),
        k_rows_left(p_.k_rows_total - kbase), v_cols_left(p_.vt_cols_total - vbase) {
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int slot = i * 256 + tid;
      const int r = slot / KCPR, c = (slot % KCPR) ^ tile_swz<KCPR>(r);
      kr[i] = r;
      kvo[i] = (int)((((long)kbase + r) * p.ldk + head * DH + c * EPC) * EB);
      if (DH != D && c * EPC >= DH) kvo[i] = INV;
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int slot = i * 256 + tid;
      const int r = slot / VCPR, c = (slot % VCPR) ^ tile_swz<VCPR>(r);
      if constexpr (VR) {                                      // rows = keys, like the K tile
        vc[i] = r;
        vvo[i] = (int)((((long)vbase + r) * p.ldvt + head * DH + c * EPC) * EB);
        if (DH != D && c * EPC >= DH) vvo[i] = INV;
      } else {
        vc[i] = c * EPC;
        vvo[i] = (int)(((long)(head * DH + r) * p.ldvt + vbase + c * EPC) * EB);
        if (DH != D && r >= DH) vvo[i] = INV;
      }
    }
  }
  __device__ __forceinline__ void stage(int buf, int tile) const {
    const int j0 = tile * KB;
    char* lk_ = ring + buf * STAGE;
    char* lv_ = ring + buf * STAGE + K_BYTES;
    const int soff_k = __builtin_amdgcn_readfirstlane((int)((long)j0 * p.ldk * EB));
    const int soff_v = VR ? __builtin_amdgcn_readfirstlane((int)((long)j0 * p.ldvt * EB)) : j0 * EB;
    const bool edge = j0 + KB > k_rows_left || j0 + KB > v_cols_left;    // uniform: only the last tile(s)
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      int v = kvo[i];
      if (edge && j0 + kr[i] >= k_rows_left) v = INV;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (__attribute__((address_space(3))) void*)(lk_ + i * 4096), 16, v, soff_k, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      int v = vvo[i];
      if (edge && j0 + vc[i] >= v_cols_left) v = INV;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void*)(lv_ + i * 4096), 16, v, soff_v, 0, 0);
    }
  }
};

// The tile loop: unrolled by two over the buffer parity (buffer and K / V split sit in the read instructions' immediates); only the
// last tile can hold keys >= lk and only it is compiled with the masking.  tile(t, buffer parity, masked).
template <typename F>
__device__ __forceinline__ void for_each_tile(int ntiles, int lk, F&& tile) {
  const bool ragged = (lk % KB) != 0;
  const int full = ragged ? ntiles - 1 : ntiles;
  int t = 0;
  for (; t + 1 < full; t += 2) {
    tile(t, std::integral_constant<int, 0>{}, std::false_type{});
    tile(t + 1, std::integral_constant<int, 1>{}, std::false_type{});
  }
  if (t < full) {
    tile(t, std::integral_constant<int, 0>{}, std::false_type{});
    if (ragged) tile(t + 1, std::integral_constant<int, 1>{}, std::true_type{});
  } else if (ragged) {
    tile(t, std::integral_constant<int, 0>{}, std::true_type{});
  }
}

// the ragged last tile t: keys >= lk score -inf (lane: keys t*KB + kb*32 + hi*16 + r)
__device__ __forceinline__ void mask_ragged(f32x16_t (&s)[2], int t, int hi, int lk) {
  const int j0 = t * KB;
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = j0 + kb * 32 + hi * 16 + r;
      if (j >= lk) s[kb][r] = -INFINITY;
    }
}

// Slow path of the lazy softmax reference (attn_kernel's tile has the whole idea): the tile's true maximum becomes the reference,
// l_run and the NO output accumulators (SP: the cross-term accumulators ox as well) are rescaled to it.  The caller re-exponentiates
// its scores against the new m_run in its own format.
template <int NO, bool WITH_OX = false>
__device__ __forceinline__ void softmax_rescale(const f32x16_t (&s)[2], float scale_log2e, float& m_run, float& l_run, f32x16_t (&o)[NO],
                                                f32x16_t* ox = nullptr) {
  float mx = s[0][0];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[kb][r]);
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float m_new = fmaxf(m_run, mx * scale_log2e);       // per query: both lane halves agree
  const float alpha = fast_exp2(m_run - m_new);             // 1 for the queries whose reference stays
  l_run *= alpha;
#pragma unroll
  for (int i = 0; i < NO; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) { o[i][r] *= alpha; if constexpr (WITH_OX) ox[i][r] *= alpha; }
  m_run = m_new;
}

// Epilogue: lane holds query l31, d = db*32 + 8g + 4hi + {0..3}.  Stored directly an instruction would write 16 bytes to each of
// 32 rows; instead the wave's 32 x D outputs go through a private LDS strip (the K/V ring is free once every wave has passed the
// barrier in here) and leave as full rows: 8 (D = 64, 16-bit) or more lanes cover one row's D*ES contiguous bytes.  Block qblk owns
// query rows (qblk * QB + i) * qstride + qcls (mask 2: one residue class; everything else 1, 0).
// DO < D (tt_encoder_attention's padded head): the strips are D wide, the NO accumulators cover the head's DO columns, DO columns are stored.
template <typename Tag, int D, int DO = D, int NO = D / 32>
__device__ __forceinline__ void attn_store_rows(const AttnP& p, char* smem, const f32x16_t (&o)[NO], float l_run, int wid, int lane,
                                                int seq, int head, int qblk, int qstride, int qcls) {
  static_assert(NO * 32 >= DO && NO * 32 <= D && (DO * Elem<Tag>::ES) % 16 == 0, "accumulators cover the stored columns");
  typedef typename Elem<Tag>::quad_t quad_t;
  constexpr int ES = Elem<Tag>::ES;
  const int l31 = lane & 31, hi = lane >> 5;
  const float l_tot = l_run + __shfl_xor(l_run, 32);
  const float inv = l_tot > 0.f ? 1.0f / l_tot : 0.f;
  __syncthreads();                                     // every wave is done with the K / V tiles
  constexpr int ROWB_O = D * ES, CPR_O = ROWB_O / 16;  // output row bytes per head, 16-byte chunks per row
  char* strip = smem + wid * (32 * ROWB_O);
#pragma unroll
  for (int db = 0; db < NO; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int byte = (db * 32 + 8 * g + 4 * hi) * ES;   // this lane's 4 consecutive d of query row l31
      const float v4[4] = {o[db][g * 4] * inv, o[db][g * 4 + 1] * inv, o[db][g * 4 + 2] * inv, o[db][g * 4 + 3] * inv};
      *(quad_t*)(strip + l31 * ROWB_O + (((byte >> 4) ^ (l31 & (CPR_O - 1))) << 4) + (byte & 15)) = f32_to_quad<Tag>(v4);
    }
  constexpr int RPP = 64 / CPR_O;                      // rows per pass
  const int oc = lane % CPR_O, orow = lane / CPR_O;
#pragma unroll
  for (int pass = 0; pass < 32 / RPP; ++pass) {
    const int r = pass * RPP + orow;
    const uint4 v = *(const uint4*)(strip + r * ROWB_O + ((oc ^ (r & (CPR_O - 1))) << 4));
    const int qr = (qblk * QB + wid * 32 + r) * qstride + qcls;
    if (qr < p.lq && (DO == D || oc * 16 < DO * ES)) *(uint4*)(p.out + (((long)seq * p.lq + qr) * p.ldo + head * DO) * ES + oc * 16) = v;
  }
}

// QP (cross-attention, D = 64, 16-bit storage): the block computes its own queries.  Q_h[128 x 64] = LN(x rows) Wq_h^T + bq_h is a
// 128 x 64 x C mini-GEMM in front of the key loop (x rows and the head's 64 rows of Wq staged slab by slab through a 3-deep
// LDS ring; LayerNorm folded into Wq by the caller, 1/sigma from the operand fragments as in tt_gemm ln_fold = 1) whose
// accumulators ARE the Q^T operand of S^T = K Q^T: lane (query l31, half hi) of fragment j holds output columns
// 32 j + 8 g + 4 hi + e; registers g = 2t, 2t+1 of fragment j are the 8 contraction slots of key step 2j + t.  The caller
// stores Wq / bq with bits 2 and 3 of the row index swapped inside every 16-row group (packing.permute_q_rows), so slot s of
// half hi is head dimension 16 (2j + t) + 8 hi + s -- what the K fragment of that step holds.  No Q tensor, no separate launch.
// VR (spatial self-attention, D = 64, 16-bit storage): V arrives as it leaves the Q | K | V projection -- [key rows, ldvt], not transposed --
// so the V projection needs no launch of its own with swapped operands.  The V tile is staged like the K tile ([64 keys][64 d], 128-byte rows,
// same swizzle) and the d-major operand of O^T += V^T P^T comes out of it through ds_read_b64_tr_b16 (tools/tr_read_probe.hip: a 16-lane
// group reads a [4 keys][16 d] block, lane i supplying the address of the 8-byte run (key i >> 2, d 4 (i & 3) ..) and receiving column i,
// keys 0..3): two such reads give the 8 keys x 1 d a lane holds of an MFMA operand.  Two address registers per lane; tile half, key block
// and d block are instruction offsets.
// SP (round 6, fp32 storage only): both products as three fp16 MFMAs on split operands (the "split16" mode of tt_gemm, same scales:
// common.h split_f16x4) -- Q is split once per block, K / V^T fragments and P per tile; the chunk pairs an x16 MFMA needs sit inside the
// batches of four the loops already read.  Two accumulators per product (hi x hi and the cross terms), combined before the softmax / at the end.
template <typename Tag, int D, int MASK, bool QP = false, bool VR = false, bool SP = false>
__global__ __launch_bounds__(256, (D == 64 && Elem<Tag>::ES == 2) ? 2 : 1) void attn_kernel(const AttnP p) {
  static_assert(!VR || (D == 64 && Elem<Tag>::ES == 2 && MASK == 0 && !QP), "row-major V: spatial self-attention, head dimension 64, 16-bit storage");
  static_assert(!SP || (Elem<Tag>::ES == 4 && !QP && !VR), "split products: the fp32-storage kernel");
  // (round 6 probe, removed: delaying the workgroup in the odd wave slot of a SIMD by 0.25-1 us so that one of the two resident workgroups
  // multiplies while the other exponentiates -- 138.3 / 2023 us -> 136.9-138.6 / 2005-2042 us at 1 792 / 7 168 keys: nothing.  Per tile a wave has
  // 16 MFMAs (512 matrix-pipe clocks) and 112 VALU of which 32 are quarter-rate exponentials (~830 issue clocks): two waves per SIMD are VALU-bound
  // at 61 % matrix-pipe use, the kernel sits at 47 %.)
  kernarg_touch<sizeof(AttnP)>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = Elem<Tag>::ES, EPC = Elem<Tag>::EPC;   // bytes per element, elements per 16-byte chunk
  typedef KvStage<ES, D, VR> Stage;
  constexpr int KCPR = Stage::KCPR, VCPR = Stage::VCPR, K_BYTES = Stage::K_BYTES, STAGE = Stage::STAGE;
  constexpr int DS = KCPR / 2, DB = D / 32;   // operand reads per K row (one chunk per lane half), 32-wide d blocks
  constexpr int PH = 16 / EPC;                // P chunks per lane per 32-key block

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const Bid3 blk = xcd_remap3<QP && TT_ATTN_QP_HEADFAST>();
  const int head = blk.y, seq = blk.z;
  const char* zero = (const char*)tt_zero_page;

  // ---- which queries does this block own, which keys do they see.
  // Temporal cross-attention (mask 2, reference quirk Q3): query q of sequence (b, frame) attends context (b*lq + q) % CB.
  // Queries of one residue class q % CB share their context, so a block takes QB queries of ONE class (row stride CB):
  // the context is block-uniform and the block stages only that context's keys (2 tiles of 64 for 78 tokens, instead of
  // 3 masked tiles over both contexts with a division per score).
  const int qstride = MASK == 2 ? p.ctx_batches : 1;
  const int qcls = MASK == 2 ? blk.x % qstride : 0;
  const int qblk = MASK == 2 ? blk.x / qstride : blk.x;
  int kbase, vbase;
  if (MASK == 0) { kbase = seq * p.k_seq_stride; vbase = seq * p.v_seq_stride; }
  else {
    const int b = p.batch0 + seq / p.frames;
    const int ctx = MASK == 1 ? b : (int)(((long)b * p.lq + qcls) % p.ctx_batches);
    kbase = ctx * p.k_seq_stride; vbase = ctx * p.v_seq_stride;
  }
  const int ntiles = (p.lk + KB - 1) / KB;

  // ---- Q^T fragments straight from global: lane (query l31) holds d = ds*16 + hi*8 .. +8
  const int qrow = (qblk * QB + wid * 32 + l31) * qstride + qcls;
  const bool qok = qrow < p.lq;
  uint4 qf[DS];
  if constexpr (!QP) {
    load_q_frags<ES, D>(p, seq, head, qrow, qok, hi, qf);
  } else {
    static_assert(!QP || (D == 64 && ES == 2 && MASK != 0), "fused query projection: cross-attention, head dimension 64, 16-bit storage");
    constexpr int QSLAB = QB * 128 + 64 * 128, QNST = 3;      // 16 KiB of x rows + 8 KiB of Wq rows per 64-deep slab
    constexpr int QINV = (int)0x80000000;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)p.qx, 0, p.qx_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rwq = __builtin_amdgcn_make_buffer_rsrc((void*)p.wq, 0, p.wq_bytes, 0x00020000);
    int xo[4], wo[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int slot = i * 256 + tid, r = slot >> 3, c = (slot & 7) ^ tile_swz<8>(r);
      const int qr = (qblk * QB + r) * qstride + qcls;
      xo[i] = qr < p.lq ? (int)((((long)seq * p.lq + qr) * p.ldqx + c * 8) * 2) : QINV;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int slot = i * 256 + tid, r = slot >> 3, c = (slot & 7) ^ tile_swz<8>(r);
      wo[i] = (int)((((long)head * 64 + r) * p.ldwq + c * 8) * 2);
    }
    const int nslab = p.qc >> 6;
    auto qstage = [&](int s) {                     // always 6 pieces (counted waits); beyond the last slab they fetch nothing
      char* dst = smem + (s % QNST) * QSLAB + wid * 1024;
      const int soff = __builtin_amdgcn_readfirstlane(s * 128);
      const bool ok = s < nslab;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(dst + i * 4096), 16, ok ? xo[i] : QINV, soff, 0, 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rwq, (__attribute__((address_space(3))) void*)(dst + QB * 128 + i * 4096), 16, ok ? wo[i] : QINV, soff, 0, 0);
    };
    f32x16_t qa[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) qa[j][r] = 0.f;
    float ls = 0.f, lq2 = 0.f;
    const unsigned qbase = lds_addr(smem);
    const int xr = wid * 32 + l31;
    unsigned xa[4], wa[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      xa[ks] = tile_off<8>(xr, ks * 2 + hi);
      wa[ks] = QB * 128 + tile_off<8>(l31, ks * 2 + hi);      // fragment j: + j * 32 rows = + 4096 bytes (same swizzle)
    }
    qstage(0); qstage(1);
    for (int s = 0; s < nslab; ++s) {
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");        // slab s has landed (slab s+1 may be in flight)
      __syncthreads();                                        // ... for every wave; the slot of slab s-1 is free
      qstage(s + 2);
      const unsigned sb = qbase + (s % QNST) * QSLAB;
      raw_u32x4_t xf[4], wf[2][4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        xf[ks] = lds_read16_raw(sb + xa[ks]);
        wf[0][ks] = lds_read16_raw(sb + wa[ks]);
        wf[1][ks] = lds_read16_raw_off<4096>(sb + wa[ks]);
      }
      lds_wait<0>();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        ln_stat<Tag>(xf[ks], ls, lq2);
#pragma unroll
        for (int j = 0; j < 2; ++j)
          qa[j] = Cvt<Tag>::mfma32(make_uint4(wf[j][ks].x, wf[j][ks].y, wf[j][ks].z, wf[j][ks].w),
                                   make_uint4(xf[ks].x, xf[ks].y, xf[ks].z, xf[ks].w), qa[j]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the empty pieces staged past the last slab
    __syncthreads();                                          // the ring is handed to the K / V^T tiles
    const float inv_c = 1.0f / (float)p.qc;
    const float sm = (ls + __shfl_xor(ls, 32)) * inv_c, sq = (lq2 + __shfl_xor(lq2, 32)) * inv_c;
    const float rs = rsqrtf(fmaxf(sq - sm * sm, 0.f) + p.ln_eps);
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) {
      const int j = ds >> 1, t = ds & 1;
      const float4 b0 = *(const float4*)(p.bq + head * 64 + 32 * j + 8 * (2 * t) + 4 * hi);
      const float4 b1 = *(const float4*)(p.bq + head * 64 + 32 * j + 8 * (2 * t + 1) + 4 * hi);
      const float v[8] = {fmaf(qa[j][(2 * t) * 4], rs, b0.x), fmaf(qa[j][(2 * t) * 4 + 1], rs, b0.y), fmaf(qa[j][(2 * t) * 4 + 2], rs, b0.z),
                          fmaf(qa[j][(2 * t) * 4 + 3], rs, b0.w), fmaf(qa[j][(2 * t + 1) * 4], rs, b1.x), fmaf(qa[j][(2 * t + 1) * 4 + 1], rs, b1.y),
                          fmaf(qa[j][(2 * t + 1) * 4 + 2], rs, b1.z), fmaf(qa[j][(2 * t + 1) * 4 + 3], rs, b1.w)};
      qf[ds] = qok ? pack8<Tag>(v) : make_uint4(0, 0, 0, 0);
    }
  }

  const Stage kv(p, smem, tid, wid, head, kbase, vbase);

  f32x16_t o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  f32x16_t ox[SP ? DB : 1];                    // SP: cross-term accumulators of O (o holds hi x hi); both are rescaled together
  uint4 qh[SP ? DS / 2 : 1], ql[SP ? DS / 2 : 1];
  if constexpr (SP) {
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) ox[i][r] = 0.f;
#pragma unroll
    for (int i = 0; i < DS / 2; ++i) {          // chunk pair (2i, 2i+1) of the query row = the 8 k-slots of one x16 MFMA
      uint2 h0, l0, h1, l1;
      split_f16x4(qf[2 * i].x, qf[2 * i].y, qf[2 * i].z, qf[2 * i].w, h0, l0);
      split_f16x4(qf[2 * i + 1].x, qf[2 * i + 1].y, qf[2 * i + 1].z, qf[2 * i + 1].w, h1, l1);
      qh[i] = make_uint4(h0.x, h0.y, h1.x, h1.y); ql[i] = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
  }

  const int pi = key_perm(l31);

  // ---- LDS addresses of the fragments this lane reads from a K / V^T tile.  The swizzle XOR depends on the lane's row, so
  // it cannot sit in the instruction's immediate; the stage (buffer parity) and the K/V split can -- the tile loop is
  // unrolled by two.  For D = 64 all 16 addresses are computed ONCE (every read is `ds_read_b128 v, vaddr offset:imm`, zero
  // address VALU in the loop); wider heads keep only the row bases and pay one XOR + add per read (register budget).
  const unsigned lds_base = lds_addr(smem);
  constexpr bool PRE = D == 64 && ES == 2;
  unsigned kaddr[PRE ? 2 : 1][PRE ? DS : 1], vaddr[PRE ? DB : 1][PRE ? 2 * PH : 1];
  if constexpr (PRE) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int ds = 0; ds < DS; ++ds) kaddr[kb][ds] = lds_base + tile_off<KCPR>(kb * 32 + pi, ds * 2 + hi);
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int k = 0; k < 2 * PH; ++k) vaddr[db][k] = lds_base + tile_off<VCPR>(db * 32 + l31, (k / PH) * (32 / EPC) + hi * PH + k % PH);
  }
  unsigned vr_addr[2] = {0u, 0u};
  if constexpr (VR) vr_read_addrs(lane, lds_base, vr_addr);
  auto k_addr = [&](int kb, int ds) -> unsigned {
    if constexpr (PRE) return kaddr[kb][ds]; else return lds_base + tile_off<KCPR>(kb * 32 + pi, ds * 2 + hi);
  };
  auto v_addr = [&](int db, int k) -> unsigned {
    if constexpr (PRE) return vaddr[db][k]; else return lds_base + tile_off<VCPR>(db * 32 + l31, (k / PH) * (32 / EPC) + hi * PH + k % PH);
  };

  // One 64-key tile.  Fragment reads are raw ds_reads (the compiler serialised visible ones: read -> wait -> MFMA, eight
  // times per key block) in batches of four, two batches in flight, retired by counted lgkmcnt waits: a batch lands under
  // the MFMAs of the one before it; the first two V^T batches are requested BEFORE the softmax and land under its VALU work.
  // A batch holds the fragments of TWO accumulators (both 32-key blocks for QK^T, two 32-wide d blocks for PV), so the
  // MFMAs of a batch alternate accumulators: a chain of four dependent 16-pass MFMAs would stall the issue for half its time.
  constexpr int NBK = DS / 2;                          // K batches: batch i = chunks ds {2i, 2i+1} of key blocks {0, 1}
  constexpr int NBV = (DB / 2) * PH;                   // V^T batches: batch i = reads k {2m, 2m+1} of d blocks {2g, 2g+1}
  static_assert(DS % 2 == 0 && DB % 2 == 0, "fragment batches of four");
  auto tile = [&](int t, auto buf_tag, auto mask_tag) {
    constexpr int BUF = decltype(buf_tag)::value;
    constexpr bool MASKED = decltype(mask_tag)::value;
    constexpr int KOFF = BUF * STAGE, VOFF = BUF * STAGE + K_BYTES;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's share of tile t has landed ...
    __syncthreads();                                           // ... and everybody's; the other buffer is free
    if (t + 1 < ntiles) kv.stage(BUF ^ 1, t + 1);
    raw_u32x4_t fa[4], fb[4];                                  // two fragment batches (K first, then V^T)
    auto read_k = [&](int i, raw_u32x4_t (&f)[4]) {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = lds_read16_raw_off<KOFF>(k_addr(j & 1, 2 * i + (j >> 1)));
    };
    auto read_v = [&](int i, raw_u32x4_t (&f)[4]) {
#pragma unroll
      for (int j = 0; j < 4; ++j) f[j] = lds_read16_raw_off<VOFF>(v_addr(2 * (i / PH) + (j & 1), 2 * (i % PH) + (j >> 1)));
    };
    // VR: fragment (db, k = kb * PH + h) = two transposing reads; offset = tile + key block kb (4096) + h (1024) + chunk bit 2 = db ^ h (64)
    raw_u32x2_t ga[8], gb[8];
    auto read_vr = [&](auto i_tag, raw_u32x2_t (&f)[8]) {
      constexpr int I = decltype(i_tag)::value;
      auto one = [&](auto j_tag) {
        constexpr int J = decltype(j_tag)::value;
        constexpr int db = 2 * (I / PH) + (J & 1), k = 2 * (I % PH) + (J >> 1), kb = k / PH, h = k % PH;
        constexpr int off = VOFF + kb * 4096 + h * 1024 + ((db ^ h) << 6);
        f[2 * J] = lds_read8_tr_off<off>(vr_addr[0]);
        f[2 * J + 1] = lds_read8_tr_off<off>(vr_addr[1]);
      };
      one(std::integral_constant<int, 0>{}); one(std::integral_constant<int, 1>{});
      one(std::integral_constant<int, 2>{}); one(std::integral_constant<int, 3>{});
    };
    f32x16_t s[2], sx[SP ? 2 : 1];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) { s[kb][r] = 0.f; if constexpr (SP) sx[kb][r] = 0.f; }
    read_k(0, fa);
    read_k(1, fb);
#pragma unroll
    for (int i = 0; i < NBK; ++i) {
      if (i + 1 < NBK) lds_wait<4>(); else lds_wait<0>();
      const raw_u32x4_t (&f)[4] = (i & 1) ? fb : fa;
      if constexpr (SP) {
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {                       // f[kb], f[kb + 2]: chunks 2i, 2i + 1 of key block kb
          uint2 h0, l0, h1, l1;
          split_f16x4(f[kb].x, f[kb].y, f[kb].z, f[kb].w, h0, l0);
          split_f16x4(f[kb + 2].x, f[kb + 2].y, f[kb + 2].z, f[kb + 2].w, h1, l1);
          const uint4 kh = make_uint4(h0.x, h0.y, h1.x, h1.y), kl = make_uint4(l0.x, l0.y, l1.x, l1.y);
          sx[kb] = Cvt<f16_tag>::mfma32(kl, qh[i], sx[kb]);
          s[kb] = Cvt<f16_tag>::mfma32(kh, qh[i], s[kb]);
          sx[kb] = Cvt<f16_tag>::mfma32(kh, ql[i], sx[kb]);
        }
      } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        s[j & 1] = Cvt<Tag>::mfma32(make_uint4(f[j].x, f[j].y, f[j].z, f[j].w), qf[2 * i + (j >> 1)], s[j & 1]);
      }
      __builtin_amdgcn_sched_barrier(0);                       // the MFMAs read the batch before it is re-filled
      if (i + 2 < NBK) { if (i & 1) read_k(i + 2, fb); else read_k(i + 2, fa); }
    }
    if constexpr (VR) {
      read_vr(std::integral_constant<int, 0>{}, ga);
      read_vr(std::integral_constant<int, 1>{}, gb);
    } else if constexpr (!SP) {
      read_v(0, fa);
      if constexpr (NBV > 1) read_v(1, fb);
    }
    // (SP requests its first V^T batches AFTER the softmax: at its register pressure -- 256 VGPRs + 160 AGPRs -- fragments that stay live
    // across the softmax get copied to accumulation registers right behind the raw read, i.e. before their data has landed: the hazard of
    // cdna guide 5.7 item 1, seen as a whole batch of keys missing from O.)
    if constexpr (SP) {                                          // 2^16 (hi x hi) + 2^5 (cross terms)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kb][r] = fmaf(sx[kb][r], 32.0f, s[kb][r] * 65536.0f);
    }
    // ---- mask + online softmax (lane: one query, keys j0 + kb*32 + hi*16 + r).  Raw scores stay unscaled: the
    // 1/sqrt(d)*log2(e) factor c is folded into the exponent, p = exp2(s*c - m*c), one FMA per score.
    if constexpr (MASKED) mask_ragged(s, t, hi, p.lk);
    // LAZY reference point, OPTIMISTIC evaluation.  Softmax is invariant to the subtracted constant, so the running "max" m_run
    // only has to keep exp2 in range.  Fast path: exponentiate against the m_run we have and look at the row sum -- if every
    // lane's partial sum of this tile is <= 2^14, no P exceeds 2^14 (fine for fp32 sums and 16-bit P) and the tile is done
    // WITHOUT computing a maximum: the 22 max instructions, the lane exchange and the rescale of 32 output registers leave the
    // stream that bounds this kernel at d = 64 (VALU, not MFMA).  Slow path (first tile: m_run = -1e30 gives inf; later only when
    // the scores outgrow the reference by ~2^8 or more): take the tile's true maximum as the new reference, rescale, redo P.
    constexpr float PSUM_OK = 16384.0f;
    float psum = 0.f;
    uint4 pf[2][PH];
    uint2 ph2[SP ? 2 : 1][SP ? PH : 1], pl2[SP ? 2 : 1][SP ? PH : 1];       // SP: the split halves of every P chunk
    auto exponentiate = [&](float m_ref) {
      psum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int h = 0; h < PH; ++h) {
          float e[EPC];
#pragma unroll
          for (int r = 0; r < EPC; ++r) { e[r] = fast_exp2(fmaf(s[kb][h * EPC + r], p.scale_log2e, -m_ref)); psum += e[r]; }
          pf[kb][h] = pack_chunk<Tag>(e);
        }
    };
    exponentiate(m_run);
    if (__any(!(psum <= PSUM_OK))) {                            // (also catches inf / NaN)
      softmax_rescale<DB, SP>(s, p.scale_log2e, m_run, l_run, o, ox);
      exponentiate(m_run);
    }
    l_run += psum;
    if constexpr (SP) {                                          // split the FINAL probabilities once (the optimistic pass may have produced inf)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int h = 0; h < PH; ++h) split_f16x4(pf[kb][h].x, pf[kb][h].y, pf[kb][h].z, pf[kb][h].w, ph2[kb][h], pl2[kb][h]);
      __builtin_amdgcn_sched_barrier(0);
      read_v(0, fa);
      if constexpr (NBV > 1) read_v(1, fb);
    }
    // ---- O^T += Vt_tile * P^T : k-slot (hi, e) of read k = kb*PH + h is key kb*32 + 16*hi + EPC*h + e
    if constexpr (VR) {                                        // (NBV = 2: both batches were requested before the softmax)
#pragma unroll
      for (int i = 0; i < NBV; ++i) {
        if (i + 1 < NBV) lds_wait<8>(); else lds_wait<0>();
        const raw_u32x2_t (&f)[8] = (i & 1) ? gb : ga;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int db = 2 * (i / PH) + (j & 1), k = 2 * (i % PH) + (j >> 1);
          o[db] = Cvt<Tag>::mfma32(make_uint4(f[2 * j].x, f[2 * j].y, f[2 * j + 1].x, f[2 * j + 1].y), pf[k / PH][k % PH], o[db]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
#pragma unroll
    for (int i = 0; i < NBV; ++i) {
      if (i + 1 < NBV) lds_wait<4>(); else lds_wait<0>();
      const raw_u32x4_t (&f)[4] = (i & 1) ? fb : fa;
      if constexpr (SP) {
        const int k0 = 2 * (i % PH), kb = k0 / PH, h0 = k0 % PH;         // f[jd], f[jd + 2]: key chunks k0, k0 + 1 of d block 2 (i / PH) + jd
        const uint4 ph = make_uint4(ph2[kb][h0].x, ph2[kb][h0].y, ph2[kb][h0 + 1].x, ph2[kb][h0 + 1].y);
        const uint4 pl = make_uint4(pl2[kb][h0].x, pl2[kb][h0].y, pl2[kb][h0 + 1].x, pl2[kb][h0 + 1].y);
#pragma unroll
        for (int jd = 0; jd < 2; ++jd) {
          const int db = 2 * (i / PH) + jd;
          uint2 vh0, vl0, vh1, vl1;
          split_f16x4(f[jd].x, f[jd].y, f[jd].z, f[jd].w, vh0, vl0);
          split_f16x4(f[jd + 2].x, f[jd + 2].y, f[jd + 2].z, f[jd + 2].w, vh1, vl1);
          const uint4 vh = make_uint4(vh0.x, vh0.y, vh1.x, vh1.y), vl = make_uint4(vl0.x, vl0.y, vl1.x, vl1.y);
          ox[db] = Cvt<f16_tag>::mfma32(vl, ph, ox[db]);
          o[db] = Cvt<f16_tag>::mfma32(vh, ph, o[db]);
          ox[db] = Cvt<f16_tag>::mfma32(vh, pl, ox[db]);
        }
      } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int db = 2 * (i / PH) + (j & 1), k = 2 * (i % PH) + (j >> 1);
        o[db] = Cvt<Tag>::mfma32(make_uint4(f[j].x, f[j].y, f[j].z, f[j].w), pf[k / PH][k % PH], o[db]);
      }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (i + 2 < NBV) { if (i & 1) read_v(i + 2, fb); else read_v(i + 2, fa); }
    }
    }
  };

  kv.stage(0, 0);
  for_each_tile(ntiles, p.lk, tile);
  if constexpr (SP) {
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[i][r] = fmaf(ox[i][r], 32.0f, o[i][r] * 65536.0f);
  }
  static_assert(4 * 32 * D * ES <= 2 * STAGE, "output strips do not fit the K/V ring");
  attn_store_rows<Tag, D>(p, smem, o, l_run, wid, lane, seq, head, qblk, qstride, qcls);
}

// ---------------------------------------------------------------------------------------------
// Spatial self-attention, software-pipelined ACROSS key tiles (round 6; VR operand layout, D = 64, 16-bit storage, lk a multiple of 64).
// attn_kernel runs a tile as QK^T -> softmax -> PV inside one wave, so a wave alternates ~512 matrix-pipe clocks with ~530 VALU issue clocks and
// the two waves of a SIMD (two resident workgroups) were measured to add up rather than overlap (matrix pipe 47 % busy).  Here iteration t of a
// wave runs S(t) = K(t) Q^T and then the softmax of tile t BESIDE O += V(t-1) P(t-1): matrix and vector instructions alternate in program order,
// which is the only overlap an in-order wave has by construction.  P is carried across the loop (the B operand of the NEXT iteration's PV);
// K(t+1) and V(t) are requested in iteration t, one iteration before they are read.  Lazy softmax reference exactly as in attn_kernel (the slow
// path rescales O after the iteration's PV: O and P(t-1) are both relative to the old reference at that point).  Same MFMA operands and summation
// order as attn_kernel: bit-identical outputs (tests/test_ops_gpu.py).  (A deeper version -- S(t+1) beside the softmax as well, two S and two P
// register sets alternating with the tile parity -- compiled to 64-register tuple copies per tile and 236-260 bytes of scratch per lane at two
// waves per SIMD, and to accumulator-file copies of every score at one: not kept.  Also measured on this kernel, one call, 1 792 / 7 168 keys:
// s_setprio(1) around the interleaved phases 125.6 -> 124.8 / 1 816 -> 1 808 us; without the sched_group_barrier hints 126.0 / 1 816: the
// compiler's own order is the same.  Per wave and tile the loop now takes ~510 ns against ~580 for attn_kernel.  Ablation builds (timing only,
// 7 168 keys, 1 826 us as built): no exponentials 1 537, no row-sum adds 1 695, NO MFMAs 732 us -- the vector / LDS skeleton is 732 us and the
// sixteen MFMAs of a tile still add most of their own time: a SIMD hides ~5 single-issue instructions beside one 32 x 32 x 16 MFMA
// (MI355X_MICROARCH.md), a d = 64 tile has 112 of them for 16 MFMAs, and the first key block's chain has no softmax work to sit beside.
// DESIGN.md 6.R6 has the floor this implies.)
template <typename Tag>
__global__ __launch_bounds__(256, 2) void attn_pipe_kernel(const AttnP p) {
  static_assert(Elem<Tag>::ES == 2, "16-bit storage");
  kernarg_touch<sizeof(AttnP)>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int D = 64, ES = 2, EPC = 8, CPR = 8;            // 128-byte tile rows (K: [64 keys][64 d]; V the same, keys as rows)
  constexpr int K_BYTES = KB * D * ES, V_BYTES = KB * D * ES, PT = (KB * CPR) / 256;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const Bid3 blk = xcd_remap3<false>();
  const int head = blk.y, seq = blk.z;
  const int kbase = seq * p.k_seq_stride, vbase = seq * p.v_seq_stride;
  const int nt = p.lk / KB;

  const int qrow = blk.x * QB + wid * 32 + l31;
  const bool qok = qrow < p.lq;
  uint4 qf[4];
  load_q_frags<ES, D>(p, seq, head, qrow, qok, hi, qf);
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)p.k, 0, p.k_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)p.vt, 0, p.vt_bytes, 0x00020000);
  // (Its own two stagers, not KvStage: K(t+1) and V(t) are staged in different iterations into separate rings, and whole tiles need no edge handling.)
  int kvo[PT], vvo[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int slot = i * 256 + tid;
    const int r = slot / CPR, c = (slot % CPR) ^ tile_swz<CPR>(r);
    kvo[i] = (int)((((long)kbase + r) * p.ldk + head * D + c * EPC) * ES);
    vvo[i] = (int)((((long)vbase + r) * p.ldvt + head * D + c * EPC) * ES);
  }
  auto stage_k = [&](int buf, int tile) {
    char* l_ = smem + buf * K_BYTES + wid * 1024;
    const int soff = __builtin_amdgcn_readfirstlane((int)((long)tile * KB * p.ldk * ES));
#pragma unroll
    for (int i = 0; i < PT; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (__attribute__((address_space(3))) void*)(l_ + i * 4096), 16, kvo[i], soff, 0, 0);
  };
  auto stage_v = [&](int buf, int tile) {
    char* l_ = smem + 2 * K_BYTES + buf * V_BYTES + wid * 1024;
    const int soff = __builtin_amdgcn_readfirstlane((int)((long)tile * KB * p.ldvt * ES));
#pragma unroll
    for (int i = 0; i < PT; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void*)(l_ + i * 4096), 16, vvo[i], soff, 0, 0);
  };

  f32x16_t o[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  uint4 P[4];                                                // probabilities of the PREVIOUS tile, chunk 2 kb + h (the B operand of its PV)
#pragma unroll
  for (int c = 0; c < 4; ++c) P[c] = make_uint4(0, 0, 0, 0);

  const int pi = key_perm(l31);
  const unsigned lds_base = lds_addr(smem);
  unsigned kaddr[4];                                         // key block 0; key block 1 is + 32 rows = + 4096 bytes (the swizzle only sees row bits 1-3)
#pragma unroll
  for (int ds = 0; ds < 4; ++ds) kaddr[ds] = lds_base + tile_off<CPR>(pi, ds * 2 + hi);
  unsigned vr_addr[2];
  vr_read_addrs(lane, lds_base, vr_addr);
  constexpr float PSUM_OK = 16384.0f;

  auto tile = [&](int t, auto buf_tag, auto pv_tag) {
    constexpr int BUF = decltype(buf_tag)::value;
    constexpr bool HAS_PV = decltype(pv_tag)::value;
    constexpr int KOFF = BUF * K_BYTES, VOFF = 2 * K_BYTES + (BUF ^ 1) * V_BYTES;            // K(t) in its own parity's buffer, V(t-1) in the other's
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's pieces of K(t) and V(t-1) have landed ...
    __syncthreads();                                           // ... and everybody's; K buffer BUF ^ 1 and V buffer BUF are free (read in iteration t-1)
    if (t + 1 < nt) stage_k(BUF ^ 1, t + 1);
    stage_v(BUF, t);
    // Matrix work of the iteration, in batches of two MFMAs.  S(t) = K(t) Q^T key block by key block (each a chain of four MFMAs on one
    // accumulator: with the lazy reference a score can be exponentiated as soon as ITS sum over d is complete, no row maximum is waited for):
    //   K0, K1 = key block 0, head-dimension chunks {0, 1}, {2, 3}      (alone)
    //   K2, K3 = key block 1                                           beside softmax chunks 0, 1 (key block 0)
    //   M0..M3 = O += V(t-1) P(t-1), key chunk M                        beside softmax chunks 2, 3 (key block 1), half a chunk per batch
    // Operand reads: two batches in flight (x, y), raw, counted waits.
    raw_u32x4_t x[2], y[2];                                    // a V batch is four 8-byte transposing reads = the same 8 registers
    auto request_k = [&](auto n_tag, raw_u32x4_t (&f)[2]) {    // batch n: key block n >> 1 (+ 32 rows = + 4096 bytes, same swizzle), chunks 2 (n & 1) + {0, 1}
      constexpr int N = decltype(n_tag)::value;
      f[0] = lds_read16_raw_off<KOFF + (N >> 1) * 4096>(kaddr[2 * (N & 1)]);
      f[1] = lds_read16_raw_off<KOFF + (N >> 1) * 4096>(kaddr[2 * (N & 1) + 1]);
    };
    auto request_v = [&](auto m_tag, raw_u32x4_t (&f)[2]) {    // V^T fragments (d block db, key chunk k = M): attn_kernel's read_vr
      constexpr int M = decltype(m_tag)::value;
      constexpr int kb = M / 2, h = M % 2;
      auto one = [&](auto db_tag) {
        constexpr int db = decltype(db_tag)::value;
        constexpr int off = VOFF + kb * 4096 + h * 1024 + ((db ^ h) << 6);
        const raw_u32x2_t lo = lds_read8_tr_off<off>(vr_addr[0]), hi2 = lds_read8_tr_off<off>(vr_addr[1]);
        f[db] = (raw_u32x4_t){lo.x, lo.y, hi2.x, hi2.y};
      };
      one(std::integral_constant<int, 0>{}); one(std::integral_constant<int, 1>{});
    };
    f32x16_t sc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) sc[kb][r] = 0.f;
    auto multiply_k = [&](int n, const raw_u32x4_t (&f)[2]) {
      const int kb = n >> 1, ds = 2 * (n & 1);
      sc[kb] = Cvt<Tag>::mfma32(make_uint4(f[0].x, f[0].y, f[0].z, f[0].w), qf[ds], sc[kb]);
      sc[kb] = Cvt<Tag>::mfma32(make_uint4(f[1].x, f[1].y, f[1].z, f[1].w), qf[ds + 1], sc[kb]);
    };
    auto multiply_v = [&](int m, const raw_u32x4_t (&f)[2]) {
#pragma unroll
      for (int db = 0; db < 2; ++db) o[db] = Cvt<Tag>::mfma32(make_uint4(f[db].x, f[db].y, f[db].z, f[db].w), P[m], o[db]);
    };
    float psum = 0.f;
    uint4 Pn[4];
    float e[8];
    auto exp_part = [&](int c, int part) {                     // 4 of the 32 scores of this lane: key block c >> 1, chunk c & 1, half `part`
      const int kb = c >> 1, h = c & 1;
#pragma unroll
      for (int r = part * 4; r < part * 4 + 4; ++r) { e[r] = fast_exp2(fmaf(sc[kb][h * 8 + r], p.scale_log2e, -m_run)); psum += e[r]; }
      if (part) Pn[c] = pack_chunk<Tag>(e);
    };
    auto exp_chunk = [&](int c) { exp_part(c, 0); exp_part(c, 1); };
    auto beside = [&](auto valu_tag) {                         // two MFMAs beside VALU vector instructions each
#if TT_ATTN_PIPE_SGB
      constexpr int VALU = decltype(valu_tag)::value;
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, VALU, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, VALU, 0);
#endif
    };
    request_k(std::integral_constant<int, 0>{}, x);
    request_k(std::integral_constant<int, 1>{}, y);
    lds_wait<2>(); multiply_k(0, x); __builtin_amdgcn_sched_barrier(0);
    request_k(std::integral_constant<int, 2>{}, x);
    lds_wait<2>(); multiply_k(1, y); __builtin_amdgcn_sched_barrier(0);
    request_k(std::integral_constant<int, 3>{}, y);
    lds_wait<2>(); multiply_k(2, x); exp_chunk(0); beside(std::integral_constant<int, 14>{}); __builtin_amdgcn_sched_barrier(0);
    if constexpr (HAS_PV) request_v(std::integral_constant<int, 0>{}, x);
    if constexpr (HAS_PV) lds_wait<4>(); else lds_wait<0>();
    multiply_k(3, y); exp_chunk(1); beside(std::integral_constant<int, 14>{}); __builtin_amdgcn_sched_barrier(0);
    if constexpr (HAS_PV) {
      request_v(std::integral_constant<int, 1>{}, y);
      lds_wait<4>(); multiply_v(0, x); exp_part(2, 0); beside(std::integral_constant<int, 7>{}); __builtin_amdgcn_sched_barrier(0);
      request_v(std::integral_constant<int, 2>{}, x);
      lds_wait<4>(); multiply_v(1, y); exp_part(2, 1); beside(std::integral_constant<int, 7>{}); __builtin_amdgcn_sched_barrier(0);
      request_v(std::integral_constant<int, 3>{}, y);
      lds_wait<4>(); multiply_v(2, x); exp_part(3, 0); beside(std::integral_constant<int, 7>{}); __builtin_amdgcn_sched_barrier(0);
      lds_wait<0>(); multiply_v(3, y); exp_part(3, 1); beside(std::integral_constant<int, 7>{}); __builtin_amdgcn_sched_barrier(0);
    } else {
      exp_chunk(2); exp_chunk(3);
    }
    if (__any(!(psum <= PSUM_OK))) {                            // the tile outgrew the reference (always on the first tile)
      softmax_rescale<2>(sc, p.scale_log2e, m_run, l_run, o);
      psum = 0.f;
      exp_chunk(0); exp_chunk(1); exp_chunk(2); exp_chunk(3);
    }
    l_run += psum;
#pragma unroll
    for (int c = 0; c < 4; ++c) P[c] = Pn[c];
  };
  typedef std::integral_constant<int, 0> B0;
  typedef std::integral_constant<int, 1> B1;

  stage_k(0, 0);
  tile(0, B0{}, std::false_type{});
  {
    int t = 1;
    for (; t + 1 < nt; t += 2) {
      tile(t, B1{}, std::true_type{});
      tile(t + 1, B0{}, std::true_type{});
    }
    if (t < nt) tile(t, B1{}, std::true_type{});
  }
  // ---- epilogue: O += V(nt-1) P(nt-1)
  auto final_pv = [&](auto buf_tag) {
    constexpr int BUF = decltype(buf_tag)::value;
    constexpr int VOFF = 2 * K_BYTES + BUF * V_BYTES;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    raw_u32x2_t g[16];
    auto one = [&](auto n_tag) {                                // fragment n = 2 k + db
      constexpr int N = decltype(n_tag)::value, k = N >> 1, db = N & 1, kb = k / 2, h = k % 2;
      constexpr int off = VOFF + kb * 4096 + h * 1024 + ((db ^ h) << 6);
      g[2 * N] = lds_read8_tr_off<off>(vr_addr[0]);
      g[2 * N + 1] = lds_read8_tr_off<off>(vr_addr[1]);
    };
    one(std::integral_constant<int, 0>{}); one(std::integral_constant<int, 1>{}); one(std::integral_constant<int, 2>{}); one(std::integral_constant<int, 3>{});
    one(std::integral_constant<int, 4>{}); one(std::integral_constant<int, 5>{}); one(std::integral_constant<int, 6>{}); one(std::integral_constant<int, 7>{});
    lds_wait<0>();
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      const int k = n >> 1, db = n & 1;
      o[db] = Cvt<Tag>::mfma32(make_uint4(g[2 * n].x, g[2 * n].y, g[2 * n + 1].x, g[2 * n + 1].y), P[k], o[db]);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  if ((nt - 1) & 1) final_pv(B1{}); else final_pv(B0{});

  attn_store_rows<Tag, D>(p, smem, o, l_run, wid, lane, seq, head, blk.x, 1, 0);
}

// ---------------------------------------------------------------------------------------------
// fp8 spatial self-attention (BASELINE config 5): Q, K, V^T arrive as OCP e4m3 bytes (tt_gemm out_fp8), both products run
// on v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales (E8M0 0x7f) -- the K = 64 form issues at twice the bf16 rate
// (tools/mfma_f8f6f4_probe.hip: 4 515 TFLOP/s against 1 745 for v_mfma_f32_32x32x16_fp8_fp8, which runs at the bf16 rate; layout
// checked there against a CPU product: lane l supplies row l & 31, k slots 32 (l >> 5) .. + 32 as 32 consecutive bytes).
// Same structure as attn_kernel (S^T = K Q^T, lane = one query, P already the "B" operand of O^T += V^T P^T) with half the
// operand bytes: a 64-key tile is 4 KiB of K + 4 KiB of V^T (D = 64), a lane reads TWO 16-byte chunks per MFMA (32 e4m3).
// k-slot maps (any map works as long as both operands use it):
//   QK^T   MFMA m of a key block: lane half hi supplies d = 16 (4m + hi) .. + 16 and 16 (4m + 2 + hi) .. + 16  (chunks 4m + hi, 4m + 2 + hi)
//   PV     one MFMA per d block: lane half hi supplies keys 16 hi .. + 16 and 32 + 16 hi .. + 16                (chunks hi, 2 + hi of the V^T row)
// P is exponentiated with a positive offset in the exponent (e4m3's subnormal floor 2^-9 would flush every probability below
// 0.002 of the row maximum; the offset moves the floor to 1.2e-4 .. 7.6e-6 of it, see the lazy reference point below) -- the
// factor cancels against the row sum, which is taken over the same scaled values.  Softmax statistics and both accumulations are fp32.
typedef long fp8x8_t;
template <typename Tag, int D>
__global__ __launch_bounds__(256, 2) void attn8_kernel(const AttnP p) {
  kernarg_touch<sizeof(AttnP)>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef KvStage<1, D, false> Stage;             // e4m3 operands; the OUTPUT element size is Elem<Tag>::ES
  constexpr int KCPR = Stage::KCPR, VCPR = Stage::VCPR, K_BYTES = Stage::K_BYTES, STAGE = Stage::STAGE;
  constexpr int JJ = D / 32, DB = D / 32;       // chunk reads per K row per lane, 32-wide d blocks
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const Bid3 blk = xcd_remap3();
  const int head = blk.y, seq = blk.z, qblk = blk.x;
  const int kbase = seq * p.k_seq_stride, vbase = seq * p.v_seq_stride;
  const int ntiles = (p.lk + KB - 1) / KB;
  const int qrow = qblk * QB + wid * 32 + l31;
  const bool qok = qrow < p.lq;
  uint4 qf[JJ];
  load_q_frags<1, D>(p, seq, head, qrow, qok, hi, qf);
  const Stage kv(p, smem, tid, wid, head, kbase, vbase);
  f32x16_t o[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const int pi = key_perm(l31);
  const unsigned lds_base = lds_addr(smem);
  unsigned kaddr[2][JJ], vaddr[DB][2];
#pragma unroll
  for (int kb = 0; kb < 2; ++kb)
#pragma unroll
    for (int jj = 0; jj < JJ; ++jj) kaddr[kb][jj] = lds_base + tile_off<KCPR>(kb * 32 + pi, 2 * jj + hi);
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) vaddr[db][kb] = lds_base + tile_off<VCPR>(db * 32 + l31, 2 * kb + hi);
  typedef int v8i_t __attribute__((ext_vector_type(8)));
  auto mfma8 = [](const v8i_t& a, const v8i_t& b, f32x16_t c) {            // 32 x 32 x 64, e4m3 x e4m3, unit scales
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
  };
  auto pack8 = [](const raw_u32x4_t& lo, const raw_u32x4_t& hi_) {
    return (v8i_t){(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi_.x, (int)hi_.y, (int)hi_.z, (int)hi_.w};
  };
  static_assert(JJ % 2 == 0, "two 16-byte chunks per K = 64 MFMA");
  v8i_t qv[JJ / 2];
#pragma unroll
  for (int m = 0; m < JJ / 2; ++m)
    qv[m] = (v8i_t){(int)qf[2 * m].x, (int)qf[2 * m].y, (int)qf[2 * m].z, (int)qf[2 * m].w,
                    (int)qf[2 * m + 1].x, (int)qf[2 * m + 1].y, (int)qf[2 * m + 1].z, (int)qf[2 * m + 1].w};
  auto tile = [&](int t, auto buf_tag, auto mask_tag) {
    constexpr int BUF = decltype(buf_tag)::value;
    constexpr bool MASKED = decltype(mask_tag)::value;
    constexpr int KOFF = BUF * STAGE, VOFF = BUF * STAGE + K_BYTES;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t + 1 < ntiles) kv.stage(BUF ^ 1, t + 1);
    raw_u32x4_t kf[2][JJ], vf[DB][2];
#pragma unroll
    for (int jj = 0; jj < JJ; ++jj)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) kf[kb][jj] = lds_read16_raw_off<KOFF>(kaddr[kb][jj]);
    f32x16_t s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
    lds_wait<0>();
#pragma unroll
    for (int m = 0; m < JJ / 2; ++m)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)             // alternate the two accumulators
        s[kb] = mfma8(pack8(kf[kb][2 * m], kf[kb][2 * m + 1]), qv[m], s[kb]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int db = 0; db < DB; ++db) vf[db][kb] = lds_read16_raw_off<VOFF>(vaddr[db][kb]);      // land under the softmax
    if constexpr (MASKED) mask_ragged(s, t, hi, p.lk);
    // lazy reference point, optimistic evaluation as in attn_kernel, with e4m3's range in mind: P' = 8 * exp2(s c - m_run), and
    // the tile is accepted when every lane's partial row sum is <= 448 -- then no P' exceeds e4m3's largest value.  The slow path
    // (first tile, or scores that outgrew the reference by ~2^5) makes the tile's true maximum the reference, so a row maximum
    // is stored as 8 .. 448 and e4m3's subnormal floor 2^-9 sits 2^-12 .. 2^-17.8 below it (eager reference + x256: 2^-17).
    constexpr float PSUM_OK = 448.0f, P_LOG2 = 3.0f;
    float psum = 0.f;
    unsigned pf[2][2][2];                                                  // [kb][h][dword]: 8 e4m3 of keys kb*32 + 16 hi + 8h ..
    auto exponentiate = [&](float shift) {
      psum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float e[8];
#pragma unroll
          for (int r = 0; r < 8; ++r) { e[r] = fast_exp2(fmaf(s[kb][h * 8 + r], p.scale_log2e, shift)); psum += e[r]; }
          int w0 = 0, w1 = 0;
          w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], w0, false);
          w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], w0, true);
          w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[4], e[5], w1, false);
          w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[6], e[7], w1, true);
          pf[kb][h][0] = (unsigned)w0; pf[kb][h][1] = (unsigned)w1;
        }
    };
    exponentiate(P_LOG2 - m_run);
    if (__any(!(psum <= PSUM_OK))) {                                       // (also catches inf / NaN: first tile, m_run = -1e30)
      softmax_rescale<DB>(s, p.scale_log2e, m_run, l_run, o);
      exponentiate(P_LOG2 - m_run);
    }
    l_run += psum;
    lds_wait<0>();
    const v8i_t pv = {(int)pf[0][0][0], (int)pf[0][0][1], (int)pf[0][1][0], (int)pf[0][1][1],
                      (int)pf[1][0][0], (int)pf[1][0][1], (int)pf[1][1][0], (int)pf[1][1][1]};
#pragma unroll
    for (int db = 0; db < DB; ++db) o[db] = mfma8(pack8(vf[db][0], vf[db][1]), pv, o[db]);
    __builtin_amdgcn_sched_barrier(0);
  };
  kv.stage(0, 0);
  for_each_tile(ntiles, p.lk, tile);
  attn_store_rows<Tag, D>(p, smem, o, l_run, wid, lane, seq, head, qblk, 1, 0);
}

// ---------------------------------------------------------------------------------------------
// tt_encoder_attention (the CLIP image / text encoders): self-attention over l = lq = lk tokens per sequence, head dimension DH = 64 or 80,
// optionally causal.  Same lane layout and the same pieces as attn_kernel (load_q_frags, KvStage, for_each_tile / mask_ragged, the lazy softmax
// reference with softmax_rescale, attn_store_rows, xcd_remap3); the tile is written plainly -- one batch of operand reads, one wait, its MFMAs --
// because the problem is 16-48 workgroups of at most five key tiles per launch: launch-bound, nothing to pipeline.
//   16-bit storage: V arrives row-major ([keys, ldv], a column slice of the fused Q | K | V projection) and is transposed on the way out of
//                   LDS by ds_read_b64_tr_b16 (the VR layout of attn_kernel, addresses computed per read instead of folded into immediates);
//   fp32 storage:   V arrives transposed ([heads * DH, ldv], tt_gemm out_col_hw) and both products run on the exact-fp32 MFMA.
// DH = 80 is a head PADDED to D = 128 staged columns: a K-tile row is 128 elements of which chunks >= 80 / EPC are requested past the buffer
// descriptor's num_records (zeros, never the next head) and are not even multiplied -- QK^T takes the DH * ES / 32 chunk pairs the head has
// (5 K-steps of 32x32x16 in 16-bit); V^T rows >= 80 of the head are zeros the same way, O^T is three 32-row blocks (rows 80..95 of the third
// are the waste: 1/6 of the PV MFMAs, and 3/8 of the ring's LDS), 80 columns are stored.  Scale 1/sqrt(80) (the host's scale_log2e).
// CAUSAL: lane = one query, key j > query scores -inf; a block stops at the tile that holds its LAST query (block-uniform: the barriers are
// per block), key 0 is visible to every query, so the first tile always gives every row a finite reference.
template <typename Tag, int DH, bool CAUSAL>
__global__ __launch_bounds__(256, 1) void enc_attn_kernel(const AttnP p) {
  kernarg_touch<sizeof(AttnP)>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = Elem<Tag>::ES, EPC = Elem<Tag>::EPC;
  constexpr bool VR = ES == 2;
  constexpr int D = DH == 64 ? 64 : 128;      // staged columns per head
  static_assert(DH == 64 || DH == 80, "head dimension 64 or 80");
  typedef KvStage<ES, D, VR, DH> Stage;
  constexpr int KCPR = Stage::KCPR, VCPR = Stage::VCPR, K_BYTES = Stage::K_BYTES, STAGE = Stage::STAGE;
  constexpr int DS = DH * ES / 32;            // chunk pairs (one chunk per lane half) of a K row that hold the head: the K-steps of QK^T
  constexpr int NO = (DH + 31) / 32;          // 32-row blocks of O^T
  constexpr int PH = 16 / EPC;                // P chunks per lane per 32-key block
  constexpr int KBATCH = ES == 4 ? DS / 2 : DS;
  static_assert(DS % KBATCH == 0, "whole batches of K fragments");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const Bid3 blk = xcd_remap3();
  const int head = blk.y, seq = blk.z, qblk = blk.x;
  const int kbase = seq * p.k_seq_stride, vbase = seq * p.v_seq_stride;
  const int qlast = min(qblk * QB + QB - 1, p.lq - 1);                         // the block's last query
  const int ntiles = CAUSAL ? qlast / KB + 1 : (p.lk + KB - 1) / KB;           // causal: tiles wholly past it are skipped
  const int lk_loop = min(p.lk, ntiles * KB);                                  // ragged only if the loop reaches the sequence's last tile

  const int qrow = qblk * QB + wid * 32 + l31;
  const bool qok = qrow < p.lq;
  uint4 qf[DS];
  load_q_frags<ES, DH>(p, seq, head, qrow, qok, hi, qf);
  const Stage kv(p, smem, tid, wid, head, kbase, vbase);

  f32x16_t o[NO];
#pragma unroll
  for (int i = 0; i < NO; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;
  const int pi = key_perm(l31);
  const unsigned lds_base = lds_addr(smem);
  const int gi = lane & 15, gg = lane >> 4;   // VR: the 16-lane groups of the transposing read

  auto tile = [&](int t, auto buf_tag, auto mask_tag) {
    constexpr int BUF = decltype(buf_tag)::value;
    constexpr bool MASKED = decltype(mask_tag)::value;
    constexpr int KOFF = BUF * STAGE, VOFF = BUF * STAGE + K_BYTES;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // this wave's share of tile t has landed ...
    __syncthreads();                                           // ... and everybody's; the other buffer is free
    if (t + 1 < ntiles) kv.stage(BUF ^ 1, t + 1);
    f32x16_t s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][r] = 0.f;
    // ---- S^T = K Q^T over the head's DS chunk pairs
#pragma unroll
    for (int b = 0; b < DS / KBATCH; ++b) {
      raw_u32x4_t kf[2][KBATCH];
#pragma unroll
      for (int i = 0; i < KBATCH; ++i)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) kf[kb][i] = lds_read16_raw_off<KOFF>(lds_base + tile_off<KCPR>(kb * 32 + pi, (b * KBATCH + i) * 2 + hi));
      lds_wait<0>();
#pragma unroll
      for (int i = 0; i < KBATCH; ++i)
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)                         // alternate the two accumulators
          s[kb] = Cvt<Tag>::mfma32(make_uint4(kf[kb][i].x, kf[kb][i].y, kf[kb][i].z, kf[kb][i].w), qf[b * KBATCH + i], s[kb]);
      __builtin_amdgcn_sched_barrier(0);                       // the MFMAs read the batch before it is re-filled
    }
    // ---- masks (lane: query qrow, keys t*KB + kb*32 + hi*16 + r) + online softmax, lazy reference as in attn_kernel
    if constexpr (MASKED) mask_ragged(s, t, hi, p.lk);
    if constexpr (CAUSAL) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t * KB + kb * 32 + hi * 16 + r > qrow) s[kb][r] = -INFINITY;
    }
    constexpr float PSUM_OK = 16384.0f;
    float psum = 0.f;
    uint4 pf[2][PH];
    auto exponentiate = [&](float m_ref) {
      psum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int h = 0; h < PH; ++h) {
          float e[EPC];
#pragma unroll
          for (int r = 0; r < EPC; ++r) { e[r] = fast_exp2(fmaf(s[kb][h * EPC + r], p.scale_log2e, -m_ref)); psum += e[r]; }
          pf[kb][h] = pack_chunk<Tag>(e);
        }
    };
    exponentiate(m_run);
    if (__any(!(psum <= PSUM_OK))) {                            // first tile (m_run = -1e30 gives inf), or scores that outgrew the reference
      softmax_rescale<NO>(s, p.scale_log2e, m_run, l_run, o);
      exponentiate(m_run);
    }
    l_run += psum;
    // ---- O^T += V^T P^T, one 32-row block of O^T at a time: k-slot (hi, e) of read k = kb*PH + h is key kb*32 + 16*hi + EPC*h + e
#pragma unroll
    for (int db = 0; db < NO; ++db) {
      if constexpr (VR) {
        // fragment k = two transposing reads of [4 keys][16 d]: lane gi of group gg supplies the 8-byte run (key + (gi >> 2), d 4 (gi & 3) ..)
        // of d block (db, gg & 1) and receives d = 16 (gg & 1) + gi of the four keys
        raw_u32x2_t g[2 * PH][2];
#pragma unroll
        for (int k = 0; k < 2 * PH; ++k)
#pragma unroll
          for (int half = 0; half < 2; ++half) {
            const int row = (k / PH) * 32 + 16 * (gg >> 1) + 8 * (k % PH) + 4 * half + (gi >> 2);
            g[k][half] = lds_read8_tr_off<VOFF>(lds_base + tile_off<VCPR>(row, db * 4 + (gg & 1) * 2 + ((gi & 3) >> 1)) + (gi & 1) * 8);
          }
        lds_wait<0>();
#pragma unroll
        for (int k = 0; k < 2 * PH; ++k)
          o[db] = Cvt<Tag>::mfma32(make_uint4(g[k][0].x, g[k][0].y, g[k][1].x, g[k][1].y), pf[k / PH][k % PH], o[db]);
      } else {
        raw_u32x4_t f[2 * PH];
#pragma unroll
        for (int k = 0; k < 2 * PH; ++k)
          f[k] = lds_read16_raw_off<VOFF>(lds_base + tile_off<VCPR>(db * 32 + l31, (k / PH) * (32 / EPC) + hi * PH + k % PH));
        lds_wait<0>();
#pragma unroll
        for (int k = 0; k < 2 * PH; ++k)
          o[db] = Cvt<Tag>::mfma32(make_uint4(f[k].x, f[k].y, f[k].z, f[k].w), pf[k / PH][k % PH], o[db]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  kv.stage(0, 0);
  for_each_tile(ntiles, lk_loop, tile);
  static_assert(4 * 32 * D * ES <= 2 * STAGE, "output strips do not fit the K/V ring");
  attn_store_rows<Tag, D, DH, NO>(p, smem, o, l_run, wid, lane, seq, head, qblk, 1, 0);
}

// two 16-bit products accumulated in fp32 in one instruction (v_dot2c_f32_bf16 / v_dot2c_f32_f16): the scores of the
// temporal kernel need neither operand unpacked
template <typename Tag> __device__ __forceinline__ float dot2_acc(unsigned a, unsigned b, float acc) { return acc; }   // f32_tag never calls it
template <> __device__ __forceinline__ float dot2_acc<bf16_tag>(unsigned a, unsigned b, float acc) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a), __builtin_bit_cast(bf16x2_t, b), acc, false);
}
template <> __device__ __forceinline__ float dot2_acc<f16_tag>(unsigned a, unsigned b, float acc) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, a), __builtin_bit_cast(f16x2_t, b), acc, false);
}

// ---------------------------------------------------------------------------------------------
// temporal self-attention: sequence = frames (<= LPU), one LPU-lane group per (batch, pixel, head).
// K/V rows of a block's units are staged in LDS (16-B loads), each lane = one query frame.
template <typename Tag, int D, int LPU>
__global__ __launch_bounds__(128) void tattn_kernel(const char* qkv, long ldqkv, char* out, long ldo, int batch,
                                                    int frames, int hw, int heads, float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = Elem<Tag>::ES, EPC = Elem<Tag>::EPC;
  constexpr bool F32 = ES == 4;
  constexpr int UPB = 128 / LPU;                 // units per block
  constexpr int ROWB = D * ES + 16;              // padded row bytes
  constexpr int UNITB = LPU * ROWB + 64;         // unit stride: the 4 units a wave touches sit 16 banks apart
  const int C = heads * D;
  const int tid = threadIdx.x;
  const long total_units = (long)batch * hw * heads;
  const long u0 = (long)blockIdx.x * UPB;
  // this lane's query row first: its latency overlaps the K/V staging round trip below
  const int ul = tid / LPU, fi = tid % LPU;
  const long u = u0 + ul;
  const bool active = u < total_units && fi < frames;
  const int h = (int)(u % heads);
  const long bp = u / heads;
  const int pix = (int)(bp % hw);
  const int b = (int)(bp / hw);
  const long qrow = ((long)b * frames + fi) * hw + pix;
  uint4 qv[D / EPC];         // the query row stays packed: 16-bit scores are dot2 products accumulated in fp32
  if (active) {
    const char* qp = qkv + (qrow * ldqkv + h * D) * ES;
#pragma unroll
    for (int c = 0; c < D / EPC; ++c) qv[c] = *(const uint4*)(qp + c * 16);
  }
  // stage K and V rows: unit u, frame f.  16-bit, D = 64: K and V share ONE LDS buffer (V waits in registers while the scores
  // are computed), which halves the LDS per block -- 8 blocks = 16 waves per CU instead of 8; the kernel is a latency-bound
  // HBM stream (load -> barrier -> score chains -> P.V in series per block), so resident waves are what hides the loads.
#ifdef TT_TATTN_NO_REUSE
  constexpr bool REUSE = false;
#else
  constexpr bool REUSE = ES == 2 && D == 64;
#endif
  const int chunks_per_row = D / EPC;
  const int nchunks = UPB * frames * chunks_per_row;
  constexpr int MAXI = REUSE ? (UPB * LPU * (D / EPC) + 127) / 128 : 1;
  auto src_of = [&](int s, int tensor, int& ldsoff) -> const char* {
    const int c = s % chunks_per_row, rf = s / chunks_per_row;
    const int f = rf % frames, sul = rf / frames;
    const long su = u0 + sul;
    ldsoff = sul * UNITB + f * ROWB + c * 16;
    if (su >= total_units) return nullptr;
    const int sh = (int)(su % heads);
    const long sbp = su / heads;
    const int spix = (int)(sbp % hw);
    const int sb = (int)(sbp / hw);
    const long row = ((long)sb * frames + f) * hw + spix;
    return qkv + (row * ldqkv + (tensor + 1) * C + sh * D + c * EPC) * ES;
  };
  uint4 vreg[MAXI];
  int off[MAXI];
  if constexpr (REUSE) {
    uint4 kreg[MAXI];
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int s_ = tid + i * 128;
      kreg[i] = vreg[i] = make_uint4(0, 0, 0, 0);
      off[i] = -1;
      if (s_ < nchunks) {
        const char* kp = src_of(s_, 0, off[i]);
        if (kp) { kreg[i] = *(const uint4*)kp; vreg[i] = *(const uint4*)(kp + (long)C * ES); }
      }
    }
#pragma unroll
    for (int i = 0; i < MAXI; ++i)
      if (off[i] >= 0) *(uint4*)(smem + off[i]) = kreg[i];
  } else {
    for (int tensor = 0; tensor < 2; ++tensor) {
      char* dst = smem + tensor * (UPB * UNITB);
      for (int s_ = tid; s_ < nchunks; s_ += 128) {
        int o;
        const char* sp = src_of(s_, tensor, o);
        *(uint4*)(dst + o) = sp ? *(const uint4*)sp : make_uint4(0, 0, 0, 0);
      }
    }
  }
  __syncthreads();
  const char* ks = smem + ul * UNITB;
  const char* vs = smem + (REUSE ? 0 : UPB * UNITB) + ul * UNITB;
  float sc[LPU];
  float mx = -INFINITY;
  if constexpr (!REUSE) { if (!active) return; }
#pragma unroll
  for (int j = 0; j < LPU; ++j) {
    float a = 0.f;
    if (j < frames && active) {
      float a1 = 0.f;        // two accumulation chains
#pragma unroll
      for (int c = 0; c < D / EPC; ++c) {
        const uint4 kv = *(const uint4*)(ks + j * ROWB + c * 16);
        if constexpr (F32) {
          a = fmaf(__uint_as_float(qv[c].x), __uint_as_float(kv.x), a);
          a1 = fmaf(__uint_as_float(qv[c].y), __uint_as_float(kv.y), a1);
          a = fmaf(__uint_as_float(qv[c].z), __uint_as_float(kv.z), a);
          a1 = fmaf(__uint_as_float(qv[c].w), __uint_as_float(kv.w), a1);
        } else {
          a = dot2_acc<Tag>(qv[c].x, kv.x, a);
          a1 = dot2_acc<Tag>(qv[c].y, kv.y, a1);
          a = dot2_acc<Tag>(qv[c].z, kv.z, a);
          a1 = dot2_acc<Tag>(qv[c].w, kv.w, a1);
        }
      }
      a = (a + a1) * scale_log2e;
      mx = fmaxf(mx, a);
    }
    sc[j] = a;
  }
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < LPU; ++j) { sc[j] = j < frames ? exp2f(sc[j] - mx) : 0.f; sum += sc[j]; }
  const float inv = 1.0f / sum;
  if constexpr (REUSE) {
    __syncthreads();                                   // every lane is done with K
#pragma unroll
    for (int i = 0; i < MAXI; ++i)
      if (off[i] >= 0) *(uint4*)(smem + off[i]) = vreg[i];
    __syncthreads();
    if (!active) return;
  }
  float acc[D];
#pragma unroll
  for (int e = 0; e < D; ++e) acc[e] = 0.f;
#pragma unroll
  for (int j = 0; j < LPU; ++j) {
    if (j < frames) {
      const float pj = sc[j] * inv;
#pragma unroll
      for (int c = 0; c < D / EPC; ++c) {
        float vf[EPC];
        unpack_chunk<Tag>(*(const uint4*)(vs + j * ROWB + c * 16), vf);
#pragma unroll
        for (int e = 0; e < EPC; ++e) acc[c * EPC + e] = fmaf(pj, vf[e], acc[c * EPC + e]);
      }
    }
  }
  char* op = out + (qrow * ldo + h * D) * ES;
#pragma unroll
  for (int c = 0; c < D / EPC; ++c) *(uint4*)(op + c * 16) = pack_chunk<Tag>(acc + c * EPC);
}

// ---- the same on the matrix cores (16-bit storage, D = 64, frames <= 16): one wave per unit (batch, pixel, head), 16 x 16 x 32 MFMAs.
//   S^T = K Q^T: lane (i = lane & 15, g = lane >> 4) loads 2 x 16 bytes of K row i and of Q row i -- head dimensions 8 g .. (its slots of k-step 0)
//   and 32 + 8 g .. (k-step 1), four lanes per 64 contiguous bytes -- straight from HBM into the operand registers.  The lane
//   then holds the scores of query column lane & 15 against keys 4 g .. 4 g + 3: softmax = 3 in-lane steps + the lane exchanges xor 16, xor 32.
//   O^T = V^T P^T: the probabilities a lane holds ARE its B operand (keys 4 g .. 4 g + 3 in slots 0..3, slots 4..7 zero); V goes through a
//   per-wave LDS tile [16 frames][64 d] and comes back transposed by ds_read_b64_tr_b16 -- group g reads the [4 keys][16 d] block of keys
//   4 g .., i.e. exactly the 4 slots of the matching A operand (the other 4 zero).  6 MFMAs and ~40 VALU per unit instead of ~1 300 VALU per lane.
template <typename Tag>
__global__ __launch_bounds__(256) void tattn_mfma_kernel(const char* qkv, long ldqkv, char* out, long ldo, int batch, int frames, int hw, int heads,
                                                         float scale_log2e, long total_units) {
  typedef float f32x4v __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) char vbuf[4][16 * 144];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = lane & 15, g = lane >> 4;
  const int C = heads * 64;
  const unsigned vb = lds_addr(vbuf[wv]);
  const unsigned v_rd = vb + (4 * g + (i >> 2)) * 144 + (i & 3) * 8;         // transposing read: (key 4 g + (i >> 2), d 4 (i & 3) ..)  (+ 32 db)
  // the six 16-byte pieces a lane loads of unit u (zeros beyond the last frame / the last unit); the NEXT unit's pieces are requested before
  // this unit's are used: two units of loads in flight per wave
  const bool rowok = i < frames;
  auto fetch = [&](long u, uint4 (&r)[6], long& orow, int& oh) {
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = make_uint4(0, 0, 0, 0);
    orow = 0; oh = 0;
    if (u >= total_units) return;
    const int h = (int)(u % heads);
    const long bp = u / heads;
    const int pix = (int)(bp % hw), b = (int)(bp / hw);
    orow = ((long)b * frames + i) * hw + pix; oh = h;
    if (rowok) {
      const char* rp = qkv + (orow * ldqkv + h * 64 + g * 8) * 2;     // head dimensions 8 g .. (k-step 0) and 32 + 8 g .. (k-step 1): 64 contiguous bytes per instruction and row
      r[0] = *(const uint4*)rp; r[1] = *(const uint4*)(rp + 64);
      r[2] = *(const uint4*)(rp + (long)C * 2); r[3] = *(const uint4*)(rp + (long)C * 2 + 64);
      r[4] = *(const uint4*)(rp + (long)C * 4); r[5] = *(const uint4*)(rp + (long)C * 4 + 64);
    }
  };
  const long stride = (long)gridDim.x * 4;
  uint4 cur[6], nxt[6];
  long orow = 0, nrow = 0;
  int h = 0, nh = 0;
  long u = (long)blockIdx.x * 4 + wv;
  fetch(u, cur, orow, h);
  for (; u < total_units; u += stride) {
    fetch(u + stride, nxt, nrow, nh);
    const uint4 q0 = cur[0], q1 = cur[1], k0 = cur[2], k1 = cur[3], v0 = cur[4], v1 = cur[5];
    f32x4v sacc = {0.f, 0.f, 0.f, 0.f};
    sacc = Cvt<Tag>::mfma16(k0, q0, sacc);
    sacc = Cvt<Tag>::mfma16(k1, q1, sacc);
    // the previous unit's transposing reads are done (their results fed MFMAs already): this wave's V tile may be overwritten
    *(uint4*)(vbuf[wv] + i * 144 + g * 16) = v0;              // V row i (zeros beyond the last frame), head dimensions 8 g .. and 32 + 8 g ..
    *(uint4*)(vbuf[wv] + i * 144 + 64 + g * 16) = v1;
    float sc[4];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) { sc[r] = (4 * g + r) < frames ? sacc[r] * scale_log2e : -INFINITY; mx = fmaxf(mx, sc[r]); }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float pr[4], sum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) { pr[r] = fast_exp2(sc[r] - mx); sum += pr[r]; }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float inv = 1.0f / sum;
    const uint4 pb = make_uint4(pack2<Tag>(pr[0], pr[1]), pack2<Tag>(pr[2], pr[3]), 0u, 0u);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                      // this wave's V tile is in LDS (one wave per tile: no barrier)
    const raw_u32x2_t t0 = lds_read8_tr_off<0>(v_rd), t1 = lds_read8_tr_off<32>(v_rd), t2 = lds_read8_tr_off<64>(v_rd), t3 = lds_read8_tr_off<96>(v_rd);
    lds_wait<0>();
    const f32x4v z = {0.f, 0.f, 0.f, 0.f};
    f32x4v o[4];
    o[0] = Cvt<Tag>::mfma16(make_uint4(t0.x, t0.y, 0u, 0u), pb, z);
    o[1] = Cvt<Tag>::mfma16(make_uint4(t1.x, t1.y, 0u, 0u), pb, z);
    o[2] = Cvt<Tag>::mfma16(make_uint4(t2.x, t2.y, 0u, 0u), pb, z);
    o[3] = Cvt<Tag>::mfma16(make_uint4(t3.x, t3.y, 0u, 0u), pb, z);
    // lane: query frame i, head dimensions 16 db + 4 g + {0..3}: four 8-byte stores, the four lane groups make 32 contiguous bytes each
    if (rowok) {
      char* op = out + (orow * ldo + h * 64 + 4 * g) * 2;
#pragma unroll
      for (int db = 0; db < 4; ++db)
        *(uint2*)(op + db * 32) = make_uint2(pack2<Tag>(o[db][0] * inv, o[db][1] * inv), pack2<Tag>(o[db][2] * inv, o[db][3] * inv));
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) cur[c] = nxt[c];
    orow = nrow; h = nh;
  }
}

// ---------------------------------------------------------------------------------------------
// Host side: which kernel a problem takes is decided ONCE (resolve_attention / resolve_temporal, from the validated arguments and the
// knobs), one tag x head-dimension dispatch turns the runtime dtype / head_dim into template arguments, and every kernel leaves
// through one launch helper.
int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
// Both A/B switches, read from the environment together, once per process, by the first call that asks for one.
struct AttnKnobs {
  int pipe = env_int("TT_ATTN_PIPE", 1);          // 0: attn_kernel for every key count of the v_rows route
  int tattn_mfma = env_int("TT_TATTN_MFMA", 1);   // 0: the per-lane temporal kernel
};
const AttnKnobs& attn_knobs() { static const AttnKnobs k; return k; }

enum class AttnRoute { FP8, QPROJ, PIPE, VROWS, SPLIT16, PLAIN };
// (asked of arguments tt_attention has validated: fp8 / qx / v_rows imply the dtype, head dimension and mask their kernels are built for)
AttnRoute resolve_attention(const TtAttnArgs& a) {
  if (a.fp8) return AttnRoute::FP8;                          // attn8_kernel
  if (a.qx) return AttnRoute::QPROJ;                         // attn_kernel<.., QP>: cross-attention with the query projection fused in
  if (a.v_rows)                                              // row-major V; whole key tiles, at least two: the software-pipelined kernel
    return attn_knobs().pipe && a.lk >= 2 * KB && a.lk % KB == 0 ? AttnRoute::PIPE : AttnRoute::VROWS;
  // TT_F32 "split16": the split-product variant of the same kernel (head dimension 128 keeps the exact-fp32 MFMA: its split variant spills 1 KiB per lane)
  if (a.dtype == TT_F32 && a.head_dim == 64 && tt_internal_f32_split()) return AttnRoute::SPLIT16;
  return AttnRoute::PLAIN;
}
// The kernel instance of a problem: launch_attention switches on it and tt_attention_kernel prints it.  d, mask: the template arguments
// as the route's instances take them (QPROJ is built for masks 1 / 2, VROWS for mask 0).
struct AttnInst { AttnRoute route; int d, mask; };
AttnInst attn_inst(const TtAttnArgs& a) {
  const AttnRoute route = resolve_attention(a);
  return AttnInst{route, a.head_dim, route == AttnRoute::QPROJ ? (a.mask == 1 ? 1 : 2) : (route == AttnRoute::VROWS ? 0 : a.mask)};
}
int attn_inst_name(const AttnInst& i, int dtype, char* name, int32_t cap) {
  const char* who = "tt_attention_kernel", *tag = tt_tag_name(dtype);
  if (i.route == AttnRoute::FP8) return tt_put_name(who, name, cap, "attn8_kernel<%s, %d>", tag, i.d);
  if (i.route == AttnRoute::PIPE) return tt_put_name(who, name, cap, "attn_pipe_kernel<%s>", tag);
  const auto tf = [](bool b) { return b ? "true" : "false"; };
  return tt_put_name(who, name, cap, "attn_kernel<%s, %d, %d, %s, %s, %s>", tag, i.d, i.mask, tf(i.route == AttnRoute::QPROJ),
                     tf(i.route == AttnRoute::VROWS), tf(i.route == AttnRoute::SPLIT16));
}
struct TattnRoute { bool mfma; int lpu; };                   // tattn_mfma_kernel or tattn_kernel<.., LPU lanes per unit>
TattnRoute resolve_temporal(int dtype, int head_dim, int frames) {
  // (one 16 x 16 MFMA tile of keys x queries per unit: tattn_mfma_kernel's own precondition)
  return TattnRoute{attn_knobs().tattn_mfma && dtype != TT_F32 && head_dim == 64 && frames <= 16, frames <= 16 ? 16 : 32};
}

// One launch.  Kernels that use dynamic LDS opt in to its size first, once per device: the mask is this instantiation's, i.e. per kernel instance.
template <auto Kernel, typename... Args>
void launch(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Args&... args) {
  static unsigned long long attr_done = 0;
  if (lds) tt_lds_opt_in((const void*)Kernel, (int)lds, &attr_done);
  hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
}
// f(Tag{}, integral_constant<int, D>{}) for the runtime dtype / head_dim (both validated by the caller)
template <typename F>
void for_tag_dim(int dtype, int head_dim, F&& f) {
  auto dim = [&](auto tag) {
    if (head_dim == 64) f(tag, std::integral_constant<int, 64>{}); else f(tag, std::integral_constant<int, 128>{});
  };
  if (dtype == TT_BF16) dim(bf16_tag{}); else if (dtype == TT_F16) dim(f16_tag{}); else dim(f32_tag{});
}
template <typename F>
void for_mask(int mask, F&& f) {
  if (mask == 0) f(std::integral_constant<int, 0>{}); else if (mask == 1) f(std::integral_constant<int, 1>{}); else f(std::integral_constant<int, 2>{});
}

// false: the route has no instance for this tag / head dimension (validation keeps such problems out)
template <typename Tag, int D>
bool launch_attention(const AttnInst& inst, const AttnP& p, hipStream_t st) {
  constexpr int ES = Elem<Tag>::ES;
  constexpr bool H64 = D == 64 && ES == 2;                   // QPROJ, PIPE, VROWS: head dimension 64, 16-bit storage
  constexpr size_t ring = 2 * (KB * D * ES + D * KB * ES);   // the K / V^T ring; it doubles as the output strips
  static_assert(ring <= 160 * 1024, "attention K/V ring exceeds the LDS");
  // mask 2: one block per (query residue class, QB queries of that class)
  const int cls = p.mask == 2 ? p.ctx_batches : 1;
  const dim3 grid(cls * ((((p.lq + cls - 1) / cls) + QB - 1) / QB), p.heads, p.nseq), block(256);
  switch (inst.route) {
    case AttnRoute::FP8:
      if constexpr (ES == 2) {
        // the K/V ring (2 x 2 x 64 x D bytes) doubles as the 4 x 32 x D*ES-byte output strips
        constexpr size_t ring8 = 2 * (KB * D + D * KB), strips = 4 * 32 * D * ES;
        launch<attn8_kernel<Tag, D>>(grid, block, ring8 > strips ? ring8 : strips, st, p);
        return true;
      }
      break;
    case AttnRoute::QPROJ:
      if constexpr (H64) {
        constexpr size_t lds = 3 * (QB * 128 + 64 * 128);    // the 3 x 24 KiB projection ring (the K / V^T ring reuses it)
        if (inst.mask == 1) launch<attn_kernel<Tag, 64, 1, true>>(grid, block, lds, st, p);
        else launch<attn_kernel<Tag, 64, 2, true>>(grid, block, lds, st, p);
        return true;
      }
      break;
    case AttnRoute::PIPE:
      if constexpr (H64) { launch<attn_pipe_kernel<Tag>>(grid, block, ring, st, p); return true; }
      break;
    case AttnRoute::VROWS:
      if constexpr (H64) { launch<attn_kernel<Tag, 64, 0, false, true>>(grid, block, ring, st, p); return true; }
      break;
    case AttnRoute::SPLIT16:
      if constexpr (ES == 4 && D == 64) {
        for_mask(inst.mask, [&](auto m) { launch<attn_kernel<Tag, D, decltype(m)::value, false, false, true>>(grid, block, ring, st, p); });
        return true;
      }
      break;
    case AttnRoute::PLAIN:
      for_mask(inst.mask, [&](auto m) { launch<attn_kernel<Tag, D, decltype(m)::value>>(grid, block, ring, st, p); });
      return true;
  }
  return false;
}

template <typename Tag, int D, int LPU>
void launch_tattn(const void* qkv, long ldqkv, void* out, long ldo, int batch, int frames, int hw, int heads, hipStream_t st) {
  constexpr int UPB = 128 / LPU;
#ifdef TT_TATTN_NO_REUSE
  constexpr bool REUSE = false;
#else
  constexpr bool REUSE = Elem<Tag>::ES == 2 && D == 64;      // K and V share the buffer (tattn_kernel)
#endif
  constexpr size_t lds = (REUSE ? 1 : 2) * UPB * (LPU * (D * Elem<Tag>::ES + 16) + 64);
  static_assert(lds <= 160 * 1024, "temporal attention staging exceeds the LDS");
  const long units = (long)batch * hw * heads;
  launch<tattn_kernel<Tag, D, LPU>>(dim3((unsigned)((units + UPB - 1) / UPB)), dim3(128), lds, st, (const char*)qkv, ldqkv, (char*)out, ldo, batch,
                                    frames, hw, heads, 1.4426950408889634f / sqrtf((float)D));
}
template <typename Tag>
void launch_tattn_mfma(const void* qkv, long ldqkv, void* out, long ldo, int batch, int frames, int hw, int heads, hipStream_t st) {
  const long units = (long)batch * hw * heads;
  long blocks = (units + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;                    // 8 blocks of 4 waves per CU, grid-stride over the units
  launch<tattn_mfma_kernel<Tag>>(dim3((unsigned)blocks), dim3(256), 0, st, (const char*)qkv, ldqkv, (char*)out, ldo, batch, frames, hw, heads,
                                 1.4426950408889634f / sqrtf(64.0f), units);
}

// what tt_attention checks of a problem, and its launch parameters
int attn_params(const TtAttnArgs* a, AttnP& p) {
  if (!a || (!a->q && !a->qx) || !a->k || !a->vt || !a->out) TT_FAIL(TT_EINVAL, "tt_attention: null operand");
  if (a->qx) {
    if (a->mask == 0 || a->head_dim != 64 || a->dtype == TT_F32 || a->fp8)
      TT_FAIL(TT_EUNSUPPORTED, "tt_attention: the fused query projection serves cross-attention (mask 1 / 2), head_dim 64, 16-bit storage");
    if (!a->wq || !a->bq || a->qc < 64 || (a->qc & 63) || (a->ldqx & 7) || (a->ldwq & 7) || !(a->ln_eps > 0.f))
      TT_FAIL(TT_EINVAL, "tt_attention: fused query projection needs wq, bq, qc %% 64 == 0, row strides %% 8 == 0, ln_eps > 0");
    // the kernel reads bq as float4 and x / wq rows as 16-byte chunks through buffer descriptors
    if ((((size_t)a->qx | (size_t)a->wq | (size_t)a->bq)) & 15)
      TT_FAIL(TT_EINVAL, "tt_attention: fused query projection needs qx, wq and bq on 16-byte boundaries");
  }
  if (a->head_dim != 64 && a->head_dim != 128) TT_FAIL(TT_EUNSUPPORTED, "tt_attention: head_dim %d (64 or 128)", a->head_dim);
  if (a->nseq <= 0 || a->lq <= 0 || a->heads <= 0 || a->lk <= 0) TT_FAIL(TT_EINVAL, "tt_attention: empty problem");
  if (a->mask < 0 || a->mask > 2) TT_FAIL(TT_EINVAL, "tt_attention: mask %d", a->mask);
  if (a->mask != 0 && (a->frames <= 0 || a->ctx_batches <= 0 || a->nseq % a->frames)) TT_FAIL(TT_EINVAL, "tt_attention: frames/ctx");
  if (a->mask != 0 && (a->batch0 < 0 || a->batch0 + a->nseq / a->frames > a->ctx_batches)) TT_FAIL(TT_EINVAL, "tt_attention: batch0 + batches exceeds ctx_batches");
  if (a->lk > a->k_seq_stride || a->lk > a->v_seq_stride) TT_FAIL(TT_EINVAL, "tt_attention: lk exceeds sequence stride");
  if (a->mask == 2 && a->k_seq_stride != a->v_seq_stride) TT_FAIL(TT_EINVAL, "tt_attention: mask 2 needs equal k/v context strides");
  if (a->dtype != TT_BF16 && a->dtype != TT_F16 && a->dtype != TT_F32) TT_FAIL(TT_EINVAL, "tt_attention: bad dtype");
  if (a->fp8 && (a->mask != 0 || a->dtype == TT_F32)) TT_FAIL(TT_EUNSUPPORTED, "tt_attention: the fp8 path serves spatial self-attention (mask 0) with 16-bit output");
  const int es = a->fp8 ? 1 : (a->dtype == TT_F32 ? 4 : 2);      // bytes per q/k/vt element
  const int eso = a->dtype == TT_F32 ? 4 : 2;
  if ((a->q && ((a->ldq * es) & 15)) || ((a->ldk * es) & 15) || ((a->ldvt * es) & 15) || ((a->ldo * eso) & 15) || (!a->v_rows && ((a->v_seq_stride * es) & 15)))
    TT_FAIL(TT_EINVAL, "tt_attention: strides must keep 16-byte chunks aligned");
  // base pointers too: K / V tiles go to LDS by 16-byte DMA, the v_rows route and the outputs use 16-byte vector accesses (a column
  // slice of a fused Q | K | V buffer offset by a non-multiple of 8 elements would otherwise be read misaligned instead of refused)
  if ((((size_t)a->q | (size_t)a->k | (size_t)a->vt | (size_t)a->out) & 15))
    TT_FAIL(TT_EINVAL, "tt_attention: q, k, vt and out must start on 16-byte boundaries");
  p.q = (const char*)a->q; p.ldq = a->ldq; p.k = (const char*)a->k; p.ldk = a->ldk;
  p.vt = (const char*)a->vt; p.ldvt = a->ldvt; p.out = (char*)a->out; p.ldo = a->ldo;
  p.nseq = a->nseq; p.lq = a->lq; p.heads = a->heads; p.mask = a->mask; p.lk = a->lk;
  p.k_seq_stride = a->k_seq_stride; p.v_seq_stride = a->v_seq_stride; p.frames = a->frames; p.ctx_batches = a->ctx_batches; p.batch0 = a->batch0;
  const int nctx = a->mask == 0 ? a->nseq : a->ctx_batches;
  p.k_rows_total = nctx * a->k_seq_stride;
  p.vt_cols_total = (long)nctx * a->v_seq_stride;
  p.v_rows = a->v_rows ? 1 : 0;
  if (a->v_rows && (a->mask != 0 || a->head_dim != 64 || a->dtype == TT_F32 || a->fp8 || a->qx))
    TT_FAIL(TT_EUNSUPPORTED, "tt_attention: v_rows (V not transposed) serves spatial self-attention (mask 0), head_dim 64, 16-bit storage");
  if (!a->v_rows && p.vt_cols_total > a->ldvt) TT_FAIL(TT_EINVAL, "tt_attention: ldvt smaller than the key columns");
  if (a->v_rows && a->ldvt < (long)a->heads * a->head_dim) TT_FAIL(TT_EINVAL, "tt_attention: v_rows needs ldvt >= heads * head_dim");
  {
    const long kb = ((long)(p.k_rows_total - 1) * a->ldk + (long)a->heads * a->head_dim) * es;
    const long vb = a->v_rows ? ((long)(p.vt_cols_total - 1) * a->ldvt + (long)a->heads * a->head_dim) * es
                              : ((long)(a->heads * a->head_dim - 1) * a->ldvt + p.vt_cols_total) * es;
    if (kb >= (1L << 31) || vb >= (1L << 31)) TT_FAIL(TT_EUNSUPPORTED, "tt_attention: K or V^T larger than 2 GiB");
    p.k_bytes = (unsigned)kb; p.vt_bytes = (unsigned)vb;
  }
  p.scale_log2e = 1.4426950408889634f / sqrtf((float)a->head_dim);
  p.qx = (const char*)a->qx; p.ldqx = a->ldqx; p.wq = (const char*)a->wq; p.ldwq = a->ldwq; p.bq = a->bq; p.qc = a->qc; p.ln_eps = a->ln_eps;
  p.qx_bytes = p.wq_bytes = 0;
  if (a->qx) {
    const long xb = (((long)a->nseq * a->lq - 1) * a->ldqx + a->qc) * 2, wb = (((long)a->heads * 64 - 1) * a->ldwq + a->qc) * 2;
    if (xb >= (1L << 31) || wb >= (1L << 31)) TT_FAIL(TT_EUNSUPPORTED, "tt_attention: x or Wq larger than 2 GiB");
    p.qx_bytes = (unsigned)xb; p.wq_bytes = (unsigned)wb;
  }
  return TT_OK;
}
}  // namespace

extern "C" int tt_attention(const TtAttnArgs* a, tt_stream_t stream) {
  AttnP p;
  if (const int rc = attn_params(a, p)) return rc;
  const AttnInst inst = attn_inst(*a);
  bool launched = false;
  for_tag_dim(a->dtype, a->head_dim, [&](auto tag, auto dim) { launched = launch_attention<decltype(tag), decltype(dim)::value>(inst, p, (hipStream_t)stream); });
  if (!launched) TT_FAIL(TT_EUNSUPPORTED, "tt_attention: no kernel instance for this route, dtype and head_dim");
  TT_CHECK_LAUNCH("tt_attention");
  return TT_OK;
}

extern "C" int tt_attention_kernel(const TtAttnArgs* a, char* name, int32_t cap) {
  AttnP p;
  if (const int rc = attn_params(a, p)) return rc;
  return attn_inst_name(attn_inst(*a), a->dtype, name, cap);
}

extern "C" int tt_temporal_attention(const void* qkv, int64_t ldqkv, void* out, int64_t ldo, int32_t batch, int32_t frames,
                                     int32_t hw, int32_t heads, int32_t head_dim, int32_t dtype, tt_stream_t stream) {
  if (!qkv || !out) TT_FAIL(TT_EINVAL, "tt_temporal_attention: null operand");
  if (head_dim != 64 && head_dim != 128) TT_FAIL(TT_EUNSUPPORTED, "tt_temporal_attention: head_dim %d", head_dim);
  if (frames <= 0 || frames > 32) TT_FAIL(TT_EUNSUPPORTED, "tt_temporal_attention: frames %d (1..32)", frames);
  if (dtype != TT_BF16 && dtype != TT_F16 && dtype != TT_F32) TT_FAIL(TT_EINVAL, "tt_temporal_attention: bad dtype");
  if (((ldqkv * (dtype == TT_F32 ? 4 : 2)) & 15) || ((ldo * (dtype == TT_F32 ? 4 : 2)) & 15)) TT_FAIL(TT_EINVAL, "tt_temporal_attention: strides");
  if ((((size_t)qkv | (size_t)out) & 15)) TT_FAIL(TT_EINVAL, "tt_temporal_attention: qkv and out must start on 16-byte boundaries");
  hipStream_t st = (hipStream_t)stream;
  const TattnRoute route = resolve_temporal(dtype, head_dim, frames);
  for_tag_dim(dtype, head_dim, [&](auto tag, auto dim) {
    typedef decltype(tag) Tag;
    constexpr int D = decltype(dim)::value;
    if constexpr (D == 64 && Elem<Tag>::ES == 2) {
      if (route.mfma) { launch_tattn_mfma<Tag>(qkv, ldqkv, out, ldo, batch, frames, hw, heads, st); return; }
    }
    if (route.lpu == 16) launch_tattn<Tag, D, 16>(qkv, ldqkv, out, ldo, batch, frames, hw, heads, st);
    else launch_tattn<Tag, D, 32>(qkv, ldqkv, out, ldo, batch, frames, hw, heads, st);
  });
  TT_CHECK_LAUNCH("tt_temporal_attention");
  return TT_OK;
}

// tt_encoder_attention: validation first (nothing is launched on a refused problem), then one kernel instance per (tag, head_dim, causal).
extern "C" int tt_encoder_attention(const TtEncAttnArgs* a, tt_stream_t stream) {
  if (!a || !a->q || !a->k || !a->v || !a->out) TT_FAIL(TT_EINVAL, "tt_encoder_attention: null operand");
  if (a->nseq <= 0 || a->l <= 0 || a->heads <= 0) TT_FAIL(TT_EINVAL, "tt_encoder_attention: empty problem");
  if (a->head_dim != 64 && a->head_dim != 80) TT_FAIL(TT_EUNSUPPORTED, "tt_encoder_attention: head_dim %d (64 or 80)", a->head_dim);
  if (a->dtype != TT_BF16 && a->dtype != TT_F16 && a->dtype != TT_F32) TT_FAIL(TT_EINVAL, "tt_encoder_attention: bad dtype");
  if (a->causal != 0 && a->causal != 1) TT_FAIL(TT_EINVAL, "tt_encoder_attention: causal %d (0 or 1)", a->causal);
  const int es = a->dtype == TT_F32 ? 4 : 2;
  const bool vrows = es == 2;                                  // 16-bit: v is V itself; fp32: v is V^T
  if (((a->ldq * es) & 15) || ((a->ldk * es) & 15) || ((a->ldv * es) & 15) || ((a->ldo * es) & 15) || (!vrows && (((long)a->v_seq_stride * es) & 15)))
    TT_FAIL(TT_EINVAL, "tt_encoder_attention: strides must keep 16-byte chunks aligned");
  if ((((size_t)a->q | (size_t)a->k | (size_t)a->v | (size_t)a->out) & 15))
    TT_FAIL(TT_EINVAL, "tt_encoder_attention: q, k, v and out must start on 16-byte boundaries");
  if (a->l > a->k_seq_stride || a->l > a->v_seq_stride) TT_FAIL(TT_EINVAL, "tt_encoder_attention: l exceeds sequence stride");
  const long c = (long)a->heads * a->head_dim;
  AttnP p = {};
  p.q = (const char*)a->q; p.ldq = a->ldq; p.k = (const char*)a->k; p.ldk = a->ldk;
  p.vt = (const char*)a->v; p.ldvt = a->ldv; p.out = (char*)a->out; p.ldo = a->ldo;
  p.nseq = a->nseq; p.lq = a->l; p.lk = a->l; p.heads = a->heads; p.mask = 0;
  p.k_seq_stride = a->k_seq_stride; p.v_seq_stride = a->v_seq_stride; p.frames = 1; p.ctx_batches = 1; p.batch0 = 0;
  p.v_rows = vrows ? 1 : 0;
  // rows of k (and of a row-major v) / columns of v^T that exist: the last sequence ends with its l-th key (fp32: with the 16-byte chunk that holds it)
  const long k_rows = (long)(a->nseq - 1) * a->k_seq_stride + a->l;
  const long v_ext = (long)(a->nseq - 1) * a->v_seq_stride + (vrows ? a->l : (a->l + 3) / 4 * 4);
  if (a->ldq < c || a->ldk < c || a->ldo < c || (vrows ? a->ldv < c : a->ldv < v_ext))
    TT_FAIL(TT_EINVAL, "tt_encoder_attention: row stride smaller than the row (heads * head_dim; fp32 v^T: the key columns)");
  const long kb = ((k_rows - 1) * a->ldk + c) * es;
  const long vb = vrows ? ((v_ext - 1) * a->ldv + c) * es : ((c - 1) * a->ldv + v_ext) * es;
  if (k_rows >= (1L << 31) || v_ext >= (1L << 31) || kb >= (1L << 31) || vb >= (1L << 31)) TT_FAIL(TT_EUNSUPPORTED, "tt_encoder_attention: K or V larger than 2 GiB");
  p.k_rows_total = (int)k_rows; p.vt_cols_total = v_ext;
  p.k_bytes = (unsigned)kb; p.vt_bytes = (unsigned)vb;
  p.scale_log2e = 1.4426950408889634f / sqrtf((float)a->head_dim);
  const dim3 grid((a->l + QB - 1) / QB, a->heads, a->nseq), block(256);
  hipStream_t st = (hipStream_t)stream;
  auto go = [&](auto tag, auto dh) {
    typedef decltype(tag) Tag;
    constexpr int DH = decltype(dh)::value, D = DH == 64 ? 64 : 128;
    constexpr size_t ring = 2 * (size_t)(2 * KB * D * Elem<Tag>::ES);    // two stages of K tile + V tile; doubles as the output strips
    static_assert(ring <= 160 * 1024, "encoder attention K/V ring exceeds the LDS");
    if (a->causal) launch<enc_attn_kernel<Tag, DH, true>>(grid, block, ring, st, p);
    else launch<enc_attn_kernel<Tag, DH, false>>(grid, block, ring, st, p);
  };
  auto dim = [&](auto tag) {
    if (a->head_dim == 64) go(tag, std::integral_constant<int, 64>{}); else go(tag, std::integral_constant<int, 80>{});
  };
  if (a->dtype == TT_BF16) dim(bf16_tag{}); else if (a->dtype == TT_F16) dim(f16_tag{}); else dim(f32_tag{});
  TT_CHECK_LAUNCH("tt_encoder_attention");
  return TT_OK;
}
