"""Attention operands whose correct output is known in closed form, for every attention entry point of include/ttvdm.h (tt_attention,
tt_temporal_attention, tt_encoder_attention): the builders, the expectations with their bounds, and a CPU emulation of the kernels'
arithmetic that tests/test_attention_closed_forms_cpu.py turns against itself (mutants).  Needs no GPU and imports no library build.

Three operand families, every value exact in the route's operand type (fp8: e4m3 -- odd multiples of 1/4 up to +-2, codes +-2^k):

F1  uniform weights (key accounting).  Q = 0 (fused query projection: constant x rows, a weight whose rows sum to zero and bq = 0, so the
    projected row is exactly 0; temporal: the Q columns of qkv are 0), so every valid key has weight exactly 1.  V holds 0 / 1 patterns that name the key: key j sets
    channel (j + 3 head + 5 seq) % 32 and channel 32 + (j // 32 + head) % 32 (head dimension 128 / 80: the pattern repeats from channel 64).
    expected = count_c / n_keys in fp64; causal: n_keys = r + 1, the count over j <= r.
    Bound |out - expected| <= (UNIT[storage] + 4 U) expected, zeros exactly zero:  the scores are exact zeros, P = exp2(0) = 1 (fp8: 8),
    the row sum n (8 n) and the PV sums count (8 count) are small integers, exact in fp32 in any order.  What is left is the reciprocal
    1 / l (one rounding, U), its product with the sum (U), the store rounding (UNIT[storage]; fp32 storage: none beyond the product) and
    one U each for a reciprocal that is not correctly rounded and for a division written as two steps: 4 U.  The per-lane temporal
    kernel normalises P before PV (p = fl(1 / n), acc += p v in fp32): its sum of `count` equal terms is not exact; the emulation below
    runs that order, and the CPU test shows it inside the same bound for every frame count of the test.

F2  selection (pairing, masking, the rescale path).  K row j is 2 H_c for the keys j of an "interesting" set I (first and last key of every
    64-key tile; keys 15, 16, 31, 32 of the first and of the last tile -- the lane sub-blocks of mask_ragged; lk - 1, lk - 2) and 0 elsewhere;
    H = Sylvester Hadamard rows (d = 80: an order-64 row in columns 0..63, the order-16 row c % 16 in 64..79, so two codes overlap in at
    most 16 of 80 columns); the code of a key is rotated per head and per context, so a read of the neighbouring head's K selects another
    key.  Query r is 2 H_c of key I[(r + 3 head + 5 seq) % |I|].  The selected score 4 d / sqrt(d) exceeds every other valid key's by
    32 nats (d = 64), 45 (128), 28.6 (80: the others reach 4 * 16 / sqrt(80)); assert_margin() checks  n_keys exp(-margin) < 2^-30  in fp64 from the storage values.  A
    selected key in a later tile outgrows the lazy softmax reference by 2^46: the slow path of softmax_rescale.  V = non-zero dyadics.
    expected = V[sel(r)] of the query's own head and context: BIT FOR BIT in 16-bit storage (the winner's P is 1 +- 2^-19 and rounds to 1,
    the others' 2^-46 vanish below half an ulp of any non-zero dyadic), within 2^-18 relative in fp32 storage (the reference point is
    fl(s c) with s c ~ 46 in exp2 units: the winner's P is exp2 of at most half an ulp of 46 = 2^-19, and the row sum carries the same P).
    Causal: sel(r) <= r with sel(r) = r (the diagonal) wherever r is in I, and trap keys: T_t (t < 4, among the last keys outside I) carries
    4 H of the code of key I[t], so every query r < T_t that selects I[t] has a key of its own code behind it.  (A reduction of "a trap for
    every query": the keys are shared by a sequence's queries, so a trap bars the queries behind it from its code; queries that select one
    of I's other keys have no trap -- the diagonal, F1's per-query key count and the causal_ge mutant cover the mask for them.)  Cross-attention: every context has its own V, so the output names the context a query saw.

F3  two levels (scale, P rounding, the fast path off the maximum).  The keys of F2 with K = H_c and Q = beta H_c: the selected key sits
    g = beta sqrt(d) nats above a zero background (d = 80: above at most g / 5), exp(g) comparable with n_keys.  V = non-zero dyadics; the
    reference is an fp64 softmax of the storage values.  Bound per element
        (u_P + 2^-18) sum_j p_j |v_jc|  +  UNIT[storage] |ref|
    - u_P sum p |v|: P enters the PV product rounded to the operand type (bf16 2^-8, fp16 2^-11, e4m3 2^-4, fp32 0), each p_j v_jc off by at
      most u_P of itself, while the row sum adds the UNROUNDED P (attn_kernel: `psum += e[r]` before pack_chunk), so nothing cancels and
      nothing else enters: sum_j |dp_j| |v_jc| / l <= u_P sum_j p_j |v_jc|.
    - 2^-18 sum p |v|: the exponent fl(s c) - m is an fp32 FMA of exact scores (<= 2^-24 relative of <= 20 exp2 units: 2^-19.7 absolute,
      2^-20.2 relative in P), v_exp_f32 (1 ulp), c = fl(log2 e / sqrt d) (2^-24 of the same exponent); the fp32 sums of l and O
      (<= 2^-24 per addition, a few tens of additions of which one term dominates).  Each is first order <= 2^-20; 2^-18 holds them all.
    - UNIT[storage] |ref|: the store rounding (and 1 / l and its product in fp32 storage).
    split16 (TT_F32 with tt_gemm_set_f32_split): P = 2^8 h + 2^-3 l with h = fp16(2^-8 P), l = fp16(8 P - 2048 h) (common.h split_f16x4).
    For P >= 2^-6 both halves are normal fp16: the pair carries P to 2^-22 relative, and the dropped l x l product is another 2^-22 of
    p v: 2^-21.  Below 2^-6, h is a subnormal and the pair carries P to the ABSOLUTE 2^-28 (the spacing 2^-24 of l, scaled by 2^-3, halved):
    relative 2^-28 / P <= 2^-28 e^g for the background.  u_P(split16) = 2^-21 + 2^-28 e^g.  Q, K and V split exactly (few-bit dyadics).
    fp8: the background 8 exp(-g) stays >= 2^-6, e4m3's smallest normal (assert_fp8_range), inside the route's documented range.
    Threshold cases: beta chosen so that a lane's partial row sum of the selected key's tile (t >= 1, reference 0 from tile 0) lands
    just under / just over PSUM_OK (16384; fp8 448): the same answer with and without the slow path; the emulation reports which ran.

Layout contracts (F1 and F2; each gives the bits of the plain run): poisoned padding (sequence strides larger than lk, the K rows and V
rows / columns in [lk, stride) hold 4 H of a selected code and +-256: a key read from there wins and the output reads +-256), strided
row views (q / qx / out = rows [cls::cb] of a wider buffer, sentinel rows in between stay untouched), batch0 (launches of batches
[1, 3) and [2, 3) give the rows of the full launch).

The emulation (emulate): fp32 scores, the lazy softmax reference per 64-key tile and 32-query wave exactly as attention.hip runs it
(optimistic pass, slow path when a lane's partial sum exceeds PSUM_OK), unrounded P in the row sum, P rounded to the route's type in
PV, fl(1 / l), store rounding.  It reads the SAME buffers the GPU test passes, with the addressing of include/ttvdm.h written out
again here (keys past the end of a buffer read as zeros, as through the kernels' buffer descriptors), so a mutant that lets a padding
key or the next sequence's first key in sees what a kernel with that defect would see."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests import error_bounds as eb

KB = 64                                   # keys per tile (attention.hip)
WAVE = 32                                 # queries per wave
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
TAG = {"bf16": "bf16_tag", "f16": "f16_tag", "f32": "f32_tag"}
FP8 = torch.float8_e4m3fn
U_P = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "fp8": 2.0 ** -4, "f32": 0.0}
LOG2E = 1.4426950408889634
POISON, SENTINEL = 256.0, 7.0
F64 = torch.float64
MUTANTS = ("drop_last", "leak_next", "double", "unmasked", "scale", "no_batch0", "causal_ge")


# ---------------------------------------------------------------------------------------------- codes, sets, values
def hadamard(n: int) -> torch.Tensor:
    h = torch.ones(1, 1, dtype=F64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n
    return h


def codes(d: int, n: int, first: int = 0) -> torch.Tensor:
    """n code rows of +-1, [n, d]; row i is Hadamard row first + i"""
    i = torch.arange(first, first + n)
    if d == 80:
        assert first + n <= 64
        return torch.cat([hadamard(64)[i], hadamard(16)[i % 16]], 1)
    assert first + n <= d
    return hadamard(d)[i]


def interesting(lk: int):
    nt = (lk + KB - 1) // KB
    s = set()
    for t in range(nt):
        s |= {t * KB, min(t * KB + KB - 1, lk - 1)}
    for t in (0, nt - 1):
        s |= {t * KB + o for o in (15, 16, 31, 32) if t * KB + o < lk}
    s |= {j for j in (lk - 1, lk - 2) if j >= 0}
    return sorted(s)


def dyadics(shape, seed: int) -> torch.Tensor:
    """non-zero odd-or-even multiples of 1/4 up to +-2 (exact in e4m3), seeded"""
    rng = np.random.RandomState(seed)
    v = rng.randint(1, 9, size=shape) / 4.0 * (rng.randint(0, 2, size=shape) * 2 - 1)
    return torch.from_numpy(v).to(F64)


def key_patterns(nctx: int, lk: int, heads: int, d: int) -> torch.Tensor:
    """F1's V [nctx, lk, heads, d] of 0 / 1"""
    v = torch.zeros(nctx, lk, heads, 64, dtype=F64)
    c, j, h = torch.meshgrid(torch.arange(nctx), torch.arange(lk), torch.arange(heads), indexing="ij")
    v[c, j, h, (j + 3 * h + 5 * c) % 32] = 1.0
    v[c, j, h, 32 + (j // 32 + h) % 32] = 1.0
    return torch.cat([v, v[..., :d - 64]], -1) if d > 64 else v


def ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def beta_for(d: int, n_keys: int, temporal: bool = False) -> float:
    """F3's query scale (exact in e4m3): g = beta sqrt(d) with exp(g) comparable with n_keys, the selected weight 0.4 .. 0.7"""
    if temporal:
        return {64: 0.375, 128: 0.25}[d] if n_keys > 8 else {64: 0.25, 128: 0.1875}[d]      # g = 3 / 2.83 nats over <= 32 frames, 2 / 2.1 over <= 8
    if n_keys <= 8:
        return {64: 0.25, 128: 0.1875, 80: 0.25}[d]
    if n_keys < 100:
        return {64: 0.5, 128: 0.375, 80: 0.5}[d]
    return {64: 0.75, 128: 0.5, 80: 0.625}[d]


# ---------------------------------------------------------------------------------------------- logical operands and expectations
def _key_code(i, h, c, n):
    return (i + h + 2 * c) % n


def _logical(family, *, d, lk, lq, seq_ids, ctx_of, nctx, heads, beta, causal=False, code0=0, seed=0):
    """Q [nseq, lq, heads, d] (None for F1), K, V [nctx, lk, heads, d], sel [nseq, lq, heads] key index (F2 / F3); fp64 storage values.
    seq_ids: the sequences' indices in the full problem (a batch0 launch is a slice of it); ctx_of [nseq, lq]."""
    I = interesting(lk)
    n = len(I)
    H = codes(d, n, code0)
    ks, qs = (1.0, beta) if family == "F3" else (2.0, 2.0)
    It = torch.tensor(I)
    K = torch.zeros(nctx, lk, heads, d, dtype=F64)
    for c in range(nctx):
        for h in range(heads):
            K[c, It, h] = ks * H[_key_code(torch.arange(n), h, c, n)]
    nseq = len(seq_ids)
    r = torch.arange(lq)
    # causal F2: trap keys.  Trap t sits at T_t, one of the last keys outside I, and carries 4 H of the code of key I[t] (t < 4): every query
    # r < T_t that selects I[t] has a key of its OWN code, twice as loud, behind it.  The keys of a sequence are shared by its queries, so
    # a trap bars the queries at or behind it from selecting its code; with four traps the codes of I's first four keys are covered.
    traps = []
    if causal and family == "F2" and lk >= 50:
        traps = sorted(j for j in range(lk) if j not in I)[-min(4, n - 1):]
        assert all(T > I[t] for t, T in enumerate(traps))
        for t, T in enumerate(traps):
            for c in range(nctx):
                for h in range(heads):
                    K[c, T, h] = 4.0 * H[_key_code(t, h, c, n)]
            if d == 80:
                K[:, T, :, 64:] = 0.0                           # (the order-64 part alone: no overlap with the codes that share its order-16 row)
    seli = torch.zeros(nseq, lq, heads, dtype=torch.long)                   # index into I
    for s, sid in enumerate(seq_ids):
        for h in range(heads):
            if not causal:
                seli[s, :, h] = (r + 3 * h + 5 * sid) % n
            else:
                for q in range(lq):
                    if q in I:
                        seli[s, q, h] = I.index(q)                          # the diagonal
                    else:
                        cand = [i for i, j in enumerate(I) if j <= q and not (i < len(traps) and q >= traps[i])]
                        seli[s, q, h] = cand[(q + 3 * h + 5 * sid) % len(cand)]
    sel = It[seli]
    if family == "F1":
        return None, K, key_patterns(nctx, lk, heads, d), None
    V = dyadics((nctx, lk, heads, d), 1000 + seed)
    Q = torch.zeros(nseq, lq, heads, d, dtype=F64)
    for h in range(heads):
        Q[:, :, h] = qs * H[_key_code(seli[:, :, h], h, ctx_of, n)]
    return Q, K, V, sel


def _softmax_ref(Q, K, V, ctx_of, d, causal):
    """fp64 softmax(Q K^T / sqrt d) V and sum_j p_j |v_jc|, per query with its own context; [nseq, lq, heads, d] each"""
    nseq, lq, heads, _ = Q.shape
    lk = K.shape[1]
    ref, wsum = torch.zeros_like(Q), torch.zeros_like(Q)
    for c in ctx_of.unique().tolist():
        s_idx, q_idx = torch.nonzero(ctx_of == c, as_tuple=True)
        q = Q[s_idx, q_idx]                                                  # [m, heads, d]
        s = torch.einsum("mhd,jhd->mhj", q, K[c]) / math.sqrt(d)
        if causal:
            s = s.masked_fill(torch.arange(lk)[None, None, :] > q_idx[:, None, None], -math.inf)
        p = torch.softmax(s, -1)
        ref[s_idx, q_idx] = torch.einsum("mhj,jhd->mhd", p, V[c])
        wsum[s_idx, q_idx] = torch.einsum("mhj,jhd->mhd", p, V[c].abs())
    return ref, wsum


def _expect(P, family, Q, K, V, sel, ctx_of, d, causal):
    """fills P.expected (+ P.wsum for F3) as [nseq, lq, heads * d]"""
    nseq, lq = ctx_of.shape
    lk = K.shape[1]
    if family == "F1":
        if causal:
            r = torch.arange(lq)
            exp = V.cumsum(1)[ctx_of, r[None, :]] / (r + 1.0)[None, :, None, None]
        else:
            exp = V.sum(1)[ctx_of] / float(lk)
    elif family == "F2":
        h = torch.arange(V.shape[2])
        exp = V[ctx_of[:, :, None], sel, h[None, None, :]]
    else:
        exp, wsum = _softmax_ref(Q, K, V, ctx_of, d, causal)
        P.wsum = wsum.reshape(nseq * lq, -1)
    P.expected = exp.reshape(nseq * lq, -1)


def margin(Q, K, sel, ctx_of, d, causal):
    """the smallest lead in nats of the selected key over every other valid key, fp64"""
    lk = K.shape[1]
    worst = math.inf
    for c in ctx_of.unique().tolist():
        s_idx, q_idx = torch.nonzero(ctx_of == c, as_tuple=True)
        s = torch.einsum("mhd,jhd->mhj", Q[s_idx, q_idx], K[c]) / math.sqrt(d)
        if causal:
            s = s.masked_fill(torch.arange(lk)[None, None, :] > q_idx[:, None, None], -math.inf)
        top = s.gather(-1, sel[s_idx, q_idx][..., None])
        worst = min(worst, float((top - s.scatter(-1, sel[s_idx, q_idx][..., None], -math.inf)).min()))
    return worst


def assert_margin(P):
    """F2: n_keys exp(-margin) < 2^-30, from the storage values in fp64"""
    assert P.family == "F2"
    if P.n_keys > 1:
        assert P.n_keys * math.exp(-P.margin) < 2.0 ** -30, (P.name, P.margin)


def assert_fp8_range(P):
    """F3 on the fp8 route: the background weight 8 exp(-g) is a normal e4m3 value"""
    assert P.ptype == "fp8" and P.family == "F3"
    assert 8.0 * math.exp(-P.g) >= 2.0 ** -6, (P.name, P.g)


def _store(t64, name, fp8=False):
    t = t64.to(FP8) if fp8 else t64.to(DT[name])
    assert torch.equal(t.to(F64), t64), "operand not exact in its storage type"
    return t


def _new(entry, family, name, dt, **kw):
    return SimpleNamespace(entry=entry, family=family, name=name, dt=dt, store=DT[dt], ptype=dt, wsum=None, margin=None, g=None, cb=1, cls=0,
                           causal=False, prenorm=False, psum_ok=16384.0, gain=1.0, kernel=None, **kw)


# ---------------------------------------------------------------------------------------------- tt_attention
def attention(family, *, dt, d=64, lk, mask=0, fp8=False, v_rows=False, qproj=False, split=False, nbatch=None, heads=2, lq=130, frames=2,
              ctx_batches=1, batch0=0, poison=False, cb=1, cls=0, beta=None):
    """A tt_attention problem.  mask 0: nseq = 2 sequences; masks 1 / 2: batches [batch0, ctx_batches) of `frames` sequences each."""
    assert not (qproj and mask == 0) and not ((fp8 or v_rows) and mask != 0)
    if mask == 0:
        nseq, nctx, seq_ids = 2, 2, [0, 1]
        ctx_of = torch.arange(nseq)[:, None].expand(nseq, lq).contiguous()
    else:
        nb = ctx_batches - batch0 if nbatch is None else nbatch
        nseq, nctx = nb * frames, ctx_batches
        seq_ids = list(range(batch0 * frames, batch0 * frames + nseq))
        b = batch0 + torch.arange(nseq)[:, None] // frames
        ctx_of = b.expand(nseq, lq).contiguous() if mask == 1 else (b * lq + torch.arange(lq)[None, :]) % ctx_batches
    if qproj:
        heads = 5
    c = heads * d
    split_mode = bool(split)                                   # the process-wide switch of the launch (tt_gemm_set_f32_split)
    split = split_mode and d == 64                             # the instance: head dimension 128 keeps the exact-fp32 MFMA in split16 mode (u_P = 0)
    beta = beta_for(d, lk) if beta is None else beta
    code0 = 1 if qproj else 0                                   # fused projection: zero-sum codes (no Hadamard row 0), see below
    Q, K, V, sel = _logical(family, d=d, lk=lk, lq=lq, seq_ids=seq_ids, ctx_of=ctx_of, nctx=nctx, heads=heads, beta=beta, code0=code0, seed=mask)
    name = f"attention-{family}-{dt}-d{d}-lk{lk}-mask{mask}" + "".join(f"-{k}" for k, v in dict(fp8=fp8, vrows=v_rows, qproj=qproj, split16=split_mode, poison=poison).items() if v)
    if mask:
        name += f"-cb{ctx_batches}-b0{batch0}"
    if cb > 1:
        name += f"-view{cls}of{cb}"
    P = _new("attention", family, name, dt, mask=mask, fp8=fp8, v_rows=v_rows, qproj=qproj, split=split, split_mode=split_mode, d=d, n_keys=lk)
    P.cb, P.cls = cb, cls
    P.ptype = "fp8" if fp8 else dt
    if fp8:
        P.psum_ok, P.gain = 448.0, 8.0
    P.g = beta * math.sqrt(d)
    P.u_p = U_P[P.ptype] + ((2.0 ** -21 + 2.0 ** -28 * math.exp(P.g)) if split else 0.0)
    m = 16 if fp8 else 8
    if poison:
        kstride = vstride = ceil_to(lk, m) + m
    else:
        vstride = ceil_to(lk, m)
        kstride = lk if (mask == 0 and not v_rows) else vstride
    tag = TAG[dt]
    tf = {True: "true", False: "false"}
    if fp8:
        P.kernel = f"attn8_kernel<{tag}, {d}>"
    elif v_rows and lk >= 2 * KB and lk % KB == 0:
        P.kernel = f"attn_pipe_kernel<{tag}>"
    else:
        P.kernel = f"attn_kernel<{tag}, {d}, {mask}, {tf[qproj]}, {tf[v_rows]}, {tf[split]}>"
    # ---- the buffers
    I = interesting(lk)
    n = len(I)
    H = codes(d, n, code0)

    def padded(t, stride, pad_rows):                           # [nctx, lk, heads, d] -> [nctx * stride, c]
        out = torch.zeros(nctx, stride, heads, d, dtype=F64)
        out[:, :lk] = t
        if poison:
            out[:, lk:] = pad_rows(stride - lk)
        return out.reshape(nctx * stride, c)

    def k_pad(np_):
        t = torch.arange(np_)
        return torch.stack([torch.stack([4.0 * H[_key_code(t % n, h, cc, n)] for h in range(heads)], 1) for cc in range(nctx)], 0)

    def v_pad(np_):
        sign = 1.0 - 2.0 * (torch.arange(np_) % 2).to(F64)
        return (POISON * sign)[None, :, None, None].expand(nctx, np_, heads, d)

    kb, vb = padded(K, kstride, k_pad), padded(V, vstride, v_pad)
    bufs = {}
    if v_rows:
        bufs["kv"] = _store(torch.cat([kb, vb], 1), dt)        # K | V as a fused projection leaves them: k = kv[:, :c], v = kv[:, c:]
    else:
        bufs["k"] = _store(kb, dt, fp8)
        bufs["vt"] = _store(vb.t().contiguous(), dt, fp8)       # [c, nctx * vstride]
    rows = nseq * lq
    if qproj:
        # x slab h of query row r holds the +-1 code the head's query should carry (a zero-sum Hadamard row: mean 0, variance 1, so
        # LN(x) = x / sqrt(1 + eps)); Wq head h = (2 or beta) I on slab h.  Q = (2 or beta) code / sqrt(1 + eps), which rounds to the exact
        # (2 or beta) code in 16-bit storage.  The kernel never centres x -- it computes (x Wq^T) rstd + bq and expects the mean folded into
        # the packed weight (rows that sum to zero) -- which is moot for these rows, whose mean is exactly 0.
        # F1: constant rows (row r holds (1 + r % 4) / 4: variance exactly 0) against a FOLDED weight, row k = 2 e_k - 2 e_(k ^ 1): every row of Wq
        # sums to zero, so x Wq^T is an exact 0 and with bq = 0 the projected query is exactly 0.
        qc = 64 * heads
        if family == "F1":
            x = ((1.0 + torch.arange(rows) % 4) / 4.0).to(F64)[:, None].expand(rows, qc)
        else:
            x = (Q / Q.abs().amax()).reshape(rows, qc)
        w = torch.zeros(c, qc, dtype=F64)
        w[torch.arange(c), torch.arange(c)] = 2.0 if family != "F3" else beta
        if family == "F1":
            w[torch.arange(c), torch.arange(c) ^ 1] = -2.0
        idx = torch.arange(c)
        perm = (idx & ~12) | ((idx & 4) << 1) | ((idx & 8) >> 1)        # packing.permute_q_rows
        xw = torch.full((rows * cb, qc), SENTINEL, dtype=F64)
        xw[cls::cb] = x
        bufs["qx"], bufs["wq"], bufs["bq"] = _store(xw, dt), _store(w[perm].contiguous(), dt), torch.zeros(c, dtype=torch.float32)
        P.w_logical, P.ln_eps = w, 1e-5
        if family != "F1":                                       # the queries the kernel forms, rounded to storage
            xc = x - x.mean(1, keepdim=True)
            q_true = (xc / torch.sqrt(xc.pow(2).mean(1, keepdim=True) + P.ln_eps)) @ w.t()
            Q = q_true.to(DT[dt]).to(F64).reshape(nseq, lq, heads, d)
    else:
        qw = torch.full((rows * cb, c), SENTINEL, dtype=F64)
        qw[cls::cb] = 0.0 if family == "F1" else Q.reshape(rows, c)
        bufs["q"] = _store(qw, dt, fp8)
    P.bufs = bufs
    P.kw = dict(nseq=nseq, lq=lq, heads=heads, head_dim=d, mask=mask, lk=lk, k_seq_stride=kstride, v_seq_stride=vstride, frames=frames,
                ctx_batches=max(ctx_batches, 1), batch0=batch0)
    P.rows, P.c = rows, c
    if family == "F2":
        P.margin = margin(Q, K, sel, ctx_of, d, False)
    _expect(P, family, Q, K, V, sel, ctx_of, d, False)
    return P


# ---------------------------------------------------------------------------------------------- tt_encoder_attention
def encoder(family, *, dt, d=64, l, causal=False, poison=False, beta=None, nseq=2, heads=2):
    c = heads * d
    ctx_of = torch.arange(nseq)[:, None].expand(nseq, l).contiguous()
    beta = beta_for(d, l) if beta is None else beta
    Q, K, V, sel = _logical(family, d=d, lk=l, lq=l, seq_ids=list(range(nseq)), ctx_of=ctx_of, nctx=nseq, heads=heads, beta=beta, causal=causal, seed=7)
    name = f"encoder-{family}-{dt}-d{d}-l{l}" + ("-causal" if causal else "") + ("-poison" if poison else "")
    P = _new("encoder", family, name, dt, d=d, n_keys=l)
    P.causal, P.g, P.u_p = causal, beta * math.sqrt(d), U_P[dt]
    P.kernel = f"enc_attn_kernel<{TAG[dt]}, {d}, {'true' if causal else 'false'}>"
    f32 = dt == "f32"
    kstride = l + 8 if poison else l
    vstride = (ceil_to(l, 4) + (4 if poison else 0)) if f32 else kstride
    I = interesting(l)
    n = len(I)
    H = codes(d, n)

    def padded(t, stride, fill):
        out = torch.zeros(nseq, stride, heads, d, dtype=F64)
        out[:, :l] = t
        if poison and stride > l:
            out[:, l:] = fill(stride - l)
        return out.reshape(nseq * stride, c)

    def k_pad(np_):
        t = torch.arange(np_)
        return torch.stack([torch.stack([4.0 * H[_key_code(t % n, h, s, n)] for h in range(heads)], 1) for s in range(nseq)], 0)

    def v_pad(np_):
        sign = 1.0 - 2.0 * (torch.arange(np_) % 2).to(F64)
        return (POISON * sign)[None, :, None, None].expand(nseq, np_, heads, d)

    kb, vb = padded(K, kstride, k_pad), padded(V, vstride, v_pad)
    # the buffers end where the entry point says they may: with the last sequence's l-th key (fp32 V^T: with the 16-byte chunk that holds it)
    k_rows = (nseq - 1) * kstride + l
    bufs = {"q": _store(torch.zeros(nseq * l, c, dtype=F64) if family == "F1" else Q.reshape(nseq * l, c), dt)}
    if f32:
        bufs["k"] = _store(kb[:k_rows].contiguous(), dt)
        bufs["vt"] = _store(vb.t()[:, :(nseq - 1) * vstride + ceil_to(l, 4)].contiguous(), dt)
    else:
        bufs["kv"] = _store(torch.cat([kb, vb], 1)[:k_rows].contiguous(), dt)
    P.bufs = bufs
    P.kw = dict(nseq=nseq, l=l, heads=heads, head_dim=d, causal=causal, k_seq_stride=kstride, v_seq_stride=vstride)
    P.rows, P.c = nseq * l, c
    if family == "F2":
        P.margin = margin(Q, K, sel, ctx_of, d, causal)
    _expect(P, family, Q, K, V, sel, ctx_of, d, causal)
    return P


# ---------------------------------------------------------------------------------------------- tt_temporal_attention
def temporal(family, *, dt, d=64, frames, poison=False, beta=None, batch=2, hw=5, heads=3):
    """unit (b, pixel p, head h) selects frame (p + h + b) % frames for every one of its query frames"""
    c = heads * d
    beta = beta_for(d, frames, True) if beta is None else beta
    ks, qs = (1.0, beta) if family == "F3" else (2.0, 2.0)
    H = codes(d, frames)
    b_, f_, p_, h_ = torch.meshgrid(torch.arange(batch), torch.arange(frames), torch.arange(hw), torch.arange(heads), indexing="ij")
    K = ks * H[(f_ + h_) % frames]                                           # [batch, frames, hw, heads, d]
    sel = (p_ + h_ + b_) % frames
    Q = qs * H[(sel + h_) % frames]
    if family == "F1":
        # key = frame, "sequence" = the unit's (b, p): the patterns of key_patterns with the unit index in place of the sequence
        V = key_patterns(batch * hw, frames, heads, d).view(batch, hw, frames, heads, d).permute(0, 2, 1, 3, 4).contiguous()
        Q = torch.zeros_like(Q)
    else:
        V = dyadics((batch, frames, hw, heads, d), 2000 + frames)
    name = f"temporal-{family}-{dt}-d{d}-f{frames}" + ("-poison" if poison else "")
    P = _new("temporal", family, name, dt, d=d, n_keys=frames)
    P.g, P.u_p = beta * math.sqrt(d), U_P[dt]
    P.mfma = dt != "f32" and d == 64 and frames <= 16
    P.prenorm = not P.mfma                                                   # tattn_kernel: p = e / sum before PV, fp32 P
    if P.prenorm:
        P.u_p = 0.0
    P.lpu = 16 if frames <= 16 else 32
    rows = batch * frames * hw
    ld = 3 * c + (16 if poison else 0)
    qkv = torch.zeros(rows, ld, dtype=F64)
    qkv[:, :3 * c] = torch.cat([t.reshape(rows, c) for t in (Q, K, V)], 1)
    if poison:
        qkv[:, 3 * c:] = POISON * (1.0 - 2.0 * (torch.arange(16) % 2).to(F64))
    P.bufs = {"qkv": _store(qkv, dt)}
    P.kw = dict(batch=batch, frames=frames, hw=hw, heads=heads, head_dim=d)
    P.rows, P.c = rows, c
    # expectations per unit, fp64
    Qu, Ku, Vu = (t.permute(0, 2, 1, 3, 4) for t in (Q, K, V))             # [batch, hw, frames, heads, d]
    if family == "F1":
        exp = (Vu.sum(2, keepdim=True) / float(frames)).expand_as(Vu)
    elif family == "F2":
        su = sel.permute(0, 2, 1, 3)                                         # [batch, hw, frames, heads]
        exp = torch.gather(Vu, 2, su[..., None].expand_as(Vu))
        s = torch.einsum("bpfhd,bpjhd->bpfhj", Qu, Ku) / math.sqrt(d)
        top = s.gather(-1, su[..., None])
        P.margin = float((top - s.scatter(-1, su[..., None], -math.inf)).min()) if frames > 1 else math.inf
    else:
        p = torch.softmax(torch.einsum("bpfhd,bpjhd->bpfhj", Qu, Ku) / math.sqrt(d), -1)
        exp = torch.einsum("bpfhj,bpjhd->bpfhd", p, Vu)
        P.wsum = torch.einsum("bpfhj,bpjhd->bpfhd", p, Vu.abs()).permute(0, 2, 1, 3, 4).reshape(rows, c)
    P.expected = exp.permute(0, 2, 1, 3, 4).reshape(rows, c)
    return P


# ---------------------------------------------------------------------------------------------- the check
def check(P, got):
    """got [rows, c] (any float type, CPU).  -> (largest err / bound over all elements, message or None).  F2 in 16-bit storage: 0 or inf."""
    got = got.to(F64)
    exp = P.expected
    assert got.shape == exp.shape, (got.shape, exp.shape)
    unit = eb.UNIT[P.store]
    if not bool(torch.isfinite(got).all()):
        return math.inf, f"{P.name}: non-finite output"
    if P.family == "F1":
        bound = (unit + 4 * eb.U) * exp
        if bool((got[exp == 0] != 0).any()):
            return math.inf, f"{P.name}: a zero entry is not exactly zero"
    elif P.family == "F2":
        if P.store != torch.float32:
            bad = got != exp
            if bool(bad.any()):
                i = torch.nonzero(bad)[0].tolist()
                return math.inf, f"{P.name}: {int(bad.sum())} elements differ from V[sel]; first at {i}: got {float(got[tuple(i)])}, expected {float(exp[tuple(i)])}"
            return 0.0, None
        bound = 2.0 ** -18 * exp.abs()
    else:
        bound = (P.u_p + 2.0 ** -18) * P.wsum + unit * exp.abs()
    err = (got - exp).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max())
    if worst > 1.0:
        i = [int(x) for x in np.unravel_index(int(ratio.argmax()), ratio.shape)]
        return worst, f"{P.name}: err/bound {worst:.3g} at {i}: got {float(got[tuple(i)])!r}, expected {float(exp[tuple(i)])!r}"
    return worst, None


# ---------------------------------------------------------------------------------------------- the emulation
def _rnd(t, ptype):
    if ptype == "f32":
        return t.to(torch.float32).to(F64)
    if ptype == "fp8":
        return t.to(torch.float32).clamp(max=448.0).to(FP8).to(F64)
    return t.to(torch.float32).to(DT[ptype]).to(F64)


def _f32(t):
    return t.to(torch.float32).to(F64)


def _tile_softmax_pv(Q, K, V, valid, P, c32):
    """One (sequence, head, context) group through the tile loop of attn_kernel / attn8_kernel / enc_attn_kernel.  Q [nq, d], K / V [nk, d]
    with nk a multiple of 64, valid [nq, nk].  -> (stored output [nq, d], a later tile took the slow path)"""
    nq, d = Q.shape
    nk = K.shape[0]
    pad = (-nq) % WAVE
    if pad:                                                    # rows beyond lq: zero queries, every key "valid" as in the kernel
        Q = torch.cat([Q, torch.zeros(pad, d, dtype=F64)], 0)
        valid = torch.cat([valid, valid[-1:].expand(pad, nk)], 0)
    S = _f32(Q @ K.t()).masked_fill(~valid, -math.inf)
    n = Q.shape[0]
    m = torch.full((n, 1), -1e30, dtype=F64)
    l = torch.zeros(n, 1, dtype=F64)
    o = torch.zeros(n, d, dtype=F64)
    shift = math.log2(P.gain)
    lane = torch.tensor([0] * 16 + [1] * 16 + [0] * 16 + [1] * 16)
    slow_later = False
    for t in range(nk // KB):
        s = S[:, t * KB:(t + 1) * KB]
        vt = V[t * KB:(t + 1) * KB]

        def expo(mref):
            return _f32(torch.exp2(_f32(s * c32 + (shift - mref))))
        p = expo(m)
        psum = torch.stack([p[:, lane == 0].sum(1), p[:, lane == 1].sum(1)], 1)
        trig = (~(psum <= P.psum_ok)).any(1).view(-1, WAVE).any(1)          # per wave
        if bool(trig.any()):
            if t > 0:
                slow_later = True
            rows = trig.repeat_interleave(WAVE)
            mx = s.max(1, keepdim=True).values
            m_new = torch.maximum(m, _f32(mx * c32))
            m_new = torch.where(torch.isnan(m_new), m, m_new)
            alpha = _f32(torch.exp2(m - m_new))
            m = torch.where(rows[:, None], m_new, m)
            l = torch.where(rows[:, None], _f32(l * alpha), l)
            o = torch.where(rows[:, None], _f32(o * alpha), o)
            p = torch.where(rows[:, None], expo(m), p)
        l = _f32(l + p.sum(1, keepdim=True))
        o = _f32(o + _rnd(p, P.ptype) @ vt)
    inv = torch.where(l > 0, _f32(1.0 / l), torch.zeros_like(l))
    return _rnd(_f32(o * inv), P.dt)[:nq], slow_later


def _full_softmax_pv(Q, K, V, valid, P, c32):
    """the temporal kernels: one pass over at most 32 keys, the true maximum as the reference"""
    s = _f32(_f32(Q @ K.t()) * c32).masked_fill(~valid, -math.inf)
    e = _f32(torch.exp2(_f32(s - s.max(1, keepdim=True).values)))
    tot = _f32(e.sum(1, keepdim=True))
    inv = _f32(1.0 / tot)
    if P.prenorm:                                              # tattn_kernel: p_j = e_j / sum, acc = fma(p_j, v_j, acc) key by key in fp32
        acc = torch.zeros(Q.shape[0], V.shape[1], dtype=F64)
        for j in range(K.shape[0]):
            if bool(valid[:, j].any()):
                acc = _f32(acc + _f32(e[:, j:j + 1] * inv) * V[j:j + 1])
        return _rnd(acc, P.dt)
    return _rnd(_f32((_rnd(e, P.ptype) @ V) * inv), P.dt)


def _rows_or_zeros(buf, r0, n, cols):
    """rows r0 .. r0 + n of a [rows, >= cols.stop] buffer as fp64, zeros past its end (the buffer descriptor's answer)"""
    out = torch.zeros(n, cols.stop - cols.start, dtype=F64)
    have = max(0, min(n, buf.shape[0] - r0))
    if have:
        out[:have] = buf[r0:r0 + have, cols].to(F64)
    return out


def emulate(P, mutant=None):
    """-> (stored output [rows, c] fp64, a later tile took the slow path).  mutant: one of MUTANTS (a kernel defect), or None."""
    assert mutant is None or mutant in MUTANTS
    d, kw = P.d, P.kw
    c32 = float(np.float32(np.float32(LOG2E) / np.sqrt(np.float32(d)))) * (1.01 if mutant == "scale" else 1.0)
    out = torch.zeros(P.rows, P.c, dtype=F64)
    slow = False

    def key_valid(nq, nk, lk, qrows=None):
        j = torch.arange(nk)[None, :]
        v = (j < lk).expand(nq, nk).clone()
        if mutant == "drop_last":
            v[:, lk - 1] = False
        if mutant == "leak_next":
            v[:, lk] = True
        if mutant == "unmasked":
            v[:] = True
        if P.causal:
            r = qrows[:, None]
            v &= (j < r) if mutant == "causal_ge" else (j <= r)
        return v

    def doubled(K, V, valid, lk, ext):
        """key lk // 2 counted twice: its copy takes the place of a masked slot, or of the first slot of `ext` further ones"""
        if mutant != "double":
            return K, V, valid
        j = lk // 2
        if lk == K.shape[0]:
            K, V = (torch.cat([t, torch.zeros(ext, t.shape[1], dtype=F64)]) for t in (K, V))
            valid = torch.cat([valid, torch.zeros(valid.shape[0], ext, dtype=torch.bool)], 1)
        K, V, valid = K.clone(), V.clone(), valid.clone()
        K[lk], V[lk], valid[:, lk] = K[j], V[j], valid[:, j]
        return K, V, valid

    if P.entry == "temporal":
        batch, frames, hw, heads = kw["batch"], kw["frames"], kw["hw"], kw["heads"]
        c = heads * d
        qkv = P.bufs["qkv"].to(F64)
        nk = 16 if P.mfma else P.lpu
        if mutant == "leak_next" and frames == nk:
            nk += 1
        for b in range(batch):
            for p in range(hw):
                rows = (b * frames + torch.arange(frames)) * hw + p
                for h in range(heads):
                    Q = qkv[rows, h * d:(h + 1) * d]
                    K = torch.zeros(nk, d, dtype=F64)
                    V = torch.zeros(nk, d, dtype=F64)
                    K[:frames], V[:frames] = qkv[rows, c + h * d:c + (h + 1) * d], qkv[rows, 2 * c + h * d:2 * c + (h + 1) * d]
                    valid = key_valid(frames, nk, frames)
                    K, V, valid = doubled(K, V, valid, frames, 1)
                    out[rows, h * d:(h + 1) * d] = _full_softmax_pv(Q, K, V, valid, P, c32)
        return out, False

    lk = kw["lk"] if P.entry == "attention" else kw["l"]
    lq = kw["lq"] if P.entry == "attention" else kw["l"]
    nseq, heads = kw["nseq"], kw["heads"]
    kstride, vstride = kw["k_seq_stride"], kw["v_seq_stride"]
    nk = ceil_to(lk + (1 if mutant == "leak_next" else 0), KB)
    if "kv" in P.bufs:
        kbuf, vbuf = P.bufs["kv"][:, :P.c], P.bufs["kv"][:, P.c:]
    else:
        kbuf, vbuf = P.bufs["k"], P.bufs["vt"].t()                          # V^T [c, columns]: key j of a context is column base + j
    if P.entry == "attention" and P.qproj:
        # the kernel's own order: (x W^T) rstd + bq with rstd from E[x^2] - E[x]^2, rounded to the storage type
        x = P.bufs["qx"][P.cls::P.cb].to(F64)
        mean, sq = x.mean(1, keepdim=True), x.pow(2).mean(1, keepdim=True)
        rs = 1.0 / torch.sqrt((sq - mean * mean).clamp_min(0) + P.ln_eps)
        qall = _rnd(_f32(_f32(x @ P.w_logical.t()) * _f32(rs)), P.dt)
    else:
        qall = P.bufs["q"][P.cls::P.cb].to(F64)
    mask = P.mask if P.entry == "attention" else 0
    b0 = 0 if (mutant == "no_batch0" or mask == 0) else kw["batch0"]
    for seq in range(nseq):
        if mask == 0:
            classes = [(torch.arange(lq), seq)]
        else:
            b = b0 + seq // kw["frames"]
            cbn = kw["ctx_batches"]
            classes = [(torch.arange(lq), b)] if mask == 1 else [(torch.arange(cl, lq, cbn), (b * lq + cl) % cbn) for cl in range(cbn) if cl < lq]
        for qrows, ctx in classes:
            for h in range(heads):
                cols = slice(h * d, (h + 1) * d)
                Q = qall[seq * lq + qrows, cols]
                K = _rows_or_zeros(kbuf, ctx * kstride, nk, cols)
                V = _rows_or_zeros(vbuf, ctx * vstride, nk, cols)
                valid = key_valid(len(qrows), nk, lk, qrows)
                K, V, valid = doubled(K, V, valid, lk, KB)
                o, s = _tile_softmax_pv(Q, K, V, valid, P, c32)
                out[seq * lq + qrows, cols] = o
                slow |= s
    return out, slow


# ---------------------------------------------------------------------------------------------- one launch on the device
def run(ops, P, dev="cuda"):
    """-> (output rows [rows, c] on the CPU, the whole output buffer incl. sentinel rows on the CPU, kernel instance name or None)"""
    b = {k: v.to(dev) for k, v in P.bufs.items()}
    wide = torch.full((P.rows * P.cb, P.c), SENTINEL, dtype=P.store, device=dev)
    out = wide[P.cls::P.cb]
    name = None
    if P.entry == "attention":
        k, v = (b["kv"][:, :P.c], b["kv"][:, P.c:]) if P.v_rows else (b["k"], b["vt"])
        extra = dict(qx=b["qx"][P.cls::P.cb], wq=b["wq"], bq=b["bq"], ln_eps=P.ln_eps) if P.qproj else {}
        q = None if P.qproj else b["q"][P.cls::P.cb]
        ops.set_f32_split(P.split_mode)
        ops.PROFILE = []
        try:
            ops.attention(q, k, v, out, v_rows=P.v_rows, **extra, **P.kw)
            torch.cuda.synchronize()
            name = ops.PROFILE[-1][0]
        finally:
            ops.PROFILE = None
            ops.set_f32_split(False)
    elif P.entry == "encoder":
        k, v = (b["kv"][:, :P.c], b["kv"][:, P.c:]) if "kv" in b else (b["k"], b["vt"])
        ops.encoder_attention(b["q"], k, v, out, **P.kw)
    else:
        ops.temporal_attention(b["qkv"], out, **P.kw)
    torch.cuda.synchronize()
    w = wide.cpu()
    return w[P.cls::P.cb], w, name


# ---------------------------------------------------------------------------------------------- the route shapes both test modules walk
FAMILIES = ("F1", "F2", "F3")


def _route(rid, make, **kw):
    r = SimpleNamespace(id=rid, make=make, entry=rid.split("-")[0], views=False, batch0=False, causal=False, fp8=False, unmasked=True, temporal=False,
                        families=FAMILIES, slow_later=None)
    r.__dict__.update(kw)
    return r


def routes():
    """Every route shape of the issue: .make(family, **variant) builds the problem; .views / .batch0: the layout contracts that apply beyond
    poisoned padding (which applies to all); .slow_later (threshold cases, F3 only): whether a tile after the first must take the slow path."""
    out = []

    def attn(rid, views=False, **kw):
        lk = kw["lk"]
        out.append(_route("attention-" + rid, lambda fam, **v: attention(fam, **{**kw, **v}), views=views, fp8=bool(kw.get("fp8")), unmasked=lk % KB != 0,
                          batch0=bool(kw.get("mask")) and kw.get("ctx_batches") == 3))

    for d in (64, 128):
        for dt, split in (("bf16", False), ("f16", False), ("f32", False), ("f32", True)):
            for lk in (40, 64, 150, 200):
                attn(f"plain-{dt}{'-split16' if split else ''}-d{d}-lk{lk}", views=lk == 150, dt=dt, d=d, lk=lk, split=split)
    for dt in ("bf16", "f16"):
        for lk in (64, 150):
            attn(f"vrows-{dt}-lk{lk}", views=lk == 150, dt=dt, lk=lk, v_rows=True)
        for lk in (128, 192, 256):
            attn(f"pipe-{dt}-lk{lk}", views=lk == 192, dt=dt, lk=lk, v_rows=True)
        for d in (64, 128):
            for lk in (64, 150):
                attn(f"fp8-{dt}-d{d}-lk{lk}", views=lk == 150, dt=dt, d=d, lk=lk, fp8=True)
    for mask in (1, 2):
        for s in (1, 5, 78):
            for cbn in (2, 3):
                for dt in ("bf16", "f16", "f32"):
                    attn(f"cross-{dt}-mask{mask}-s{s}-cb{cbn}", views=s == 78 and cbn == 3, dt=dt, lk=s, mask=mask, ctx_batches=cbn)
                for dt in ("bf16", "f16"):
                    attn(f"qproj-{dt}-mask{mask}-s{s}-cb{cbn}", views=s == 78 and cbn == 3, dt=dt, lk=s, mask=mask, ctx_batches=cbn, qproj=True)
    for frames in (1, 4, 14, 16, 17, 25, 32):
        for d in (64, 128):
            for dt in ("bf16", "f16", "f32"):
                lpu = 16 if frames <= 16 else 32
                out.append(_route(f"temporal-{dt}-d{d}-f{frames}", lambda fam, dt=dt, d=d, frames=frames, **v: temporal(fam, dt=dt, d=d, frames=frames, **v),
                                  unmasked=frames < lpu, temporal=True))
    for l in (1, 50, 77, 130, 257):
        for d in (64, 80):
            for causal in (False, True):
                for dt in ("bf16", "f16", "f32"):
                    out.append(_route(f"encoder-{dt}-d{d}-l{l}{'-causal' if causal else ''}",
                                      lambda fam, dt=dt, d=d, l=l, causal=causal, **v: encoder(fam, dt=dt, d=d, l=l, causal=causal, **v),
                                      causal=causal, unmasked=l % KB != 0))
    # F3 just under / just over the slow-path threshold of each tile kernel: e^g + 31 against PSUM_OK 16384 (g = 9.5 / 10), fp8 8 (e^g + 31) against 448 (g = 3 / 3.5)
    for over, b16, b8 in ((False, 1.1875, 0.375), (True, 1.25, 0.4375)):
        w = "over" if over else "under"
        for dt in ("bf16", "f16"):
            for rid, kw in ((f"plain-{dt}-lk200", dict(dt=dt, lk=200, beta=b16)), (f"pipe-{dt}-lk192", dict(dt=dt, lk=192, v_rows=True, beta=b16)),
                            (f"fp8-{dt}-lk150", dict(dt=dt, lk=150, fp8=True, beta=b8))):
                out.append(_route(f"attention-{rid}-threshold-{w}", lambda fam, kw=kw, **v: attention(fam, **{**kw, **v}), families=("F3",), slow_later=over,
                                  fp8=bool(kw.get("fp8"))))
            out.append(_route(f"encoder-{dt}-d64-l130-threshold-{w}", lambda fam, dt=dt, b=b16, **v: encoder(fam, dt=dt, l=130, beta=b, **v), families=("F3",), slow_later=over))
    return out


def mutants_for(route, P):
    """the defects that change what this route shape computes (the others leave it bit for bit alone, or are another route's)"""
    m = ["drop_last"] + (["double"] if P.n_keys > 1 else [])          # (a single key counted twice is the same softmax)
    if not route.causal:
        m.append("leak_next")
        if route.unmasked:
            m.append("unmasked")
    else:
        m.append("causal_ge")
    if P.n_keys > 1 and not route.fp8:
        m.append("scale")                  # (fp8: u_P = 2^-4 hides a 1 % scale error; F1 and F2 do not depend on the scale)
    if P.entry == "attention" and P.mask != 0 and P.kw["batch0"] > 0:
        m.append("no_batch0")
    return m
