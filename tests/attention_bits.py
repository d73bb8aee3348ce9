"""The cases of tests/test_attention_bits_gpu.py, shared with tests/golden/make_attention_bits.py (which records their output hashes from
the library of the commit that is the reference).  Every case is the smallest shape at which one piece the attention kernels share can
go wrong: two query blocks with the second nearly empty (lq = 130), every arm of the tile driver (ragged only / one full tile / two full +
ragged / three full + ragged keys), the slow path of the lazy softmax reference on a later tile, both cross-attention masks with and
without the fused query projection, the row-major-V route on attn_kernel (one tile, ragged) and on attn_pipe_kernel (two, three, four
tiles: both parities of its epilogue), fp8, and the temporal kernels with a unit count that is no multiple of a block's units.

run_case(ops, case) -> (output tensor on the device, fp32 reference on the CPU, rtol, atol); operands are seeded (utils/synthetic.py)."""
import hashlib

import torch
import torch.nn.functional as F

from this_and_that_vdm_amd.utils.synthetic import hash_uniform

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
# the tolerances of tests/test_ops_gpu.py (the neighbouring tests of the same kernels)
TOL = {"f16": 1e-3, "bf16": 1.6e-2, "f32": 2e-5}
NSEQ, HEADS, LQ = 2, 2, 130


def _cases():
    out = []
    for dt in ("bf16", "f16"):
        for d in (64, 128):
            out += [dict(kind="plain", dt=dt, d=d, lk=lk) for lk in (40, 64, 150, 200)]
    out += [dict(kind="plain", dt="f32", d=64, lk=lk, split=sp) for sp in (False, True) for lk in (40, 64, 150, 200)]
    out += [dict(kind="plain", dt="f32", d=128, lk=150)]
    out += [dict(kind="plain", dt="bf16", d=64, lk=200, growth=40.0)]
    out += [dict(kind="cross", dt=dt, mask=m) for dt in ("bf16", "f16", "f32") for m in (1, 2)]
    out += [dict(kind="qproj", dt=dt, mask=m) for dt in ("bf16", "f16") for m in (1, 2)]
    out += [dict(kind="vrows", dt=dt, lk=lk) for dt in ("bf16", "f16") for lk in (64, 128, 192, 256, 150)]
    out += [dict(kind="fp8", dt=dt, d=d, lk=lk) for dt in ("bf16", "f16") for d in (64, 128) for lk in (64, 150)]
    out += [dict(kind="temporal", dt=dt, d=d, frames=f) for dt in ("bf16", "f32") for d in (64, 128) for f in (14, 25)]
    return out


def case_id(c):
    return "-".join(f"{k}={v}" for k, v in c.items())


CASES = _cases()


def _u(*shape, seed, dtype=torch.float32, scale=1.7):
    """seeded uniform values (unit variance at scale 1.7), rounded through the storage type"""
    n = 1
    for s in shape:
        n *= s
    return (hash_uniform(n, seed).view(*shape) * scale).to(dtype)


def _sdpa(q, k, v, heads):
    n, lq, c = q.shape
    d = c // heads
    qh, kh, vh = [t.float().view(t.shape[0], -1, heads, d).transpose(1, 2) for t in (q, k, v)]
    return F.scaled_dot_product_attention(qh, kh, vh).transpose(1, 2).reshape(n, lq, c)


def _vt(v, pad):
    """[n, l, c] -> V^T [c, n * lp] with every sequence padded to a multiple of `pad` columns"""
    n, l, c = v.shape
    lp = (l + pad - 1) // pad * pad
    vt = torch.zeros(c, n * lp, dtype=torch.uint8 if v.dtype == torch.float8_e4m3fn else v.dtype)
    vt.view(c, n, lp)[:, :, :l] = (v.view(torch.uint8) if v.dtype == torch.float8_e4m3fn else v).permute(2, 0, 1)
    return (vt.view(v.dtype) if v.dtype == torch.float8_e4m3fn else vt), lp


def _cross_ref(q, kc, vc, heads, mask, b, f, hw):
    c = q.shape[-1]
    if mask == 1:                                   # frame n sees the context of batch n // f
        return _sdpa(q.view(b * f, hw, c), kc.repeat_interleave(f, 0), vc.repeat_interleave(f, 0), heads)
    sel = (torch.arange(b)[:, None] * hw + torch.arange(hw)[None]) % b          # token (b, p) sees context (b * hw + p) % B
    qt = q.view(b, f, hw, c).permute(0, 2, 1, 3).reshape(b * hw, f, c)
    return _sdpa(qt, kc[sel.reshape(-1)], vc[sel.reshape(-1)], heads).view(b, hw, f, c).permute(0, 2, 1, 3).reshape(b * f, hw, c)


def run_case(ops, case):
    kind, dtype = case["kind"], DT[case["dt"]]
    tol = TOL[case["dt"]]
    if kind == "temporal":
        b, hw, heads, d, frames = 1, 5, 3, case["d"], case["frames"]
        c = heads * d
        qkv = _u(b * frames * hw, 3 * c, seed=1, dtype=dtype)
        out = torch.empty(b * frames * hw, c, dtype=dtype, device="cuda")
        ops.temporal_attention(qkv.cuda(), out, batch=b, frames=frames, hw=hw, heads=heads, head_dim=d)
        t = qkv.view(b, frames, hw, 3, c).permute(3, 0, 2, 1, 4).reshape(3, b * hw, frames, c)
        return out, _sdpa(t[0], t[1], t[2], heads).view(b, hw, frames, c).permute(0, 2, 1, 3).reshape(-1, c), tol, tol
    if kind in ("cross", "qproj"):
        b, f, hw, s, sp, d, mask = 2, 2, LQ, 78, 80, 64, case["mask"]
        heads = 5 if kind == "qproj" else HEADS                                  # qc = 320: five 64-deep slabs
        c = heads * d
        kc, vc = _u(b, s, c, seed=6, dtype=dtype), _u(b, s, c, seed=7, dtype=dtype)
        kpad = torch.zeros(b, sp, c, dtype=dtype)
        kpad[:, :s] = kc
        vt, _ = _vt(vc, 8)
        kw = dict(nseq=b * f, lq=hw, heads=heads, head_dim=d, mask=mask, lk=s, k_seq_stride=sp, v_seq_stride=sp, frames=f, ctx_batches=b)
        out = torch.full((b * f * hw, c), float("nan"), dtype=dtype, device="cuda")
        if kind == "cross":
            q = _u(b * f * hw, c, seed=1, dtype=dtype)
            ops.attention(q.cuda(), kpad.reshape(-1, c).cuda(), vt.cuda(), out, **kw)
            return out, _cross_ref(q.float(), kc.float(), vc.float(), heads, mask, b, f, hw).reshape(-1, c), tol, tol
        from this_and_that_vdm_amd.packing import fold_layernorm, permute_q_rows, zero_sum_round
        x = (_u(b * f * hw, c, seed=1, scale=2.6) + _u(b * f * hw, 1, seed=9)).to(dtype)
        wq = _u(c, c, seed=2, dtype=dtype, scale=1.7 * c ** -0.5)
        g, be = _u(c, seed=4, scale=0.35) + 1, _u(c, seed=5, scale=0.5)
        wf, bf = fold_layernorm(wq.float(), None, g, be)
        wq_p, bq_p = permute_q_rows(zero_sum_round(wf, dtype).cuda()), permute_q_rows(bf.cuda())
        ops.attention(None, kpad.reshape(-1, c).cuda(), vt.cuda(), out, qx=x.cuda(), wq=wq_p, bq=bq_p, ln_eps=1e-5, **kw)
        q_ref = F.linear(F.layer_norm(x.float(), (c,), g, be, 1e-5), wq.float())
        return out, _cross_ref(q_ref, kc.float(), vc.float(), heads, mask, b, f, hw).reshape(-1, c), 2 * tol, 2 * tol     # (test_attention_fused_query_projection's)
    d = case.get("d", 64)
    lk, c = case["lk"], HEADS * d
    q, k, v = _u(NSEQ, LQ, c, seed=1), _u(NSEQ, lk, c, seed=2), _u(NSEQ, lk, c, seed=3)
    if case.get("growth"):                          # key j leans towards query 5 by j / lk * growth: the later tiles outgrow the reference
        ramp = torch.linspace(0.0, 1.0, lk)[None, :, None]
        k = k * 0.3 + ramp * case["growth"] * q[:, 5:6] / q[:, 5:6].norm(dim=-1, keepdim=True) / HEADS ** 0.5
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    kw = dict(nseq=NSEQ, lq=LQ, heads=HEADS, head_dim=d, mask=0, lk=lk, k_seq_stride=lk)
    out = torch.full((NSEQ * LQ, c), float("nan"), dtype=dtype, device="cuda")
    if kind == "fp8":
        q8, k8, v8 = (t.to(ops.FP8) for t in (q, k, v))
        vt, lp = _vt(v8, 16)
        ops.attention(q8.reshape(-1, c).cuda(), k8.reshape(-1, c).cuda(), vt.cuda(), out, v_seq_stride=lp, **kw)
        return out, _sdpa(q8.float(), k8.float(), v8.float(), HEADS).reshape(-1, c), 3e-2, 3e-2          # (test_attention_fp8's)
    if kind == "vrows":
        kv = torch.cat([k, v], dim=2).reshape(NSEQ * lk, 2 * c).cuda()            # K | V as a fused projection leaves them
        ops.attention(q.reshape(-1, c).cuda(), kv[:, :c], kv[:, c:], out, v_seq_stride=lk, v_rows=True, **kw)
    else:
        vt, lp = _vt(v, 8)
        ops.set_f32_split(bool(case.get("split")))
        try:
            ops.attention(q.reshape(-1, c).cuda(), k.reshape(-1, c).cuda(), vt.cuda(), out, v_seq_stride=lp, **kw)
        finally:
            ops.set_f32_split(False)
    return out, _sdpa(q, k, v, HEADS).reshape(-1, c), tol, tol


def output_hash(out):
    torch.cuda.synchronize()
    return hashlib.sha256(out.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()
