"""numpy restatement of tt_tensor_stats (include/ttvdm.h) that works on the BIT PATTERNS: every value is widened to its fp32 bits with
integer arithmetic, counts and exponent bins come from those bits, extrema from comparing them, the sums from fp64.  Not a test module:
the CPU tests pin it against hand-written cases, the GPU tests pin the kernel against it."""
import numpy as np

THRESHOLDS = (448.0, 65520.0, 16773120.0, 32768.0)
INF = np.uint32(0x7f800000)


def _e4m3_table() -> np.ndarray:
    """fp32 bits of the 256 OCP e4m3 bytes: S.EEEE.MMM, bias 7, no infinity, S.1111.111 = NaN, subnormals m * 2^-9"""
    tab = np.zeros(256, np.uint32)
    for b in range(256):
        s, e, m = (b >> 7) << 31, (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            bits = 0x7fc00000
        elif e == 0:
            bits = int(np.float32(m * 2.0 ** -9).view(np.uint32))         # 0, or a normal fp32 number: m <= 7
        else:
            bits = ((e - 7 + 127) << 23) | (m << 20)
        tab[b] = s | bits
    return tab


_E4M3 = _e4m3_table()


def widen_bits(raw: np.ndarray, dtype: str) -> np.ndarray:
    """storage bits (uint32 for "f32", uint16 for "f16" / "bf16", uint8 for "e4m3"), any shape -> fp32 bits, flattened"""
    raw = np.ascontiguousarray(raw).reshape(-1)
    if dtype == "f32":
        return raw.view(np.uint32).copy()
    if dtype == "bf16":
        return raw.view(np.uint16).astype(np.uint32) << np.uint32(16)
    if dtype == "f16":
        h = raw.view(np.uint16).astype(np.uint32)
        s, e, m = (h >> 15) << 31, (h >> 10) & 31, h & 1023
        normal = s | ((e + 112) << 23) | (m << 13)
        special = s | np.uint32(0x7f800000) | (m << 13)
        # subnormal: m * 2^-24, exact in fp32 (normal there)
        sub = s | (m.astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)
        return np.where(e == 31, special, np.where(e == 0, sub, normal)).astype(np.uint32)
    if dtype == "e4m3":
        return _E4M3[raw.view(np.uint8)]
    raise ValueError(dtype)


def _key(u: np.ndarray) -> np.ndarray:
    """fp32 bits -> uint32 keys ordered like the values, -0 below +0"""
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k: int) -> int:
    return (k & 0x7fffffff) if k >> 31 else (~k & 0xffffffff)


def _f32(bits: int) -> float:
    return float(np.uint32(bits).view(np.float32))


def reference(raw: np.ndarray, dtype: str, thresholds=THRESHOLDS) -> dict:
    """the record of the values whose storage bits are `raw` (only the values to be counted: a strided view is gathered first);
    ``sum_abs`` (fp64 sum of |x| over finite values) is extra: the GPU tests' bound on ``sum`` is stated in it"""
    u = widen_bits(raw, dtype)
    a = u & np.uint32(0x7fffffff)
    nan, inf = a > INF, a == INF
    fin = a < INF
    zero = a == 0
    fnz = fin & ~zero
    rec = dict(count=int(u.size), n_nan=int(nan.sum()), n_pinf=int((inf & (u >> 31 == 0)).sum()), n_ninf=int((inf & (u >> 31 != 0)).sum()),
               n_zero=int(zero.sum()))
    af = a[fnz]
    tb = [int(np.float32(t).view(np.uint32)) for t in thresholds]
    rec["n_ge"] = [int((af >= np.uint32(t)).sum()) for t in tb]
    bins = np.clip((af >> 23).astype(np.int64) - 127 + 40, 0, 63)
    rec["hist"] = [int(c) for c in np.bincount(bins, minlength=64)]
    vals = u[fin].view(np.float32).astype(np.float64)
    rec["sum"] = float(vals.sum())
    rec["sum_sq"] = float((vals * vals).sum())
    rec["sum_abs"] = float(np.abs(vals).sum())
    rec["max_abs"] = _f32(int(af.max())) if af.size else 0.0
    rec["min_abs_nonzero"] = _f32(int(af.min())) if af.size else float("inf")
    k = _key(u[fin])
    rec["max_val"] = _f32(_unkey(int(k.max()))) if k.size else float("-inf")
    rec["min_val"] = _f32(_unkey(int(k.min()))) if k.size else float("inf")
    return rec


def merge(r0: dict, r1: dict) -> dict:
    """the record of the two value sets together, from their records (what accumulate computes)"""
    out = {k: r0[k] + r1[k] for k in ("count", "n_nan", "n_pinf", "n_ninf", "n_zero", "sum", "sum_sq", "sum_abs")}
    out["n_ge"] = [x + y for x, y in zip(r0["n_ge"], r1["n_ge"])]
    out["hist"] = [x + y for x, y in zip(r0["hist"], r1["hist"])]
    out["max_abs"], out["min_abs_nonzero"] = max(r0["max_abs"], r1["max_abs"]), min(r0["min_abs_nonzero"], r1["min_abs_nonzero"])
    bits = lambda v: int(_key(np.array([np.float32(v).view(np.uint32)], np.uint32))[0])
    out["max_val"] = max((r0["max_val"], r1["max_val"]), key=bits)
    out["min_val"] = min((r0["min_val"], r1["min_val"]), key=bits)
    return out


EXACT_FIELDS = ("count", "n_nan", "n_pinf", "n_ninf", "n_zero", "n_ge", "hist", "max_abs", "min_abs_nonzero", "max_val", "min_val")


def same_float(x: float, y: float) -> bool:
    """bit equality of two fp32 values held as Python floats (tells -0 from +0)"""
    return np.float32(x).view(np.uint32) == np.float32(y).view(np.uint32)


def assert_matches(got: dict, ref: dict, what="") -> None:
    """every integer field and every extremum equal; sum_sq within 2 n 2^-53 ref, sum within 2 n 2^-53 sum|x| -- bounds that hold for
    ANY summation order of n fp64 additions (error <= (n - 1) u sum|terms| to first order, u = 2^-53; the factor 2 covers the higher
    orders and the reference's own rounding), because the square of an fp32 value is exact in fp64"""
    for f in EXACT_FIELDS:
        g, r = got[f], ref[f]
        if isinstance(r, float):
            assert same_float(g, r), f"{what}: {f}: got {g!r}, expected {r!r}"
        else:
            assert g == r, f"{what}: {f}: got {g!r}, expected {r!r}"
    n = max(ref["count"], 1)
    bound = 2.0 * n * 2.0 ** -53
    assert abs(got["sum_sq"] - ref["sum_sq"]) <= bound * ref["sum_sq"], f"{what}: sum_sq {got['sum_sq']!r} vs {ref['sum_sq']!r}"
    assert abs(got["sum"] - ref["sum"]) <= bound * ref["sum_abs"], f"{what}: sum {got['sum']!r} vs {ref['sum']!r} (sum|x| {ref['sum_abs']!r})"
