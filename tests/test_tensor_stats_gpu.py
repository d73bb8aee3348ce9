"""GPU: tt_tensor_stats against the bit-pattern reference (tests/tensor_stats_reference.py).  Every integer field and every extremum
must be equal; sum_sq within 2 n 2^-53 ref and sum within 2 n 2^-53 sum|x| (bounds for any summation order, derived in
tensor_stats_reference.assert_matches).  Shapes are the smallest at which each route of the kernel can go wrong: one element, a ragged
row, a padded view (scalar route), a padded view whose rows allow 16-byte loads (row route), a misaligned base, several workgroups (the
partials + finalize launches), more 16-byte loads than one grid has lanes plus a ragged tail (the grid-stride loop), no rows at all,
and one tensor of more than 2^31 elements."""
import numpy as np
import pytest
import torch

from tests import tensor_stats_reference as R
from this_and_that_vdm_amd import audit, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "e4m3": torch.float8_e4m3fn}
BITS = {"f32": torch.int32, "f16": torch.int16, "bf16": torch.int16, "e4m3": torch.uint8}
NP_BITS = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16, "e4m3": np.uint8}


def planted_f32():
    """NaN, +-inf, +-0, subnormals, the ends of the histogram, and the values just below, at and above each threshold"""
    out = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1e-40, -1e-45, 2.0 ** -41, 2.0 ** -40, 2.0 ** 23, 3e38, -3.3e38, 65504.0, 65519.9]
    for t in R.THRESHOLDS:
        t32 = np.float32(t)
        out += [float(np.nextafter(t32, np.float32(0))), float(t32), float(np.nextafter(t32, np.float32(np.inf))), -float(t32)]
    return out


def make_values(dtype: str, n: int, seed: int) -> torch.Tensor:
    """n values of `dtype` on the device as storage bits (an int tensor): a wide spread of magnitudes with the planted values scattered in"""
    rng = np.random.default_rng(seed)
    if dtype == "e4m3":
        return torch.from_numpy(rng.integers(0, 256, n, dtype=np.uint8)).to(DEV)          # every byte: NaN, +-0, subnormals, +-448 included
    v = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 18, n))).astype(np.float32)
    plant = np.array(planted_f32(), np.float32)
    pos = rng.choice(n, size=min(n, plant.size), replace=False)
    v[pos] = plant[:pos.size]
    t = torch.from_numpy(v).to(DEV).to(DTYPES[dtype])          # (rounding to the 16-bit types moves the planted values; the reference reads the result)
    if dtype == "f16" and n >= 4:                              # fp16's own subnormals and its largest value
        t.view(torch.int16)[:4] = torch.tensor([0x0001, -0x8000 + 0x03ff, 0x7bff, 0x0400], dtype=torch.int16, device=DEV)
    return t.view(BITS[dtype])


def stats_of(t: torch.Tensor, **kw) -> dict:
    return audit.decode(ops.tensor_stats(t, **kw))[0]


def ref_of(bits: torch.Tensor, dtype: str) -> dict:
    return R.reference(bits.contiguous().cpu().numpy().view(NP_BITS[dtype]), dtype)


def view_case(dtype: str, shape, ld: int, offset: int, seed: int):
    """a [rows, cols] view with row stride ld starting `offset` elements into its buffer; everything outside the view holds NaN / 1e30"""
    rows, cols = shape
    buf = torch.empty(offset + rows * ld + 16, dtype=BITS[dtype], device=DEV).view(DTYPES[dtype])
    if dtype == "e4m3":
        buf.view(torch.uint8).fill_(0x7f)                      # NaN
    else:
        buf[0::2] = float("nan")
        buf[1::2] = 1e30
    view = buf[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    vals = make_values(dtype, rows * cols, seed).view(rows, cols)
    view.view(BITS[dtype]).copy_(vals)
    return view, vals


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("shape,ld,offset", [
    ((1, 1), 1, 0), ((1, 7), 7, 0), ((3, 8), 8, 0),
    ((5, 9), 16, 0),                   # padded rows, ragged columns: the scalar route
    ((64, 320), 320, 0),               # several workgroups: partials + finalize
    ((64, 320), 336, 0),               # padded rows that still allow 16-byte loads: the row route
    ((130, 1283), 1283, 1),            # the base one element into the buffer: misaligned, scalar route
], ids=lambda v: str(v).replace(" ", ""))
def test_matches_reference(dtype, shape, ld, offset):
    view, vals = view_case(dtype, shape, ld, offset, seed=shape[0] * 1000 + shape[1])
    assert view.data_ptr() % 16 == (offset * view.element_size()) % 16
    got, ref = stats_of(view), ref_of(vals, dtype)
    R.assert_matches(got, ref, f"{dtype} {shape} ld {ld} offset {offset}")
    assert got["n_nan"] + got["n_pinf"] + got["n_ninf"] + got["n_zero"] + sum(got["hist"]) == got["count"] == shape[0] * shape[1]


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_grid_stride_loop_and_ragged_tail(dtype):
    """more 16-byte loads than grid x block lanes, so the loop runs more than once, and a tail that fills no whole load"""
    max_grid, block, per_load = ops.tensor_stats_launch(DTYPES[dtype])
    n = (max_grid * block + 3 * block + 37) * per_load + per_load - 1
    assert n // per_load > max_grid * block and n % per_load
    bits = make_values(dtype, n, seed=11)
    R.assert_matches(stats_of(bits.view(DTYPES[dtype]).view(1, n)), ref_of(bits, dtype), f"{dtype} flat {n}")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_no_rows(dtype):
    empty = audit.decode(audit.empty_record().tobytes())[0]
    x = torch.empty((0, 8), dtype=BITS[dtype], device=DEV).view(DTYPES[dtype])
    assert stats_of(x) == empty and stats_of(torch.empty((4, 0), device=DEV)) == empty
    rec = ops.tensor_stats(make_values(dtype, 100, 5).view(DTYPES[dtype]))
    before = audit.decode(rec)[0]
    ops.tensor_stats(x, out=rec, accumulate=True)              # accumulating nothing leaves the record as it is
    assert audit.decode(rec)[0] == before and before["count"] == 100


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_accumulate_equals_the_concatenation(dtype):
    a, b = make_values(dtype, 64 * 320, 21), make_values(dtype, 5 * 9, 22)
    buf = torch.zeros(3 * ops.STATS_BYTES, dtype=torch.uint8, device=DEV)
    ops.tensor_stats(a.view(DTYPES[dtype]), out=buf, slot=1)
    rec = ops.tensor_stats(b.view(DTYPES[dtype]), out=buf, slot=1, accumulate=True)
    assert rec.data_ptr() == buf.data_ptr() + ops.STATS_BYTES
    R.assert_matches(audit.decode(rec)[0], ref_of(torch.cat([a, b]), dtype), f"{dtype} accumulate")
    assert not buf[:ops.STATS_BYTES].any() and not buf[2 * ops.STATS_BYTES:].any()          # the neighbouring slots are untouched
    # ... and into the empty record, which is how the audit starts every slot
    buf2 = torch.from_numpy(np.frombuffer(audit.empty_record().tobytes(), np.uint8).copy()).to(DEV)
    ops.tensor_stats(a.view(DTYPES[dtype]), out=buf2, accumulate=True)
    assert audit.decode(buf2)[0] == audit.decode(ops.tensor_stats(a.view(DTYPES[dtype])))[0]


def test_two_calls_give_identical_bytes():
    max_grid, block, per_load = ops.tensor_stats_launch(torch.bfloat16)
    x = make_values("bf16", max_grid * block * per_load + 12345, 31).view(torch.bfloat16)
    r0, r1 = ops.tensor_stats(x), ops.tensor_stats(x)
    assert torch.equal(r0, r1)
    y = make_values("f32", 130 * 1283, 32).view(torch.float32).view(130, 1283)
    assert torch.equal(ops.tensor_stats(y), ops.tensor_stats(y))


def test_captured_accumulating_launch_replays():
    xs = [make_values("f16", 64 * 320, 40 + i) for i in range(3)]
    x = torch.zeros(64, 320, dtype=torch.float16, device=DEV)
    rec = torch.from_numpy(np.frombuffer(audit.empty_record().tobytes(), np.uint8).copy()).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm-up outside the capture (the workspace of the stream)
        ops.tensor_stats(x, out=torch.empty_like(rec))
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.tensor_stats(x, out=rec, accumulate=True)
    assert audit.decode(rec)[0]["count"] == 0                   # capturing launched nothing
    for v in xs:
        x.view(torch.int16).copy_(v.view(64, 320))
        graph.replay()
    R.assert_matches(audit.decode(rec)[0], ref_of(torch.cat(xs), "f16"), "three replays")


def test_more_than_2_31_elements():
    """bf16 zeros with a handful of planted values in the last rows; the expected record is the planted rows' plus the zeros before them"""
    rows, cols = (1 << 21) + 8, 1024
    assert rows * cols > 1 << 31
    x = torch.zeros((rows, cols), dtype=torch.bfloat16, device=DEV)
    tail = x[-2:]
    tail[0, 5], tail[0, 1000], tail[1, 0], tail[1, 7], tail[1, 1023] = 3.0, -5.0, float("inf"), float("nan"), 70000.0
    tail[1, 1022], tail[0, 0] = -2.0 ** -30, -0.0
    ref = R.reference(tail.view(torch.int16).cpu().numpy().view(np.uint16), "bf16")
    ref["count"] += (rows - 2) * cols
    ref["n_zero"] += (rows - 2) * cols
    got = stats_of(x)
    R.assert_matches(got, ref, "2^31 + 8192 bf16 elements")
    assert (got["n_pinf"], got["n_nan"], got["max_abs"], got["min_val"], got["n_zero"]) == (1, 1, 70144.0, -5.0, rows * cols - 6)
    del x
    torch.cuda.empty_cache()


def test_refusals_name_the_cause():
    x = torch.zeros(8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="thr\\[1\\] = -1"):
        ops.tensor_stats(x, thresholds=(1.0, -1.0, 2.0, 3.0))
    with pytest.raises(RuntimeError, match="NaN"):
        ops.tensor_stats(x, thresholds=(1.0, 1.0, float("nan"), 3.0))
    with pytest.raises(RuntimeError, match="last dimension must be contiguous"):
        ops.tensor_stats(x.t())
    with pytest.raises(RuntimeError, match="collapse to one row stride"):
        ops.tensor_stats(torch.zeros(4, 6, 8, device=DEV)[:, :3, :5])
    with pytest.raises(RuntimeError, match="float8_e4m3fn, got torch.int32"):
        ops.tensor_stats(x.view(torch.int32))
    with pytest.raises(RuntimeError, match="accumulate needs"):
        ops.tensor_stats(x, accumulate=True)
    with pytest.raises(RuntimeError, match="holding record 1"):
        ops.tensor_stats(x, out=torch.zeros(ops.STATS_BYTES, dtype=torch.uint8, device=DEV), slot=1)
    # the C entry point's own refusals
    import ctypes as C
    from this_and_that_vdm_amd import _lib
    lib, thr = _lib.load(), (C.c_float * 4)(*ops.STATS_THRESHOLDS)
    rec = torch.zeros(ops.STATS_BYTES + 8, dtype=torch.uint8, device=DEV)
    big = torch.zeros(64, 320, device=DEV)
    call = lambda *a: (lib.tt_tensor_stats(*a), lib.tt_last_error().decode())
    assert call(big.data_ptr(), 320, 64, 320, 2, thr, rec.data_ptr(), None, 0, 0, None)[0] == -1 and "workspace" in lib.tt_last_error().decode()
    code, msg = call(big.data_ptr(), 100, 64, 320, 2, thr, rec.data_ptr(), None, 0, 0, None)
    assert code == -1 and "row stride 100 < cols 320" in msg
    code, msg = call(big.data_ptr(), 320, 64, 320, 7, thr, rec.data_ptr(), None, 0, 0, None)
    assert code == -1 and "bad dtype 7" in msg
    code, msg = call(big.data_ptr(), 320, 64, 320, 2, thr, rec.data_ptr() + 4, None, 0, 0, None)
    assert code == -1 and "rec is not 8-byte aligned" in msg
    code, msg = call(big.data_ptr(), 320, -1, 320, 2, thr, rec.data_ptr(), None, 0, 0, None)
    assert code == -1 and "negative" in msg
    torch.cuda.synchronize()
    assert not rec.any()                                        # a refused call launched nothing
