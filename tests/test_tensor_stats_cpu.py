"""CPU: the numpy reference of tt_tensor_stats against hand-written cases, audit.decode / RangeAuditReport on fabricated records, and
the ctypes mirror of TtTensorStats against the sizes and offsets include/ttvdm.h writes down."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from tests import tensor_stats_reference as R
from this_and_that_vdm_amd import _lib, audit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def f32(*vals):
    return np.array(vals, np.float32).view(np.uint32)


def test_reference_counts_classes_and_extrema():
    sub = float(np.uint32(1).view(np.float32))                  # the smallest fp32 subnormal, 2^-149
    r = R.reference(f32(0.0, -0.0, float("nan"), INF, -INF, sub, 1.0, -3.0, 2.0 ** -41, 2.0 ** 23, 2.0 ** 30), "f32")
    assert (r["count"], r["n_nan"], r["n_pinf"], r["n_ninf"], r["n_zero"]) == (11, 1, 1, 1, 2)
    hist = [0] * 64
    hist[0] = 2                    # the subnormal and 2^-41 (below the first bin's 2^-40)
    hist[40] = 1                   # 1.0
    hist[41] = 1                   # 3.0
    hist[63] = 2                   # 2^23 (bin 63's lower edge) and 2^30 (clamped)
    assert r["hist"] == hist
    assert r["max_abs"] == 2.0 ** 30 and r["min_abs_nonzero"] == sub
    assert r["max_val"] == 2.0 ** 30 and r["min_val"] == -3.0
    assert r["sum"] == 0.0 + sub + 1.0 - 3.0 + 2.0 ** -41 + 2.0 ** 23 + 2.0 ** 30
    assert r["sum_sq"] == 1.0 + 9.0 + 2.0 ** -82 + 2.0 ** 46 + 2.0 ** 60
    assert r["n_ge"] == [2, 2, 1, 2]


def test_reference_thresholds_at_the_edges():
    below_fp16 = float(np.nextafter(np.float32(65520.0), np.float32(0)))          # 65519.996
    r = R.reference(f32(65504.0, below_fp16, 65520.0, -65520.0, 448.0, 448.5, 447.99, 16773120.0, -16773119.0, 32768.0), "f32")
    #             >= 448  >= 65520  >= 65520 * 2^8  >= 32768
    assert r["n_ge"] == [9, 4, 1, 7]
    assert np.float32(65519.9) < np.float32(65520.0) and R.reference(f32(65519.9), "f32")["n_ge"][1] == 0
    # fp16: 65504 is the largest finite value, the next pattern is inf
    r = R.reference(np.array([0x7bff, 0x7c00, 0xfc00, 0x7e00, 0x0001, 0x8000, 0x5f00], np.uint16), "f16")
    assert (r["n_pinf"], r["n_ninf"], r["n_nan"], r["n_zero"]) == (1, 1, 1, 1)
    assert r["max_abs"] == 65504.0 and r["min_abs_nonzero"] == 2.0 ** -24 and r["n_ge"] == [2, 0, 0, 1]       # 0x5f00 = 448.0
    assert r["hist"][40 - 24] == 1 and r["hist"][40 + 15] == 1 and r["hist"][40 + 8] == 1
    # bf16: the top 16 bits of fp32
    r = R.reference(np.array([0x477f, 0x4780, 0x7f80, 0xff80, 0x7fc0, 0x0001], np.uint16), "bf16")            # 65280, 65536, +-inf, NaN, 2^-133
    assert r["n_ge"] == [2, 1, 0, 2] and r["max_abs"] == 65536.0 and r["hist"][0] == 1 and r["n_pinf"] == r["n_ninf"] == r["n_nan"] == 1


def test_reference_e4m3_has_no_infinity_and_clips_at_448():
    r = R.reference(np.array([0x7e, 0xfe, 0x7f, 0xff, 0x00, 0x80, 0x01, 0x38, 0x77], np.uint8), "e4m3")
    # 0x7e = 448, 0xfe = -448, 0x7f / 0xff NaN, +-0, 0x01 = 2^-9 (smallest subnormal), 0x38 = 1.0, 0x77 = 240
    assert (r["n_nan"], r["n_pinf"], r["n_ninf"], r["n_zero"]) == (2, 0, 0, 2)
    assert r["n_ge"][0] == 2 and r["max_abs"] == 448.0 and r["min_abs_nonzero"] == 2.0 ** -9
    assert r["max_val"] == 448.0 and r["min_val"] == -448.0 and r["sum"] == 2.0 ** -9 + 1.0 + 240.0
    vals = R.widen_bits(np.arange(256, dtype=np.uint8), "e4m3").view(np.float32)
    assert vals[0x40] == 2.0 and vals[0x08] == 2.0 ** -6 and vals[0x07] == 7 * 2.0 ** -9 and vals[0xc0] == -2.0
    assert np.isnan(vals[[0x7f, 0xff]]).all() and np.isfinite(np.delete(vals, [0x7f, 0xff])).all()


def test_reference_orders_signed_zeros_and_handles_empty_sets():
    r = R.reference(f32(-0.0, 0.0), "f32")
    assert R.same_float(r["max_val"], 0.0) and R.same_float(r["min_val"], -0.0)
    assert r["max_abs"] == 0.0 and r["min_abs_nonzero"] == INF and r["n_zero"] == 2
    r = R.reference(f32(float("nan"), INF), "f32")
    assert (r["max_abs"], r["min_abs_nonzero"], r["max_val"], r["min_val"]) == (0.0, INF, -INF, INF) and r["sum"] == 0.0
    r = R.reference(np.zeros(0, np.uint32), "f32")
    assert r["count"] == 0 and (r["max_abs"], r["min_abs_nonzero"], r["max_val"], r["min_val"]) == (0.0, INF, -INF, INF)


def test_reference_widens_fp16_like_numpy():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    got = R.widen_bits(h, "f16").view(np.float32)
    want = h.view(np.float16).astype(np.float32)
    fin = np.isfinite(want)
    assert (got[fin].view(np.uint32) == want[fin].view(np.uint32)).all() and (np.isnan(got) == np.isnan(want)).all()
    assert (got[np.isinf(want)] == want[np.isinf(want)]).all()


def test_merge_is_the_record_of_the_union():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(100).astype(np.float32), (rng.standard_normal(57) * 1e5).astype(np.float32)
    b[:3] = [np.nan, np.inf, -0.0]
    ra, rb = R.reference(a.view(np.uint32), "f32"), R.reference(b.view(np.uint32), "f32")
    R.assert_matches(R.merge(ra, rb), R.reference(np.concatenate([a, b]).view(np.uint32), "f32"), "merge")


def test_struct_layout_matches_the_header_comment():
    """the byte offsets include/ttvdm.h writes next to each field, the 616 bytes it states, the ctypes mirror and audit's numpy type"""
    text = open(os.path.join(REPO, "include", "ttvdm.h")).read()
    block = text[text.index("TtTensorStats -- "):text.index("max_val / min_val order the bit patterns")]
    assert int(re.search(r"TtTensorStats -- (\d+) bytes", block).group(1)) == ctypes.sizeof(_lib.TtTensorStats) == audit.STATS_DTYPE.itemsize == 616
    stated = {name: int(off) for off, name in re.findall(r"(?<![a-z_])\[\s*(\d+)\]\s+(?:(?:uint64|double|float)\s+)?([a-z_]+)", block)}
    assert set(stated) == {n for n, _ in _lib.TtTensorStats._fields_}, stated
    for name, _ in _lib.TtTensorStats._fields_:
        assert getattr(_lib.TtTensorStats, name).offset == stated[name] == audit.STATS_DTYPE.fields[name][1], name
    # ... and the C compiler's view of the struct the header declares
    import subprocess
    import tempfile
    fields = [n for n, _ in _lib.TtTensorStats._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ttvdm.h"\nint main(){printf("%zu", sizeof(TtTensorStats));' +
           "".join(f'printf(" %zu", offsetof(TtTensorStats, {n}));' for n in fields) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        nums = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert nums == [616] + [stated[n] for n in fields]


def _record(**kw):
    r = audit.empty_record()
    for k, v in kw.items():
        r[k] = v
    return r


def _row(site, dtype, **kw):
    return dict(site=site, shape=[4, 8], dtype=dtype, record=audit.decode(_record(**kw).tobytes())[0])


def test_decode_round_trips_records():
    hist = np.zeros(64, np.uint64)
    hist[40] = 5
    raw = _record(count=7, n_nan=1, n_zero=1, n_ge=[1, 0, 0, 0], hist=hist, sum=2.5, sum_sq=9.25, max_abs=500.0, min_abs_nonzero=1.0,
                  max_val=500.0, min_val=-1.5).tobytes() + audit.empty_record().tobytes()
    recs = audit.decode(raw)
    assert len(recs) == 2 and audit.decode(raw, 1) == recs[:1]
    a, e = recs
    assert (a["count"], a["n_nan"], a["n_zero"], a["n_ge"], a["hist"][40], sum(a["hist"])) == (7, 1, 1, [1, 0, 0, 0], 5, 5)
    assert (a["sum"], a["sum_sq"], a["max_abs"], a["min_abs_nonzero"], a["max_val"], a["min_val"]) == (2.5, 9.25, 500.0, 1.0, 500.0, -1.5)
    assert all(type(a[k]) is int for k in ("count", "n_nan")) and type(a["sum"]) is float
    assert (e["count"], e["max_abs"], e["min_abs_nonzero"], e["max_val"], e["min_val"]) == (0, 0.0, INF, -INF, INF)
    import torch
    assert audit.decode(torch.from_numpy(np.frombuffer(raw, np.uint8).copy())) == recs
    with pytest.raises(ValueError, match="whole number"):
        audit.decode(raw[:-1])


def _fabricated_report():
    h = lambda **bins: [bins.get(f"b{i}", 0) for i in range(64)]
    rows = [
        _row("unet.a/gemm#0", "f32", count=100, hist=h(b40=90, b10=10), max_abs=3.0, min_abs_nonzero=2.0 ** -30),
        _row("unet.b/gemm#0", "f32", count=100, n_ge=[9, 4, 0, 5], hist=h(b56=4, b45=96), max_abs=70000.0),
        _row("unet.b/attention#0", "e4m3", count=64, n_ge=[3, 0, 0, 0], n_zero=16, hist=h(b48=48), max_abs=448.0),
        _row("unet.c/gemm#0", "f32", count=50, n_ge=[50, 50, 2, 50], hist=h(b63=50), max_abs=3.4e38),
        _row("unet.d/layernorm#0", "f16", count=10, n_pinf=2, n_nan=1, hist=h(b40=7), max_abs=1.0),
    ]
    return audit.RangeAuditReport(rows)


def test_report_verdicts_worst_and_nonfinite():
    rep = _fabricated_report()
    assert [r["site"] for r in rep.nonfinite()] == ["unet.d/layernorm#0"]
    assert [r["site"] for r in rep.worst(2)] == ["unet.c/gemm#0", "unet.b/gemm#0"]
    v = rep.verdict("fp16")
    assert v["first"] == "unet.b/gemm#0" and [(s["site"], s["count"]) for s in v["sites"]] == \
        [("unet.b/gemm#0", 4), ("unet.c/gemm#0", 50), ("unet.d/layernorm#0", 2)]
    assert v["sites"][0]["share"] == 0.04
    assert v["flush_share"] == 10 / (100 + 100 + 48 + 50 + 7)              # bin 10 = [2^-30, 2^-29): below fp16's 2^-25
    v = rep.verdict("bf16")
    assert v["first"] == "unet.c/gemm#0" and v["sites"][0]["count"] is None and len(v["sites"]) == 1 and v["flush_share"] == 0.0
    v = rep.verdict("split16")
    assert v["first"] == "unet.c/gemm#0" and v["sites"][0]["count"] == 2 and v["considered"] == 3
    assert v["flush_share"] == 10 / 250                                    # bin 10 is below 2^-28 as well
    v = rep.verdict("fp8_attention")
    assert v["first"] == "unet.b/attention#0" and v["sites"][0]["count"] == 3 and v["flush_share"] == 16 / 64 and v["considered"] == 1
    with pytest.raises(ValueError):
        rep.verdict("fp4")
    with pytest.raises(RuntimeError, match="65520"):
        audit.RangeAuditReport(rep.rows, thresholds=(1.0, 2.0, 3.0, 4.0)).verdict("fp16")
    assert "unet.b/gemm#0" in rep.table()


def test_report_to_json_is_strict_json():
    rep = _fabricated_report()
    doc = json.loads(rep.to_json(), parse_constant=lambda c: pytest.fail(f"non-standard JSON constant {c}"))
    assert doc["thresholds"] == [448.0, 65520.0, 16773120.0, 32768.0] and [r["site"] for r in doc["rows"]] == rep.sites()
    assert doc["rows"][0]["record"]["max_val"] == "-inf" and doc["rows"][0]["record"]["min_val"] == "inf"
    assert doc["rows"][1]["record"]["n_ge"] == [9, 4, 0, 5] and doc["rows"][1]["shape"] == [4, 8] and doc["rows"][2]["dtype"] == "e4m3"


def test_site_names_are_unique_in_a_step_and_repeat_across_steps():
    """the naming rules, on the host alone: module paths from the hook stack, ordinals per (module, op), regions restarting them"""
    a = audit.RangeAudit()
    a._paths = {1: "unet.blk"}
    assert a.site_name("gemm") == "<top>/gemm#0" and a.site_name("gemm") == "<top>/gemm#1"
    steps = []
    for _ in range(2):
        with a.region("step"):
            names = [a.site_name("gemm")]
            a._stack.append("unet.blk")
            names += [a.site_name("gemm"), a.site_name("gemm"), a.site_name("attention")]
            a._stack.append(None)                     # a module nobody named: the enclosing watched module's name stands
            names.append(a.site_name("gemm"))
            del a._stack[:]
            steps.append(names)
    assert steps[0] == steps[1] == ["<step>/gemm#0", "unet.blk/gemm#0", "unet.blk/gemm#1", "unet.blk/attention#0", "unet.blk/gemm#2"]
    assert a.site_name("gemm") == "<top>/gemm#2"     # after the loop: on from where the calls before it stopped
    assert a.generation < audit.RangeAudit().generation
