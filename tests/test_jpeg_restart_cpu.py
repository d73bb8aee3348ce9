"""CPU: restart intervals in the JPEG export and import -- the format and the host half.  The restatement of
tests/jpeg_restart_reference.py against Pillow (libjpeg-turbo): its files equal ``save(..., restart_marker_blocks / restart_marker_rows)``
byte for byte and its decoder gives Pillow's pixels on them; a frame whose file holds a stuffed byte directly before a marker (FF 00 FF
Dn); tt_jpeg_parse_spans through ctypes: the header field by field, the spans against the restatement's walker, every refusal by code
and text, a marker-less file as one span; the new host routines under the address and undefined-behaviour sanitizers in a stand-alone
program; and ``encode_jpeg``'s argument refusals, which come before any device is touched.

Everything here is equality: a baseline JPEG is integers from end to end."""
import ctypes as C
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_reference as ref
from tests import jpeg_restart_reference as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (h, w, ch, subsampling): one MCU; several MCU rows; odd sizes with dummy blocks; grey; 36 MCUs (17 markers at Ri = 2: the number wraps twice)
SHAPES = [(16, 16, 3, 2), (40, 56, 3, 2), (33, 17, 3, 2), (40, 56, 3, 0), (33, 17, 3, 0), (24, 40, 1, 0), (48, 48, 3, 0)]
SHAPE_IDS = ["16x16-420", "40x56-420", "33x17-420", "40x56-444", "33x17-444", "24x40-grey", "48x48-444"]
QUALITIES = (75, 92)


def intervals_of(h, w, ch, sub):
    """-> [(Ri in MCUs, Pillow's keyword)]: 1, 2, 7 (divides none of the MCU counts), one and two MCU rows, more than the frame has"""
    row, mcus = rr.mcus_per_row(w, ch, sub), rr.mcus_of(h, w, ch, sub)
    return [(1, dict(restart_marker_blocks=1)), (2, dict(restart_marker_blocks=2)), (7, dict(restart_marker_blocks=7)), (row, dict(restart_marker_rows=1)),
            (2 * row, dict(restart_marker_rows=2)), (mcus + 5, dict(restart_marker_blocks=mcus + 5))]


def pillow_file(frame, quality, sub, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(buf, format="JPEG", quality=quality, subsampling=sub, **kw)
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


def frames_of(h, w, ch):
    return {"smooth": ref.smooth_frame(h, w, 1, ch), "noise": ref.noise_frame(h, w, 2, ch)}


# the frame whose Ri = 1 file holds FF 00 FF Dn: a stuffed byte directly before a marker (found by a search over seeds with the restatement)
STUFFED = dict(frame=ref.noise_frame(16, 64, 0, 3), quality=90, sub=0, ri=1)
STUFFED_PATTERN = re.compile(rb"\xff\x00\xff[\xd0-\xd7]")


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


# ---- the restatement against Pillow
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_restatement_writes_pillows_files_and_decodes_them_to_pillows_pixels(shape):
    h, w, ch, sub = shape                          # (Ri = 7 divides 40 x 56's 35 MCUs in 4:4:4 and no other count: no marker behind a full last interval)
    for name, frame in frames_of(h, w, ch).items():
        for quality in QUALITIES:
            for ri, kw in intervals_of(h, w, ch, sub):
                want = pillow_file(frame, quality, sub, **kw)
                got = rr.jpeg_file(frame, quality, sub, ri)
                assert got == want, (name, quality, ri, len(got), len(want))
                at = want.index(b"\xff\xda")
                assert want[at - 6:at] == b"\xff\xdd\x00\x04" + struct.pack(">H", ri)                      # DRI directly before SOS
                hd = rr.parse(want)
                assert hd["ri"] == ri and len(hd["spans"]) == rr.markers_of(h, w, ch, sub, ri) + 1
                pixels, status = rr.decode(want)
                assert status == 0 and np.array_equal(pixels, pillow_pixels(want)), (name, quality, ri)
                assert np.array_equal(pixels, pillow_pixels(pillow_file(frame, quality, sub))), "markers change no pixel"


def test_the_marker_number_wraps_past_seven_twice():
    data = rr.jpeg_file(ref.noise_frame(48, 48, 2, 3), 75, 0, 2)
    hd = rr.parse(data)
    numbers = [data[at + n + 1] - 0xd0 for at, n in hd["spans"][:-1]]
    assert numbers == [k % 8 for k in range(17)]


def test_a_stuffed_byte_directly_before_a_marker():
    data = rr.jpeg_file(STUFFED["frame"], STUFFED["quality"], STUFFED["sub"], STUFFED["ri"])
    ends = {at + n for at, n in rr.parse(data)["spans"][:-1]}
    hits = [m.start() for m in STUFFED_PATTERN.finditer(data) if m.start() + 2 in ends]
    assert hits, "the file no longer holds FF 00 FF Dn in front of a real marker: find another seed"
    assert data == pillow_file(STUFFED["frame"], STUFFED["quality"], STUFFED["sub"], restart_marker_blocks=1)
    pixels, status = rr.decode(data)
    assert status == 0 and np.array_equal(pixels, pillow_pixels(data))


def library_tables(counts):
    from this_and_that_vdm_amd import export
    return [(t.bits, t.huffval) for t in (export.jpeg_optimized_table(counts[k]) for k in range(4))]


def test_optimized_tables_count_with_the_predictor_resets(lib):
    """the counts differ from the marker-less counts, and Pillow decodes the restatement's optimized files to the restatement's pixels"""
    frame = ref.smooth_frame(40, 56, 1, 3)
    coefs, comps, _ = ref.coefficients(frame, 75, 2)
    assert not np.array_equal(rr.symbol_counts(coefs, comps, 6), ref.symbol_counts(coefs, comps))
    assert np.array_equal(rr.symbol_counts(coefs, comps, 0), ref.symbol_counts(coefs, comps))
    data = rr.jpeg_file(frame, 75, 2, 4, tables=library_tables)
    pixels, status = rr.decode(data)
    assert status == 0 and np.array_equal(pixels, pillow_pixels(data))


# ---- tt_jpeg_parse_spans
def _parse_spans(lib, data):
    from this_and_that_vdm_amd import _lib
    hd = _lib.TtJpegHeader()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    ri, count = C.c_int32(-1), C.c_int64(-1)
    rc = lib.tt_jpeg_parse_spans(buf.ctypes.data if buf.size else None, buf.size, C.byref(hd), C.byref(ri), None, None, 0, C.byref(count))
    if rc != 0:
        return rc, lib.tt_last_error().decode(), hd, ri.value, []
    offs, lens = np.full(count.value, -1, dtype=np.int64), np.full(count.value, -1, dtype=np.int64)
    rc = lib.tt_jpeg_parse_spans(buf.ctypes.data, buf.size, C.byref(hd), C.byref(ri), offs.ctypes.data, lens.ctypes.data, count.value, C.byref(count))
    return rc, lib.tt_last_error().decode(), hd, ri.value, list(zip(offs.tolist(), lens.tolist()))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_parse_spans_reads_what_the_restatement_reads(lib, shape):
    h, w, ch, sub = shape
    frame = ref.noise_frame(h, w, 2, ch)
    for ri, kw in intervals_of(h, w, ch, sub):
        data = pillow_file(frame, 92, sub, comment=b"skipped", **kw)
        rc, msg, hd, got_ri, spans = _parse_spans(lib, data)
        want = rr.parse(data)
        assert rc == 0, msg
        assert (hd.h, hd.w, hd.ch, hd.subsampling, got_ri) == (h, w, ch, want["sub"], ri)
        assert (hd.scan_offset, hd.scan_bytes) == (want["scan_offset"], want["scan_bytes"]) and data[hd.scan_offset + hd.scan_bytes:] == b"\xff\xd9"
        assert spans == want["spans"]
        assert list(hd.dc_table)[:ch] == want["dc"] and list(hd.ac_table)[:ch] == want["ac"]
        assert [list(q) for q in hd.quant][:ch] == want["quant"]
        for slot, key in enumerate((0x00, 0x10, 0x01, 0x11)):
            bits, vals = want["tables"].get(key, ([0] * 16, []))
            assert list(hd.bits[slot]) == bits and list(hd.huffval[slot])[:len(vals)] == vals, slot


def test_a_file_without_markers_is_one_span_the_scan_range_of_tt_jpeg_parse(lib):
    from this_and_that_vdm_amd import _lib
    for data in (pillow_file(ref.noise_frame(37, 53, 2, 3), 90, 2), rr.with_dri(pillow_file(ref.noise_frame(37, 53, 2, 3), 90, 2), 0),
                 pillow_file(ref.noise_frame(37, 53, 2, 3), 90, 2, restart_marker_blocks=1000)):
        rc, msg, hd, ri, spans = _parse_spans(lib, data)
        assert rc == 0 and len(spans) == 1, msg
        plain = bytearray(data)
        if b"\xff\xdd\x00\x04" in data:                                                                  # tt_jpeg_parse refuses a non-zero DRI: take it out
            at = data.index(b"\xff\xdd\x00\x04")
            del plain[at:at + 6]
            spans = [(spans[0][0] - 6, spans[0][1])]
        old = _lib.TtJpegHeader()
        buf = np.frombuffer(bytes(plain), dtype=np.uint8)
        assert lib.tt_jpeg_parse(buf.ctypes.data, buf.size, C.byref(old)) == 0
        assert spans == [(old.scan_offset, old.scan_bytes)]


def test_parse_spans_refuses_by_name(lib):
    frame = ref.noise_frame(48, 48, 2, 3)
    good = rr.jpeg_file(frame, 75, 0, 2)                                        # 36 MCUs, 17 markers
    plain = rr.jpeg_file(frame, 75, 0, 0)
    hd, hp = rr.parse(good), rr.parse(plain)
    marker = lambda k: hd["spans"][k][0] + hd["spans"][k][1]                     # where the k-th marker stands
    renumbered = bytearray(good)
    renumbered[marker(3) + 1] = 0xd5
    at = hp["scan_offset"] + 20
    rows = [
        (bytes(renumbered), -1, "restart marker 3 at byte %d is RST5 where RST3 is due" % marker(3)),
        (good[:marker(3)] + good[marker(3) + 2:], -1, "is RST4 where RST3 is due"),                      # a marker deleted: the next one is early
        (good[:marker(16)] + good[marker(16) + 2:], -1, "16 restart markers where a restart interval of 2 over 36 MCUs has 17"),
        (good[:marker(16)] + b"\xff\xd0\xff\xd1" + good[marker(16) + 2:], -1, "18 restart markers where"),     # one marker more, in order
        (rr.with_dri(plain, 3), -1, "0 restart markers where a restart interval of 3 over 36 MCUs has 11"),
        (plain[:at] + b"\xff\xd0" + plain[at:], -1, "in a file with no DRI segment"),
        (rr.with_dri(plain, 0)[:at + 6] + b"\xff\xd0" + plain[at:], -1, "in a file whose DRI segment says 0"),
        (rr.with_dri(good, 3), -1, "two DRI segments that disagree (restart intervals of 2 and 3 MCUs)"),
    ]
    for i, (data, code, fragment) in enumerate(rows):
        rc, msg, _, _, _ = _parse_spans(lib, data)
        assert rc == code and fragment in msg and msg.startswith("tt_jpeg_parse_spans:"), (i, fragment, rc, msg)
    # what rule 1 refuses, it refuses here with rule 1's text; two DRI segments that agree are accepted
    rc, msg, _, _, _ = _parse_spans(lib, pillow_file(frame, 75, 1, restart_marker_blocks=2))
    assert rc == -2 and "4:2:2" in msg and msg.startswith("tt_jpeg_parse:"), msg
    rc, msg, _, _, _ = _parse_spans(lib, pillow_file(frame, 75, 0, restart_marker_blocks=2, progressive=True))
    assert rc == -2 and "progressive" in msg, msg
    rc, msg, _, _, _ = _parse_spans(lib, good[:marker(5) + 1])
    assert rc == -1 and "ends before EOI" in msg, msg
    rc, msg, _, ri, spans = _parse_spans(lib, rr.with_dri(good, 2))
    assert rc == 0 and ri == 2 and len(spans) == 18, msg
    # the span arrays: a cap below the count, one array without the other
    from this_and_that_vdm_amd import _lib
    hdr, r, n = _lib.TtJpegHeader(), C.c_int32(0), C.c_int64(0)
    buf, offs, lens = np.frombuffer(good, dtype=np.uint8), np.zeros(17, dtype=np.int64), np.zeros(17, dtype=np.int64)
    assert lib.tt_jpeg_parse_spans(buf.ctypes.data, buf.size, C.byref(hdr), C.byref(r), offs.ctypes.data, lens.ctypes.data, 17, C.byref(n)) == -1
    assert b"span_cap too small: 17 for 18 spans" in lib.tt_last_error()
    assert lib.tt_jpeg_parse_spans(buf.ctypes.data, buf.size, C.byref(hdr), C.byref(r), offs.ctypes.data, None, 17, C.byref(n)) == -1
    assert b"go together" in lib.tt_last_error()


def test_ingest_parse_jpeg_carries_the_interval_and_the_spans(lib):
    from this_and_that_vdm_amd import ingest
    data = pillow_file(ref.noise_frame(40, 56, 2, 3), 75, 2, restart_marker_rows=1)
    hd = ingest.parse_jpeg(data)
    assert hd.restart_interval == 4 and hd.spans.tolist() == [list(s) for s in rr.parse(data)["spans"]]
    one = ingest.parse_jpeg(pillow_file(ref.noise_frame(40, 56, 2, 3), 75, 2))
    assert one.restart_interval == 0 and one.spans.tolist() == [[one.scan_offset, one.scan_bytes]]
    at, n = rr.parse(data)["spans"][1]
    with pytest.raises(ValueError, match="tt_jpeg_parse_spans: .*is RST2 where RST1 is due"):
        ingest.parse_jpeg(data[:at + n + 1] + b"\xd2" + data[at + n + 2:])


# ---- encode_jpeg's arguments: refused before a device is touched
def test_encode_jpeg_refuses_its_restart_arguments():
    from this_and_that_vdm_amd import export
    frames = np.zeros((1, 16, 16, 3), dtype=np.uint8)
    for kw, text in [(dict(restart_interval=2, restart_rows=1), "at most one of the two"), (dict(restart_interval=-1), "restart_interval -1"),
                     (dict(restart_rows=-2), "restart_rows -2"), (dict(restart_interval=65536), "65536 MCUs"), (dict(restart_interval=True), "restart_interval True"),
                     (dict(restart_interval=1.5), "restart_interval 1.5")]:
        with pytest.raises(ValueError, match=text):
            export.encode_jpeg(frames, **kw)
    with pytest.raises(ValueError, match="a restart interval of 66000 MCUs"):                            # rows x MCUs per row: 33000 x 2
        export.encode_jpeg(np.zeros((1, 8, 16, 3), dtype=np.uint8), subsampling="4:4:4", restart_rows=33000)
    for who in (export.write_jpegs, export.write_mjpeg):                                                # both pass the options through
        with pytest.raises(ValueError, match="at most one of the two"):
            who(frames, os.devnull, restart_interval=2, restart_rows=1)


# ---- the device entry points: refused before the first HIP call, so this needs no GPU
def test_the_library_refuses_before_any_launch(lib):
    P = 0x10000                                                                                          # fake aligned pointers: every call returns before a HIP call
    assert lib.tt_jpeg_scan_restart(P, 1, 16, 16, 3, 2, 65536, 2 * P, 1, 3 * P, 1 << 20, 4 * P, 5 * P, 1 << 20, None) == -1 and b"restart_interval = 65536" in lib.tt_last_error()
    assert lib.tt_jpeg_scan_restart(P, 1, 16, 16, 3, 2, -1, 2 * P, 1, 3 * P, 1 << 20, 4 * P, 5 * P, 1 << 20, None) == -1 and b"restart_interval = -1" in lib.tt_last_error()
    assert lib.tt_jpeg_scan_restart(P, 1, 16, 16, 3, 2, 1, 2 * P, 1, 3 * P, 16, 4 * P, 5 * P, 1 << 20, None) == -1 and b"tt_jpeg_scan_restart: cap too small" in lib.tt_last_error()
    assert lib.tt_jpeg_counts_restart(P, 1, 16, 16, 3, 2, 70000, 2 * P, None) == -1 and b"restart_interval = 70000" in lib.tt_last_error()
    args = (P, 64, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P, 64)
    rest = (1, 16, 16, 3, 2, 7 * P, 1, 8 * P, 9 * P, 10 * P, 1 << 20, None)
    assert lib.tt_jpeg_entropy_spans(*args, 65536, *rest) == -2 and b"65536 spans: more than one grid covers (65535)" in lib.tt_last_error()
    assert lib.tt_jpeg_entropy_spans(*args, 0, *rest) == -1 and b"nspans = 0" in lib.tt_last_error()
    assert lib.tt_jpeg_entropy_spans(P, 64, 2 * P, 3 * P, None, 5 * P, 6 * P, 64, 4, *rest) == -1 and b"null span_frame" in lib.tt_last_error()
    assert lib.tt_jpeg_entropy_spans(P, 64, 2 * P, 3 * P, 4 * P + 2, 5 * P, 6 * P, 64, 4, *rest) == -1 and b"not 4-byte aligned" in lib.tt_last_error()
    # one MCU row of 8187 grey MCUs with a marker behind each, nine times: more spans than one call takes, named by decode_jpeg before any upload
    from this_and_that_vdm_amd import ingest
    wide = pillow_file(np.zeros((8, 65496, 1), dtype=np.uint8), 50, 0, restart_marker_blocks=1)
    assert len(ingest.parse_jpeg(wide).spans) == 8187
    with pytest.raises(ValueError, match="73683 restart intervals in 9 files: more spans than one call decodes"):
        ingest.decode_jpeg([wide] * 9, "cuda:0")


# ---- the host code under the sanitizers, on its own
def test_jpeg_restart_host_under_address_and_undefined_sanitizers(tmp_path):
    """jpeg_host.cpp, png_host.cpp, lib.cpp and tests/jpeg_restart_host_check.cpp (its own main) built with the host compiler and run as a
    child process: nothing is preloaded and nothing of it runs under Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    exe = str(tmp_path / "jpeg_restart_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
           os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "jpeg_restart_host_check.cpp"), os.path.join(csrc, "jpeg_host.cpp"),
           os.path.join(csrc, "png_host.cpp"), os.path.join(csrc, "lib.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler's sanitizer runtime is missing: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
