"""CPU: progressive JPEG files in the import -- the format and the host half.  The restatement of tests/jpeg_progressive_reference.py
against Pillow (libjpeg-turbo): its serial decoders and its emulation of the device schemes give Pillow's pixels on Pillow's own
``progressive=True`` files; its WRITER's files, under scan scripts Pillow never writes, decode in Pillow to exactly what the baseline file
of the same coefficients decodes to (so a completed progression is not smoothed) and in the restatement to the same; then
tt_jpeg_parse_progressive through ctypes: every field against the restatement's parser, every refusal of rule 1b by code and text; the
device entry point's refusals, which come before any HIP call; and the host parser under the address and undefined-behaviour sanitizers
in a stand-alone program over truncations and byte edits of good files.

Everything here is equality: a JPEG is integers from end to end."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import jpeg_progressive_reference as pr
from tests import jpeg_reference as ref
from tests.jpeg_reference import _segment

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOI = b"\xff\xd9"
# (h, w, ch, subsampling): partial MCUs in 4:2:0 (Y blocks the MCU grid pads), 4:4:4, grey; one block
SHAPES = [(17, 23, 3, 2), (24, 40, 3, 0), (33, 40, 1, 0), (8, 8, 1, 0)]
SHAPE_IDS = ["17x23-420", "24x40-444", "33x40-grey", "8x8-grey"]


def pillow_progressive(frame, quality, sub):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(buf, format="JPEG", quality=quality, subsampling=sub, progressive=True)
    return buf.getvalue()


def pillow_pixels(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


def written(h, w, ch, sub, script, quality=75, seed=3):
    """(the writer's progressive file, the baseline file of the same coefficients)"""
    frame = ref.noise_frame(h, w, seed, ch) // 2 + ref.smooth_frame(h, w, seed, ch) // 2
    coefs, comps, _ = ref.coefficients(frame, quality, sub)
    return pr.progressive_file(coefs, h, w, ch, quality, sub, script), ref.file_of(ref.scan_bytes(coefs, comps), h, w, ch, quality, sub)


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def parse(lib, data):
    """tt_jpeg_parse_progressive's two calls -> (rc, header, scans, text)"""
    from this_and_that_vdm_amd import _lib
    hd, count = _lib.TtJpegProgressiveHeader(), C.c_int64(-1)
    buf = np.frombuffer(data, dtype=np.uint8)
    rc = lib.tt_jpeg_parse_progressive(buf.ctypes.data, buf.size, C.byref(hd), None, 0, C.byref(count))
    if rc != 0:
        return rc, hd, [], lib.tt_last_error().decode()
    rows = (_lib.TtJpegScan * count.value)()
    rc = lib.tt_jpeg_parse_progressive(buf.ctypes.data, buf.size, C.byref(hd), C.cast(rows, C.c_void_p), count.value, C.byref(count))
    return rc, hd, list(rows), lib.tt_last_error().decode()


# ---- the restatement against Pillow
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("quality", (30, 95))
def test_the_restatement_decodes_pillows_progressive_files_to_pillows_pixels(shape, quality):
    h, w, ch, sub = shape
    for frame in (ref.smooth_frame(h, w, 1, ch), ref.noise_frame(h, w, 2, ch), ref.flat_frame(h, w, 200, ch)):
        data = pillow_progressive(frame, quality, sub)
        hd = pr.parse(data)
        assert [(s["comps"], s["ss"], s["se"], s["ah"], s["al"]) for s in hd["scans"]] == (pr.PILLOW_GREY if ch == 1 else pr.PILLOW_COLOUR)
        want = pillow_pixels(data)
        for lanes in (None, (64, 4), (1024, 256)):
            got, status = pr.decode(data, lanes)
            assert status == 0 and np.array_equal(got, want), (shape, quality, lanes)


@pytest.mark.parametrize("name", sorted(pr.SCRIPTS))
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_writers_scripts_decode_in_pillow_to_the_baseline_files_pixels(name, shape):
    """the property the import rests on: a COMPLETE progression is the inverse DCT of its coefficients in libjpeg -- no smoothing --
    whatever the script; and the restatement's decoders agree"""
    h, w, ch, sub = shape
    data, base = written(h, w, ch, sub, pr.SCRIPTS[name](ch))
    want = pillow_pixels(base)
    assert np.array_equal(pillow_pixels(data), want)
    for lanes in (None, (64, 4)):
        got, status = pr.decode(data, lanes)
        assert status == 0 and np.array_equal(got, want), (name, shape, lanes)


def test_the_device_schemes_carry_their_state_over_several_sequences():
    """a short sequence (4 lanes of 64 bits) makes every scan of a noisy frame span many: the carried state, EOB runs across lanes and the
    refinement's recorded positions all come into play, and the coefficients equal the serial decoders'"""
    data = pillow_progressive(ref.noise_frame(40, 56, 5, 3), 95, 2)
    hd = pr.parse(data)
    assert max(s["bytes"] for s in hd["scans"]) * 8 > 20 * 4 * 64
    serial, lanes = pr.entropy(data, hd), pr.entropy(data, hd, (64, 4))
    assert serial[1] == 0 and lanes[1] == 0 and np.array_equal(serial[0], lanes[0])


# ---- tt_jpeg_parse_progressive
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_parser_reads_what_the_restatement_reads(lib, shape):
    h, w, ch, sub = shape
    files = [pillow_progressive(ref.smooth_frame(h, w, 1, ch), 75, sub)] + [written(h, w, ch, sub, pr.SCRIPTS[n](ch))[0] for n in sorted(pr.SCRIPTS)]
    for data in files:
        want = pr.parse(data)
        rc, hd, scans, text = parse(lib, data)
        assert rc == 0, text
        assert (hd.h, hd.w, hd.ch, hd.subsampling, hd.nscans) == (h, w, ch, want["sub"], len(want["scans"]))
        assert [list(hd.quant[c]) for c in range(ch)] == want["quant"]
        for got, sc in zip(scans, want["scans"]):
            assert (got.comps, got.ss, got.se, got.ah, got.al, got.offset, got.bytes) == \
                (sum(1 << c for c in sc["comps"]), sc["ss"], sc["se"], sc["ah"], sc["al"], sc["offset"], sc["bytes"])
            for slot in range(3):
                bits, vals = sc["tables"].get(slot, ([0] * 16, []))
                assert list(got.bits[slot]) == list(bits) and list(got.huffval[slot]) == list(vals) + [0] * (256 - len(vals))


def test_ingest_parse_jpeg_progressive_carries_the_scans(lib):
    from this_and_that_vdm_amd import ingest
    data = pillow_progressive(ref.smooth_frame(17, 23, 1, 3), 75, 2)
    hd = ingest.parse_jpeg_progressive(data)
    assert (hd.height, hd.width, hd.channels, hd.subsampling) == (17, 23, 3, "4:2:0") and hd.quant.shape == (3, 64)
    assert [(s.components, s.ss, s.se, s.ah, s.al) for s in hd.scans] == pr.PILLOW_COLOUR
    want = pr.parse(data)["scans"]
    assert [(s.offset, s.bytes) for s in hd.scans] == [(s["offset"], s["bytes"]) for s in want]
    assert hd.scans[0].bits.shape == (3, 16) and hd.scans[0].huffval.shape == (3, 256) and not hd.scans[6].bits.any()
    with pytest.raises(ValueError, match="progressive"):                                                  # the baseline parser keeps refusing the file
        ingest.parse_jpeg(data)
    with pytest.raises(ValueError, match="tt_jpeg_parse_spans"):
        ingest.parse_jpeg_progressive(ref.jpeg_file(ref.smooth_frame(16, 16, 0, 3)))


def _sos(data, hd, k):
    """where scan k's SOS payload begins"""
    return hd["scans"][k]["offset"] - (4 + 2 * len(hd["scans"][k]["comps"]))


def _patched(data, at, value):
    return data[:at] + bytes([value]) + data[at + 1:]


def _with_sos(data, hd, k, payload):
    """scan k's SOS segment replaced by one with another payload"""
    at = _sos(data, hd, k) - 4
    return data[:at] + _segment(0xda, payload) + data[hd["scans"][k]["offset"]:]


def test_the_parser_refuses_by_name(lib):
    colour, _ = written(16, 16, 3, 2, pr.PILLOW_COLOUR)
    grey, _ = written(8, 8, 1, 0, pr.PILLOW_GREY)
    hc, hg = pr.parse(colour), pr.parse(grey)
    assert parse(lib, colour)[0] == 0 and parse(lib, grey)[0] == 0
    end = lambda hd, k: hd["scans"][k]["offset"] + hd["scans"][k]["bytes"]
    sof = colour.index(b"\xff\xc2")
    dqt = colour.index(b"\xff\xdb")
    many = [((0,), 0, 0, 0, 3)] + [((0,), k, k, 0, 3) for k in range(1, 64)]
    for al in (2, 1, 0):
        many += [((0,), 0, 0, al + 1, al)] + [((0,), k, k, al + 1, al) for k in range(1, 64)]
    assert len(many) == 256
    cases = [
        # T.81 G.1.1.1.1 and the progression bookkeeping: TT_EINVAL
        (_patched(colour, _sos(colour, hc, 0) + 8, 5), -1, "a DC scan with Se = 5"),
        (_with_sos(colour, hc, 1, bytes([2, 1, 0, 2, 0, 1, 5, 2])), -1, "an AC scan of 2 components"),
        (_patched(_patched(colour, _sos(colour, hc, 1) + 3, 5), _sos(colour, hc, 1) + 4, 3), -1, "band 5 to 3"),
        (_patched(colour, _sos(colour, hc, 0) + 9, 0x0e), -1, "Al = 14"),
        (_patched(colour, _sos(colour, hc, 0) + 9, 0x10), -1, "successive approximation Ah = 1, Al = 0 where coefficient 0 of component 0 is new"),
        (_patched(colour, _sos(colour, hc, 9) + 5, 0x21), -1, "successive approximation Ah = 2, Al = 1 where coefficient 1 of component 0 stands at Al 1"),
        (_patched(grey, _sos(grey, hg, 5) + 5, 0x20), -1, "successive approximation Ah = 2, Al = 0"),
        (pr.progressive_file(np.zeros((1, 64), np.int16), 8, 8, 1, 75, 0, [((0,), 1, 63, 0, 0), ((0,), 0, 0, 0, 0)]), -1, "an AC scan of component 0 before its DC scan"),
        (_with_sos(colour, hc, 0, bytes([2, 2, 0x10, 3, 0x20, 0, 0, 1])), -1, "component subset"),
        (_with_sos(colour, hc, 0, bytes([3, 2, 0x10, 1, 0x00, 3, 0x20, 0, 0, 1])), -1, "component subset"),
        (_patched(colour, _sos(colour, hc, 1) + 1, 9), -1, "names component 9, which the frame does not have"),
        (colour[:end(hc, 3)], -1, "ends before EOI"),
        (colour[:hc["scans"][3]["offset"] + 1], -1, "ends before EOI"),
        # not decoded: TT_EUNSUPPORTED
        (colour[:2] + _segment(0xdd, b"\x00\x04") + colour[2:], -2, "restart intervals in a progressive file"),
        (colour[:end(hc, 0)] + _segment(0xdb, bytes(65)) + colour[end(hc, 0):], -2, "a DQT behind the first SOS"),
        (pr.progressive_file(np.zeros((1, 64), np.int16), 8, 8, 1, 75, 0, many + [((0,), 0, 0, 0, 0)]), -2, "more than 256 scans"),
        # the incomplete progression: a complete file with its last refinement scans cut out and EOI put back
        (colour[:end(hc, 6)] + EOI, -2, "incomplete progression: coefficient 1 of component 0 has not reached Al = 0"),
        (colour[:end(hc, 5)] + EOI, -2, "incomplete progression: coefficient 0 of component 0 has not reached Al = 0"),
        (grey[:end(hg, 1)] + EOI, -2, "incomplete progression: coefficient 0 of component 0 has not reached Al = 0"),
        (written(8, 8, 1, 0, [((0,), 0, 0, 0, 0), ((0,), 1, 5, 0, 0)])[0], -2, "incomplete progression: coefficient 6 of component 0 was never sent"),
        # what tt_jpeg_parse refuses as well
        (_patched(colour, sof + 4, 12), -2, "12-bit"),
        (_patched(colour, sof + 1, 0xca), -2, "arithmetic"),
        (_patched(colour, sof + 1, 0xc1), -2, "extended sequential"),
        (colour[:2] + _segment(0xee, b"Adobe\x00\x64\x00\x00\x00\x00\x01") + colour[2:], -2, "Adobe"),
        (_patched(colour, dqt + 4, 0x10), -2, "16-bit DQT"),
        (_patched(colour, sof + 11, 0x21), -2, "sampling 2x1 / 1x1 / 1x1"),
        (ref.jpeg_file(ref.smooth_frame(16, 16, 0, 3)), -2, "a baseline (SOF0) file: tt_jpeg_parse_spans"),
        (b"\x00" + colour[1:], -1, "no SOI marker"),
    ]
    for data, code, text in cases:
        rc, _, _, said = parse(lib, data)
        assert rc == code and text in said and said.startswith("tt_jpeg_parse_progressive: "), (text, rc, said)
    # the 256-scan file itself is fine: the limit is TT_JPEG_MAX_SCANS scans, not fewer
    rc, hd, scans, said = parse(lib, pr.progressive_file(np.zeros((1, 64), np.int16), 8, 8, 1, 75, 0, many))
    assert rc == 0 and hd.nscans == 256 and len(scans) == 256, said
    # a table a scan names but no DHT defines
    no_dht = colour[:colour.index(b"\xff\xc4")] + colour[_sos(colour, hc, 0) - 4:]
    rc, _, _, said = parse(lib, no_dht)
    assert rc == -2 and "missing DC Huffman table" in said


def test_the_existing_parsers_keep_refusing_progressive_files(lib):
    from this_and_that_vdm_amd import _lib
    data = pillow_progressive(ref.smooth_frame(16, 16, 0, 3), 75, 2)
    buf = np.frombuffer(data, dtype=np.uint8)
    hd, ri, count = _lib.TtJpegHeader(), C.c_int32(0), C.c_int64(0)
    assert lib.tt_jpeg_parse(buf.ctypes.data, buf.size, C.byref(hd)) == -2 and b"SOF2: progressive" in lib.tt_last_error()
    assert lib.tt_jpeg_parse_spans(buf.ctypes.data, buf.size, C.byref(hd), C.byref(ri), None, None, 0, C.byref(count)) == -2 and b"SOF2: progressive" in lib.tt_last_error()


# ---- the device entry point: refused before the first HIP call, so this needs no GPU
def test_the_library_refuses_before_any_launch(lib):
    P = 0x10000                                                                                          # fake aligned pointers: every call returns before a HIP call
    ptrs = dict(scans=P, offsets=2 * P, lengths=3 * P, desc=4 * P, tables=5 * P, coeffs=6 * P, status=7 * P, ws=8 * P)

    def call(n=1, nscans=10, max_bytes=64, scans_bytes=64, h=16, w=16, ch=3, sub=2, ws_bytes=1 << 30, **over):
        a = dict(ptrs, **over)
        return lib.tt_jpeg_entropy_progressive(a["scans"], scans_bytes, a["offsets"], a["lengths"], a["desc"], a["tables"], max_bytes, n, nscans, h, w, ch, sub,
                                               a["coeffs"], a["status"], a["ws"], ws_bytes, None), lib.tt_last_error().decode()

    for name in ptrs:
        assert call(**{name: None}) == (-1, f"tt_jpeg_entropy_progressive: null {name}")
    for kw, code, text in [(dict(n=0), -1, "empty problem"), (dict(nscans=0), -1, "nscans = 0"), (dict(nscans=257), -2, "257 scans a frame (at most 256)"),
                           (dict(n=300, nscans=256), -2, "more items than one grid covers (65535)"), (dict(max_bytes=0), -1, "empty scans"),
                           (dict(scans_bytes=0), -1, "empty scans"), (dict(max_bytes=1 << 28), -2, "a scan below 2^28 bytes"), (dict(ch=2), -1, "2 channels"),
                           (dict(sub=1), -1, "subsampling = 1"), (dict(offsets=2 * P + 4), -1, "offsets is not 8-byte aligned"),
                           (dict(lengths=3 * P + 2), -1, "lengths is not 4-byte aligned"), (dict(desc=4 * P + 8), -1, "desc is not 16-byte aligned"),
                           (dict(tables=5 * P + 8), -1, "tables is not 16-byte aligned"), (dict(coeffs=6 * P + 8), -1, "coeffs is not 16-byte aligned"),
                           (dict(status=7 * P + 2), -1, "status is not 4-byte aligned"), (dict(ws=8 * P + 8), -1, "ws is not 16-byte aligned"),
                           (dict(ws_bytes=lib.tt_jpeg_entropy_progressive_ws_bytes(1, 10, 64, 16, 16, 3, 2) - 1), -1, "ws too small")]:
        rc, said = call(**kw)
        assert rc == code and text in said, (kw, rc, said)
    need = lib.tt_jpeg_entropy_progressive_ws_bytes(2, 10, 1000, 17, 23, 3, 2)
    assert need >= lib.tt_jpeg_entropy_ws_bytes(20, 1000) + 4 * 20 + 12 * 2 * lib.tt_jpeg_blocks(17, 23, 3, 2) and need % 16 == 0
    assert lib.tt_abi_version() == 11


def test_decode_jpeg_without_the_keyword_refuses_before_any_upload(lib):
    """the default keeps the refusal by name, and the keyword does not reach a device before the files are parsed"""
    from this_and_that_vdm_amd import ingest
    data = pillow_progressive(ref.smooth_frame(16, 16, 0, 3), 75, 2)
    with pytest.raises(ValueError, match="decode_jpeg: file 0: tt_jpeg_parse: SOF2: progressive"):
        ingest.decode_jpeg([data], "cuda:0")
    cut = data[:pr.parse(data)["scans"][7]["offset"]] + EOI
    with pytest.raises(ValueError, match="decode_jpeg: file 1: tt_jpeg_parse_progressive: incomplete progression"):
        ingest.decode_jpeg([data, cut], "cuda:0", progressive=True)
    other = pillow_progressive(ref.smooth_frame(16, 24, 0, 3), 75, 2)
    with pytest.raises(ValueError, match="one geometry and subsampling per call"):
        ingest.decode_jpeg([ref.jpeg_file(ref.smooth_frame(16, 16, 0, 3)), other], "cuda:0", progressive=True)


# ---- the host code under the sanitizers, on its own
def test_jpeg_progressive_host_under_address_and_undefined_sanitizers(tmp_path):
    """jpeg_host.cpp, png_host.cpp, lib.cpp and tests/jpeg_progressive_host_check.cpp (its own main) built with the host compiler and run
    as a child process over good files written here: nothing is preloaded and nothing of it runs under Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    exe = str(tmp_path / "jpeg_progressive_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
           os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "jpeg_progressive_host_check.cpp"), os.path.join(csrc, "jpeg_host.cpp"),
           os.path.join(csrc, "png_host.cpp"), os.path.join(csrc, "lib.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler's sanitizer runtime is missing: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-4000:]
    files = {"pillow_420.jpg": pillow_progressive(ref.smooth_frame(16, 16, 1, 3), 75, 2), "pillow_grey.jpg": pillow_progressive(ref.smooth_frame(8, 8, 1, 1), 75, 0),
             "separate_dc_444.jpg": written(8, 8, 3, 0, pr.script_separate_dc(3))[0]}
    paths = []
    for name, data in files.items():
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as fh:
            fh.write(data)
    r = subprocess.run([exe, *paths], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
