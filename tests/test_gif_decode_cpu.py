"""CPU: the GIF import of include/ttvdm.h ("GIF import") before any kernel runs -- the restatement of tests/gif_decode_reference.py
against Pillow on files Pillow wrote, on the 72 handcrafted composition files (outside Pillow's two departures from GIF89a, decided by
a predicate on the parsed header) and on the format's corner cases; tt_gif_parse through ``ingest.parse_gif`` field for field against
the restatement's parser; every refusal by name in a child process that sees no GPU; and the parser under the address and
undefined-behaviour sanitizers in a stand-alone program.  Equality throughout."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gif_decode_reference as g
from tests import gif_decode_refusals as refusals
from this_and_that_vdm_amd.ingest import decode_gif, parse_gif          # the feature under test: without it nothing here is collected

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def video(f, h, w, seed):
    """a moving bright square over a smooth background with a little noise: frames that differ in a small rectangle"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 127 // max(w + h - 2, 1))], axis=-1).astype(np.uint8)
    out = np.repeat(base[None], f, axis=0)
    for i in range(f):
        y0, x0 = (3 * i) % max(h - 4, 1), (5 * i) % max(w - 4, 1)
        out[i, y0:y0 + 4, x0:x0 + 4] = rng.integers(0, 256, size=3)
    return out


def pillow_file(frames, **kw):
    from PIL import Image
    ims = [Image.fromarray(fr) for fr in frames]
    buf = io.BytesIO()
    ims[0].save(buf, format="GIF", save_all=len(ims) > 1, append_images=ims[1:], **kw)
    return buf.getvalue()


def pillow_written():
    """-> [(name, bytes)]: default, optimize, disposal 1 / 2, interlace, transparency; 1 to 5 frames, 8 x 8 to 130 x 150"""
    out = []
    for f, h, w in ((1, 8, 8), (2, 17, 13), (3, 40, 56), (5, 130, 150)):
        v = video(f, h, w, f)
        out.append((f"default-{f}x{h}x{w}", pillow_file(v)))
        out.append((f"optimize-{f}x{h}x{w}", pillow_file(v, optimize=True)))
        out.append((f"disposal1-{f}x{h}x{w}", pillow_file(v, disposal=1, duration=70, loop=2)))
        out.append((f"disposal2-{f}x{h}x{w}", pillow_file(v, disposal=2)))
        out.append((f"interlace-{f}x{h}x{w}", pillow_file(v, interlace=True)))
        from PIL import Image
        pal = [Image.fromarray(fr).convert("P", palette=Image.ADAPTIVE, colors=32) for fr in v]
        buf = io.BytesIO()
        pal[0].save(buf, format="GIF", save_all=f > 1, append_images=pal[1:], transparency=3, disposal=2)
        out.append((f"transparency-{f}x{h}x{w}", buf.getvalue()))
    return out


def corner_cases():
    """-> [(name, bytes)]: sub-blocks of 1, 100 and 255 bytes, minimum code sizes 2, 5 and 8, interlace, a 160 x 120 noise frame with five
    table overflows, the same frame with a deferred clear and a random one with a deferred clear"""
    rng = np.random.default_rng(5)
    out = []
    for size in (1, 100, 255):
        out.append((f"sub-block-{size}", g.gif_file(40, 30, [dict(indices=rng.integers(0, 64, size=(30, 40)))], global_table=rng.integers(0, 256, size=(64, 3)),
                                                    sub_block=size)))
    for mcs in (2, 5, 8):
        n = 1 << mcs
        out.append((f"min-code-size-{mcs}", g.gif_file(23, 19, [dict(indices=rng.integers(0, n, size=(19, 23)))], global_table=rng.integers(0, 256, size=(n, 3)))))
    out.append(("interlace", g.gif_file(21, 19, [dict(indices=rng.integers(0, 16, size=(19, 21)), interlace=True)], global_table=rng.integers(0, 256, size=(16, 3)))))
    # a noise frame in which no pair of neighbours repeats (row j of 256 pixels steps by 2 j + 1): every pixel costs a code
    at = np.arange(160 * 120)
    noise, table = ((at % 256) * (1 + 2 * (at // 256)) % 256).reshape(120, 160), rng.integers(0, 256, size=(256, 3))
    out.append(("overflows", g.gif_file(160, 120, [dict(indices=noise)], global_table=table)))
    out.append(("deferred-clear", g.gif_file(160, 120, [dict(indices=noise, deferred=True)], global_table=table)))
    # ... and random noise, whose strings behind the full table use its entries
    out.append(("deferred-clear-random", g.gif_file(160, 120, [dict(indices=rng.integers(0, 256, size=(120, 160)), deferred=True)], global_table=table)))
    return out


def test_the_restatement_equals_pillow_on_pillows_files():
    for name, data in pillow_written():
        hd = g.parse(data)
        assert not g.outside_pillows_envelope(hd), name
        got, status = g.decode(data)
        assert status == [0] * len(got) and np.array_equal(got, g.pillow_frames(data)), name
    crops = g.parse(pillow_file(video(5, 130, 150, 5)))["frames"]
    assert any((fr["w"], fr["h"]) != (150, 130) for fr in crops), "Pillow no longer writes cropped difference rectangles for this video"


def test_the_restatement_equals_pillow_on_the_handcrafted_files_inside_the_envelope():
    files = g.handcrafted_files()
    assert len(files) == 72
    left_out = 0
    for name, data in files:
        hd = g.parse(data)
        if g.outside_pillows_envelope(hd):
            left_out += 1
            continue
        got, status = g.decode(data)
        assert status == [0, 0, 0, 0] and np.array_equal(got, g.pillow_frames(data)), name
    assert left_out <= 8, left_out


def test_the_restatement_equals_pillow_on_the_corner_cases():
    for name, data in corner_cases():
        got, status = g.decode(data)
        assert status == [0] and np.array_equal(got, g.pillow_frames(data)), name
    noise = g.parse(dict(corner_cases())["overflows"])["frames"][0]
    assert sum(1 for code, _, _ in g.read_codes(noise["data"], 8) if code == 256) == 6                    # the first clear code and five overflows
    for name in ("deferred-clear", "deferred-clear-random"):
        codes = g.read_codes(g.parse(dict(corner_cases())[name])["frames"][0]["data"], 8)
        assert sum(1 for code, _, _ in codes if code == 256) == 1 and max(r for _, r, _ in codes) > 4096   # 12-bit codes run on behind the full table
    assert sum(1 for code, r, _ in codes if r > 4096 and code >= 258) > 100                                # ... and name its entries


def test_parse_gif_reads_what_the_restatement_reads(lib):
    from this_and_that_vdm_amd import ingest
    files = pillow_written() + g.handcrafted_files()[::7] + corner_cases()[:4] + [("two frames", refusals.GOOD)]
    files.append(("no trailer, GIF87a", g.gif_file(9, 9, [dict(indices=np.zeros((4, 5)), left=2, top=3, gce=False)], global_table=np.zeros((2, 3)), loop=None,
                                                   trailer=False, version=b"GIF87a")))
    for name, data in files:
        want, hd = g.parse(data), ingest.parse_gif(data)
        assert (hd.height, hd.width, hd.background, hd.loop, hd.frames) == (want["height"], want["width"], want["background"], want["loop"], len(want["frames"])), name
        assert hd.version == int(data[3:5])
        at = 0
        for f, fr in enumerate(want["frames"]):
            assert hd.rectangles[f].tolist() == [fr["left"], fr["top"], fr["w"], fr["h"]], (name, f)
            assert (hd.durations[f], hd.disposal[f], hd.transparent[f], hd.interlace[f], hd.min_code_size[f], hd.local[f]) == \
                   (fr["delay"] / 100.0, fr["disposal"], fr["transparent"], fr["interlace"], fr["min_code_size"], fr["local"]), (name, f)
            assert np.array_equal(hd.palettes[f], fr["palette"]), (name, f)
            assert hd.spans[f].tolist() == [at, len(fr["data"])] and hd.data[at:at + len(fr["data"])].tobytes() == fr["data"], (name, f)
            at += len(fr["data"])
        assert hd.data.size == at


def test_every_refusal_is_answered_by_name_without_a_device():
    got = refusals.run_child()
    assert got["good"] == [0, ""]
    for name, _, code, fragment in refusals.FILES:
        rc, msg = got["file:" + name]
        assert rc == code and fragment in msg and msg.startswith("tt_gif_parse:"), (name, rc, msg)
    for fault, code, fragment in refusals.DEC_ROWS:
        rc, msg = got["dec:" + refusals.row_id(fault)]
        assert rc == code and fragment in msg and msg.startswith("tt_gif_decode_indices:"), (fault, rc, msg)
    for fault, code, fragment in refusals.CMP_ROWS:
        rc, msg = got["cmp:" + refusals.row_id(fault)]
        assert rc == code and fragment in msg and msg.startswith("tt_gif_compose:"), (fault, rc, msg)
    valid, *refused = got["sizes"]
    # the derived bound: 8 * 1000 / 6 + 3 segment records of five words, three frame records of 32 bytes, each part a multiple of 16
    assert valid == 96 + 5 * (-(-(8 * 1000 // 6 + 3) * 4 // 16) * 16) and refused == [0, 0, 0, 0]


def test_the_python_layer_names_the_cause_and_the_frame(lib, tmp_path):
    from this_and_that_vdm_amd import ingest
    with pytest.raises(ValueError, match="decode_gif: decodes on the HIP device, got cpu"):
        ingest.decode_gif(refusals.GOOD, "cpu")
    for name, data, _, fragment in refusals.FILES:
        with pytest.raises(ValueError) as e:
            ingest.decode_gif(data, "cuda:0")                      # refused by the parser: no device is touched
        assert fragment in str(e.value) and str(e.value).startswith("decode_gif: tt_gif_parse:"), (name, str(e.value))
    with pytest.raises(ValueError, match="frame 1's rectangle"):
        ingest.parse_gif(dict((n, d) for n, d, _, _ in refusals.FILES)["leaves the screen"])
    empty = g.gif_file(5, 4, [dict(indices=np.zeros((4, 5)), stream=b"")], global_table=np.zeros((4, 3)))   # an image whose data is the terminator alone
    assert ingest.parse_gif(empty).spans.tolist() == [[0, 0]]
    with pytest.raises(ValueError, match=r"decode_gif: frame 0 is corrupt or short \(no image data at all\)"):
        ingest.decode_gif(empty, "cuda:0")                         # named before a device is touched
    path = tmp_path / "bad.gif"
    path.write_bytes(b"GIF89a")
    with pytest.raises(ValueError, match="ends inside the logical screen descriptor"):
        ingest.read_gif(str(path))


def test_gif_host_under_address_and_undefined_sanitizers(tmp_path):
    """gif_host.cpp, lib.cpp and tests/gif_decode_host_check.cpp (its own main) built with the host compiler and run as a child process:
    nothing is preloaded and nothing of it runs under Python."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    csrc = os.path.join(REPO, "this_and_that_vdm_amd", "csrc")
    exe = str(tmp_path / "gif_decode_host_check")
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I",
           os.path.join(REPO, "include"), "-I", csrc, os.path.join(REPO, "tests", "gif_decode_host_check.cpp"), os.path.join(csrc, "gif_host.cpp"),
           os.path.join(csrc, "lib.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr or "sanitize" in built.stderr):
        pytest.skip("the compiler's sanitizer runtime is missing: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
