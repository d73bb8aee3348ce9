"""CPU: the segmented LZW format of include/ttvdm.h ("GIF LZW on the device") before any kernel runs -- the two host constructions of
tests/gif_lzw_reference.py against each other and against the host coder, the streams read back by the textbook decoder and by Pillow,
the inputs on the format's edges (found by search, asserted to be what they claim), every refusal of tt_gif_lzw_frames in a child
process that sees no GPU, and the two size functions against the longest streams.  Equality throughout."""
import io
import os
import struct

import numpy as np
import pytest

from tests import gif_lzw_reference as lz
from tests import gif_lzw_refusals as refusals
from tests import gif_reference as ref

NPIX = 384
SEGMENTS = (1, 2, 7, 64, 100, NPIX, NPIX + 1)
INPUTS = {"random": lambda mcs: lz.random_indices(NPIX, mcs, 20 + mcs), "constant": lambda mcs: np.full(NPIX, (1 << mcs) - 1, dtype=np.uint8),
          "checker": lambda mcs: lz.checker(NPIX)}


@pytest.fixture(scope="module")
def lib():
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("mcs", [2, 5, 8])
@pytest.mark.parametrize("kind", list(INPUTS))
def test_both_constructions_agree_and_decode(lib, kind, mcs):
    from this_and_that_vdm_amd import export
    px = INPUTS[kind](mcs)
    for segment in SEGMENTS:
        data = lz.restate(px, mcs, segment)
        assert data == lz.splice(px, mcs, segment, export.lzw_frame), (kind, mcs, segment)
        back, clears, _, used = ref.lzw_decode(data)             # the decoder itself asserts fewer than 8 padding bits
        assert np.array_equal(back, px) and used == len(data)
        assert clears >= -(-NPIX // segment), (segment, clears)
        if segment >= NPIX:
            assert data == export.lzw_frame(px, mcs)             # rule 8


def test_the_default_segment_is_the_built_one(lib):
    from this_and_that_vdm_amd import _lib
    assert lz.SEGMENT_DEFAULT == _lib.TT_LZW_SEGMENT and 9216 <= _lib.TT_LZW_SEGMENT_MAX == refusals.SEGMENT_MAX
    header = open(os.path.join(os.path.dirname(_lib.CSRC), "..", "include", "ttvdm.h")).read()
    assert f"#define TT_LZW_SEGMENT {_lib.TT_LZW_SEGMENT}\n" in header and f"#define TT_LZW_SEGMENT_MAX {_lib.TT_LZW_SEGMENT_MAX}\n" in header


def test_a_file_of_restated_streams_opens_in_pillow(lib):
    from PIL import Image, ImageSequence
    rng = np.random.default_rng(31)
    f, h, w = 3, 16, 24
    idx = rng.integers(0, 200, size=(f, h, w)).astype(np.uint8)
    pal = rng.integers(0, 256, size=(f, 256, 3)).astype(np.uint8)
    out = [b"GIF89a", struct.pack("<HHBBB", w, h, 0x70, 0, 0)]                # the container as write_gif_indexed writes it
    for i in range(f):
        out += [b"\x21\xf9\x04" + struct.pack("<BHB", 0, 5, 0) + b"\x00", b"\x2c" + struct.pack("<HHHHB", 0, 0, w, h, 0x80 | 7), pal[i].tobytes(),
                lz.restate(idx[i], 8, 100)]
    im = Image.open(io.BytesIO(b"".join(out) + b"\x3b"))
    frames = [np.asarray(fr.convert("RGB")) for fr in ImageSequence.Iterator(im)]
    assert len(frames) == f and im.size == (w, h)
    for i in range(f):
        assert np.array_equal(frames[i], pal[i][idx[i]]), i


# ---- the edges
def test_the_width_bump_input_is_one():
    px = lz.find_width_bump(2)
    codes, closing = lz.segment_codes(px, 2)
    assert closing == codes[-1][1] + 1                                        # the closing code is one bit wider than the last data code
    data = lz.restate(px, 2, px.size)
    assert lz.read_codes(data)[-1] == (5, closing) and np.array_equal(ref.lzw_decode(data)[0], px)
    two = np.concatenate([px, px])                                            # ... and the same as a clear code between two segments
    stream = lz.read_codes(lz.restate(two, 2, px.size))
    assert stream[len(codes) + 1] == (4, closing) and np.array_equal(ref.lzw_decode(lz.restate(two, 2, px.size))[0], two)


@pytest.mark.parametrize("target", [254, 255, 256, 510])
def test_the_sub_block_boundary_inputs_are_what_they_claim(target):
    px = lz.find_data_bytes(target)
    data = lz.restate(px, 8, 64)
    assert lz.data_bytes(data) == target
    blocks, pos = [], 1
    while data[pos]:
        blocks.append(data[pos])
        pos += 1 + data[pos]
    want = [255] * (target // 255) + ([target % 255] if target % 255 else [])  # no empty sub-block behind a full one
    assert blocks == want and pos == len(data) - 1 and len(data) == 2 + target + len(want)
    assert np.array_equal(ref.lzw_decode(data)[0], px)


def test_the_table_full_input_resets_inside_one_segment(lib):
    from this_and_that_vdm_amd import export
    px = lz.table_full_input()
    assert px.size == 9216 <= refusals.SEGMENT_MAX
    codes, _ = lz.segment_codes(px, 8)
    assert (256, 12) in codes                                                 # a clear code at 12 bits inside the segment
    data = lz.restate(px, 8, px.size)
    back, clears, widest, _ = ref.lzw_decode(data)
    assert clears >= 2 and widest == 12 and np.array_equal(back, px) and data == export.lzw_frame(px, 8)


# ---- the entry point's host half
def test_every_refusal_precedes_the_device():
    got = refusals.run_child()
    for fault, code, fragment in refusals.ROWS:
        rc, msg = got[refusals.row_id(fault)]
        assert rc == code and fragment in msg and msg.startswith("tt_gif_lzw_frames:"), (fault, rc, msg)
    for fault in refusals.SIZE_FAULTS:
        assert got["sizes:" + refusals.row_id(fault)] == [0, 0], fault
    assert got["sizes:n=0"][1] == 0
    bound, ws = got["sizes:valid"]
    assert bound > 0 and bound % 16 == 0 and ws > 0 and ws % 16 == 0


@pytest.mark.parametrize("npix,segment", [(1, 1), (255, 1), (4096, 1), (4096, 7), (9216, 9216), (9216, 0), (20000, 4096)])
def test_the_bounds_cover_the_longest_streams(lib, npix, segment):
    # all-distinct neighbours at min_code_size 8: no pair repeats inside a short segment, so every pixel costs a code
    px = (np.arange(npix) * 89 % 256).astype(np.uint8) if segment == 1 else lz.random_indices(npix, 8, npix)
    data = lz.restate(px, 8, segment or None)
    bound = lib.tt_gif_lzw_frames_bound(npix, segment)
    assert bound % 16 == 0 and len(data) <= bound, (len(data), bound)
    seg = segment or lz.SEGMENT_DEFAULT
    most = max(len(lz.segment_codes(px[at:at + seg], 8)[0]) for at in range(0, npix, seg))
    nseg = -(-npix // seg)
    # the workspace holds at least two words and the codes (uint16) of every segment
    assert lib.tt_gif_lzw_frames_ws_bytes(2, npix, segment) >= 2 * nseg * (8 + 2 * most)


def test_the_python_layer_refuses_before_it_touches_a_device(lib):
    from this_and_that_vdm_amd import export
    idx = np.zeros((2, 4, 4), dtype=np.uint8)
    pal = np.zeros((2, 256, 3), dtype=np.uint8)
    for fn, args in ((export.write_gif_indexed, (idx, pal, [1, 1], io.BytesIO())), (export.write_gif, (np.zeros((2, 4, 4, 3), dtype=np.uint8), io.BytesIO()))):
        for bad in ("gpu", "", None):
            with pytest.raises(ValueError, match="lzw"):
                fn(*args, lzw=bad)
