"""GPU: progressive JPEG files decoded on the device (include/ttvdm.h, "JPEG import", rule 4b).  ``ingest.decode_jpeg(...,
progressive=True)`` of Pillow's own ``progressive=True`` files against ``np.asarray(Image.open(f))`` -- one block, partial MCUs whose Y
plane has real blocks the MCU grid pads, grey / 4:4:4 / 4:2:0, three qualities, four kinds of frame --; the scan scripts Pillow never
writes, from the writer of tests/jpeg_progressive_reference.py, several scripts in ONE call; scans longer than one sequence of the
decoder; EOB runs over a whole frame; one call that mixes a baseline file, a Pillow file and a writer's file; a scan cut short and a
flipped byte inside an AC refinement, each run through the restatement's emulation of the kernel first; ``DevicePixels.from_jpeg``.

Nothing here is a tolerance: the format is integers from end to end, so equality is the bound."""
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_progressive_reference as pr
from tests import jpeg_reference as ref
from this_and_that_vdm_amd import _lib, ingest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = {"grey": (1, 0), "444": (3, 0), "420": (3, 2)}

if not os.path.exists(_lib.LIB_PATH):
    _lib.build()


def _pillow(frame, quality, sub, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame[..., 0] if frame.shape[2] == 1 else frame).save(buf, format="JPEG", quality=quality, subsampling=sub, **kw)
    return buf.getvalue()


def _pillow_pixels(data):
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


def _written(h, w, ch, sub, script, quality=75, seed=3):
    frame = ref.noise_frame(h, w, seed, ch) // 2 + ref.smooth_frame(h, w, seed, ch) // 2
    coefs, comps, _ = ref.coefficients(frame, quality, sub)
    return pr.progressive_file(coefs, h, w, ch, quality, sub, script), ref.file_of(ref.scan_bytes(coefs, comps), h, w, ch, quality, sub)


# ---- 1. Pillow's own progressive files: the twelve files of a size and format (3 qualities x 4 frames) are one call
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("size", [(8, 8), (17, 23), (40, 24), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_pillows_progressive_files_decode_to_pillows_pixels(size, fmt):
    (h, w), (ch, sub) = size, FORMATS[fmt]
    frames = [ref.smooth_frame(h, w, 1, ch), ref.noise_frame(h, w, 2, ch), ref.checker_frame(h, w, ch), ref.flat_frame(h, w, 77, ch)]
    files = [_pillow(f, q, sub, progressive=True) for q in (30, 75, 95) for f in frames]
    assert all(b"\xff\xc2" in f for f in files)
    got = ingest.decode_jpeg(files, DEV, progressive=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (len(files), h, w, ch)
    got = got.cpu().numpy()
    for i, f in enumerate(files):
        assert np.array_equal(got[i], _pillow_pixels(f)), (size, fmt, i)


# ---- 2. the writer's scripts: every script of a shape in ONE call (frames with different scan scripts and scan counts share it)
@pytest.mark.parametrize("shape", [(17, 23, 3, 2), (24, 40, 3, 0), (33, 40, 1, 0), (8, 8, 1, 0)], ids=["17x23-420", "24x40-444", "33x40-grey", "8x8-grey"])
def test_the_writers_scripts_in_one_call_equal_the_restatement_and_pillow(shape):
    h, w, ch, sub = shape
    names = sorted(pr.SCRIPTS)
    files = [_written(h, w, ch, sub, pr.SCRIPTS[n](ch), seed=k)[0] for k, n in enumerate(names)]
    assert len({len(ingest.parse_jpeg_progressive(f).scans) for f in files}) > 1
    got = ingest.decode_jpeg(files, DEV, progressive=True).cpu().numpy()
    for i, f in enumerate(files):
        want, status = pr.decode(f, (1024, 256))
        assert status == 0 and np.array_equal(want, _pillow_pixels(f))
        assert np.array_equal(got[i], want), (shape, names[i])


def test_the_coefficients_equal_the_restatements_scan_by_scan_layout():
    """the entropy stage on its own: the coefficient buffer a 4:2:0 file with partial MCUs leaves, dummy blocks included"""
    from this_and_that_vdm_amd import ops
    data = _pillow(ref.noise_frame(17, 23, 4, 3), 75, 2, progressive=True)
    hd = ingest.parse_jpeg_progressive(data)
    want, status = pr.entropy(data, pr.parse(data))
    assert status == 0
    n = len(hd.scans)
    blob = np.frombuffer(b"".join(data[s.offset:s.offset + s.bytes] for s in hd.scans), dtype=np.uint8).copy()
    lens = np.array([s.bytes for s in hd.scans], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    desc = np.zeros((n, 8), dtype=np.int32)
    tables = np.zeros((n, 3, 256), dtype=np.uint32)
    for i, s in enumerate(hd.scans):
        desc[i, :5] = (sum(1 << c for c in s.components), s.ss, s.se, s.ah, s.al)
        for slot in (s.components if (s.ss == 0 and s.ah == 0) else ((0,) if s.ss else ())):
            tables[i, slot] = ingest.jpeg_decode_table(s.bits[slot], s.huffval[slot])
    dev = lambda a: torch.from_numpy(a).to(DEV)
    coeffs, st = ops.jpeg_entropy_progressive(dev(blob), dev(offs), dev(lens), dev(desc), dev(tables.view(np.int32)), int(lens.max()), 1, (17, 23, 3), "4:2:0")
    assert st.cpu().tolist() == [0] and np.array_equal(coeffs.cpu().numpy()[0], want)


# ---- 3. more than one sequence per scan
def test_scans_longer_than_one_sequence_carry_their_state():
    """512 x 512 grey noise at quality 95: an AC-first scan and an AC-refinement scan each longer than tt_jpeg_sequence_bits (asserted
    from the parsed header), so the carried state of the lanes and the staged windows of the refinement's walk are both exercised"""
    data = _pillow(ref.noise_frame(512, 512, 6, 1), 95, 0, progressive=True)
    hd = ingest.parse_jpeg_progressive(data)
    seq = _lib.load().tt_jpeg_sequence_bits()
    assert any(s.ss > 0 and s.ah == 0 and 8 * s.bytes > seq for s in hd.scans)
    assert any(s.ss > 0 and s.ah > 0 and 8 * s.bytes > seq for s in hd.scans)
    got = ingest.decode_jpeg([data], DEV, progressive=True).cpu().numpy()
    assert np.array_equal(got[0], _pillow_pixels(data))


# ---- 4. long EOB runs
def test_a_flat_frame_is_one_eob_run_per_scan():
    """1024 x 1024 grey, flat: 16 384 blocks are a single EOB14 symbol per AC scan (Pillow writes 2-byte AC scans: asserted)"""
    data = _pillow(ref.flat_frame(1024, 1024, 131, 1), 75, 0, progressive=True)
    hd = ingest.parse_jpeg_progressive(data)
    assert all(s.bytes == 2 for s in hd.scans if s.ss > 0)
    got = ingest.decode_jpeg([data], DEV, progressive=True).cpu().numpy()
    assert np.array_equal(got[0], _pillow_pixels(data))
    colour = [_pillow(ref.flat_frame(64, 64, v, 3), 75, sub, progressive=True) for v, sub in ((9, 2), (250, 0))]
    for f in colour:
        assert np.array_equal(ingest.decode_jpeg(f, DEV, progressive=True).cpu().numpy()[0], _pillow_pixels(f))


# ---- 5. one call with mixed inputs
def test_one_call_mixes_baseline_pillow_progressive_and_written_files():
    h, w, ch, sub = 17, 23, 3, 2
    base = _pillow(ref.smooth_frame(h, w, 5, ch), 85, sub)
    prog = _pillow(ref.noise_frame(h, w, 6, ch), 60, sub, progressive=True)
    odd = _written(h, w, ch, sub, pr.script_separate_dc(ch))[0]
    files = [prog, base, odd, base, prog]
    got = ingest.decode_jpeg(files, DEV, progressive=True)
    assert tuple(got.shape) == (5, h, w, ch) and got.is_contiguous()
    for i, f in enumerate(files):
        assert np.array_equal(got[i].cpu().numpy(), _pillow_pixels(f)), i
    alone = ingest.decode_jpeg([base], DEV)
    assert torch.equal(got[1], alone[0]) and torch.equal(got[3], alone[0])
    assert torch.equal(ingest.decode_jpeg([base, base], DEV, progressive=True), ingest.decode_jpeg([base, base], DEV))
    with pytest.raises(ValueError, match="file 0: tt_jpeg_parse: SOF2: progressive"):                    # the default keeps refusing
        ingest.decode_jpeg(files, DEV)


# ---- 6. corrupt inputs: built on the CPU and run through the emulation of the kernel first
def test_a_cut_scan_and_a_flipped_byte_are_named_and_nothing_faults():
    h, w, ch, sub = 40, 24, 3, 2
    good = _pillow(ref.noise_frame(h, w, 8, ch), 90, sub, progressive=True)
    hd = pr.parse(good)
    cases = []
    for k in (0, 1, 5, 9):                                               # DC first, AC first, AC refine 2 -> 1, AC refine 1 -> 0: the scan's second half is cut out
        sc = hd["scans"][k]
        cases.append(good[:sc["offset"] + sc["bytes"] // 2] + good[sc["offset"] + sc["bytes"]:])
    sc = hd["scans"][9]                                                  # a byte flipped inside the last AC refinement: the first flip the emulation rejects
    for at in range(sc["offset"] + 2, sc["offset"] + sc["bytes"] - 2):
        if good[at] in (0x00, 0xff) or good[at - 1] == 0xff or good[at] ^ 0x55 == 0xff:
            continue
        flipped = good[:at] + bytes([good[at] ^ 0x55]) + good[at + 1:]
        if pr.decode(flipped, (1024, 256))[1]:
            cases.append(flipped)
            break
    assert len(cases) == 5
    for data in cases:
        assert ingest.parse_jpeg_progressive(data).height == h       # the container is whole: only the device sees the damage
        status = pr.decode(data, (1024, 256))[1]                        # what the kernel will do with it, known before it is sent
        assert status != 0
        with pytest.raises(ValueError, match=rf"decode_jpeg: frame 1 is corrupt or truncated \(.*; status {status}\)"):
            ingest.decode_jpeg([good, data, good], DEV, progressive=True)
    # ... and the frames beside a corrupt one are untouched by it: the good file alone, after all of the above
    assert np.array_equal(ingest.decode_jpeg([good], DEV, progressive=True).cpu().numpy()[0], _pillow_pixels(good))


# ---- 7. the request path
def test_from_jpeg_takes_a_progressive_file(tmp_path):
    from PIL import Image
    from this_and_that_vdm_amd.svd.pipeline_utils import DevicePixels
    path = str(tmp_path / "web.jpg")
    Image.fromarray(ref.smooth_frame(96, 160, 4, 3)).save(path, quality=80, progressive=True, subsampling=2)
    with Image.open(path) as im:
        want = np.asarray(im.convert("RGB"))
    pixels = DevicePixels.from_jpeg(path, DEV)
    assert tuple(pixels.shape) == (1, 96, 160, 3) and np.array_equal(pixels.pixels.cpu().numpy()[0], want)
