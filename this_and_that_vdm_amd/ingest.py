"""Baseline and progressive JPEG files decoded on the device (include/ttvdm.h, "JPEG import"): a clip folder im_0.jpg .. im_{F-1}.jpg, a folder
``export.write_jpegs`` wrote, a Motion-JPEG AVI or a request's image become uint8 [F, H, W, ch] NHWC device tensors holding byte for
byte what ``np.asarray(PIL.Image.open(f))`` holds.  The host reads the files' headers (tt_jpeg_parse_spans) and builds the decode tables
(tt_jpeg_decode_table); only the compressed scans cross to the device, where they are unstuffed, entropy-decoded, dequantised,
inverted, upsampled and converted.  There is no CPU fallback and no Pillow here.

Restart intervals: a file with a DRI segment and RSTn markers (``export.write_jpegs(..., restart_rows=1)``'s, a camera's) is cut into
the spans between its markers, and the entropy decoder gives every span a workgroup of its own instead of one per frame.  A file
without them is one span and decodes through the same launches as before; the reference dataset's own im_0.jpg files carry none.

Progressive files (SOF2: what web images usually are, ``PIL.save(progressive=True)``'s): ``decode_jpeg(..., progressive=True)`` reads
every scan's place, band, Ah / Al and tables (tt_jpeg_parse_progressive), uploads the scans' bytes, and the device applies them round by
round into the baseline route's coefficient buffer (tt_jpeg_entropy_progressive: DC first, DC refine, AC first, AC refine); the same
reconstruction then runs.  A call may mix baseline and progressive files and scan scripts.  Without the keyword a progressive file is
refused by name, as before; ``DevicePixels.from_jpeg`` -- the request path -- passes it.

Not applied: EXIF orientation (``load_image`` of the reference applies it; rotate the result when the files carry one).  Refused by
name: arithmetic and 12-bit files, 4:2:2, CMYK / Adobe files, restart markers out of order or count, several scans in a baseline file;
in a progressive file restart intervals, a DQT between scans and an INCOMPLETE progression (libjpeg smooths those; they are not decoded
differently); progressive files altogether unless ``progressive=True``.

Animated GIFs (include/ttvdm.h, "GIF import"): ``decode_gif`` / ``read_gif`` turn the file ``export.write_gif`` (or Pillow, or imageio)
wrote into uint8 [F, H, W, 3] on the device, per frame the canvas Pillow shows after ``seek(f)``.  The host walks the container
(tt_gif_parse); the LZW streams, the interlace and the composition run on the device."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check

_SUBSAMPLING = {_lib.TT_JPEG_444: "4:4:4", _lib.TT_JPEG_420: "4:2:0"}


@dataclass
class JpegHeader:
    """What ``parse_jpeg`` reads from one file: the geometry, ``subsampling`` ("4:4:4" / "4:2:0"; grey files are "4:4:4"), the byte range
    of the entropy-coded scan, ``quant`` uint8 [3, 64] (per component, natural order), ``dc_table`` / ``ac_table`` (per component, 0 or
    1), the Huffman tables DC 0, AC 0, DC 1, AC 1 as ``bits`` uint8 [4, 16] and ``huffval`` uint8 [4, 256], ``restart_interval`` (MCUs; 0:
    none) and ``spans``: int64 [S, 2], per restart interval of the scan its byte offset in the file and its stuffed length, markers
    excluded -- one row, the scan's range, for a file without markers."""
    height: int
    width: int
    channels: int
    subsampling: str
    scan_offset: int
    scan_bytes: int
    quant: np.ndarray
    dc_table: list
    ac_table: list
    bits: np.ndarray
    huffval: np.ndarray
    restart_interval: int = 0
    spans: np.ndarray = None


def parse_jpeg(data: bytes) -> JpegHeader:
    """One baseline JPEG file -> its header and the spans of its scan (tt_jpeg_parse_spans: once to count the spans, once to take
    them); ValueError with the library's text for what is refused."""
    lib = _lib.load()
    hd = _lib.TtJpegHeader()
    buf = np.frombuffer(data, dtype=np.uint8)
    at = buf.ctypes.data if buf.size else None
    ri, count = C.c_int32(0), C.c_int64(0)
    rc = lib.tt_jpeg_parse_spans(at, buf.size, C.byref(hd), C.byref(ri), None, None, 0, C.byref(count))
    if rc == 0:
        offs, lens = np.zeros(count.value, dtype=np.int64), np.zeros(count.value, dtype=np.int64)
        rc = lib.tt_jpeg_parse_spans(at, buf.size, C.byref(hd), C.byref(ri), offs.ctypes.data, lens.ctypes.data, offs.size, C.byref(count))
    if rc != 0:
        raise ValueError(lib.tt_last_error().decode(errors="replace"))
    return JpegHeader(hd.h, hd.w, hd.ch, _SUBSAMPLING[hd.subsampling], hd.scan_offset, hd.scan_bytes,
                      np.ctypeslib.as_array(hd.quant).copy(), list(hd.dc_table)[:hd.ch], list(hd.ac_table)[:hd.ch],
                      np.ctypeslib.as_array(hd.bits).copy(), np.ctypeslib.as_array(hd.huffval).copy(), ri.value, np.stack([offs, lens], axis=1))


@dataclass
class JpegScan:
    """One scan of a progressive file: ``components`` (indices into the frame's components, ascending), the band ``ss`` .. ``se``, ``ah`` /
    ``al``, the byte range of its entropy-coded segment in the file, and the Huffman tables in force at its SOS as ``bits`` uint8 [3, 16]
    / ``huffval`` uint8 [3, 256]: a DC-first scan's DC table of component c at [c], an AC scan's AC table at [0], zeros for a DC-refine scan."""
    components: tuple
    ss: int
    se: int
    ah: int
    al: int
    offset: int
    bytes: int
    bits: np.ndarray
    huffval: np.ndarray


@dataclass
class JpegProgressiveHeader:
    """What ``parse_jpeg_progressive`` reads from one progressive (SOF2) file: the geometry, ``subsampling``, ``quant`` uint8 [3, 64] (per
    component, natural order) and the ``scans`` in file order."""
    height: int
    width: int
    channels: int
    subsampling: str
    quant: np.ndarray
    scans: list


def parse_jpeg_progressive(data: bytes) -> JpegProgressiveHeader:
    """One progressive JPEG file -> its header and scans (tt_jpeg_parse_progressive: once to count the scans, once to take them);
    ValueError with the library's text for what is refused -- a baseline file, an incomplete progression and the rest of rule 1b."""
    lib = _lib.load()
    hd = _lib.TtJpegProgressiveHeader()
    buf = np.frombuffer(data, dtype=np.uint8)
    at = buf.ctypes.data if buf.size else None
    count = C.c_int64(0)
    rc = lib.tt_jpeg_parse_progressive(at, buf.size, C.byref(hd), None, 0, C.byref(count))
    if rc == 0:
        rows = (_lib.TtJpegScan * count.value)()
        rc = lib.tt_jpeg_parse_progressive(at, buf.size, C.byref(hd), C.cast(rows, C.c_void_p), count.value, C.byref(count))
    if rc != 0:
        raise ValueError(lib.tt_last_error().decode(errors="replace"))
    scans = [JpegScan(tuple(c for c in range(3) if r.comps >> c & 1), r.ss, r.se, r.ah, r.al, r.offset, r.bytes,
                      np.ctypeslib.as_array(r.bits).copy(), np.ctypeslib.as_array(r.huffval).copy()) for r in rows]
    return JpegProgressiveHeader(hd.h, hd.w, hd.ch, _SUBSAMPLING[hd.subsampling], np.ctypeslib.as_array(hd.quant).copy(), scans)


def jpeg_decode_table(bits, huffval) -> np.ndarray:
    """BITS [16] and HUFFVAL (up to 256 symbols by ascending code) -> uint32 [256]: the table the decoder reads (tt_jpeg_decode_table)"""
    b = np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1)
    v = np.zeros(256, dtype=np.uint8)
    vals = np.asarray(huffval, dtype=np.uint8).reshape(-1)
    if b.size != 16 or vals.size > 256:
        raise ValueError(f"jpeg_decode_table: 16 BITS and at most 256 symbols, got {b.size} and {vals.size}")
    v[:vals.size] = vals
    out = np.zeros(_lib.TT_JPEG_DECODE_WORDS, dtype=np.uint32)
    check(_lib.load().tt_jpeg_decode_table(b.ctypes.data, v.ctypes.data, out.ctypes.data), "tt_jpeg_decode_table")
    return out


def jpeg_decode_set(tables, dc_table=(0, 1, 1), ac_table=(0, 1, 1)) -> np.ndarray:
    """Four (BITS, HUFFVAL) pairs -- DC 0, AC 0, DC 1, AC 1 -- and the components' table indices -> uint32 [1028]: one frame's table set.
    The defaults are the export's map: luminance on the tables 0, both chrominance components on the tables 1 (pass
    ``export.jpeg_standard_tables()`` in ITS order DC lum, AC lum, DC chr, AC chr: the same slots)."""
    out = np.zeros(_lib.TT_JPEG_DECODE_SET_WORDS, dtype=np.uint32)
    for k, t in enumerate(tables):
        bits, vals = (t.bits, t.huffval) if hasattr(t, "bits") else t
        out[k * 256:(k + 1) * 256] = jpeg_decode_table(bits, vals)
    word = 0
    for c, (d, a) in enumerate(zip(dc_table, ac_table)):
        if d not in (0, 1) or a not in (0, 1):
            raise ValueError(f"jpeg_decode_set: table indices are 0 or 1, got DC {d} / AC {a} for component {c}")
        word |= (d << (2 * c)) | (a << (2 * c + 1))
    out[4 * 256] = word
    return out


def _read(f) -> bytes:
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    with open(os.fspath(f), "rb") as fh:
        return fh.read()


def decode_jpeg(files, device, progressive: bool = False) -> torch.Tensor:
    """JPEG files of ONE geometry and subsampling -- bytes or paths, one or a list -- -> uint8 [F, H, W, ch] on ``device``, ch 1
    (grey) or 3 (RGB): Pillow's decoded pixels, byte for byte.  One upload (the scans, end to end), one readback (a status word per
    frame).  Files with restart markers are decoded span by span, one workgroup each; the files of a call may carry different restart
    intervals, or none.  ``progressive=True``: a progressive (SOF2) file is accepted as well and takes the scan-by-scan route
    (tt_jpeg_parse_progressive / tt_jpeg_entropy_progressive); the files of a call may mix baseline and progressive files and scan
    scripts, every baseline file goes through the launches it goes through without the keyword, and the frames come back in file order.
    The default refuses progressive files by name, as before.  ValueError: a file the parser refuses (its text names the cause), files
    that differ in size or subsampling, more than 65535 spans in all, a frame whose scan is corrupt or truncated (the frame is named)."""
    items = list(files) if isinstance(files, (list, tuple)) else [files]
    if not items:
        raise ValueError("decode_jpeg: no files")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"decode_jpeg: decodes on the HIP device, got {device} (there is no CPU fallback)")
    datas, heads = [], []
    for i, f in enumerate(items):
        data = _read(f)
        try:
            try:
                hd = parse_jpeg(data)
            except ValueError as e:
                if not (progressive and "SOF2: progressive" in str(e)):
                    raise
                hd = parse_jpeg_progressive(data)
        except ValueError as e:
            raise ValueError(f"decode_jpeg: file {i}: {e}") from None
        if heads and (hd.height, hd.width, hd.channels, hd.subsampling) != (heads[0].height, heads[0].width, heads[0].channels, heads[0].subsampling):
            raise ValueError(f"decode_jpeg: file {i} is {hd.height} x {hd.width} x {hd.channels} {hd.subsampling}, file 0 is {heads[0].height} x "
                             f"{heads[0].width} x {heads[0].channels} {heads[0].subsampling}: one geometry and subsampling per call")
        if isinstance(hd, JpegHeader) and hd.scan_bytes < 1:
            raise ValueError(f"decode_jpeg: file {i}: an empty scan")
        heads.append(hd)
        datas.append(data)
    base = [i for i, h in enumerate(heads) if isinstance(h, JpegHeader)]
    prog = [i for i, h in enumerate(heads) if not isinstance(h, JpegHeader)]
    parts = []
    if base:
        parts.append((base, _decode_baseline([heads[i] for i in base], [datas[i] for i in base], device, base)))
    if prog:
        parts.append((prog, _decode_progressive([heads[i] for i in prog], [datas[i] for i in prog], device, prog)))
    for index, (status, _) in parts:                                                               # one readback a route
        for k, s in enumerate(status.cpu().tolist()):
            if s:
                why = ", ".join(text for bit, text in _lib.TT_JPEG_STATUS.items() if s & bit)
                raise ValueError(f"decode_jpeg: frame {index[k]} is corrupt or truncated ({why}; status {s})")
    if len(parts) == 1:
        return parts[0][1][1]
    h0 = heads[0]
    out = torch.empty((len(heads), h0.height, h0.width, h0.channels), dtype=torch.uint8, device=device)
    for index, (_, frames) in parts:
        out[torch.tensor(index, device=device)] = frames
    return out


def _decode_baseline(heads, datas, device, index):
    """decode_jpeg's baseline route: the files' scans (or restart spans) -> (status int32 [F], frames); ``index``: the files' places in
    the call, for the texts"""
    from . import ops
    blobs = [d[h.scan_offset:h.scan_offset + h.scan_bytes] for h, d in zip(heads, datas)]
    h0 = heads[0]
    lens = np.array([len(b) for b in blobs], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    marked = any(len(h.spans) > 1 for h in heads)
    if marked:                                                                                     # before any upload
        # every span: where it lies in the uploaded scans, its frame, its first block there and its blocks (Ri MCUs; the last may be shorter)
        blocks = _lib.load().tt_jpeg_blocks(h0.height, h0.width, h0.channels, ops.JPEG_SUBSAMPLING[h0.subsampling])
        bpm = 1 if h0.channels == 1 else (6 if h0.subsampling == "4:2:0" else 3)
        rows = []
        for i, h in enumerate(heads):
            per = h.restart_interval * bpm if len(h.spans) > 1 else blocks
            for k, (o, n) in enumerate(h.spans.tolist()):
                rows.append((offs[i] + o - h.scan_offset, n, i, k * per, min(per, blocks - k * per)))
        if len(rows) > _lib.TT_JPEG_MAX_SPANS:
            raise ValueError(f"decode_jpeg: {len(rows)} restart intervals in {len(heads)} files: more spans than one call decodes ({_lib.TT_JPEG_MAX_SPANS})")
        rows = np.array(rows, dtype=np.int64)
        if rows[:, 1].min() < 1:
            i = index[int(rows[int(rows[:, 1].argmin()), 2])]
            raise ValueError(f"decode_jpeg: file {i}: an empty restart interval")
    same_tables = all(np.array_equal(h.bits, h0.bits) and np.array_equal(h.huffval, h0.huffval) and h.dc_table == h0.dc_table and h.ac_table == h0.ac_table
                      for h in heads[1:])
    same_quant = all(np.array_equal(h.quant, h0.quant) for h in heads[1:])

    def table_set(h):
        pad = [0] * (3 - h.channels)
        return jpeg_decode_set([(h.bits[k], h.huffval[k]) for k in range(4)], h.dc_table + pad, h.ac_table + pad)

    sets = np.stack([table_set(h) for h in (heads[:1] if same_tables else heads)])
    quant = np.stack([h.quant for h in (heads[:1] if same_quant else heads)])
    scans = torch.from_numpy(np.frombuffer(b"".join(blobs), dtype=np.uint8).copy()).to(device)
    shape = (h0.height, h0.width, h0.channels)
    tables = torch.from_numpy(sets.view(np.int32)).to(device)
    if marked:
        cols = torch.from_numpy(np.ascontiguousarray(rows.T)).to(device)                       # one more small upload: five numbers a span
        coeffs, status = ops.jpeg_entropy_spans(scans, cols[0].contiguous(), cols[1].to(torch.int32), cols[2].to(torch.int32), cols[3].to(torch.int32),
                                                cols[4].to(torch.int32), int(rows[:, 1].max()), len(heads), shape, h0.subsampling, tables)
    else:
        coeffs, status = ops.jpeg_entropy(scans, torch.from_numpy(offs).to(device), torch.from_numpy(lens.astype(np.int32)).to(device), int(lens.max()), shape,
                                          h0.subsampling, tables)
    return status, ops.jpeg_pixels(coeffs, shape, h0.subsampling, torch.from_numpy(quant).to(device))


def _progressive_items(heads, datas, index):
    """The (file, scan) items of tt_jpeg_entropy_progressive: item f S + s is scan s of file f, S the most scans a file has -> (the
    segments end to end, offsets int64 [F S], lengths int32 [F S], desc int32 [F S, 8], tables uint32 [F S, 3, 256])"""
    n, most = len(heads), max(len(h.scans) for h in heads)
    if n * most > _lib.TT_JPEG_MAX_ITEMS:
        raise ValueError(f"decode_jpeg: {n} progressive files of up to {most} scans: more scans than one call decodes ({_lib.TT_JPEG_MAX_ITEMS})")
    offs, lens = np.zeros(n * most, dtype=np.int64), np.zeros(n * most, dtype=np.int32)
    desc = np.zeros((n * most, _lib.TT_JPEG_SCAN_WORDS), dtype=np.int32)
    tables = np.zeros((n * most, 3, _lib.TT_JPEG_DECODE_WORDS), dtype=np.uint32)
    blobs, at, made = [], 0, {}

    def table(bits, huffval):
        key = bits.tobytes() + huffval.tobytes()
        if key not in made:
            made[key] = jpeg_decode_table(bits, huffval)
        return made[key]

    for i, (h, data) in enumerate(zip(heads, datas)):
        for s, sc in enumerate(h.scans):
            item = i * most + s
            blobs.append(data[sc.offset:sc.offset + sc.bytes])
            offs[item], lens[item] = at, sc.bytes
            at += sc.bytes
            desc[item, :5] = (sum(1 << c for c in sc.components), sc.ss, sc.se, sc.ah, sc.al)
            try:
                if sc.ss == 0 and sc.ah == 0:
                    for c in sc.components:
                        tables[item, c] = table(sc.bits[c], sc.huffval[c])
                elif sc.ss > 0:
                    tables[item, 0] = table(sc.bits[0], sc.huffval[0])
            except RuntimeError as e:
                raise ValueError(f"decode_jpeg: file {index[i]}: scan {s}: {e}") from None
    if at < 1:
        raise ValueError(f"decode_jpeg: file {index[0]}: empty scans")
    return np.frombuffer(b"".join(blobs), dtype=np.uint8).copy(), offs, lens, desc, tables


def _decode_progressive(heads, datas, device, index):
    """decode_jpeg's progressive route: every scan of every file in one call -> (status int32 [F], frames)"""
    from . import ops
    h0 = heads[0]
    blob, offs, lens, desc, tables = _progressive_items(heads, datas, index)
    shape = (h0.height, h0.width, h0.channels)
    coeffs, status = ops.jpeg_entropy_progressive(torch.from_numpy(blob).to(device), torch.from_numpy(offs).to(device), torch.from_numpy(lens).to(device),
                                                  torch.from_numpy(desc).to(device), torch.from_numpy(tables.view(np.int32)).to(device), max(int(lens.max()), 1),
                                                  len(heads), shape, h0.subsampling)
    same_quant = all(np.array_equal(h.quant, h0.quant) for h in heads[1:])
    quant = np.stack([h.quant for h in (heads[:1] if same_quant else heads)])
    return status, ops.jpeg_pixels(coeffs, shape, h0.subsampling, torch.from_numpy(quant).to(device))


def read_jpegs(folder, pattern: str = "im_{idx}.jpg", device="cuda", progressive: bool = False) -> torch.Tensor:
    """``folder/pattern.format(idx=i)`` for i = 0, 1, ... up to the first missing index -- the layout the data loaders read a clip from
    and ``export.write_jpegs`` writes -- decoded by ``decode_jpeg``; ``progressive`` is passed on to it."""
    paths = []
    while os.path.exists(os.path.join(folder, pattern.format(idx=len(paths)))):
        paths.append(os.path.join(folder, pattern.format(idx=len(paths))))
        if len(paths) > 1 and paths[-1] == paths[-2]:
            raise ValueError(f"read_jpegs: pattern {pattern!r} names two frames alike (use {{idx}})")
    if not paths:
        raise ValueError(f"read_jpegs: {os.path.join(folder, pattern.format(idx=0))} does not exist")
    return decode_jpeg(paths, device, progressive=progressive)


def read_mjpeg_video(path, device="cuda") -> torch.Tensor:
    """The frames of a Motion-JPEG AVI (``export.write_mjpeg``'s) decoded by ``decode_jpeg``."""
    from . import export
    return decode_jpeg(export.read_mjpeg_frames(path), device)


# ---- animated GIFs (include/ttvdm.h, "GIF import"): the container on the host, LZW, interlace and composition on the device
@dataclass
class GifHeader:
    """What ``parse_gif`` reads from one file: the logical screen (``height``, ``width``, ``background`` index), ``loop`` (the NETSCAPE2.0
    count, 0 for ever; None without the block), and per frame ``rectangles`` int32 [F, 4] (left, top, w, h), ``durations`` (seconds),
    ``disposal`` (bits 0 .. 7), ``transparent`` (index, -1 for none), ``interlace``, ``min_code_size``, ``palettes`` uint8 [F, 256, 3] (the
    local table, else the global one, zero-padded), ``local`` (the frame has a table of its own), and ``spans`` int64 [F, 2]: where the
    frame's LZW bytes lie in ``data`` (the sub-blocks' payload of all frames, end to end) and how many they are."""
    height: int
    width: int
    background: int
    loop: object
    version: int
    rectangles: np.ndarray
    durations: list
    disposal: list
    transparent: list
    interlace: list
    min_code_size: list
    palettes: np.ndarray
    local: list
    spans: np.ndarray
    data: np.ndarray

    @property
    def frames(self) -> int:
        return len(self.disposal)


def parse_gif(data: bytes) -> GifHeader:
    """One GIF87a / GIF89a file -> its header, its frames' tables and their LZW bytes (tt_gif_parse: once to count, once to take them);
    ValueError with the library's text, which names the cause and the frame, for what is refused."""
    lib = _lib.load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    at = buf.ctypes.data if buf.size else None
    hd = _lib.TtGifHeader()
    rc = lib.tt_gif_parse(at, buf.size, C.byref(hd), None, 0, None, 0)
    if rc == 0:
        frames = (_lib.TtGifFrame * hd.frames)()
        upload = np.zeros(max(hd.data_bytes, 1), dtype=np.uint8)
        rc = lib.tt_gif_parse(at, buf.size, C.byref(hd), C.cast(frames, C.c_void_p), hd.frames, upload.ctypes.data, hd.data_bytes)
    if rc != 0:
        raise ValueError(lib.tt_last_error().decode(errors="replace"))
    rec = np.frombuffer(frames, dtype=np.uint8).reshape(hd.frames, C.sizeof(_lib.TtGifFrame))
    ints = rec[:, :40].copy().view(np.int32)                                                       # left .. local_colors
    spans = rec[:, 40:56].copy().view(np.int64)
    return GifHeader(hd.height, hd.width, hd.background, None if hd.loop < 0 else hd.loop, hd.version, ints[:, 0:4].copy(),
                     [v / 100.0 for v in ints[:, 7].tolist()], ints[:, 6].tolist(), ints[:, 5].tolist(), [bool(v) for v in ints[:, 4].tolist()],
                     ints[:, 8].tolist(), rec[:, 56:].reshape(hd.frames, 256, 3).copy(), [bool(v) for v in ints[:, 9].tolist()], spans,
                     upload[:hd.data_bytes])


def decode_gif(file, device, info: bool = False):
    """One GIF file -- bytes or a path -- -> uint8 [F, H, W, 3] on ``device``: per frame the canvas after it is drawn, byte for byte
    what Pillow's ``seek(f)`` + ``convert("RGB")`` holds (outside Pillow's two departures from GIF89a that include/ttvdm.h names).  One
    upload of the compressed bytes, a small upload of the tables, one readback (a status word per frame).  ``info=True``: also the
    ``GifHeader``.  ValueError: a file the parser refuses (its text names the cause and the frame), a frame whose LZW stream is corrupt
    or short (the frame is named), a ``device`` that is not the HIP device."""
    from . import ops
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"decode_gif: decodes on the HIP device, got {device} (there is no CPU fallback)")
    try:
        hd = parse_gif(_read(file))
    except ValueError as e:
        raise ValueError(f"decode_gif: {e}") from None
    n = hd.frames
    if hd.data.size < 1:
        raise ValueError("decode_gif: frame 0 is corrupt or short (no image data at all)")
    rect = hd.rectangles.astype(np.int64)
    npix = rect[:, 2] * rect[:, 3]
    map_offsets = np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64)
    rows = np.where(np.array(hd.interlace), rect[:, 3], 0)
    cols = np.stack([hd.spans[:, 0], map_offsets, hd.spans[:, 1], npix, np.array(hd.min_code_size, dtype=np.int64), rows]).astype(np.int64)
    # rule 5: the fill colour of disposal 2 and the canvas before frame 0
    pal = hd.palettes.astype(np.uint32)
    packed = pal[:, :, 0] | (pal[:, :, 1] << 8) | (pal[:, :, 2] << 16)
    table = (_lib.TtGifComposeFrame * n)()
    for f in range(n):
        t = hd.transparent[f]
        table[f] = _lib.TtGifComposeFrame(*hd.rectangles[f].tolist(), t, hd.disposal[f], int(packed[f, t if t >= 0 else hd.background]), 0, int(map_offsets[f]))
    initial = int(packed[0, hd.transparent[0] if hd.transparent[0] >= 0 else 0])
    blob = np.concatenate([cols.view(np.uint8).reshape(-1), np.frombuffer(table, dtype=np.uint8), hd.palettes.reshape(-1)])      # the tables: one upload
    data = torch.from_numpy(hd.data.copy()).to(device)
    small = torch.from_numpy(blob).to(device)
    words = small[:cols.size * 8].view(torch.int64).view(6, n)
    at = cols.size * 8
    rowsize = C.sizeof(_lib.TtGifComposeFrame)
    maps, status = ops.gif_indices(data, words[0].contiguous(), words[2].to(torch.int32), words[3].to(torch.int32), words[4].to(torch.int32),
                                   words[5].to(torch.int32), words[1].contiguous(), int(npix.sum()))
    frames = ops.gif_compose(maps, small[at:at + n * rowsize].view(n, rowsize), small[at + n * rowsize:].view(n, 256, 3), (hd.height, hd.width), initial)
    for i, s in enumerate(status.cpu().tolist()):
        if s:
            why = ", ".join(text for bit, text in _lib.TT_GIF_DEC_STATUS.items() if s & bit)
            raise ValueError(f"decode_gif: frame {i} is corrupt or short ({why}; status {s})")
    return (frames, hd) if info else frames


def read_gif(path, device="cuda") -> torch.Tensor:
    """The frames of a GIF file (``export.write_gif``'s, Pillow's, imageio's) decoded by ``decode_gif``."""
    return decode_gif(path, device)


# ---- PNG files (include/ttvdm.h, "PNG import"): the container on the host, a general zlib inflate and the inverse row filters on the device
@dataclass
class PngHeader:
    """What ``parse_png`` reads from one file: the geometry, ``channels`` (1 / 2 / 3 / 4 for colour types 0 / 4 / 2 / 6), ``bit_depth``,
    ``color_type``, ``interlace``; ``spans`` int64 [S, 2]: every IDAT / fdAT payload's byte offset in the file and its length, with
    ``span_frames`` [S] (the frame it belongs to; -1: the IDAT of a default image that is no frame); ``idat`` (offset, bytes): the default
    image's zlib stream in ``data`` (all payloads end to end).  For an animated file ``plays`` (acTL; None without it), ``announced``
    (acTL's frame count), ``default_is_frame`` and per fcTL ``frames``: dicts of sequence, width, height, x, y, delay_num, delay_den,
    dispose, blend, spans, data_offset, data_bytes (the frame's zlib stream in ``data``)."""
    height: int
    width: int
    channels: int
    bit_depth: int
    color_type: int
    interlace: int
    spans: np.ndarray
    span_frames: list
    idat: tuple
    plays: object
    announced: int
    default_is_frame: bool
    frames: list
    data: np.ndarray


def parse_png(data: bytes) -> PngHeader:
    """One PNG / APNG file -> its header, its spans and its compressed bytes (tt_png_parse: once to count, once to take them); ValueError
    with the library's text, which names the cause, for what is refused."""
    lib = _lib.load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    at = buf.ctypes.data if buf.size else None
    hd = _lib.TtPngHeader()
    rc = lib.tt_png_parse(at, buf.size, C.byref(hd), None, 0, None, 0, None, 0)
    if rc == 0:
        spans = (_lib.TtPngSpan * max(hd.spans, 1))()
        frames = (_lib.TtPngFrame * max(hd.frames, 1))()
        upload = np.zeros(max(hd.data_bytes, 1), dtype=np.uint8)
        rc = lib.tt_png_parse(at, buf.size, C.byref(hd), C.cast(spans, C.c_void_p), hd.spans, C.cast(frames, C.c_void_p), hd.frames, upload.ctypes.data, hd.data_bytes)
    if rc != 0:
        raise ValueError(lib.tt_last_error().decode(errors="replace"))
    names = [n for n, _ in _lib.TtPngFrame._fields_]
    return PngHeader(hd.height, hd.width, hd.channels, hd.bit_depth, hd.color_type, hd.interlace,
                     np.array([[spans[i].file_offset, spans[i].bytes] for i in range(hd.spans)], dtype=np.int64).reshape(-1, 2),
                     [spans[i].frame for i in range(hd.spans)], (hd.idat_offset, hd.idat_bytes), None if hd.plays < 0 else hd.plays, hd.announced,
                     bool(hd.default_is_frame), [{n: getattr(frames[i], n) for n in names} for i in range(hd.frames)], upload[:hd.data_bytes])


def _png_decode_streams(who: str, heads: list, streams: list, device, label: str) -> torch.Tensor:
    """zlib streams of one geometry (``streams[i]``: a uint8 array) -> uint8 [N, H, W, ch]: one upload of the bytes, one of five numbers a
    stream, the inflate and the unfilter, one readback of the status words"""
    from . import ops
    lib = _lib.load()
    h0 = heads[0]
    shape = (h0.height, h0.width, h0.channels)
    n = len(streams)
    if n > _lib.TT_INFLATE_MAX_STREAMS:
        raise ValueError(f"{who}: {n} {label}s: more than one call decodes ({_lib.TT_INFLATE_MAX_STREAMS})")
    expected, stride = lib.tt_png_stream_bytes(*shape), lib.tt_png_frame_stride(*shape)
    if expected < 1 or n * stride >= 1 << 31:
        raise ValueError(f"{who}: {n} {label}s of {shape[0]} x {shape[1]} x {shape[2]}: {n * stride} bytes of filtered rows (fewer than 2^31 in one call)")
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    if int(lens.sum()) >= 1 << 29:
        raise ValueError(f"{who}: {int(lens.sum())} compressed bytes in one call (fewer than 2^29)")
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    cols = np.stack([offs, np.arange(n, dtype=np.int64) * stride, lens, np.full(n, expected, dtype=np.int64)])
    blob = torch.from_numpy(np.concatenate([np.asarray(s, dtype=np.uint8).reshape(-1) for s in streams])).to(device)
    words = torch.from_numpy(cols).to(device)                                                       # the small upload: four numbers a stream
    filtered, status = ops.png_inflate(blob, words[0].contiguous(), words[2].to(torch.int32), words[3].to(torch.int32), words[1].contiguous(), int(expected),
                                       int(n * stride))
    pixels, bad_rows = ops.png_unfilter(filtered.view(n, stride), shape)
    both = torch.stack([status, bad_rows]).cpu().tolist()                                            # the one readback
    for i, (s, t) in enumerate(zip(*both)):
        if s or t:
            why = [text for bit, text in _lib.TT_INFLATE_STATUS.items() if s & bit] + [text for bit, text in _lib.TT_PNG_UNFILTER_STATUS.items() if t & bit]
            raise ValueError(f"{who}: {label} {i} is corrupt or truncated ({', '.join(why)}; status {s}, rows {t})")
    return pixels


def decode_png(files, device) -> torch.Tensor:
    """8-bit PNG files of ONE geometry and colour type -- bytes or paths, one or a list -- -> uint8 [F, H, W, ch] on ``device``, ch 1 / 2 /
    3 / 4 for grey / grey + alpha / RGB / RGBA: ``np.asarray(PIL.Image.open(f))``, byte for byte (a grey file comes back as [..., 1]).  One
    upload of the compressed bytes, one small upload of per-file numbers, one readback (the status words).  Of an animated PNG the default
    image (IDAT) is decoded, as ``Image.open`` shows it.  The CRCs of the IDAT chunks are not verified (Pillow does not either); the
    Adler-32 of the data is, on the device.  ValueError: a file the parser refuses (its text names the cause: palette, 16-bit and
    sub-byte depths, interlace, ...), files that differ in size or colour type, a file whose stream is corrupt or truncated (the file is
    named), a ``device`` that is not the HIP device."""
    items = list(files) if isinstance(files, (list, tuple)) else [files]
    if not items:
        raise ValueError("decode_png: no files")
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"decode_png: decodes on the HIP device, got {device} (there is no CPU fallback)")
    heads, streams = [], []
    for i, f in enumerate(items):
        try:
            hd = parse_png(_read(f))
        except ValueError as e:
            raise ValueError(f"decode_png: file {i}: {e}") from None
        if heads and (hd.height, hd.width, hd.channels) != (heads[0].height, heads[0].width, heads[0].channels):
            raise ValueError(f"decode_png: file {i} is {hd.height} x {hd.width} x {hd.channels}, file 0 is {heads[0].height} x {heads[0].width} x "
                             f"{heads[0].channels}: one geometry and colour type per call")
        heads.append(hd)
        streams.append(hd.data[hd.idat[0]:hd.idat[0] + hd.idat[1]])
    return _png_decode_streams("decode_png", heads, streams, device, "file")


def read_pngs(folder, pattern: str = "{idx}.png", device="cuda") -> torch.Tensor:
    """``folder/pattern.format(idx=i)`` for i = 0, 1, ... up to the first missing index -- the layout ``export.write_pngs`` writes and the
    reference's scripts pass clips around in -- decoded by ``decode_png``."""
    paths = []
    while os.path.exists(os.path.join(folder, pattern.format(idx=len(paths)))):
        paths.append(os.path.join(folder, pattern.format(idx=len(paths))))
        if len(paths) > 1 and paths[-1] == paths[-2]:
            raise ValueError(f"read_pngs: pattern {pattern!r} names two frames alike (use {{idx}})")
    if not paths:
        raise ValueError(f"read_pngs: {os.path.join(folder, pattern.format(idx=0))} does not exist")
    return decode_png(paths, device)


def read_apng(path, device="cuda") -> torch.Tensor:
    """Every frame of an animated PNG -- a path or bytes -- whose frames all cover the canvas with dispose 0 and blend 0 (what
    ``export.write_apng`` writes) -> uint8 [F, H, W, ch].  ValueError: a file without fcTL chunks, or an fcTL that names a region, a
    dispose or a blend operation (the frame and the field are named: those are not built)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"read_apng: decodes on the HIP device, got {device} (there is no CPU fallback)")
    try:
        hd = parse_png(_read(path))
    except ValueError as e:
        raise ValueError(f"read_apng: {e}") from None
    if not hd.frames:
        raise ValueError("read_apng: not an animated PNG (no fcTL chunk); decode_png reads it")
    for i, fr in enumerate(hd.frames):
        if (fr["width"], fr["height"], fr["x"], fr["y"]) != (hd.width, hd.height, 0, 0):
            raise ValueError(f"read_apng: frame {i}'s fcTL names the region {fr['width']} x {fr['height']} at ({fr['x']}, {fr['y']}) of a {hd.width} x {hd.height} "
                             "canvas: frames that do not cover the canvas are not built")
        if fr["dispose"] != 0 or fr["blend"] != 0:
            raise ValueError(f"read_apng: frame {i}'s fcTL names dispose {fr['dispose']} / blend {fr['blend']}: only dispose 0 and blend 0 are built")
    streams = [hd.data[fr["data_offset"]:fr["data_offset"] + fr["data_bytes"]] for fr in hd.frames]
    return _png_decode_streams("read_apng", [hd], streams, device, "frame")
