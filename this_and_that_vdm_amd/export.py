"""Frames -> file: a video written as an animated GIF, its 256-colour palettes and index maps computed on the device
(``tt_color_hist`` / ``tt_palette_map``; the median cut and the LZW coder are host routines of the same library -- include/ttvdm.h
states all four rule by rule).

    q = write_gif(pipe(..., output_type="device").frames[0], "combined.gif", duration=0.05)
    q.frame_psnr                          # how far each written frame is from its source, dB

``quantize_frames``: ONE histogram launch, one readback of the histograms, a median cut over the occupied bins per palette (host,
integers), the palettes' upload, ``refine`` Lloyd iterations (map with per-entry sums, read 256 records back, move every used entry to
the rounded mean of its pixels), the final map, and ONE readback of the indices (one byte per pixel, not three) and the exact error
sums.  Everything is integer arithmetic: the same frames give the same file every time, from host and from device copies alike.
``write_gif(..., lzw="device")`` moves the LZW coder to the device too (``tt_gif_lzw_frames``): every frame's index map is coded where the
palette map left it, in independent segments that each start behind a clear code -- the same pixels for every decoder, a file a few
per cent larger, the stage some fifteen times faster at 576 x 1024.  The default, ``lzw="host"``, writes the bytes it always wrote.
Not here: dithering, transparency, frame differencing.

... and as PNG files, lossless (``tt_png_filter`` / ``tt_png_tokens`` / ``tt_png_emit``; code lengths and block headers are host
routines of the library):

    write_pngs(pipe(..., output_type="device").frames[0], folder)        # folder/0.png, 1.png, ...
    write_apng(frames, "combined.png", duration=0.05)

``png_streams``: ONE filter launch and ONE tokens launch for all frames, one readback of 1152 bytes per 32 KiB stripe, package-merge and
the dynamic-block headers on the host, one upload of the tables and headers, ONE emit launch, one readback of the finished compressed
streams -- the filtered bytes never leave the device.  Not here: LZ77 matches beyond distance 1, a stored-block fallback, 16-bit or
palette PNGs, interlace, ancillary chunks.

... and as baseline JPEG files and a Motion-JPEG AVI (``tt_jpeg_coeffs`` / ``tt_jpeg_scan``; the quantiser and Huffman tables are host
routines of the library):

    write_jpegs(pipe(..., output_type="device").frames[0], folder)       # folder/im_0.jpg, im_1.jpg, ...: the data loaders' layout
    write_mjpeg(frames, "clip.avi", fps=4)                               # Motion-JPEG, NOT H.264: a browser will not play it

``encode_jpeg``: ONE launch from pixels to zig-zag coefficients for all frames, then the bits of every block, a scan for their
positions, the bits themselves and the byte stuffing, with no host round trip in between when the standard Huffman tables are used;
the lengths and the finished scans are read back.  With the standard tables the scan equals libjpeg's (Pillow's) byte for byte.
Restart intervals: ``restart_interval`` / ``restart_rows``.  Not here: progressive or arithmetic coding, 4:2:2, EXIF / ICC, CMYK, 12 bits,
trellis quantisation (the decoder is ingest.py)."""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import check
from .metrics import _describe, _on_device

BIN_DTYPE = np.dtype([("count", "<u4"), ("sum_r", "<u4"), ("sum_g", "<u4"), ("sum_b", "<u4")])


@dataclass
class QuantizedVideo:
    """``indices`` uint8 [F, H, W] and ``palettes`` uint8 [F or 1, 256, 3] (entries from ``ncolors`` on are zeros), both numpy on the
    host: frame f is ``palettes[f if per frame else 0][indices[f]]``.  ``ncolors`` int32 [F or 1]; ``frame_sse`` int64 [F], the exact
    sum of squared channel differences between a frame and its source; ``frame_psnr`` fp64 [F] from it (``inf`` where it is 0).
    ``palette``: "frame" or "global"."""
    indices: np.ndarray
    palettes: np.ndarray
    ncolors: np.ndarray
    frame_sse: np.ndarray
    frame_psnr: np.ndarray
    palette: str = "frame"

    @property
    def psnr(self) -> float:
        """the video's PSNR in dB, from the error sum over all frames"""
        return float(_psnr(np.asarray(self.frame_sse.sum()), self.indices.size * 3))

    def frames(self) -> np.ndarray:
        """the quantised video as uint8 [F, H, W, 3]"""
        f = self.indices.shape[0]
        which = np.arange(f) if self.palettes.shape[0] == f else np.zeros(f, dtype=np.int64)
        return np.stack([self.palettes[which[i]][self.indices[i]] for i in range(f)], 0)


def _psnr(sse, values):
    mse = np.asarray(sse, dtype=np.float64) / float(values)
    with np.errstate(divide="ignore"):
        return np.where(mse == 0.0, np.inf, 10.0 * np.log10(255.0 * 255.0 / mse))


def _frames_u8(frames, who: str, rgb: bool = True) -> torch.Tensor:
    """what ``metrics.compare_frames`` takes -> contiguous uint8 [F, H, W, 3] on the device (a host input is uploaded once).  Floating-point
    frames in [0, 1] become ``rint(clamp(x, 0, 1) * 255)`` in fp32, the rounding tt_frames_out states for its kind 1.  ``rgb=False``
    (the PNG export): 1 to 4 channels."""
    x, shape, kind = _describe(frames, who)
    if len(shape) == 5 and shape[0] == 1:             # a pipeline's output for one video
        x, shape = x[0], shape[1:]
    if len(shape) != 4:
        raise ValueError(f"{who}: one video per file -- frames [F, H, W, 3], got a batch of {shape[0]} videos {shape}; pass them one at a time")
    if rgb and shape[-1] != 3:
        raise ValueError(f"{who}: RGB frames (3 channels), got {shape[-1]} in {shape}")
    device = x.device if torch.is_tensor(x) else torch.device("cuda")
    x = _on_device(x, device)
    if kind != "uint8":
        x = torch.round(x.clamp(0.0, 1.0) * 255.0).to(torch.uint8)
    return x


# ---- the host routines of the library
def median_cut(hist: np.ndarray, colors: int = 256, boxes: bool = False):
    """one histogram (numpy, 32768 bins of BIN_DTYPE or [32768, 4] integers) -> (palette uint8 [256, 3], ncolors); with ``boxes`` also the
    box index of every bin (int32 [32768], -1 for an empty bin) (tt_palette_median_cut)"""
    lib = _lib.load()
    h = np.ascontiguousarray(np.asarray(hist).view(np.uint32).reshape(_lib.TT_GIF_BINS, 4))
    pal = np.zeros((256, 3), dtype=np.uint8)
    n = C.c_int32(0)
    box = np.empty(_lib.TT_GIF_BINS, dtype=np.int32) if boxes else None
    check(lib.tt_palette_median_cut(h.ctypes.data, int(colors), pal.ctypes.data, C.byref(n), box.ctypes.data if boxes else None),
          "tt_palette_median_cut")
    return (pal, n.value, box) if boxes else (pal, n.value)


def lloyd_step(palettes: np.ndarray, stats: np.ndarray) -> np.ndarray:
    """palettes uint8 [P, 256, 3] and the map's per-entry records [P, 256, 4] (pixels, sum R, sum G, sum B) -> the next palettes: every
    entry with pixels moves to their mean, rounded half up, (2 sum + count) // (2 count); an entry without pixels stays"""
    st = np.asarray(stats).view(np.uint32).reshape(palettes.shape[0], 256, 4).astype(np.int64)
    count = st[..., :1]
    mean = (2 * st[..., 1:] + count) // np.maximum(2 * count, 1)
    return np.where(count > 0, mean, palettes).astype(np.uint8)


def lzw_frame(indices: np.ndarray, min_code_size: int) -> bytes:
    """one frame's indices -> its GIF image data: the min-code-size byte, the sub-blocks, the terminator (tt_gif_lzw)"""
    lib = _lib.load()
    idx = np.ascontiguousarray(indices, dtype=np.uint8).reshape(-1)
    cap = lib.tt_gif_lzw_bound(idx.size)
    out = np.empty(max(int(cap), 1), dtype=np.uint8)
    n = C.c_int64(0)
    check(lib.tt_gif_lzw(idx.ctypes.data, idx.size, int(min_code_size), out.ctypes.data, cap, C.byref(n)), "tt_gif_lzw")
    return out[:n.value].tobytes()


def lzw_frames_device(indices, min_code_sizes, segment=None) -> list:
    """every frame's indices -> its GIF image data (bytes), coded on the device in independent segments (tt_gif_lzw_frames; include/ttvdm.h,
    "GIF LZW on the device").  ``indices``: uint8 [F, H, W] or [F, npix], a device tensor (used where it is) or a host array (uploaded
    once); ``min_code_sizes``: an int or one per frame; ``segment``: pixels per segment, None for the built default.  One readback of the
    lengths and the status words, one of the bytes in use.  ValueError, naming the frame, when a frame's status is set."""
    from . import ops
    if not torch.is_tensor(indices):
        indices = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.uint8))
    if not indices.is_cuda:
        indices = indices.to("cuda")
    sizes = [int(min_code_sizes)] if isinstance(min_code_sizes, (int, np.integer)) else [int(v) for v in min_code_sizes]
    data, lengths, status = ops.gif_lzw(indices.contiguous(), sizes, segment)
    head = torch.stack([lengths, status]).cpu().numpy()                                        # readback 1: lengths and status
    for i, st in enumerate(head[1]):
        if st:
            why = " and ".join(text for bit, text in _lib.TT_GIF_LZW_STATUS.items() if st & bit)
            raise ValueError(f"lzw_frames_device: frame {i} holds {why} (min_code_size {sizes[i if len(sizes) > 1 else 0]})")
    used = data[:, :int(head[0].max())].cpu().numpy()                                          # readback 2: the bytes in use
    return [used[i, :int(head[0][i])].tobytes() for i in range(used.shape[0])]


# ---- frames -> indices and palettes
def quantize_frames(frames, colors: int = 256, palette: str = "frame", refine: int = 0) -> QuantizedVideo:
    """Quantise a video to at most ``colors`` (1 .. 256) colours per palette.  ``frames``: what ``metrics.compare_frames`` takes -- a
    device uint8 / float32 NHWC tensor [F, H, W, 3], ``DevicePixels``, a numpy array, a list of PIL images or a pipeline's "pil" / "np" /
    "device" output for ONE video (a batch of several videos is refused: one file per video).  ``palette``: "frame" (one per frame) or
    "global" (one for the video).  ``refine``: Lloyd iterations after the median cut (each costs one more map launch and a 4 KB
    readback per palette)."""
    return _quantize(frames, colors, palette, refine)[0]


def _quantize(frames, colors: int = 256, palette: str = "frame", refine: int = 0):
    """``quantize_frames``' work -> (the QuantizedVideo, the index tensor uint8 [F, H, W] that the palette map left on the device)"""
    from . import ops
    if palette not in ("frame", "global"):
        raise ValueError(f"quantize_frames: palette {palette!r} ('frame' or 'global')")
    if not 1 <= int(colors) <= 256:
        raise ValueError(f"quantize_frames: colors = {colors} (1 to 256)")
    if int(refine) < 0:
        raise ValueError(f"quantize_frames: refine = {refine}")
    x = _frames_u8(frames, "quantize_frames")
    f, h, w, _ = x.shape
    hist = ops.color_hist(x, per_frame=palette == "frame").cpu().numpy()                       # readback 1: the histograms
    cut = [median_cut(hh, colors) for hh in hist]
    palettes = np.stack([p for p, _ in cut], 0)
    ncolors = np.array([k for _, k in cut], dtype=np.int32)
    pal_dev = torch.from_numpy(palettes).to(x.device)
    for _ in range(int(refine)):
        _, _, stats = ops.palette_map(x, pal_dev, ncolors, stats=True)
        palettes = lloyd_step(palettes, stats.cpu().numpy())
        pal_dev = torch.from_numpy(palettes).to(x.device)
    indices, sse, _ = ops.palette_map(x, pal_dev, ncolors)
    packed = torch.cat([indices.reshape(-1), sse.view(torch.uint8)]).cpu().numpy()             # the ONE readback of the result
    npix = f * h * w
    frame_sse = packed[npix:].view("<i8").copy()
    return QuantizedVideo(packed[:npix].reshape(f, h, w), palettes, ncolors, frame_sse, _psnr(frame_sse, h * w * 3), palette), indices


# ---- indices and palettes -> file
def _table(palette: np.ndarray, ncolors: int):
    """-> (bits, the colour table's bytes): 2^bits >= ncolors entries (at least 2), zeros behind the last colour"""
    bits = max(1, int(ncolors - 1).bit_length())
    tab = np.zeros((1 << bits, 3), dtype=np.uint8)
    tab[:ncolors] = palette[:ncolors]
    return bits, tab.tobytes()


def _write(path_or_file, data: bytes) -> None:
    """``data`` to a binary file object, or to a new file at a path"""
    if hasattr(path_or_file, "write"):
        path_or_file.write(data)
    else:
        with open(path_or_file, "wb") as fh:
            fh.write(data)


def _write_numbered(who: str, files: list, folder, pattern: str) -> list:
    """``files`` as ``folder/pattern.format(idx=i)``; returns the paths.  The folder is made when it does not exist."""
    import os
    os.makedirs(folder, exist_ok=True)
    paths = [os.path.join(folder, pattern.format(idx=i)) for i in range(len(files))]
    if len(set(paths)) != len(paths):
        raise ValueError(f"{who}: pattern {pattern!r} names two frames alike (use {{idx}})")
    for path, data in zip(paths, files):
        _write(path, data)
    return paths


def write_gif_indexed(indices, palettes, ncolors, path_or_file, duration: float = 0.05, loop=0, palette=None, lzw: str = "host", segment=None) -> None:
    """Host indices uint8 [F, H, W], palettes uint8 [F or 1, 256, 3] and ncolors [F or 1] -> a GIF89a file (a path or a binary file
    object).  ``duration``: seconds per frame, written in centiseconds, rounded and at least 1.  ``loop``: repetitions in the
    NETSCAPE2.0 block (0: for ever); None: no such block.  ``palette``: "frame" writes a local colour table per frame, "global" one
    global table; None: "global" when there is one palette for several frames.  Table sizes are the next power of two, padded with zeros;
    the LZW minimum code size is max(2, bits).  ``lzw``: "host" (tt_gif_lzw, one stream per frame) or "device" (tt_gif_lzw_frames:
    the indices are uploaded and coded in independent segments of ``segment`` pixels, None for the built default; every decoder reads
    the same pixels, the file is a little larger)."""
    _write_gif_indexed(indices, palettes, ncolors, path_or_file, duration, loop, palette, lzw, segment, None)


def _write_gif_indexed(indices, palettes, ncolors, path_or_file, duration, loop, palette, lzw, segment, on_device) -> None:
    """``write_gif_indexed``; ``on_device``: the same indices as a device tensor, when the caller has one (``lzw="device"`` codes that)"""
    if lzw not in ("host", "device"):
        raise ValueError(f"write_gif: lzw {lzw!r} ('host' or 'device')")
    indices = np.ascontiguousarray(indices, dtype=np.uint8)
    palettes = np.ascontiguousarray(palettes, dtype=np.uint8)
    ncolors = np.atleast_1d(np.asarray(ncolors)).astype(np.int64)
    if indices.ndim != 3 or 0 in indices.shape:
        raise ValueError(f"write_gif: indices are [F, H, W], got {indices.shape}")
    f, h, w = indices.shape
    if palettes.ndim != 3 or palettes.shape[1:] != (256, 3) or palettes.shape[0] not in (1, f) or ncolors.shape != (palettes.shape[0],):
        raise ValueError(f"write_gif: palettes [F or 1, 256, 3] with one ncolors each, got {palettes.shape} and {ncolors.shape}")
    if ncolors.min() < 1 or ncolors.max() > 256:
        raise ValueError(f"write_gif: ncolors {ncolors.tolist()} (1 to 256)")
    if h > 65535 or w > 65535:
        raise ValueError(f"write_gif: a GIF frame is at most 65535 pixels a side, got {h} x {w}")
    if palette is None:
        palette = "global" if palettes.shape[0] == 1 and f > 1 else "frame"
    if palette not in ("frame", "global") or (palette == "global" and palettes.shape[0] != 1):
        raise ValueError(f"write_gif: palette {palette!r} with {palettes.shape[0]} palettes for {f} frames")
    if loop is not None and not 0 <= int(loop) <= 65535:
        raise ValueError(f"write_gif: loop = {loop} (0 to 65535, or None)")
    delay = min(65535, max(1, int(round(float(duration) * 100.0))))
    which = np.arange(f) if palettes.shape[0] == f else np.zeros(f, dtype=np.int64)
    for i in range(f):
        if int(indices[i].max()) >= ncolors[which[i]]:
            raise ValueError(f"write_gif: frame {i} holds index {int(indices[i].max())} with {int(ncolors[which[i]])} colours")
    sizes = [max(2, _table(palettes[which[i]], int(ncolors[which[i]]))[0]) for i in range(f)]
    if lzw == "device":
        coded = lzw_frames_device(indices if on_device is None else on_device, sizes, segment)
    out = [b"GIF89a"]
    if palette == "global":
        bits, table = _table(palettes[0], int(ncolors[0]))
        out += [struct.pack("<HHBBB", w, h, 0x80 | 0x70 | (bits - 1), 0, 0), table]
    else:
        out.append(struct.pack("<HHBBB", w, h, 0x70, 0, 0))
    if loop is not None:
        out.append(b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", int(loop)) + b"\x00")
    for i in range(f):
        out.append(b"\x21\xf9\x04" + struct.pack("<BHB", 0, delay, 0) + b"\x00")
        bits, table = _table(palettes[which[i]], int(ncolors[which[i]]))
        if palette == "global":
            out.append(b"\x2c" + struct.pack("<HHHHB", 0, 0, w, h, 0))
        else:
            out += [b"\x2c" + struct.pack("<HHHHB", 0, 0, w, h, 0x80 | (bits - 1)), table]
        out.append(coded[i] if lzw == "device" else lzw_frame(indices[i], sizes[i]))
    out.append(b"\x3b")
    _write(path_or_file, b"".join(out))


def write_gif(frames, path_or_file, duration: float = 0.05, loop=0, lzw: str = "host", segment=None, **quantize_kwargs) -> QuantizedVideo:
    """``quantize_frames(frames, **quantize_kwargs)`` written by ``write_gif_indexed``; returns the QuantizedVideo.  ``duration`` is
    seconds per frame (what ``imageio.mimsave(path, frames, duration=0.05)`` took).  ``lzw="device"`` codes the index tensor that the
    palette map left on the device, in segments of ``segment`` pixels (``write_gif_indexed``); it is not uploaded again."""
    if lzw not in ("host", "device"):
        raise ValueError(f"write_gif: lzw {lzw!r} ('host' or 'device')")
    if lzw == "host":
        q = quantize_frames(frames, **quantize_kwargs)
        write_gif_indexed(q.indices, q.palettes, q.ncolors, path_or_file, duration=duration, loop=loop, palette=q.palette)
        return q
    q, on_device = _quantize(frames, **quantize_kwargs)
    _write_gif_indexed(q.indices, q.palettes, q.ncolors, path_or_file, duration, loop, q.palette, lzw, segment, on_device)
    return q


# ---- frames -> PNG files: the row filter, the run tokens and the Huffman-coded bits are made on the device (include/ttvdm.h, "PNG
# export", rules 1 - 7); the host sees 1152 bytes of symbol counts per 32 KiB stripe and the finished compressed streams
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
PNG_COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
ADLER_MOD = 65521


def png_code_lengths(counts, limit: int = 15) -> np.ndarray:
    """symbol counts (at most 286) -> uint8 code lengths that minimise sum count x length with no length above ``limit``
    (tt_png_code_lengths: package-merge)"""
    lib = _lib.load()
    c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    out = np.zeros(c.size, dtype=np.uint8)
    check(lib.tt_png_code_lengths(c.ctypes.data, c.size, int(limit), out.ctypes.data), "tt_png_code_lengths")
    return out


def png_block_header(counts, lengths):
    """one stripe's 286 symbol counts and code lengths -> (the dynamic-block header's bits as a uint8 array of 0 / 1 in stream order, the
    stripe's exact size in bits up to and with the three header bits of the stored block behind it) (tt_png_block_header)"""
    lib = _lib.load()
    c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    ln = np.ascontiguousarray(lengths, dtype=np.uint8).reshape(-1)
    if c.size != _lib.TT_PNG_SYMS or ln.size != _lib.TT_PNG_SYMS:
        raise ValueError(f"png_block_header: {_lib.TT_PNG_SYMS} counts and lengths, got {c.size} and {ln.size}")
    words = np.zeros(_lib.TT_PNG_HEADER_WORDS, dtype=np.uint32)
    bits = C.c_int64(0)
    check(lib.tt_png_block_header(c.ctypes.data, ln.ctypes.data, words.ctypes.data, words.size, C.byref(bits)), "tt_png_block_header")
    return np.unpackbits(words[1:].view(np.uint8), bitorder="little")[:int(words[0])], bits.value


def png_plan(records: np.ndarray):
    """the records of ``ops.png_tokens`` on the host [S, 288] -> (tables int32 [S, 288], headers int32 [S, 72], total bytes): per stripe
    the reversed canonical codes with their lengths and the stripe's byte offset, and its block header (tt_png_plan)"""
    lib = _lib.load()
    rec = np.ascontiguousarray(records).view(np.uint32).reshape(-1, _lib.TT_PNG_RECORD_WORDS)
    tables = np.zeros((rec.shape[0], _lib.TT_PNG_TABLE_WORDS), dtype=np.uint32)
    headers = np.zeros((rec.shape[0], _lib.TT_PNG_HEADER_WORDS), dtype=np.uint32)
    total = C.c_int64(0)
    check(lib.tt_png_plan(rec.ctypes.data, rec.shape[0], tables.ctypes.data, headers.ctypes.data, C.byref(total)), "tt_png_plan")
    return tables.view(np.int32), headers.view(np.int32), total.value


def _adler_of_stripes(rec: np.ndarray, lens) -> int:
    """the Adler-32 of a stream from its stripes' (s1, s2) pairs, each started from (1, 0), as zlib's adler32_combine joins two:
    s1 = s1a + s1b - 1, s2 = s2a + s2b + len_b (s1a - 1), mod 65 521"""
    s1, s2 = 1, 0
    for (b1, b2), n in zip(rec, lens):
        s2 = (s2 + int(b2) + n * (s1 - 1)) % ADLER_MOD
        s1 = (s1 + int(b1) - 1) % ADLER_MOD
    return (s2 << 16) | s1


@dataclass
class PngStreams:
    """``streams``: per frame the zlib stream of its filtered bytes (the payload of IDAT); ``height``, ``width``, ``channels``"""
    streams: list
    height: int
    width: int
    channels: int


def png_streams(frames, filter="adaptive") -> PngStreams:
    """Frames -> their zlib streams.  ONE filter launch and ONE tokens launch for all frames, one readback of the stripes' records, the
    code lengths and block headers on the host, one upload each of the tables and the headers, ONE emit launch, one readback of the
    finished stripes.  Per frame the stream is 78 01, its stripes, 01 00 00 FF FF, the Adler-32 big-endian."""
    from . import ops
    if filter not in ops.PNG_FILTERS and not (type(filter) is int and 0 <= filter <= 5):
        raise ValueError(f"encode_png: filter {filter!r} (one of {sorted(ops.PNG_FILTERS)}, or 0 to 5)")
    x = _frames_u8(frames, "encode_png", rgb=False)
    f, h, w, ch = x.shape
    if h >= 1 << 31 or w >= 1 << 31:
        raise ValueError(f"encode_png: a PNG is below 2^31 pixels a side, got {h} x {w}")
    filtered = ops.png_filter(x, filter)
    records = ops.png_tokens(filtered, (h, w, ch))
    rec = records.cpu().numpy().view(np.uint32)                                                # readback 1: 1152 bytes per stripe
    tables, headers, total = png_plan(rec)
    out = ops.png_emit(filtered, (h, w, ch), torch.from_numpy(tables).to(x.device), torch.from_numpy(headers).to(x.device), total)
    data = out.cpu().numpy()                                                                   # readback 2: the finished stripes
    stripes = rec.shape[0] // f
    stream_bytes = h * (1 + w * ch)
    lens = [min(_lib.TT_PNG_STRIPE, stream_bytes - k * _lib.TT_PNG_STRIPE) for k in range(stripes)]
    offsets = (tables[::stripes, 286].astype(np.int64) & 0xffffffff) | (tables[::stripes, 287].astype(np.int64) << 32)
    ends = list(offsets[1:]) + [total]
    streams = []
    for i in range(f):
        adler = _adler_of_stripes(rec[i * stripes:(i + 1) * stripes, 286:288], lens)
        streams.append(b"".join((b"\x78\x01", data[int(offsets[i]):int(ends[i])].tobytes(), b"\x01\x00\x00\xff\xff", struct.pack(">I", adler))))
    return PngStreams(streams, h, w, ch)


def _png_chunk(tag: bytes, *parts: bytes) -> bytes:
    import zlib
    crc = zlib.crc32(tag)
    for p in parts:
        crc = zlib.crc32(p, crc)
    return b"".join((struct.pack(">I", sum(len(p) for p in parts)), tag, *parts, struct.pack(">I", crc)))


def _png_ihdr(s: PngStreams) -> bytes:
    return _png_chunk(b"IHDR", struct.pack(">IIBBBBB", s.width, s.height, 8, PNG_COLOR_TYPE[s.channels], 0, 0, 0))


def png_files(s: PngStreams) -> list:
    """per frame the file: signature, IHDR (8 bit, colour type by channels: 0, 4, 2, 6; no interlace), ONE IDAT, IEND"""
    head, end = PNG_SIGNATURE + _png_ihdr(s), _png_chunk(b"IEND")
    return [b"".join((head, _png_chunk(b"IDAT", z), end)) for z in s.streams]


def encode_png(frames, filter="adaptive") -> list:
    """Frames -> one PNG file (bytes) per frame.  ``frames``: what ``write_gif`` takes, with 1 to 4 channels (grey, grey + alpha, RGB,
    RGBA) -- a device uint8 / float32 NHWC tensor, ``DevicePixels``, numpy, a list of PIL images or a pipeline's "pil" / "np" / "device"
    output for ONE video; floating-point frames are rounded as for ``write_gif``.  ``filter``: "adaptive" (per row the type with the
    least sum of absolute signed residuals), or "none" / "sub" / "up" / "average" / "paeth" on every row.  Lossless; the same frames
    give the same bytes from host and device copies alike."""
    return png_files(png_streams(frames, filter))


def write_pngs(frames, folder, pattern: str = "{idx}.png", filter="adaptive") -> list:
    """``encode_png`` written as ``folder/pattern.format(idx=i)`` -- 0.png, 1.png, ... by default -- ; returns the paths.  The folder is
    made when it does not exist."""
    return _write_numbered("write_pngs", encode_png(frames, filter), folder, pattern)


def write_apng(frames, path_or_file, duration: float = 0.05, loop: int = 0, filter="adaptive") -> None:
    """The frames as ONE animated PNG: acTL (frames, ``loop`` plays; 0: for ever), then per frame an fcTL and the frame's stream -- the
    first as IDAT, so that a viewer without APNG shows it, the others as fdAT; the streams are ``encode_png``'s.  Every frame covers the
    canvas, dispose and blend 0.  Delay: the fraction round(duration 1000) / 1000 seconds, the numerator kept within 0 .. 65535."""
    if not 0 <= int(loop) < 1 << 31:
        raise ValueError(f"write_apng: loop = {loop} (0: for ever, or the number of plays)")
    delay = min(65535, max(0, int(round(float(duration) * 1000.0))))
    s = png_streams(frames, filter)
    out = [PNG_SIGNATURE, _png_ihdr(s), _png_chunk(b"acTL", struct.pack(">II", len(s.streams), int(loop)))]
    seq = 0
    for i, z in enumerate(s.streams):
        out.append(_png_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, s.width, s.height, 0, 0, delay, 1000, 0, 0)))
        seq += 1
        if i == 0:
            out.append(_png_chunk(b"IDAT", z))
        else:
            out.append(_png_chunk(b"fdAT", struct.pack(">I", seq), z))
            seq += 1
    out.append(_png_chunk(b"IEND"))
    _write(path_or_file, b"".join(out))


# ---- frames -> baseline JPEG files and a Motion-JPEG AVI: colour conversion, chroma downsampling, the integer DCT, the quantiser, the
# Huffman-coded bits and the byte stuffing are made on the device (include/ttvdm.h, "JPEG export", rules 1 - 8); the host sees the
# finished scans and their lengths (and 4 KiB of symbol counts per frame when it makes optimized tables)
JPEG_TABLE_NAMES = ("DC luminance", "AC luminance", "DC chrominance", "AC chrominance")
_JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_JPEG_STANDARD = {}          # device -> the standard code tables there


@dataclass
class JpegTable:
    """One Huffman table: ``bits`` (codes per length 1 .. 16), ``huffval`` (the symbols by ascending code) -- what a DHT marker holds --
    and ``codes`` uint32 [256]: per symbol its code | length << 16, what the device reads."""
    bits: list
    huffval: list
    codes: np.ndarray


def jpeg_quant_tables(quality: int) -> np.ndarray:
    """-> uint8 [2, 64]: the luminance and chrominance quantiser tables of ``quality`` in natural order (tt_jpeg_quant_tables)"""
    out = np.zeros((2, 64), dtype=np.uint8)
    check(_lib.load().tt_jpeg_quant_tables(int(quality), out.ctypes.data), "tt_jpeg_quant_tables")
    return out


def _jpeg_table(call, what: str) -> JpegTable:
    bits, vals, codes, n = np.zeros(16, dtype=np.uint8), np.zeros(256, dtype=np.uint8), np.zeros(256, dtype=np.uint32), C.c_int32(0)
    check(call(bits.ctypes.data, vals.ctypes.data, C.byref(n), codes.ctypes.data), what)
    return JpegTable(bits.tolist(), vals[:n.value].tolist(), codes)


def jpeg_standard_tables() -> list:
    """-> the four T.81 Annex K.3 tables, in the order of JPEG_TABLE_NAMES (tt_jpeg_standard_table)"""
    lib = _lib.load()
    return [_jpeg_table(lambda *a, k=k: lib.tt_jpeg_standard_table(k, *a), "tt_jpeg_standard_table") for k in range(4)]


def jpeg_optimized_table(counts) -> JpegTable:
    """256 symbol counts -> the table with the least total bits among codes of at most 15 bits that leave the all-ones code free
    (tt_jpeg_optimized_table)"""
    lib = _lib.load()
    c = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    if c.size != 256:
        raise ValueError(f"jpeg_optimized_table: 256 counts, got {c.size}")
    return _jpeg_table(lambda *a: lib.tt_jpeg_optimized_table(c.ctypes.data, *a), "tt_jpeg_optimized_table")


def _jpeg_segment(marker: int, payload: bytes) -> bytes:
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload


def jpeg_file(scan: bytes, height: int, width: int, channels: int, quality: int, subsampling: str, tables: list, restart_interval: int = 0) -> bytes:
    """one frame's entropy-coded scan -> its file (rule 8): SOI, APP0 JFIF 1.01, a DQT marker per quantiser table, SOF0, a DHT marker
    per Huffman table, with a ``restart_interval`` DRI, SOS, the scan, EOI -- the layout libjpeg writes"""
    qt = jpeg_quant_tables(quality)
    grey = channels == 1
    out = [b"\xff\xd8", _jpeg_segment(0xe0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for i in range(1 if grey else 2):
        out.append(_jpeg_segment(0xdb, bytes([i]) + bytes(int(qt[i][z]) for z in _JPEG_ZIGZAG)))
    luma = 0x22 if (not grey and subsampling == "4:2:0") else 0x11
    sof = struct.pack(">BHHB", 8, height, width, 1 if grey else 3) + bytes([1, luma, 0]) + (b"" if grey else bytes([2, 0x11, 1, 3, 0x11, 1]))
    out.append(_jpeg_segment(0xc0, sof))
    for i in range(2 if grey else 4):
        out.append(_jpeg_segment(0xc4, bytes([((i & 1) << 4) | (i >> 1)]) + bytes(tables[i].bits) + bytes(tables[i].huffval)))
    if restart_interval:
        out.append(_jpeg_segment(0xdd, struct.pack(">H", restart_interval)))
    sos = bytes([1 if grey else 3, 1, 0x00]) + (b"" if grey else bytes([2, 0x11, 3, 0x11])) + bytes([0, 63, 0])
    out += [_jpeg_segment(0xda, sos), scan, b"\xff\xd9"]
    return b"".join(out)


def _jpeg_args(quality, subsampling, huffman, who: str):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"{who}: quality {quality!r} (an integer, 1 to 100)")
    if subsampling not in ("4:4:4", "4:2:0"):
        raise ValueError(f"{who}: subsampling {subsampling!r} ('4:4:4' or '4:2:0'; 4:2:2 is not offered)")
    if huffman not in ("standard", "optimized"):
        raise ValueError(f"{who}: huffman {huffman!r} ('standard' or 'optimized')")
    return int(quality)


def _jpeg_restart_interval(restart_interval, restart_rows, height: int, width: int, channels: int, subsampling: str, who: str) -> int:
    """Pillow's two options -> the interval in MCUs (0: none); rows are counted in the frame's MCUs per row"""
    for name, v in (("restart_interval", restart_interval), ("restart_rows", restart_rows)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
            raise ValueError(f"{who}: {name} {v!r} (an integer, 0 or more)")
    if restart_interval and restart_rows:
        raise ValueError(f"{who}: restart_interval {restart_interval} and restart_rows {restart_rows}: at most one of the two")
    side = 16 if (channels == 3 and subsampling == "4:2:0") else 8
    ri = int(restart_interval) or int(restart_rows) * -(-width // side)
    if ri > 65535:
        raise ValueError(f"{who}: a restart interval of {ri} MCUs (DRI holds 65535 at most; it is not clipped)")
    return ri


def encode_jpeg(frames, quality: int = 75, subsampling: str = "4:2:0", huffman: str = "standard", restart_interval: int = 0, restart_rows: int = 0) -> list:
    """Frames -> one baseline JPEG file (bytes) per frame.  ``frames``: what ``write_gif`` takes, with 1 channel (grey, [F, H, W, 1]) or
    3 (RGB) -- a device uint8 / float32 NHWC tensor, ``DevicePixels``, numpy, a list of PIL images or a pipeline's "pil" / "np" /
    "device" output for ONE video; floating-point frames are rounded as for ``write_gif``.  ``quality`` 1 .. 100 scales the Annex K
    quantiser tables as libjpeg does; ``subsampling`` "4:2:0" or "4:4:4" (a grey frame has no chroma and ignores it); ``huffman``
    "standard" (the Annex K.3 tables: no host round trip between the first launch and the readback, and the scan equals libjpeg's
    byte for byte) or "optimized" (per-frame tables from symbol counts taken on the device: one more readback of 4 KiB per frame).
    ``restart_interval`` (in MCUs) or ``restart_rows`` (in MCU rows; at most one of the two, Pillow's ``restart_marker_blocks`` /
    ``restart_marker_rows``) writes a DRI segment and a restart marker every that many MCUs, as libjpeg does: a decoder may then take
    every interval on its own (``ingest.decode_jpeg`` gives each its own workgroup); the default 0 writes none, today's bytes.
    Only the finished scans and their lengths cross to the host.  The same frames give the same bytes from host and device copies."""
    from . import ops
    quality = _jpeg_args(quality, subsampling, huffman, "encode_jpeg")
    src, shape, _ = _describe(frames, "encode_jpeg")
    if shape[-1] not in (1, 3):
        raise ValueError(f"encode_jpeg: 1 (grey) or 3 (RGB) channels -- JPEG has no alpha --, got {shape[-1]} in {shape}")
    if shape[-3] > 65535 or shape[-2] > 65535:
        raise ValueError(f"encode_jpeg: a JPEG is at most 65535 pixels a side, got {shape[-3]} x {shape[-2]}")
    ri = _jpeg_restart_interval(restart_interval, restart_rows, shape[-3], shape[-2], shape[-1], subsampling, "encode_jpeg")      # before any upload
    x = _frames_u8(src, "encode_jpeg", rgb=False)
    f, h, w, ch = x.shape
    optimized = huffman == "optimized"
    coeffs, counts = ops.jpeg_coeffs(x, quality, subsampling, counts=optimized and not ri)
    if optimized and ri:
        counts = ops.jpeg_counts_restart(coeffs, (h, w, ch), subsampling, ri)                  # the predictors reset where the scan's do
    if optimized:
        cnt = counts.cpu().numpy().view(np.uint32)                                             # the extra readback: 4 KiB per frame
        per_frame = [[jpeg_optimized_table(cnt[i, k]) for k in range(4)] for i in range(f)]
        tables = torch.from_numpy(np.stack([np.stack([t.codes for t in ts]) for ts in per_frame]).view(np.int32)).to(x.device)
    else:
        standard = jpeg_standard_tables()
        per_frame = [standard] * f
        tables = _JPEG_STANDARD.get(x.device)
        if tables is None:
            tables = _JPEG_STANDARD[x.device] = torch.from_numpy(np.stack([t.codes for t in standard]).view(np.int32)[None]).to(x.device)
    out, lengths = ops.jpeg_scan(coeffs, (h, w, ch), subsampling, tables, restart_interval=ri)
    lens = lengths.cpu().numpy().astype(np.int64)                                              # readback 1: one length per frame
    packed = torch.cat([out[i, :int(lens[i])] for i in range(f)]).cpu().numpy()                # readback 2: the finished scans, no padding
    ends = np.cumsum(lens)
    return [jpeg_file(packed[int(e - n):int(e)].tobytes(), h, w, ch, quality, subsampling, per_frame[i], ri) for i, (e, n) in enumerate(zip(ends, lens))]


def write_jpegs(frames, folder, pattern: str = "im_{idx}.jpg", **kw) -> list:
    """``encode_jpeg(frames, **kw)`` written as ``folder/pattern.format(idx=i)`` -- im_0.jpg, im_1.jpg, ...: the layout the data loaders
    read a clip from -- ; returns the paths.  The folder is made when it does not exist."""
    return _write_numbered("write_jpegs", encode_jpeg(frames, **kw), folder, pattern)


def _jpeg_size(data: bytes):
    """(height, width) from a baseline JPEG's SOF0"""
    at = 2
    while at + 4 <= len(data) and data[at] == 0xff:
        (size,) = struct.unpack(">H", data[at + 2:at + 4])
        if data[at + 1] == 0xc0:
            return struct.unpack(">HH", data[at + 5:at + 9])
        at += 2 + size
    raise ValueError("write_mjpeg: a frame is not a baseline JPEG (no SOF0)")


def _riff_chunk(tag: bytes, payload: bytes) -> bytes:
    return tag + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


def mjpeg_avi(files: list, fps=4) -> bytes:
    """JPEG files of one size -> a Motion-JPEG AVI: RIFF 'AVI ', LIST hdrl (avih, LIST strl (strh vids / MJPG with rate / scale = fps,
    strf: a BITMAPINFOHEADER, compression MJPG, 24 bits)), LIST movi (one 00dc chunk per frame, padded to even), idx1 (every frame a
    key frame, offsets from the movi tag).  Motion-JPEG is NOT H.264: a browser does not play it."""
    from fractions import Fraction
    if not files:
        raise ValueError("write_mjpeg: no frames")
    rate = Fraction(fps).limit_denominator(100000) if not isinstance(fps, Fraction) else fps
    if rate <= 0 or rate.numerator >= 1 << 32:
        raise ValueError(f"write_mjpeg: fps = {fps} (positive)")
    sizes = {_jpeg_size(d) for d in files}
    if len(sizes) != 1:
        raise ValueError(f"write_mjpeg: frames of several sizes: {sorted(sizes)}")
    (h, w), n, largest = sizes.pop(), len(files), max(len(d) for d in files)
    movi, index, at = [b"movi"], [], 4
    for d in files:
        index.append(struct.pack("<4sIII", b"00dc", 0x10, at, len(d)))
        chunk = _riff_chunk(b"00dc", d)
        movi.append(chunk)
        at += len(chunk)
    usec = int(round(1e6 / float(rate)))
    avih = struct.pack("<14I", usec, int(largest * float(rate)) + 1, 0, 0x10, n, 0, 1, largest, w, h, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIhhhh", b"vids", b"MJPG", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, n, largest, 0xffffffff, 0, 0, 0, w, h)
    strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
    strl = _riff_chunk(b"LIST", b"strl" + _riff_chunk(b"strh", strh) + _riff_chunk(b"strf", strf))
    hdrl = _riff_chunk(b"LIST", b"hdrl" + _riff_chunk(b"avih", avih) + strl)
    body = b"AVI " + hdrl + _riff_chunk(b"LIST", b"".join(movi)) + _riff_chunk(b"idx1", b"".join(index))
    if len(body) >= 1 << 32:
        raise ValueError(f"write_mjpeg: {len(body)} bytes do not fit a RIFF file (below 4 GiB)")
    return b"RIFF" + struct.pack("<I", len(body)) + body


def write_mjpeg(frames, path_or_file, fps=4, **kw) -> None:
    """``encode_jpeg(frames, **kw)`` as ONE Motion-JPEG AVI (``mjpeg_avi``) at ``fps`` frames a second (an integer, a float or a Fraction);
    a path or a binary file object.  NOT H.264 and not what a browser plays."""
    _write(path_or_file, mjpeg_avi(encode_jpeg(frames, **kw), fps))


def read_mjpeg(path_or_bytes) -> dict:
    """A small RIFF walker for the AVI ``write_mjpeg`` writes -> {"frames": [bytes], "fps": Fraction, "width", "height", "total_frames",
    "handler", "compression", "index": [(flags, offset, size)]}.  Raises ValueError where the structure is not consistent: a chunk
    that overruns its parent, a RIFF size that is not the file's, an idx1 entry that does not point at its 00dc chunk."""
    from fractions import Fraction
    if isinstance(path_or_bytes, (bytes, bytearray)):
        data = bytes(path_or_bytes)
    else:
        with open(path_or_bytes, "rb") as fh:
            data = fh.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("read_mjpeg: not a RIFF AVI file")
    if struct.unpack("<I", data[4:8])[0] != len(data) - 8:
        raise ValueError(f"read_mjpeg: the RIFF size {struct.unpack('<I', data[4:8])[0]} is not the file's {len(data) - 8}")
    info = {"frames": [], "index": []}
    movi_at = None
    frame_at = []

    def walk(at, end):
        nonlocal movi_at
        while at < end:
            if at + 8 > end:
                raise ValueError(f"read_mjpeg: a chunk header at {at} overruns its parent (ends at {end})")
            tag, (size,) = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])
            body, stop = at + 8, at + 8 + size
            if stop > end:
                raise ValueError(f"read_mjpeg: chunk {tag!r} at {at} overruns its parent ({stop} > {end})")
            if tag == b"LIST":
                if data[body:body + 4] == b"movi":
                    movi_at = body
                walk(body + 4, stop)
            elif tag == b"avih":
                v = struct.unpack("<14I", data[body:stop])
                info.update(usec_per_frame=v[0], total_frames=v[4], streams=v[6], width=v[8], height=v[9])
            elif tag == b"strh":
                v = struct.unpack("<4s4sIHHIIIIIIIIhhhh", data[body:stop])
                info.update(stream_type=v[0], handler=v[1], fps=Fraction(v[7], v[6]), stream_length=v[9])
            elif tag == b"strf":
                v = struct.unpack("<IiiHH4sIiiII", data[body:stop])
                info.update(strf_width=v[1], strf_height=v[2], bit_count=v[4], compression=v[5])
            elif tag == b"00dc":
                frame_at.append(at)
                info["frames"].append(data[body:stop])
            elif tag == b"idx1":
                if size % 16:
                    raise ValueError(f"read_mjpeg: idx1 of {size} bytes")
                for i in range(0, size, 16):
                    ck, flags, off, sz = struct.unpack("<4sIII", data[body + i:body + i + 16])
                    if ck != b"00dc":
                        raise ValueError(f"read_mjpeg: idx1 entry {i // 16} names {ck!r}")
                    info["index"].append((flags, off, sz))
            at = stop + (size & 1)

    walk(12, len(data))
    if movi_at is None or len(info["index"]) != len(frame_at):
        raise ValueError(f"read_mjpeg: {len(frame_at)} frame chunks and {len(info['index'])} idx1 entries")
    for i, ((flags, off, sz), at) in enumerate(zip(info["index"], frame_at)):
        if movi_at + off != at or sz != len(info["frames"][i]):
            raise ValueError(f"read_mjpeg: idx1 entry {i} (offset {off}, size {sz}) does not point at its chunk at {at - movi_at} of {len(info['frames'][i])} bytes")
    return info


def read_mjpeg_frames(path) -> list:
    """the JPEG files inside a Motion-JPEG AVI, in order (``read_mjpeg``'s frames)"""
    return read_mjpeg(path)["frames"]
