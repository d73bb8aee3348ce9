"""Frames -> file: a video written as an animated GIF, its 256-colour palettes and index maps computed on the device
(``tt_color_hist`` / ``tt_palette_map``; the median cut and the LZW coder are host routines of the same library -- include/ttvdm.h
states all four rule by rule).

    q = write_gif(pipe(..., output_type="device").frames[0], "combined.gif", duration=0.05)
    q.frame_psnr                          # how far each written frame is from its source, dB

``quantize_frames``: ONE histogram launch, one readback of the histograms, a median cut over the occupied bins per palette (host,
integers), the palettes' upload, ``refine`` Lloyd iterations (map with per-entry sums, read 256 records back, move every used entry to
the rounded mean of its pixels), the final map, and ONE readback of the indices (one byte per pixel, not three) and the exact error
sums.  Everything is integer arithmetic: the same frames give the same file every time, from host and from device copies alike.
Not here: dithering, transparency, frame differencing."""
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


def _frames_u8(frames, who: str) -> torch.Tensor:
    """what ``metrics.compare_frames`` takes -> contiguous uint8 [F, H, W, 3] on the device (a host input is uploaded once).  Floating-point
    frames in [0, 1] become ``rint(clamp(x, 0, 1) * 255)`` in fp32, the rounding tt_frames_out states for its kind 1."""
    x, shape, kind = _describe(frames, who)
    if len(shape) == 5 and shape[0] == 1:             # a pipeline's output for one video
        x, shape = x[0], shape[1:]
    if len(shape) != 4:
        raise ValueError(f"{who}: one video per file -- frames [F, H, W, 3], got a batch of {shape[0]} videos {shape}; pass them one at a time")
    if shape[-1] != 3:
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


# ---- frames -> indices and palettes
def quantize_frames(frames, colors: int = 256, palette: str = "frame", refine: int = 0) -> QuantizedVideo:
    """Quantise a video to at most ``colors`` (1 .. 256) colours per palette.  ``frames``: what ``metrics.compare_frames`` takes -- a
    device uint8 / float32 NHWC tensor [F, H, W, 3], ``DevicePixels``, a numpy array, a list of PIL images or a pipeline's "pil" / "np" /
    "device" output for ONE video (a batch of several videos is refused: one file per video).  ``palette``: "frame" (one per frame) or
    "global" (one for the video).  ``refine``: Lloyd iterations after the median cut (each costs one more map launch and a 4 KB
    readback per palette)."""
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
    return QuantizedVideo(packed[:npix].reshape(f, h, w), palettes, ncolors, frame_sse, _psnr(frame_sse, h * w * 3), palette)


# ---- indices and palettes -> file
def _table(palette: np.ndarray, ncolors: int):
    """-> (bits, the colour table's bytes): 2^bits >= ncolors entries (at least 2), zeros behind the last colour"""
    bits = max(1, int(ncolors - 1).bit_length())
    tab = np.zeros((1 << bits, 3), dtype=np.uint8)
    tab[:ncolors] = palette[:ncolors]
    return bits, tab.tobytes()


def write_gif_indexed(indices, palettes, ncolors, path_or_file, duration: float = 0.05, loop=0, palette=None) -> None:
    """Host indices uint8 [F, H, W], palettes uint8 [F or 1, 256, 3] and ncolors [F or 1] -> a GIF89a file (a path or a binary file
    object).  ``duration``: seconds per frame, written in centiseconds, rounded and at least 1.  ``loop``: repetitions in the
    NETSCAPE2.0 block (0: for ever); None: no such block.  ``palette``: "frame" writes a local colour table per frame, "global" one
    global table; None: "global" when there is one palette for several frames.  Table sizes are the next power of two, padded with zeros;
    the LZW minimum code size is max(2, bits)."""
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
        out.append(lzw_frame(indices[i], max(2, bits)))
    out.append(b"\x3b")
    data = b"".join(out)
    if hasattr(path_or_file, "write"):
        path_or_file.write(data)
    else:
        with open(path_or_file, "wb") as fh:
            fh.write(data)


def write_gif(frames, path_or_file, duration: float = 0.05, loop=0, **quantize_kwargs) -> QuantizedVideo:
    """``quantize_frames(frames, **quantize_kwargs)`` written by ``write_gif_indexed``; returns the QuantizedVideo.  ``duration`` is
    seconds per frame (what ``imageio.mimsave(path, frames, duration=0.05)`` took)."""
    q = quantize_frames(frames, **quantize_kwargs)
    write_gif_indexed(q.indices, q.palettes, q.ncolors, path_or_file, duration=duration, loop=loop, palette=q.palette)
    return q
