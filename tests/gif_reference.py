"""numpy restatements of the GIF export's four integer routines as include/ttvdm.h states them -- the colour histogram, the median
cut, the palette map and the Lloyd step -- written for clarity, not speed, plus the synthetic frames the tests and the benchmark tool
quantise and a plain LZW decoder that reports what a code stream did."""
import numpy as np

BINS = 32768


def field_frame(h, w, f=2, sigma=0.0, rng=None):
    """the smooth colour field of the tests (x the column, y the row), plus N(0, sigma^2) noise, clipped and truncated to uint8"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([128 + 100 * np.sin(x / 37 + f / 3) * np.cos(y / 29),
                     128 + 90 * np.cos(x / 53 - f / 5) + 0 * y,
                     128 + 80 * np.sin((x + y) / 41 + f / 7)], -1)
    if sigma:
        base = base + rng.normal(0.0, sigma, base.shape)
    return np.clip(base, 0, 255).astype(np.uint8)



def bins_of(pixels):
    """pixels [..., 3] uint8 -> bin r5 << 10 | g5 << 5 | b5"""
    p = pixels.astype(np.int64) >> 3
    return (p[..., 0] << 10) | (p[..., 1] << 5) | p[..., 2]


def color_hist(frames, per_frame=True):
    """frames [N, H, W, 3] uint8 -> int64 [N or 1, 32768, 4]: per bin (pixels, sum R, sum G, sum B) by np.bincount"""
    groups = frames.reshape(frames.shape[0], -1, 3) if per_frame else frames.reshape(1, -1, 3)
    out = np.zeros((groups.shape[0], BINS, 4), dtype=np.int64)
    for i, px in enumerate(groups):
        b = bins_of(px)
        out[i, :, 0] = np.bincount(b, minlength=BINS)
        for c in range(3):
            out[i, :, 1 + c] = np.bincount(b, weights=px[:, c].astype(np.float64), minlength=BINS).astype(np.int64)   # < 2^53: exact
    return out


def median_cut(hist, colors):
    """hist int [32768, 4] -> (palette uint8 [256, 3], ncolors, boxes: a list of arrays of bin numbers).  The header's rules 1 - 5."""
    hist = np.asarray(hist, dtype=np.int64)
    occupied = np.nonzero(hist[:, 0])[0]
    assert occupied.size, "a histogram without a pixel"
    coords = np.stack([occupied >> 10, (occupied >> 5) & 31, occupied & 31], 1)     # of the occupied bins, in bin order
    count = hist[occupied, 0]
    boxes = [np.arange(occupied.size)]                                               # positions into `occupied`
    while len(boxes) < colors:
        pick, best = -1, -1
        for i, b in enumerate(boxes):
            if b.size > 1 and count[b].sum() > best:                                 # strictly larger: the earliest keeps a tie
                pick, best = i, count[b].sum()
        if pick < 0:
            break
        b = boxes[pick]
        extent = coords[b].max(0) - coords[b].min(0)
        axis = int(np.argmax(extent))                                                # the first maximum: R, then G, then B
        c = coords[b, axis]
        at = np.bincount(c, weights=count[b].astype(np.float64), minlength=32).astype(np.int64)
        t = int(np.nonzero(2 * np.cumsum(at) >= best)[0][0])
        if t == c.max():
            t = int(c[c < t].max())
        boxes[pick], new = b[c <= t], b[c > t]
        boxes.append(new)
    palette = np.zeros((256, 3), dtype=np.uint8)
    for k, b in enumerate(boxes):
        n = count[b].sum()
        palette[k] = (2 * hist[occupied[b], 1:].sum(0) + n) // (2 * n)
    return palette, len(boxes), [occupied[b] for b in boxes]


def palette_map(frames, palettes, ncolors, chunk=8192):
    """frames [N, H, W, 3], palettes [N or 1, 256, 3], ncolors [N or 1] -> (indices uint8 [N, H, W], sse int64 [N], stats int64
    [N or 1, 256, 4]) by brute force: np.argmin over the first ncolors squared distances returns the FIRST minimum"""
    n, h, w, _ = frames.shape
    npal = palettes.shape[0]
    idx = np.zeros((n, h * w), dtype=np.uint8)
    sse = np.zeros(n, dtype=np.int64)
    stats = np.zeros((npal, 256, 4), dtype=np.int64)
    for f in range(n):
        pi = f if npal == n and n > 1 else 0
        pal = palettes[pi, :int(ncolors[pi])].astype(np.int64)
        px = frames[f].reshape(-1, 3).astype(np.int64)
        for s in range(0, px.shape[0], chunk):
            d = ((px[s:s + chunk, None, :] - pal[None, :, :]) ** 2).sum(-1)
            k = np.argmin(d, axis=1)
            idx[f, s:s + chunk] = k
            sse[f] += d[np.arange(k.size), k].sum()
        k = idx[f].astype(np.int64)
        stats[pi, :, 0] += np.bincount(k, minlength=256)
        for c in range(3):
            stats[pi, :, 1 + c] += np.bincount(k, weights=px[:, c].astype(np.float64), minlength=256).astype(np.int64)
    return idx.reshape(n, h, w), sse, stats


def lloyd_step(palettes, stats):
    """every entry with pixels -> their mean rounded half up, (2 sum + count) // (2 count); an entry without pixels stays"""
    out = palettes.copy()
    for p in range(palettes.shape[0]):
        for k in range(256):
            n = int(stats[p, k, 0])
            if n:
                out[p, k] = [(2 * int(stats[p, k, 1 + c]) + n) // (2 * n) for c in range(3)]
    return out


def quantize(frames, colors=256, palette="frame", refine=0):
    """the whole of export.quantize_frames on the host -> (indices, palettes, ncolors, sse, [sse before each Lloyd step])"""
    hist = color_hist(frames, per_frame=palette == "frame")
    cut = [median_cut(h, colors) for h in hist]
    palettes = np.stack([c[0] for c in cut], 0)
    ncolors = np.array([c[1] for c in cut], dtype=np.int32)
    trail = []
    for _ in range(refine):
        _, sse, stats = palette_map(frames, palettes, ncolors)
        trail.append(sse)
        palettes = lloyd_step(palettes, stats)
    idx, sse, _ = palette_map(frames, palettes, ncolors)
    return idx, palettes, ncolors, sse, trail


def psnr(a, b):
    mse = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()
    return np.inf if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def lzw_decode(data):
    """GIF image data (min-code-size byte, sub-blocks, terminator) -> (indices, clear codes seen, the widest code read, bytes used).
    The textbook decoder of GIF89a appendix F; a code it cannot know raises."""
    mcs = data[0]
    pos, payload = 1, bytearray()
    while data[pos]:
        payload += data[pos + 1:pos + 1 + data[pos]]
        pos += 1 + data[pos]
    pos += 1
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    bits = int.from_bytes(bytes(payload), "little")
    out, clears, widest, at = [], 0, 0, 0
    width, table, prev = mcs + 1, None, None
    while True:
        assert at + width <= 8 * len(payload), "the stream ends without an end-of-information code"
        code = (bits >> at) & ((1 << width) - 1)
        at += width
        widest = max(widest, width)
        if code == clear:
            clears += 1
            table = [[i] for i in range(clear)] + [None, None]
            width, prev = mcs + 1, None
            continue
        if code == eoi:
            break
        assert table is not None, "the stream does not start with a clear code"
        if prev is None:
            entry = table[code]
        else:
            if code < len(table):
                entry = table[code]
            else:
                assert code == len(table) and len(table) < 4096, f"code {code} with {len(table)} entries"
                entry = prev + [prev[0]]
            if len(table) < 4096:
                table.append(prev + [entry[0]])
                if len(table) == (1 << width) and width < 12:
                    width += 1
        out += entry
        prev = entry
    assert 8 * len(payload) - at < 8, "whole bytes of padding behind the end-of-information code"
    return np.array(out, dtype=np.uint8), clears, widest, pos
