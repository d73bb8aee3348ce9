"""A numpy / pure-Python restatement of the PNG export's format (include/ttvdm.h, "PNG export", rules 1 - 7): the row filters, the
stripes, the run tokens with their symbol counts and Adler pairs, a package-merge of its own, the dynamic-block header, the stripes'
bits, the zlib stream and the file.  Code lengths are ARGUMENTS wherever bits are made, so the library's tie rule does not matter
here: ``lengths_fn(counts, limit)`` supplies them (this module's ``package_merge`` or the library's tt_png_code_lengths)."""
import struct
import zlib

import numpy as np

STRIPE = 32768
SYMS = 286
ADLER = 65521
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951 3.2.5: the length symbols 257 .. 285, their base lengths and extra bits
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---- the committed generator of the size checks: smooth sinusoids, Gaussian noise of sigma 3, one flat rectangle
def generator_frame(h, w, seed=0, ch=3):
    rng = np.random.default_rng(1000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for c in range(ch):
        fx, fy, ph = 2 * np.pi * (1.5 + c) / w, 2 * np.pi * (1.0 + 0.5 * c) / h, 0.7 * c + 0.3 * seed
        planes.append(128 + 60 * np.sin(fx * x + ph) * np.cos(fy * y) + 40 * np.sin(0.5 * fx * x + 1.3 * fy * y + ph))
    img = np.stack(planes, -1) + rng.normal(0.0, 3.0, size=(h, w, ch))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    img[h // 4:h // 2, w // 3:2 * w // 3] = np.array([30, 200, 90, 255][:ch], dtype=np.uint8)
    return img


# ---- rule 1: the filter
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_frame(frame, kind):
    """frame uint8 [h, w, ch] -> (the filtered stream uint8 [h (1 + w ch)], the row types)"""
    h, w, ch = frame.shape
    rows = frame.reshape(h, w * ch).astype(np.int64)
    out = np.zeros((h, 1 + w * ch), dtype=np.uint8)
    types = []
    for y in range(h):
        x = rows[y]
        b = rows[y - 1] if y else np.zeros_like(x)
        a = np.concatenate([np.zeros(ch, dtype=np.int64), x[:-ch]]) if w * ch > ch else np.zeros_like(x)
        c = np.concatenate([np.zeros(ch, dtype=np.int64), b[:-ch]]) if w * ch > ch else np.zeros_like(x)
        cand = [x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]
        cand = [v & 255 for v in cand]
        if kind == 5:
            cost = [int(np.where(v < 128, v, 256 - v).sum()) for v in cand]
            t = cost.index(min(cost))                                     # the lowest type on a tie
        else:
            t = kind
        out[y, 0], out[y, 1:] = t, cand[t]
        types.append(t)
    return out.reshape(-1), types


# ---- rules 2 and 3: stripes, tokens, records
def stripes_of(stream):
    return [stream[i:i + STRIPE] for i in range(0, len(stream), STRIPE)]


def length_symbol(m):
    """match length 3 .. 258 -> (symbol, extra bits, their value)"""
    k = max(i for i, base in enumerate(LENGTH_BASE) if base <= m)
    return 257 + k, LENGTH_EXTRA[k], m - LENGTH_BASE[k]


def tokens_of(stripe):
    """-> a list of tokens in order: an int 0 .. 255 is that literal, ("m", length) a match at distance 1"""
    s = np.asarray(stripe, dtype=np.uint8)
    edges = np.concatenate([[0], np.flatnonzero(s[1:] != s[:-1]) + 1, [s.size]])
    out = []
    for start, end in zip(edges[:-1].tolist(), edges[1:].tolist()):
        v, run = int(s[start]), end - start
        out.append(v)
        if run == 1:
            continue
        full, r = divmod(run - 1, 258)
        out += [("m", 258)] * full
        out += [("m", r)] if r >= 3 else [v] * r
    return out


def counts_of(tokens):
    c = np.zeros(SYMS, dtype=np.int64)
    for t in tokens:
        c[t if isinstance(t, int) else length_symbol(t[1])[0]] += 1
    c[256] = 1
    return c


def adler_pair(stripe):
    """(s1, s2) of the stripe's bytes, started from (1, 0), byte by byte in exact integers"""
    b = np.asarray(stripe, dtype=np.int64)
    s1 = 1 + np.cumsum(b)
    return int(s1[-1] % ADLER), int(s1.sum() % ADLER)


def adler_combine(pairs, lens):
    s1, s2 = 1, 0
    for (b1, b2), n in zip(pairs, lens):
        s1, s2 = (s1 + b1 - 1) % ADLER, (s2 + b2 + n * (s1 - 1)) % ADLER
    return (s2 << 16) | s1


def record_of(stripe):
    """what tt_png_tokens writes for the stripe: 286 counts, s1, s2"""
    return np.concatenate([counts_of(tokens_of(stripe)), adler_pair(stripe)])


# ---- rule 4: a package-merge of this module's own, on explicit symbol multisets
def package_merge(counts, limit):
    counts = [int(c) for c in counts]
    used = sorted((c, s) for s, c in enumerate(counts) if c)
    lengths = np.zeros(len(counts), dtype=np.int64)
    if len(used) == 1:
        lengths[used[0][1]] = 1
        return lengths
    assert used and (1 << limit) >= len(used)
    leaves = [(c, (s,)) for c, s in used]
    items = list(leaves)
    for _ in range(limit - 1):
        packs = [(items[i][0] + items[i + 1][0], items[i][1] + items[i + 1][1]) for i in range(0, len(items) - 1, 2)]
        items = sorted(leaves + packs, key=lambda it: it[0])[:2 * len(used) - 2]
    for _, syms in items[:2 * len(used) - 2]:
        for s in syms:
            lengths[s] += 1
    return lengths


def cost(counts, lengths):
    return int((np.asarray(counts, dtype=np.int64) * np.asarray(lengths, dtype=np.int64)).sum())


def kraft(lengths, limit):
    """the Kraft sum times 2^limit"""
    return sum(1 << (limit - int(v)) for v in lengths if v)


def canonical(lengths):
    """RFC 1951 3.2.2 -> the codes, as integers read from the most significant bit"""
    lengths = [int(v) for v in lengths]
    per = [0] * 17
    for v in lengths:
        per[v] += 1
    per[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + per[b - 1]) << 1
        nxt[b] = code
    codes = []
    for v in lengths:
        codes.append(nxt[v] if v else 0)
        nxt[v] += 1 if v else 0
    return codes


# ---- rule 5: the block header
def cl_tokens(lengths):
    """literal/length code lengths [286] -> (HLIT + 257, the code-length tokens (symbol, extra bits, value)) under the greedy rule"""
    lengths = [int(v) for v in lengths]
    hlit = max(257, max(i for i, v in enumerate(lengths) if v) + 1)
    seq = lengths[:hlit] + [1]
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                t = min(run, 138)
                out.append((18, 7, t - 11))
                run -= t
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                t = min(run, 6)
                out.append((16, 2, t - 3))
                run -= t
        out += [(v, 0, 0)] * run
    return hlit, out


def cl_counts(lengths):
    c = np.zeros(19, dtype=np.int64)
    for sym, _, _ in cl_tokens(lengths)[1]:
        c[sym] += 1
    return c


class Bits:
    """a bit string in stream order (bit 0 of byte 0 first)"""
    def __init__(self):
        self.vals, self.widths = [], []

    def put(self, value, width):
        """``value`` from its least significant bit"""
        self.vals.append(value)
        self.widths.append(width)

    def code(self, code, width):
        """a Huffman code: from its most significant bit"""
        self.put(int(format(code, f"0{width}b")[::-1], 2) if width else 0, width)

    def array(self):
        vals, widths = np.asarray(self.vals, dtype=np.int64), np.asarray(self.widths, dtype=np.int64)
        starts = np.cumsum(widths) - widths
        idx = np.arange(int(widths.sum())) - np.repeat(starts, widths)
        return ((np.repeat(vals, widths) >> idx) & 1).astype(np.uint8)


def header_bits(lengths, cl_lengths, bits=None):
    """the dynamic-block header of a stripe whose literal/length code has ``lengths``; ``cl_lengths`` [19] code the code-length symbols"""
    bits = bits or Bits()
    hlit, toks = cl_tokens(lengths)
    cl_lengths = [int(v) for v in cl_lengths]
    codes = canonical(cl_lengths)
    hclen = max(4, max(i for i, s in enumerate(CL_ORDER) if cl_lengths[s]) + 1)
    bits.put(0, 1)
    bits.put(2, 2)
    bits.put(hlit - 257, 5)
    bits.put(0, 5)
    bits.put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        bits.put(cl_lengths[s], 3)
    for sym, nextra, extra in toks:
        bits.code(codes[sym], cl_lengths[sym])
        bits.put(extra, nextra)
    return bits


def stripe_bits(stripe, lengths, cl_lengths):
    """rule 6: the stripe's bits up to and with the three header bits of the empty stored block"""
    lengths = [int(v) for v in lengths]
    codes = canonical(lengths)
    bits = header_bits(lengths, cl_lengths)
    for t in tokens_of(stripe):
        if isinstance(t, int):
            bits.code(codes[t], lengths[t])
        else:
            sym, nextra, extra = length_symbol(t[1])
            bits.code(codes[sym], lengths[sym])
            bits.put(extra, nextra)
            bits.put(0, 1)                                                 # the one distance code
    bits.code(codes[256], lengths[256])
    bits.put(0, 3)
    return bits.array()


def stripe_bytes(stripe, lengths_fn):
    counts = counts_of(tokens_of(stripe))
    lengths = lengths_fn(counts, 15)
    cl_lengths = lengths_fn(cl_counts(lengths), 7)
    return np.packbits(stripe_bits(stripe, lengths, cl_lengths), bitorder="little").tobytes() + b"\x00\x00\xff\xff"


# ---- rule 7: the stream and the file
def zlib_stream(stream, lengths_fn=package_merge):
    parts = stripes_of(stream)
    adler = adler_combine([adler_pair(p) for p in parts], [len(p) for p in parts])
    return b"\x78\x01" + b"".join(stripe_bytes(p, lengths_fn) for p in parts) + b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler)


def chunk(tag, data=b""):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def png_file(frame, kind=5, lengths_fn=package_merge):
    h, w, ch = frame.shape
    stream, _ = filter_frame(frame, kind)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, COLOR_TYPE[ch], 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib_stream(stream, lengths_fn)) + chunk(b"IEND")


def chunks_of(data):
    """a PNG file -> [(tag, payload, crc is right)]"""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack(">I", data[at:at + 4])
        tag, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        out.append((tag, payload, crc == zlib.crc32(tag + payload)))
        at += 12 + n
    return out
