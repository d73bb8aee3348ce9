"""A numpy / Python restatement of the JPEG export's format rules (include/ttvdm.h, "JPEG export", rules 1 - 8), written from the rules
and ITU-T T.81: quantiser tables, component planes, zig-zag coefficients in scan order, symbol counts, the entropy-coded scan and the
file.  Slow and plain on purpose; the tests hold the library to it byte for byte, and hold IT to Pillow's baseline encoder."""
import struct

import numpy as np

S444, S420 = 0, 2
SUBSAMPLING = {"4:4:4": S444, "4:2:0": S420}

LUM_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
         18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHR_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def _zigzag():
    order, (y, x) = [], (0, 0)
    for _ in range(64):
        order.append(y * 8 + x)
        if (y + x) % 2 == 0:                       # moving up and to the right
            if x == 7:
                y += 1
            elif y == 0:
                x += 1
            else:
                y, x = y - 1, x + 1
        else:                                      # moving down and to the left
            if y == 7:
                x += 1
            elif x == 0:
                y += 1
            else:
                y, x = y + 1, x - 1
    return order


ZIGZAG = _zigzag()                                  # ZIGZAG[k]: the natural (row-major) index of the k-th coefficient of the scan

# T.81 Annex K.3: BITS (codes per length 1 .. 16) and HUFFVAL of the four typical tables
STD_BITS = {
    "dc_lum": [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0],
    "dc_chr": [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0],
    "ac_lum": [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
    "ac_chr": [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
}
STD_VALS = {
    "dc_lum": list(range(12)),
    "dc_chr": list(range(12)),
    "ac_lum": [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
               0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
               0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
               0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
               0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
               0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
               0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
               0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
    "ac_chr": [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
               0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
               0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
               0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
               0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
               0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
               0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
               0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa],
}
TABLE_NAMES = ("dc_lum", "ac_lum", "dc_chr", "ac_chr")           # the order of the library's counts and code tables
assert all(len(STD_VALS[k]) == sum(STD_BITS[k]) for k in TABLE_NAMES)


# ---- frames the tests use
def smooth_frame(h, w, seed=0, ch=3):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((h, w, ch), dtype=np.uint8)
    for c in range(ch):
        v = 128 + 90 * np.sin((x * (0.11 + 0.03 * c) + seed) * 0.7) * np.cos(y * (0.09 + 0.02 * c) - seed) + 0.4 * (x - y) * (c - 1)
        out[..., c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out


def noise_frame(h, w, seed=0, ch=3):
    return np.random.default_rng(1000 + seed).integers(0, 256, size=(h, w, ch), dtype=np.int64).astype(np.uint8)


def checker_frame(h, w, ch=3):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], ch, axis=2)


def flat_frame(h, w, value, ch=3):
    return np.full((h, w, ch), value, dtype=np.uint8)


# ---- rule 1
def quant_tables(quality):
    """-> (luminance, chrominance): 64 integers each in natural (row-major) order"""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (LUM_Q, CHR_Q))


# ---- rules 2 and 3
def _cdiv(a, b):
    return -(-a // b)


def _edge(plane, rows, cols):
    h, w = plane.shape
    return plane[np.minimum(np.arange(rows), h - 1)][:, np.minimum(np.arange(cols), w - 1)]


def planes(frame, sub):
    """frame uint8 [h, w, ch] -> the component planes (int64), each padded to whole 8 x 8 blocks as rule 3 states"""
    h, w, ch = frame.shape
    f = frame.astype(np.int64)
    if ch == 1:
        return [_edge(f[..., 0], _cdiv(h, 8) * 8, _cdiv(w, 8) * 8)]
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if sub == S444:
        return [_edge(p, _cdiv(h, 8) * 8, _cdiv(w, 8) * 8) for p in (y, cb, cr)]
    out = [_edge(y, _cdiv(h, 8) * 8, _cdiv(w, 8) * 8)]
    hc, wc = _cdiv(h, 2), _cdiv(w, 2)
    bw, bh = _cdiv(wc, 8), _cdiv(hc, 8)
    for p in (cb, cr):
        full = _edge(p, 2 * hc, 16 * bw)
        bias = np.where(np.arange(8 * bw) % 2 == 0, 1, 2)[None, :]
        down = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] + bias) >> 2
        out.append(_edge(down, 8 * bh, 8 * bw))       # the DOWNSAMPLED rows are repeated
    return out


# ---- rule 4
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jfdctint's pass over the last axis of d [..., 8]; ``first``: the row pass (PASS1_BITS up), else the column pass (PASS1_BITS down)"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    out = np.empty_like(d)
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2], out[..., 6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    out[..., 7], out[..., 5], out[..., 3], out[..., 1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return out


def fdct(blocks):
    """blocks int64 [..., 8, 8] of samples -> the forward DCT scaled by 8"""
    rows = _fdct_1d(blocks - 128, True)
    return np.swapaxes(_fdct_1d(np.swapaxes(rows, -1, -2), False), -1, -2)


def quantize(d, table):
    q = 8 * np.asarray(table, dtype=np.int64).reshape(8, 8)
    return np.sign(d) * ((np.abs(d) + (q >> 1)) // q)


def _plane_blocks(plane, table):
    """-> quantised coefficients [block rows, block cols, 64] in zig-zag order"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
    return quantize(fdct(b), table).reshape(bh, bw, 64)[..., ZIGZAG]


def blocks_per_frame(h, w, ch, sub):
    if ch == 1:
        return _cdiv(h, 8) * _cdiv(w, 8)
    return 3 * _cdiv(h, 8) * _cdiv(w, 8) if sub == S444 else 6 * _cdiv(h, 16) * _cdiv(w, 16)


def coefficients(frame, quality, sub):
    """-> (int16 [blocks in scan order, 64] zig-zag, component of every block: 0 Y, 1 Cb, 2 Cr, dummy [blocks] bool)"""
    h, w, ch = frame.shape
    lum, chrom = quant_tables(quality)
    pl = planes(frame, sub)
    yb = _plane_blocks(pl[0], lum)
    coefs, comps, dummy = [], [], []
    if ch == 1 or sub == S444:
        rest = [_plane_blocks(p, chrom) for p in pl[1:]]
        for by in range(yb.shape[0]):
            for bx in range(yb.shape[1]):
                for c, blocks in enumerate([yb] + rest):
                    coefs.append(blocks[by, bx])
                    comps.append(c)
                    dummy.append(False)
    else:
        cbb, crb = _plane_blocks(pl[1], chrom), _plane_blocks(pl[2], chrom)
        for my in range(cbb.shape[0]):
            for mx in range(cbb.shape[1]):
                for k in range(4):
                    by, bx = 2 * my + (k >> 1), 2 * mx + (k & 1)
                    if by < yb.shape[0] and bx < yb.shape[1]:
                        coefs.append(yb[by, bx])
                        dummy.append(False)
                    else:                           # a dummy block: the DC of the block coded just before it in this MCU, no AC
                        z = np.zeros(64, dtype=np.int64)
                        z[0] = coefs[-1][0]
                        coefs.append(z)
                        dummy.append(True)
                    comps.append(0)
                coefs += [cbb[my, mx], crb[my, mx]]
                comps += [1, 2]
                dummy += [False, False]
    return np.stack(coefs).astype(np.int16), np.array(comps), np.array(dummy)


# ---- rule 6
def _category(v):
    return int(abs(int(v))).bit_length()


def block_symbols(block, pred):
    """one block's zig-zag coefficients and the DC before it -> [(table 0 DC / 1 AC, symbol, magnitude bits, how many)]"""
    diff = int(block[0]) - pred
    n = _category(diff)
    out = [(0, n, (diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)]
    run = 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((1, 0xF0, 0, 0))
            run -= 16
        n = _category(v)
        out.append((1, (run << 4) | n, (v if v >= 0 else v - 1) & ((1 << n) - 1), n))
        run = 0
    if run > 0:
        out.append((1, 0x00, 0, 0))
    return out


def symbols(coefs, comps):
    """-> per block its symbols as block_symbols gives them, the table index (0 .. 3 of TABLE_NAMES) in place of 0 / 1"""
    pred = [0, 0, 0]
    out = []
    for block, c in zip(coefs, comps):
        out.append([(t + (2 if c else 0), s, bits, n) for t, s, bits, n in block_symbols(block, pred[c])])
        pred[c] = int(block[0])
    return out


def symbol_counts(coefs, comps):
    counts = np.zeros((4, 256), dtype=np.int64)
    for blk in symbols(coefs, comps):
        for t, s, _, _ in blk:
            counts[t, s] += 1
    return counts


def codes_of(bits, vals):
    """BITS and HUFFVAL -> {symbol: (code, length)}, T.81 Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def standard_tables():
    """-> [(BITS, HUFFVAL)] in the order of TABLE_NAMES"""
    return [(STD_BITS[k], STD_VALS[k]) for k in TABLE_NAMES]


def scan_bytes(coefs, comps, tables=None):
    """the entropy-coded segment: codes MSB first, a 00 behind every FF, the last byte filled with one-bits"""
    codes = [codes_of(b, v) for b, v in (tables or standard_tables())]
    acc, nacc, out = 0, 0, bytearray()
    for blk in symbols(coefs, comps):
        for t, s, bits, n in blk:
            code, length = codes[t][s]
            acc = (acc << (length + n)) | (code << n) | bits
            nacc += length + n
        while nacc >= 8:
            nacc -= 8
            byte = (acc >> nacc) & 0xff
            out.append(byte)
            if byte == 0xff:
                out.append(0)
        acc &= (1 << nacc) - 1
    if nacc:
        byte = ((acc << (8 - nacc)) | ((1 << (8 - nacc)) - 1)) & 0xff
        out.append(byte)
        if byte == 0xff:
            out.append(0)
    return bytes(out)


# ---- rule 8
def _segment(marker, payload):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + payload


def file_of(scan, h, w, ch, quality, sub, tables=None):
    tables = tables or standard_tables()
    qt = quant_tables(quality)
    ncomp = 1 if ch == 1 else 3
    out = [b"\xff\xd8", _segment(0xe0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for i in range(1 if ncomp == 1 else 2):
        out.append(_segment(0xdb, bytes([i]) + bytes(qt[i][z] for z in ZIGZAG)))
    samp = 0x22 if (ncomp == 3 and sub == S420) else 0x11
    sof = struct.pack(">BHHB", 8, h, w, ncomp) + bytes([1, samp, 0])
    if ncomp == 3:
        sof += bytes([2, 0x11, 1, 3, 0x11, 1])
    out.append(_segment(0xc0, sof))
    for i in range(2 if ncomp == 1 else 4):
        bits, vals = tables[i]
        out.append(_segment(0xc4, bytes([((i & 1) << 4) | (i >> 1)]) + bytes(bits) + bytes(vals)))
    sos = bytes([ncomp, 1, 0x00]) + (bytes([2, 0x11, 3, 0x11]) if ncomp == 3 else b"") + bytes([0, 63, 0])
    out += [_segment(0xda, sos), scan, b"\xff\xd9"]
    return b"".join(out)


def jpeg_file(frame, quality=75, sub=S420, tables=None):
    """one frame -> its file; ``tables``: [(BITS, HUFFVAL)] x 4 (or a function of the symbol counts that gives them), else Annex K's"""
    coefs, comps, _ = coefficients(frame, quality, sub)
    if callable(tables):
        tables = tables(symbol_counts(coefs, comps))
    h, w, ch = frame.shape
    return file_of(scan_bytes(coefs, comps, tables), h, w, ch, quality, sub, tables)


def segments_of(data):
    """a baseline JPEG file -> ([(marker, payload)] up to and with SOS, the entropy-coded bytes between SOS and EOI)"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    at, out = 2, []
    while True:
        assert data[at] == 0xff
        marker = data[at + 1]
        (size,) = struct.unpack(">H", data[at + 2:at + 4])
        out.append((marker, data[at + 4:at + 2 + size]))
        at += 2 + size
        if marker == 0xda:
            return out, data[at:-2]


def dqt_payloads(data):
    """the 65-byte (id, 64 entries) units of all DQT markers of a file, in order (one marker may carry several)"""
    out = []
    for marker, payload in segments_of(data)[0]:
        if marker == 0xdb:
            assert len(payload) % 65 == 0
            out += [payload[i:i + 65] for i in range(0, len(payload), 65)]
    return out


def dht_tables(data):
    """{(class << 4 | id): (BITS, HUFFVAL)} of a file"""
    out = {}
    for marker, payload in segments_of(data)[0]:
        at = 0
        while marker == 0xc4 and at < len(payload):
            bits = list(payload[at + 1:at + 17])
            out[payload[at]] = (bits, list(payload[at + 17:at + 17 + sum(bits)]))
            at += 17 + sum(bits)
    return out
