"""A numpy / Python restatement of the JPEG import's rules (include/ttvdm.h, "JPEG import", rules 1 - 6), written from the rules and
ITU-T T.81: a header parser, a plain sequential Huffman decoder, an emulation of rule 4's lanes and passes (the same speculative
outcomes as the kernel, parametrised by the subsequence length S and the lane count) and the reconstruction -- dequantiser, the
jidctint inverse DCT, fancy h2v2 chroma upsampling, the YCbCr -> RGB conversion.  Slow and plain on purpose; the tests hold the library
to it bit for bit, and hold IT to Pillow's decoder."""
import struct

import numpy as np

from tests.jpeg_reference import S420, S444, ZIGZAG, _cdiv, blocks_per_frame

MARKER, CODE, BLOCKS, TAIL = 1, 2, 4, 8          # the status bits


# ---- rule 1
def parse(data):
    """a baseline file -> dict(h, w, ch, sub, scan (the stuffed bytes), quant [ch][64] natural order, dc / ac (per component: table
    index), tables {class << 4 | index: (BITS, HUFFVAL)})"""
    assert data[:2] == b"\xff\xd8"
    at, quant, tables, out = 2, {}, {}, {}
    while True:
        assert data[at] == 0xff
        marker = data[at + 1]
        (size,) = struct.unpack(">H", data[at + 2:at + 4])
        p = data[at + 4:at + 2 + size]
        at += 2 + size
        if marker == 0xdb:
            for i in range(0, len(p), 65):
                assert p[i] >> 4 == 0
                nat = [0] * 64
                for z in range(64):
                    nat[ZIGZAG[z]] = p[i + 1 + z]
                quant[p[i] & 15] = nat
        elif marker == 0xc4:
            i = 0
            while i < len(p):
                bits = list(p[i + 1:i + 17])
                tables[p[i]] = (bits, list(p[i + 17:i + 17 + sum(bits)]))
                i += 17 + sum(bits)
        elif marker == 0xc0:
            prec, h, w, nc = struct.unpack(">BHHB", p[:6])
            assert prec == 8 and nc in (1, 3)
            comps = [(p[6 + 3 * c], p[7 + 3 * c], p[8 + 3 * c]) for c in range(nc)]
            out.update(h=h, w=w, ch=nc, sub=S420 if (nc == 3 and comps[0][1] == 0x22) else S444)
            assert nc == 1 or (comps[0][1] in (0x11, 0x22) and comps[1][1] == comps[2][1] == 0x11)
        elif marker == 0xda:
            assert p[0] == out["ch"]
            out["dc"] = [p[2 + 2 * c] >> 4 for c in range(p[0])]
            out["ac"] = [p[2 + 2 * c] & 15 for c in range(p[0])]
            out["quant"] = [quant[q] for _, _, q in comps]
            out["tables"] = tables
            end = data.rindex(b"\xff\xd9")
            out["scan"] = data[at:end]
            return out
        else:
            assert marker not in (0xc1, 0xc2, 0xdd) or (marker == 0xdd and p == b"\x00\x00")


# ---- rule 2
class DecodeTable:
    """BITS / HUFFVAL -> code lookup: ``find(v16, limit)`` gives (length, symbol) of the code that heads the 16 bits v16, or None when no
    code of at most ``limit`` bits does"""

    def __init__(self, bits, vals):
        self.by_len = {}
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                self.by_len[(length, code)] = vals[k]
                code += 1
                k += 1
            code <<= 1
        assert code <= 1 << 17

    def find(self, v16, limit=16):
        for length in range(1, min(limit, 16) + 1):
            sym = self.by_len.get((length, v16 >> (16 - length)))
            if sym is not None:
                return length, sym
        return None


def decode_set(hd):
    """the header's tables in the kernel's slots: [DC 0, AC 0, DC 1, AC 1] (None for an absent one)"""
    return [DecodeTable(*hd["tables"][key]) if key in hd["tables"] else None for key in (0x00, 0x10, 0x01, 0x11)]


# ---- rule 3
def unstuff(scan):
    """-> (plain bytes, marker status)"""
    out, status, i = bytearray(), 0, 0
    while i < len(scan):
        out.append(scan[i])
        if scan[i] == 0xff:
            if i + 1 < len(scan) and scan[i + 1] == 0:
                i += 1
            else:
                status |= MARKER
        i += 1
    return bytes(out), status


# ---- rule 4
class Stream:
    def __init__(self, plain):
        self.L = 8 * len(plain)
        self.value = int.from_bytes(plain, "big") if plain else 0

    def peek(self, p, n):
        """the n bits at p (zeros beyond L)"""
        end = p + n
        if end <= self.L:
            return (self.value >> (self.L - end)) & ((1 << n) - 1)
        return ((self.value << (end - self.L)) >> 0) & ((1 << n) - 1)


def _span(stream, tabs, dc, ac, bpm, start, end, state, write=None, block=0):
    """f_i: the whole symbols that start in [max(p, start), end); state (p, m, z) -> (exit state, blocks completed, status).  ``write``:
    a function (block, zig-zag index, value)"""
    p, m, z = state
    done, status = 0, 0
    if p < start:
        return state, 0, 0
    while p < end:
        avail = stream.L - p
        comp = (0 if m < 4 else m - 3) if bpm == 6 else m
        t = tabs[(ac[comp] if z else dc[comp]) * 2 + (1 if z else 0)]
        v = stream.peek(p, 32)
        hit = t.find(v >> 16) if t is not None else None
        if hit is None:
            if avail < 16:
                break
            status |= CODE
            p += 1
            continue
        length, sym = hit
        n = sym & 15
        if length + n > avail:
            break
        raw = (v >> (32 - length - n)) & ((1 << n) - 1) if n else 0
        value = (raw if raw >> (n - 1) else raw - (1 << n) + 1) if n else 0
        p += length + n
        ends = False
        if z == 0:
            if sym > 11:
                status |= CODE
            if write:
                write(block + done, 0, value)
            z = 1
        elif n == 0:
            if sym >> 4 == 15:
                z += 16
                ends = z > 63
            else:
                ends = True
        else:
            z += sym >> 4
            if z > 63:
                ends, status = True, status | CODE
            else:
                if write:
                    write(block + done, z, value)
                z += 1
                ends = z > 63
        if ends:
            z, m, done = 0, (m + 1) % bpm, done + 1
    return (p, m, z), done, status


def _finish(stream, plain, coeffs, comps_of, total, found, p, status):
    if found != total:
        status |= BLOCKS
    left = stream.L - min(p, stream.L)
    if left >= 8 or (left and (plain[-1] & ((1 << left) - 1)) != (1 << left) - 1):
        status |= TAIL
    pred = [0, 0, 0]
    for b in range(total):                       # DC differences -> absolute, int32 stored as int16
        c = comps_of(b)
        pred[c] += int(coeffs[b, 0])
        coeffs[b, 0] = np.int16(((pred[c] + 32768) & 0xffff) - 32768)
    return coeffs, status


def _component_of(bpm):
    return (lambda b: 0 if b % 6 < 4 else b % 6 - 3) if bpm == 6 else (lambda b: b % bpm)


def entropy_sequential(scan, tabs, dc, ac, h, w, ch, sub):
    """the plain decoder: one pass from bit 0 -> (coeffs int16 [blocks, 64] zig-zag scan order, status)"""
    plain, status = unstuff(scan)
    stream = Stream(plain)
    total = blocks_per_frame(h, w, ch, sub)
    bpm = 1 if ch == 1 else (6 if sub == S420 else 3)
    coeffs = np.zeros((total, 64), dtype=np.int16)

    def write(b, z, v):
        if b < total:
            coeffs[b, z] = v

    state, found, st = _span(stream, tabs, dc, ac, bpm, 0, stream.L, (0, 0, 0), write)
    return _finish(stream, plain, coeffs, _component_of(bpm), total, found, state[0], status | st)


def entropy_lanes(scan, tabs, dc, ac, h, w, ch, sub, S=1024, lanes=256):
    """rule 4 as the kernel runs it -> (coeffs, status, the passes every sequence took)"""
    plain, status = unstuff(scan)
    stream = Stream(plain)
    total = blocks_per_frame(h, w, ch, sub)
    bpm = 1 if ch == 1 else (6 if sub == S420 else 3)
    coeffs = np.zeros((total, 64), dtype=np.int16)

    def write(b, z, v):
        if b < total:
            coeffs[b, z] = v

    carried, base, passes = (0, 0, 0), 0, []
    for q in range(_cdiv(stream.L, S * lanes)):
        spans = [(q * S * lanes + i * S, min(q * S * lanes + (i + 1) * S, stream.L)) for i in range(lanes)]
        used = [carried] + [(spans[i][0], 0, 0) for i in range(1, lanes)]
        res = [_span(stream, tabs, dc, ac, bpm, *spans[i], used[i]) for i in range(lanes)]
        count = 1
        for _ in range(1, lanes):
            entry = [carried] + [res[i - 1][0] for i in range(1, lanes)]
            changed = [spans[i][0] < stream.L and entry[i] != used[i] for i in range(lanes)]       # a lane behind the end never asks for a pass
            if not any(changed):
                break
            count += 1
            for i in range(lanes):
                if changed[i]:
                    used[i] = entry[i]
            res = [_span(stream, tabs, dc, ac, bpm, *spans[i], used[i]) if changed[i] else res[i] for i in range(lanes)]
        passes.append(count)
        for i in range(lanes):
            status |= _span(stream, tabs, dc, ac, bpm, *spans[i], used[i], write, base)[2]
            base += res[i][1]
        carried = res[min(lanes - 1, (stream.L - q * S * lanes - 1) // S)][0]                            # the last lane with bits of the stream
    coeffs, status = _finish(stream, plain, coeffs, _component_of(bpm), total, base, carried[0], status)
    return coeffs, status, passes


# ---- rule 5
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_1d(d, n):
    """jidctint's pass over the last axis of d [..., 8] (int64), descaled by n"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (d[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    tmp2, tmp3 = z1 - i6 * 15137, z1 + i2 * 6270
    tmp0, tmp1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    z1, z2, z3, z4 = i7 + i1, i5 + i3, i7 + i3, i5 + i1
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = i7 * 2446, i5 * 16819, i3 * 25172, i1 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = np.empty_like(d)
    out[..., 0], out[..., 7] = _descale(t10 + a3, n), _descale(t10 - a3, n)
    out[..., 1], out[..., 6] = _descale(t11 + a2, n), _descale(t11 - a2, n)
    out[..., 2], out[..., 5] = _descale(t12 + a1, n), _descale(t12 - a1, n)
    out[..., 3], out[..., 4] = _descale(t13 + a0, n), _descale(t13 - a0, n)
    return out


def block_samples(coefs, table):
    """coefs [..., 64] zig-zag, table 64 natural -> samples int64 [..., 8, 8] in 0 .. 255"""
    nat = np.zeros(coefs.shape, dtype=np.int64)
    nat[..., ZIGZAG] = coefs.astype(np.int64)
    d = (nat * np.asarray(table, dtype=np.int64)).reshape(*coefs.shape[:-1], 8, 8)
    cols = np.swapaxes(_idct_1d(np.swapaxes(d, -1, -2), 11), -1, -2)
    return np.clip(_idct_1d(cols, 18) + 128, 0, 255)


def _plane(samples, rows, cols):
    """samples [rows x cols blocks, 8, 8] in raster order -> one plane"""
    return samples.reshape(rows, cols, 8, 8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)


def upsample_h2v2(s, hc, wc):
    """the REAL hc x wc samples of a chroma plane -> 2 hc x 2 wc (rule 5)"""
    s = s[:hc, :wc].astype(np.int64)
    if wc <= 2:
        return np.repeat(np.repeat(s, 2, axis=0), 2, axis=1)
    r = np.arange(hc)
    v = np.empty((2 * hc, wc), dtype=np.int64)
    v[0::2] = 3 * s + s[np.maximum(r - 1, 0)]
    v[1::2] = 3 * s + s[np.minimum(r + 1, hc - 1)]
    c = np.arange(wc)
    out = np.empty((2 * hc, 2 * wc), dtype=np.int64)
    out[:, 0::2] = (3 * v + v[:, np.maximum(c - 1, 0)] + 8) >> 4
    out[:, 1::2] = (3 * v + v[:, np.minimum(c + 1, wc - 1)] + 7) >> 4
    return out


def pixels(coeffs, quant, h, w, ch, sub):
    """coeffs int16 [blocks, 64] (scan order, absolute DC), quant [ch][64] -> uint8 [h, w, ch]"""
    bh, bw = _cdiv(h, 8), _cdiv(w, 8)
    if ch == 1:
        return _plane(block_samples(coeffs, quant[0]), bh, bw)[:h, :w, None].astype(np.uint8)
    if sub == S444:
        y, cb, cr = (_plane(block_samples(coeffs[c::3], quant[c]), bh, bw)[:h, :w] for c in range(3))
    else:
        my, mx = _cdiv(h, 16), _cdiv(w, 16)
        mcus = coeffs.reshape(my, mx, 6, 64)
        ys = block_samples(mcus[:, :, :4], quant[0]).reshape(my, mx, 2, 2, 8, 8)          # MCU row, MCU col, block row, block col
        y = ys.transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16)[:h, :w]
        hc, wc = _cdiv(h, 2), _cdiv(w, 2)
        cb, cr = (upsample_h2v2(_plane(block_samples(mcus[:, :, 4 + c], quant[1 + c]), my, mx), hc, wc)[:h, :w] for c in range(2))
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data, lanes=None):
    """a file -> (uint8 [h, w, ch], status); ``lanes``: (S, lane count) runs the emulation of the parallel decoder"""
    hd = parse(data)
    args = (hd["scan"], decode_set(hd), hd["dc"], hd["ac"], hd["h"], hd["w"], hd["ch"], hd["sub"])
    coeffs, status = entropy_lanes(*args, *lanes)[:2] if lanes else entropy_sequential(*args)
    return pixels(coeffs, hd["quant"], hd["h"], hd["w"], hd["ch"], hd["sub"]), status
