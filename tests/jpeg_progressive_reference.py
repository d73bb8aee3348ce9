"""A numpy / Python restatement of the JPEG import's progressive rules (include/ttvdm.h, "JPEG import", rules 1b and 4b), written from
the rules, ITU-T T.81 Annex G and libjpeg's jdphuff.c / jcphuff.c: a parser of SOF2 files, a plain serial decoder per scan kind, an
emulation of the four device schemes (rule 4's lanes and passes for the first scans, the bit-k rule of a DC refinement, the masks /
walk / replay of an AC refinement), and a progressive WRITER that turns the quantised coefficients of ``jpeg_reference.coefficients``
and any valid scan script into a file with per-scan Huffman tables.  Integers only; slow and plain on purpose.  The tests hold the
library to it bit for bit and hold IT to Pillow's decoder."""
import struct

import numpy as np

from tests.jpeg_decode_reference import BLOCKS, CODE, TAIL, DecodeTable, Stream, pixels, unstuff
from tests.jpeg_reference import S420, S444, ZIGZAG, _cdiv, _segment, blocks_per_frame, quant_tables
from tests.png_reference import package_merge

SPAN = 16                                           # the status bit a descriptor no scan has sets; a parsed file never does
LANE_BLOCKS_MAX, SCAN_BLOCKS_MAX, MASK_STAGE = 1 << 22, 0x7fffffff, 1024

# Pillow's (libjpeg's jpeg_simple_progression) scripts, for comparison with what the parser reads
PILLOW_COLOUR = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
                 ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
PILLOW_GREY = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]


def _every(ch):
    return tuple(range(1 if ch == 1 else 3))


# ---- the scripts the tests cover: (components, Ss, Se, Ah, Al) per scan
def script_spectral(ch):
    """spectral selection only: every Al = 0"""
    out = [(_every(ch), 0, 0, 0, 0)]
    for c in _every(ch):
        out += [((c,), 1, 5, 0, 0), ((c,), 6, 63, 0, 0)]
    return out


def script_two_refinements(ch):
    """Al 2 -> 1 -> 0 for every coefficient"""
    out = [(_every(ch), 0, 0, 0, 2)] + [((c,), 1, 63, 0, 2) for c in _every(ch)]
    for al in (1, 0):
        out += [(_every(ch), 0, 0, al + 1, al)] + [((c,), 1, 63, al + 1, al) for c in _every(ch)]
    return out


def script_separate_dc(ch):
    """per-component DC scans (first and refinement) instead of interleaved ones"""
    out = [((c,), 0, 0, 0, 1) for c in _every(ch)] + [((c,), 1, 63, 0, 1) for c in _every(ch)]
    return out + [((c,), 0, 0, 1, 0) for c in reversed(_every(ch))] + [((c,), 1, 63, 1, 0) for c in _every(ch)]


def script_bands_1_and_2_63(ch):
    """the bands 1 .. 1 and 2 .. 63, each with one refinement"""
    out = [(_every(ch), 0, 0, 0, 0)]
    for c in _every(ch):
        out += [((c,), 1, 1, 0, 1), ((c,), 2, 63, 0, 1), ((c,), 2, 63, 1, 0), ((c,), 1, 1, 1, 0)]
    return out


def script_band_per_coefficient(ch):
    """component 0: one scan a coefficient, first and refinement (2 x 63 scans); the others 1 .. 63 at once"""
    out = [(_every(ch), 0, 0, 0, 0)] + [((0,), k, k, 0, 1) for k in range(1, 64)] + [((c,), 1, 63, 0, 0) for c in _every(ch)[1:]]
    return out + [((0,), k, k, 1, 0) for k in range(63, 0, -1)]


SCRIPTS = {"spectral": script_spectral, "two_refinements": script_two_refinements, "separate_dc": script_separate_dc,
           "bands_1_and_2_63": script_bands_1_and_2_63, "band_per_coefficient": script_band_per_coefficient}


# ---- the block map (rule 4b): the scan's block order -> [(block of the layout, component)]
def scan_order(h, w, ch, sub, comps):
    total = blocks_per_frame(h, w, ch, sub)
    if ch == 1:
        return [(k, 0) for k in range(total)]
    bpm = 6 if sub == S420 else 3
    if len(comps) == 3:
        return [(k, (0 if k % 6 < 4 else k % 6 - 3) if bpm == 6 else k % 3) for k in range(total)]
    (c,) = comps
    if bpm == 3:
        return [(3 * k + c, c) for k in range(total // 3)]
    mx = _cdiv(w, 16)
    if c:
        return [(6 * k + 3 + c, c) for k in range(total // 6)]
    return [(((by >> 1) * mx + (bx >> 1)) * 6 + (by & 1) * 2 + (bx & 1), 0) for by in range(_cdiv(h, 8)) for bx in range(_cdiv(w, 8))]


# ---- rule 1b
def parse(data):
    """a progressive file -> dict(h, w, ch, sub, quant [ch][64] natural order, scans: [dict(comps, ss, se, ah, al, offset, bytes,
    tables {slot: (BITS, HUFFVAL)})]): a DC-first scan's slot c is component c's DC table, an AC scan's slot 0 its AC table"""
    assert data[:2] == b"\xff\xd8"
    at, quant, tables, out, scans, comps = 2, {}, {}, {}, [], []
    while True:
        while data[at] == 0xff and data[at + 1] == 0xff:
            at += 1
        assert data[at] == 0xff
        marker = data[at + 1]
        if marker == 0xd9:
            break
        (size,) = struct.unpack(">H", data[at + 2:at + 4])
        p = data[at + 4:at + 2 + size]
        at += 2 + size
        if marker == 0xdb:
            assert not scans
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
        elif marker == 0xc2:
            prec, h, w, nc = struct.unpack(">BHHB", p[:6])
            assert prec == 8 and nc in (1, 3)
            comps = [(p[6 + 3 * c], p[7 + 3 * c], p[8 + 3 * c]) for c in range(nc)]
            out.update(h=h, w=w, ch=nc, sub=S420 if (nc == 3 and comps[0][1] == 0x22) else S444)
        elif marker == 0xda:
            ids = [c[0] for c in comps]
            which = [ids.index(p[1 + 2 * i]) for i in range(p[0])]
            ss, se, a = p[1 + 2 * p[0]:4 + 2 * p[0]]
            sc = dict(comps=tuple(sorted(which)), ss=ss, se=se, ah=a >> 4, al=a & 15, offset=at, tables={})
            for i, c in enumerate(which):
                if ss == 0 and a >> 4 == 0:
                    sc["tables"][c] = tables[p[2 + 2 * i] >> 4]
                elif ss > 0:
                    sc["tables"][0] = tables[0x10 | (p[2 + 2 * i] & 15)]
            while not (data[at] == 0xff and data[at + 1] != 0):
                at += 1
            sc["bytes"] = at - sc["offset"]
            scans.append(sc)
        else:
            assert marker not in (0xc0, 0xc1, 0xdd) or (marker == 0xdd and p == b"\x00\x00")
    out["quant"] = [quant[q] for _, _, q in comps]
    out["scans"] = scans
    return out


def _decode_tables(sc):
    return [DecodeTable(*sc["tables"][k]) if k in sc["tables"] else None for k in range(3)]


def _extend(raw, n):
    return (raw if raw >> (n - 1) else raw - (1 << n) + 1) if n else 0


def _i16(v):
    return np.int16(((int(v) + 32768) & 0xffff) - 32768)


def _tail(stream, plain, p):
    left = stream.L - min(p, stream.L)
    return TAIL if left >= 8 or (left and (plain[-1] & ((1 << left) - 1)) != (1 << left) - 1) else 0


# ---- first scans: f_i of rule 4b
def _first_span(stream, tabs, sc, order, inter, bpm, start, end, state, write=None, block=0):
    """the whole symbols that start in [max(p, start), end); state (p, m, z) -> (exit state, blocks completed, status)"""
    p, m, z = state
    dc, ss, se = sc["ss"] == 0, sc["ss"], sc["se"]
    done, status = 0, 0
    if p < start:
        return state, 0, 0
    while p < end:
        avail = stream.L - p
        slot = ((0 if m < 4 else m - 3) if bpm == 6 else min(m, 2)) if (dc and inter) else (sc["comps"][0] if dc else 0)
        t = tabs[slot]
        v = stream.peek(p, 32)
        hit = t.find(v >> 16) if t is not None else None
        if hit is None:
            if avail < 16:
                break
            status |= CODE
            p += 1
            continue
        length, sym = hit
        n, r = sym & 15, sym >> 4
        if not dc and n == 0 and r < 15:
            if length + r > avail:
                break
            extra = (v >> (32 - length - r)) & ((1 << r) - 1) if r else 0
            p += length + r
            done = min(done + (1 << r) + extra, LANE_BLOCKS_MAX)
            z = ss
            continue
        if length + n > avail:
            break
        value = _extend((v >> (32 - length - n)) & ((1 << n) - 1) if n else 0, n)
        p += length + n
        ends = False
        if dc:
            if sym > 11:
                status |= CODE
            if write:
                write(block + done, 0, value)
            if inter:
                m = (m + 1) % bpm
            ends = True
        elif n == 0:
            z += 16
            ends = z > se
        else:
            z += r
            if z > se:
                ends, status = True, status | CODE
            else:
                if write:
                    write(block + done, z, value << sc["al"])
                z += 1
                ends = z > se
        if ends:
            if not dc:
                z = ss
            done = min(done + 1, LANE_BLOCKS_MAX)
    return (p, m, z), done, status


def _dc_prefix(coeffs, order, al):
    pred = [0, 0, 0]
    for lb, c in order:
        pred[c] += int(coeffs[lb, 0])
        coeffs[lb, 0] = _i16(pred[c] << al)


def _first_scan(coeffs, sc, order, inter, bpm, plain, lanes):
    stream, tabs = Stream(plain), _decode_tables(sc)
    dc = sc["ss"] == 0

    def write(k, z, v):
        if k < len(order):
            coeffs[order[k][0], z] = _i16(v)

    true0 = (0, 0, 0 if dc else sc["ss"])
    status = 0
    if lanes is None:
        state, base, status = _first_span(stream, tabs, sc, order, inter, bpm, 0, stream.L, true0, write)
    else:
        S, nl = lanes
        carried, base = true0, 0
        for q in range(_cdiv(stream.L, S * nl)):
            spans = [(q * S * nl + i * S, min(q * S * nl + (i + 1) * S, stream.L)) for i in range(nl)]
            used = [carried] + [(spans[i][0], 0, true0[2]) for i in range(1, nl)]
            res = [_first_span(stream, tabs, sc, order, inter, bpm, *spans[i], used[i]) for i in range(nl)]
            for _ in range(1, nl):
                entry = [carried] + [res[i - 1][0] for i in range(1, nl)]
                changed = [spans[i][0] < stream.L and entry[i] != used[i] for i in range(nl)]
                if not any(changed):
                    break
                for i in range(nl):
                    if changed[i]:
                        used[i] = entry[i]
                res = [_first_span(stream, tabs, sc, order, inter, bpm, *spans[i], used[i]) if changed[i] else res[i] for i in range(nl)]
            first = base
            for i in range(nl):
                status |= _first_span(stream, tabs, sc, order, inter, bpm, *spans[i], used[i], write, first)[2]
                first += res[i][1]
            base = min(first, SCAN_BLOCKS_MAX)
            carried = res[min(nl - 1, (stream.L - q * S * nl - 1) // S)][0]
        state = carried
    if base != len(order):
        status |= BLOCKS
    status |= _tail(stream, plain, state[0])
    if dc:
        _dc_prefix(coeffs, order, sc["al"])
    return status


# ---- DC refinement: bit k is block k's
def _dc_refine(coeffs, sc, order, plain):
    L = 8 * len(plain)
    for k, (lb, _) in enumerate(order):
        if k < L and (plain[k >> 3] >> (7 - (k & 7))) & 1:
            coeffs[lb, 0] = _i16(int(coeffs[lb, 0]) | (1 << sc["al"]))
    return (BLOCKS if L < len(order) else 0) | _tail(Stream(plain), plain, min(len(order), L))


# ---- AC refinement
def _refine_coef(coeffs, lb, z, bit, p1):
    c = int(coeffs[lb, z])
    if bit and (c & p1) == 0:
        coeffs[lb, z] = _i16(c + p1 if c >= 0 else c - p1)


def _ac_refine_serial(coeffs, sc, order, plain):
    """libjpeg's decode_mcu_AC_refine over the scan's blocks: reads coefficients and bits as it goes"""
    stream, t = Stream(plain), _decode_tables(sc)[0]
    ss, se, p1 = sc["ss"], sc["se"], 1 << sc["al"]
    p, run, status = 0, 0, 0
    for lb, _ in order:
        z = ss
        if run == 0:
            while z <= se:
                hit = t.find(stream.peek(p, 16))
                assert hit is not None, "the serial decoder takes valid streams"
                length, sym = hit
                p += length
                r, s = sym >> 4, sym & 15
                value = 0
                if s:
                    assert s == 1
                    value = p1 if stream.peek(p, 1) else -p1
                    p += 1
                elif r < 15:
                    run = (1 << r) + (stream.peek(p, r) if r else 0)
                    p += r
                    break
                while z <= se:
                    if coeffs[lb, z]:
                        _refine_coef(coeffs, lb, z, stream.peek(p, 1), p1)
                        p += 1
                    else:
                        r -= 1
                        if r < 0:
                            break
                    z += 1
                if s and z <= se:
                    coeffs[lb, z] = _i16(value)
                z += 1
        if run > 0:
            while z <= se:
                if coeffs[lb, z]:
                    _refine_coef(coeffs, lb, z, stream.peek(p, 1), p1)
                    p += 1
                z += 1
            run -= 1
    assert p <= stream.L
    return status | _tail(stream, plain, p)


def _ac_refine_device(coeffs, sc, order, plain, window_bits=1 << 18):
    """rule 4b's masks, walk and replay.  The walk's stages change nothing it computes (a stage only refills LDS), so they are not
    emulated; ``window_bits`` is kept for the bound on the stages, which is asserted"""
    stream, t = Stream(plain), _decode_tables(sc)[0]
    ss, se, p1, L = sc["ss"], sc["se"], 1 << sc["al"], 8 * len(plain)
    band = ((1 << (se + 1)) - 1) & ~((1 << ss) - 1)
    masks = [sum(1 << z for z in range(ss, se + 1) if coeffs[lb, z]) for lb, _ in order]
    n = len(order)
    starts, status = [None] * n, 0
    p, b, z, run, fresh, steps = 0, 0, ss, 0, True, 0
    while b < n and p <= L:
        steps += 1
        M = masks[b]
        if run:
            starts[b] = (p, True)
            p += bin(M).count("1")
            run, b = run - 1, b + 1
            continue
        if fresh:
            starts[b], fresh = (p, False), False
        avail = L - p
        v = stream.peek(p, 32)
        hit = t.find(v >> 16) if t is not None else None
        if hit is None or hit[0] > avail:
            if hit is None and avail >= 16:
                status |= CODE
            break
        length, sym = hit
        r, s = sym >> 4, sym & 15
        ahead = ~((1 << z) - 1)
        if s == 0 and r < 15:
            if length + r > avail:
                break
            run = (1 << r) + ((v >> (32 - length - r)) & ((1 << r) - 1) if r else 0) - 1
            p += length + r + bin(M & ahead).count("1")
            b, z, fresh = b + 1, ss, True
            continue
        if s > 1:
            status |= CODE
        sign = 1 if s else 0
        if length + sign > avail:
            break
        zeros = ~M & band & ahead
        for _ in range(r):
            zeros &= zeros - 1
        k = (zeros & -zeros).bit_length() - 1 if zeros else se + 1
        p += length + sign + bin(M & ahead & ((1 << k) - 1)).count("1")
        if k > se and s:
            status |= CODE
        z = k + 1
        if z > se:
            b, z, fresh = b + 1, ss, True
    assert steps <= (L // (window_bits - 31) + n // MASK_STAGE + 2) * (window_bits + MASK_STAGE)
    if b != n or p > L:
        status |= BLOCKS
    status |= _tail(stream, plain, p)

    def bit(q):
        return stream.peek(q, 1) if q < L else 0

    for k in range(min(b, n)):
        lb = order[k][0]
        q, in_run = starts[k]
        zz = ss
        for _ in range(64):
            if in_run or zz > se or q >= L:
                break
            v = stream.peek(q, 32)
            hit = t.find(v >> 16) if t is not None else None
            if hit is None or hit[0] > L - q:
                break
            length, sym = hit
            r, s = sym >> 4, sym & 15
            if s == 0 and r < 15:
                q += length + r
                in_run = True
                break
            value = p1 if (v >> (31 - length)) & 1 else -p1
            q += length + (1 if s else 0)
            while zz <= se:
                if coeffs[lb, zz]:
                    _refine_coef(coeffs, lb, zz, bit(q), p1)
                    q += 1
                else:
                    r -= 1
                    if r < 0:
                        break
                zz += 1
            if s and zz <= se:
                coeffs[lb, zz] = _i16(value)
            zz += 1
        if in_run:
            while zz <= se:
                if coeffs[lb, zz]:
                    _refine_coef(coeffs, lb, zz, bit(q), p1)
                    q += 1
                zz += 1
    return status


# ---- a whole file
def entropy(data, hd, lanes=None):
    """every scan applied in file order -> (coeffs int16 [blocks, 64] of the layout, status).  ``lanes``: None -- the serial decoders --
    or (S, lane count) -- the device schemes"""
    h, w, ch, sub = hd["h"], hd["w"], hd["ch"], hd["sub"]
    coeffs = np.zeros((blocks_per_frame(h, w, ch, sub), 64), dtype=np.int16)
    bpm = 1 if ch == 1 else (6 if sub == S420 else 3)
    status = 0
    for sc in hd["scans"]:
        plain, st = unstuff(data[sc["offset"]:sc["offset"] + sc["bytes"]])
        status |= st
        order = scan_order(h, w, ch, sub, sc["comps"])
        inter = ch == 3 and len(sc["comps"]) == 3
        if sc["ah"] == 0:
            status |= _first_scan(coeffs, sc, order, inter, bpm, plain, lanes)
        elif sc["ss"] == 0:
            status |= _dc_refine(coeffs, sc, order, plain)
        elif lanes is None:
            status |= _ac_refine_serial(coeffs, sc, order, plain)
        else:
            status |= _ac_refine_device(coeffs, sc, order, plain, lanes[0] * lanes[1])
    return coeffs, status


def decode(data, lanes=None):
    """a progressive file -> (uint8 [h, w, ch], status)"""
    hd = parse(data)
    coeffs, status = entropy(data, hd, lanes)
    return pixels(coeffs, hd["quant"], hd["h"], hd["w"], hd["ch"], hd["sub"]), status


# ---- the writer (jcphuff.c's four encoders over a scan's blocks)
def optimal_table(counts):
    """symbol counts {symbol: n} -> (BITS, HUFFVAL): a length-limited (16) Huffman code in which no code is all one-bits: a reserved
    symbol of count 1, first in the leaf order, takes a longest code and is dropped"""
    shifted = [1] + [int(counts.get(s, 0)) for s in range(256)]
    lengths = package_merge(shifted, 16)
    assert lengths[0] == max(lengths)
    bits = [sum(1 for s in range(256) if lengths[s + 1] == n) for n in range(1, 17)]
    vals = [s for n in range(1, 17) for s in range(256) if lengths[s + 1] == n]
    return bits, vals


def _category(v):
    return int(abs(int(v))).bit_length()


def _scan_items(coefs, sc_comps, ss, se, ah, al, order, inter):
    """the scan's symbols and raw bits in order: ("S", table slot, symbol) and ("B", value, bit count)"""
    out = []
    if ss == 0 and ah == 0:
        pred = [0, 0, 0]
        for lb, c in order:
            v = int(coefs[lb, 0]) >> al
            diff, pred[c] = v - pred[c], v
            n = _category(diff)
            out += [("S", c, n), ("B", (diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)]
        return out
    if ss == 0:
        return [("B", (int(coefs[lb, 0]) >> al) & 1, 1) for lb, _ in order]
    eobrun, pending = 0, []                        # pending: the correction bits of the blocks inside the EOB run

    def flush_run():
        nonlocal eobrun, pending
        if eobrun:
            n = eobrun.bit_length() - 1
            out.append(("S", 0, n << 4))
            if n:
                out.append(("B", eobrun & ((1 << n) - 1), n))
            eobrun = 0
        out.extend(("B", b, 1) for b in pending)
        pending = []

    for lb, _ in order:
        mag = [abs(int(coefs[lb, k])) >> al for k in range(64)]
        r, mine = 0, []                            # mine: this block's correction bits since its last code
        if ah == 0:
            for k in range(ss, se + 1):
                if mag[k] == 0:
                    r += 1
                    continue
                flush_run()
                while r > 15:
                    out.append(("S", 0, 0xf0))
                    r -= 16
                n = mag[k].bit_length()
                out += [("S", 0, (r << 4) | n), ("B", (mag[k] if coefs[lb, k] > 0 else ~mag[k]) & ((1 << n) - 1), n)]
                r = 0
            if r:
                eobrun += 1
                if eobrun == 0x7fff:
                    flush_run()
            continue
        last_new = max([k for k in range(ss, se + 1) if mag[k] == 1], default=0)
        for k in range(ss, se + 1):
            if mag[k] == 0:
                r += 1
                continue
            while r > 15 and k <= last_new:
                flush_run()
                out.append(("S", 0, 0xf0))
                r -= 16
                out.extend(("B", b, 1) for b in mine)
                mine = []
            if mag[k] > 1:
                mine.append(mag[k] & 1)
                continue
            flush_run()
            out += [("S", 0, (r << 4) | 1), ("B", 0 if coefs[lb, k] < 0 else 1, 1)]
            out.extend(("B", b, 1) for b in mine)
            mine, r = [], 0
        if r or mine:
            eobrun += 1
            pending += mine
            if eobrun == 0x7fff or len(pending) > 1000 - 64 + 1:
                flush_run()
    flush_run()
    return out


def _pack(items, codes):
    acc, nacc, out = 0, 0, bytearray()
    for kind, a, b in items:
        if kind == "S":
            code, length = codes[a][b]
        else:
            code, length = a, b
        acc, nacc = (acc << length) | code, nacc + length
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


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def progressive_file(coefs, h, w, ch, quality, sub, script):
    """the quantised coefficients of ``jpeg_reference.coefficients`` (the layout: scan order of the baseline scan, dummy blocks included)
    and a scan script -> a progressive file; every scan carries Huffman tables built from its own counts"""
    qt = quant_tables(quality)
    ncomp = 1 if ch == 1 else 3
    out = [b"\xff\xd8", _segment(0xe0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for i in range(1 if ncomp == 1 else 2):
        out.append(_segment(0xdb, bytes([i]) + bytes(qt[i][z] for z in ZIGZAG)))
    sof = struct.pack(">BHHB", 8, h, w, ncomp) + bytes([1, 0x22 if (ncomp == 3 and sub == S420) else 0x11, 0])
    if ncomp == 3:
        sof += bytes([2, 0x11, 1, 3, 0x11, 1])
    out.append(_segment(0xc2, sof))
    for comps, ss, se, ah, al in script:
        order = scan_order(h, w, ch, sub, comps)
        inter = ncomp == 3 and len(comps) == 3
        items = _scan_items(coefs, comps, ss, se, ah, al, order, inter)
        counts = {}
        for kind, a, b in items:
            if kind == "S":
                counts.setdefault(a, {})
                counts[a][b] = counts[a].get(b, 0) + 1
        codes = {}
        for slot, cnt in sorted(counts.items()):
            bits, vals = optimal_table(cnt)
            codes[slot] = _codes(bits, vals)
            out.append(_segment(0xc4, bytes([(0x10 if ss else 0x00) | slot]) + bytes(bits) + bytes(vals)))
        sos = bytes([len(comps)]) + b"".join(bytes([c + 1, (c << 4) if ss == 0 else 0]) for c in comps) + bytes([ss, se, (ah << 4) | al])
        out += [_segment(0xda, sos), _pack(items, codes)]
    out.append(b"\xff\xd9")
    return b"".join(out)
