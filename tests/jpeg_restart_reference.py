"""A numpy / Python restatement of the two restart-interval rules (include/ttvdm.h: "JPEG export" rule 6a, "JPEG import" rules 1a and
4a), written from the rules and ITU-T T.81 on top of tests/jpeg_reference.py and tests/jpeg_decode_reference.py, which stay as they
are.  The encoder side: the scan with the DC predictors reset and pad + RSTn behind every interval but the last, the symbol counts with
the same resets, the file with its DRI segment.  The decoder side: a scan walker of its own (the decode restatement's parser asserts
"no DRI") that cuts the scan into spans, and a plain sequential decoder run span by span.  Slow and plain on purpose; the tests hold
the library to it byte for byte, and hold IT to Pillow's restart_marker_blocks / restart_marker_rows."""
import struct

import numpy as np

from tests import jpeg_decode_reference as dec
from tests import jpeg_reference as ref


def blocks_per_mcu(ch, sub):
    return 1 if ch == 1 else (6 if sub == ref.S420 else 3)


def mcus_per_row(w, ch, sub):
    return ref._cdiv(w, 16 if (ch == 3 and sub == ref.S420) else 8)


def mcus_of(h, w, ch, sub):
    return ref.blocks_per_frame(h, w, ch, sub) // blocks_per_mcu(ch, sub)


def markers_of(h, w, ch, sub, ri):
    """how many RSTn a frame's scan holds: none behind the last interval"""
    return ref._cdiv(mcus_of(h, w, ch, sub), ri) - 1 if ri else 0


# ---- export rule 6a
def interval_symbols(coefs, comps, ri_blocks):
    """-> [the symbols of one interval's blocks, as ref.symbols gives them: the predictors are 0 at its first MCU]"""
    n = len(coefs)
    step = ri_blocks or n
    return [ref.symbols(coefs[at:at + step], comps[at:at + step]) for at in range(0, n, step)]


def symbol_counts(coefs, comps, ri_blocks):
    counts = np.zeros((4, 256), dtype=np.int64)
    for interval in interval_symbols(coefs, comps, ri_blocks):
        for blk in interval:
            for t, s, _, _ in blk:
                counts[t, s] += 1
    return counts


def scan_bytes(coefs, comps, ri_blocks, tables=None):
    """the entropy-coded segment with restart intervals of ``ri_blocks`` blocks (0: none).  Every interval is ref.scan_bytes of its own
    blocks -- codes MSB first, a 00 behind every FF, the last byte filled with one-bits and STUFFED when that makes it FF --; FF D0 + (k
    mod 8), not stuffed, stands behind the k-th interval unless it is the last"""
    n = len(coefs)
    step = ri_blocks or n
    out = bytearray()
    for k, at in enumerate(range(0, n, step)):
        out += ref.scan_bytes(coefs[at:at + step], comps[at:at + step], tables)
        if at + step < n:
            out += bytes([0xff, 0xd0 + (k & 7)])
    return bytes(out)


def with_dri(data, ri):
    """the file with FF DD 00 04 Ri directly before SOS"""
    at = 2
    while data[at + 1] != 0xda:
        at += 2 + struct.unpack(">H", data[at + 2:at + 4])[0]
    return data[:at] + b"\xff\xdd\x00\x04" + struct.pack(">H", ri) + data[at:]


def jpeg_file(frame, quality=75, sub=ref.S420, ri=0, tables=None):
    """one frame -> its file with a restart interval of ``ri`` MCUs; ``tables`` as ref.jpeg_file takes them (a function gets the counts
    taken with the predictor resets)"""
    coefs, comps, _ = ref.coefficients(frame, quality, sub)
    h, w, ch = frame.shape
    ri_blocks = ri * blocks_per_mcu(ch, sub)
    if callable(tables):
        tables = tables(symbol_counts(coefs, comps, ri_blocks))
    data = ref.file_of(scan_bytes(coefs, comps, ri_blocks, tables), h, w, ch, quality, sub, tables)
    return with_dri(data, ri) if ri else data


# ---- import rules 1a and 4a
def parse(data):
    """a baseline file, with or without DRI -> dec.parse's dict, plus ``ri`` and ``spans``: [(byte offset in the file, stuffed length)]
    per restart interval, markers excluded.  AssertionError for markers out of order or count."""
    at, ri, plain = 2, 0, bytearray(data[:2])
    while True:                                     # the file without its DRI segments: what dec.parse reads
        assert data[at] == 0xff
        marker = data[at + 1]
        (size,) = struct.unpack(">H", data[at + 2:at + 4])
        if marker == 0xdd:
            (ri,) = struct.unpack(">H", data[at + 4:at + 6])
        else:
            plain += data[at:at + 2 + size]
        at += 2 + size
        if marker == 0xda:
            break
    hd = dec.parse(bytes(plain) + data[at:])
    end = data.rindex(b"\xff\xd9")
    spans, first, i, k = [], at, at, 0
    while i < end:
        if data[i] == 0xff and 0xd0 <= data[i + 1] <= 0xd7:
            assert ri and data[i + 1] == 0xd0 + (k & 7), (i, k, ri)
            spans.append((first, i - first))
            first, i, k = i + 2, i + 2, k + 1
        else:
            i += 2 if (data[i] == 0xff and data[i + 1] == 0) else 1
    spans.append((first, end - first))
    assert k == markers_of(hd["h"], hd["w"], hd["ch"], hd["sub"], ri), (k, ri)
    hd.update(ri=ri, spans=spans, scan_offset=at, scan_bytes=end - at)
    return hd


def entropy(data, hd):
    """span by span, each from the true state (0, 0, 0) and with its own DC prefix sum -> (coeffs int16 [blocks, 64], status)"""
    h, w, ch, sub = hd["h"], hd["w"], hd["ch"], hd["sub"]
    total, bpm = ref.blocks_per_frame(h, w, ch, sub), blocks_per_mcu(ch, sub)
    per = hd["ri"] * bpm if len(hd["spans"]) > 1 else total
    tabs = dec.decode_set(hd)
    coeffs = np.zeros((total, 64), dtype=np.int16)
    status = 0
    for k, (at, n) in enumerate(hd["spans"]):
        first, count = k * per, min(per, total - k * per)
        part = coeffs[first:first + count]
        plain, st = dec.unstuff(data[at:at + n])
        stream = dec.Stream(plain)

        def write(b, z, v, part=part, count=count):
            if b < count:
                part[b, z] = v

        state, found, st2 = dec._span(stream, tabs, hd["dc"], hd["ac"], bpm, 0, stream.L, (0, 0, 0), write)
        _, st3 = dec._finish(stream, plain, part, dec._component_of(bpm), count, found, state[0], st | st2)
        status |= st3
    return coeffs, status


def decode(data):
    """a file -> (uint8 [h, w, ch], status)"""
    hd = parse(data)
    coeffs, status = entropy(data, hd)
    return dec.pixels(coeffs, hd["quant"], hd["h"], hd["w"], hd["ch"], hd["sub"]), status
