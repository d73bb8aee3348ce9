"""The segmented LZW stream of include/ttvdm.h ("GIF LZW on the device", rules 1 - 6) stated twice on the host, and searches for the inputs
that sit on its edges.

`restate` follows the rules with a Python dictionary for the string table (rule 7: greedy LZW has one answer, whatever the table is).
`splice` does not code anything: it takes the streams that the host coder (export.lzw_frame, tt_gif_lzw) gives for each segment alone,
reads their codes back, drops the leading clear and the end-of-information code as rule 2 says, and packs the codes of all segments
behind one another -- the widths come from the host coder's own streams, not from a formula.  Neither shares code with the kernels."""
import numpy as np

MAX_BITS, MAX_CODES = 12, 4096
SEGMENT_DEFAULT = 16384                            # TT_LZW_SEGMENT


def segment_codes(pixels, mcs):
    """rule 3: one segment's pixels -> ([(code, width)], the width of the code that closes the segment (rule 4))"""
    clear = 1 << mcs
    table, nxt, width = {}, clear + 2, mcs + 1
    out = []
    prefix = int(pixels[0])
    for c in pixels[1:]:
        c = int(c)
        if (prefix, c) in table:
            prefix = table[(prefix, c)]
            continue
        out.append((prefix, width))
        if nxt < MAX_CODES:
            table[(prefix, c)] = nxt
            if nxt == 1 << width and width < MAX_BITS:
                width += 1
            nxt += 1
        else:
            out.append((clear, width))
            table, nxt, width = {}, clear + 2, mcs + 1
        prefix = c
    out.append((prefix, width))
    if nxt == 1 << width and width < MAX_BITS:
        width += 1
    return out, width


def frame_data(codes):
    """rules 5 and 6 behind the min-code-size byte: [(code, width)] -> the sub-blocks and the terminator"""
    acc = nbits = 0
    for code, width in codes:
        acc |= code << nbits
        nbits += width
    payload = acc.to_bytes((nbits + 7) // 8, "little")
    out = bytearray()
    for at in range(0, len(payload), 255):
        block = payload[at:at + 255]
        out += bytes([len(block)]) + block
    return bytes(out) + b"\x00"


def restate(indices, mcs, segment=None):
    """rules 1 - 6: one frame's indices -> its image data"""
    px = np.asarray(indices, dtype=np.uint8).reshape(-1)
    segment = SEGMENT_DEFAULT if segment is None else int(segment)
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    stream, width = [], mcs + 1
    for at in range(0, px.size, segment):
        stream.append((clear, width))
        codes, width = segment_codes(px[at:at + segment], mcs)
        stream += codes
    stream.append((eoi, width))
    return bytes([mcs]) + frame_data(stream)


def read_codes(data):
    """image data -> [(code, width)] up to and including the end-of-information code, by the decoder's width rule (a decoder makes an
    entry with every code but the first behind a clear code, and widens when the table reaches 2^width)"""
    mcs = data[0]
    pos, payload = 1, bytearray()
    while data[pos]:
        payload += data[pos + 1:pos + 1 + data[pos]]
        pos += 1 + data[pos]
    bits = int.from_bytes(bytes(payload), "little")
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    out, at, width, size, first = [], 0, mcs + 1, clear + 2, True
    while True:
        code = (bits >> at) & ((1 << width) - 1)
        out.append((code, width))
        at += width
        if code == eoi:
            return out
        if code == clear:
            width, size, first = mcs + 1, clear + 2, True
            continue
        if not first and size < MAX_CODES:
            size += 1
            if size == 1 << width and width < MAX_BITS:
                width += 1
        first = False


def splice(indices, mcs, segment, lzw_frame):
    """the second construction: `lzw_frame` (the host coder) on every segment alone, its streams' codes spliced by rule 2"""
    px = np.asarray(indices, dtype=np.uint8).reshape(-1)
    segment = SEGMENT_DEFAULT if segment is None else int(segment)
    clear, eoi = 1 << mcs, (1 << mcs) + 1
    stream = [(clear, mcs + 1)]
    parts = [px[at:at + segment] for at in range(0, px.size, segment)]
    for i, part in enumerate(parts):
        codes = read_codes(lzw_frame(part, mcs))
        assert codes[0] == (clear, mcs + 1) and codes[-1][0] == eoi
        stream += codes[1:-1]
        stream.append((eoi if i == len(parts) - 1 else clear, codes[-1][1]))        # rule 4: at the width of the coder's own closing code
    return bytes([mcs]) + frame_data(stream)


# ---- inputs
def random_indices(npix, mcs, seed):
    return np.random.default_rng(seed).integers(0, 1 << mcs, size=npix, dtype=np.int64).astype(np.uint8)


def checker(npix, width=7):
    i = np.arange(npix)
    return ((i % width + i // width) & 1).astype(np.uint8)


def data_bytes(data):
    """image data -> the bytes of its sub-blocks together"""
    return len(data) - 2 - (len(data) - 2 + 255) // 256


# ---- searches (CPU, a few milliseconds each)
def find_width_bump(mcs=2, segment=None):
    """the shortest run of random indices whose (only) segment's closing code is one bit wider than its last data code"""
    for npix in range(2, 200):
        px = random_indices(npix, mcs, 100 + npix)
        codes, closing = segment_codes(px[:segment] if segment else px, mcs)
        if closing == codes[-1][1] + 1:
            return px
    raise AssertionError("no width bump found")


def find_data_bytes(target, mcs=8, segment=64):
    """random indices whose segmented stream holds exactly `target` data bytes"""
    for seed in range(64):
        lo, hi = 1, 2 * target
        while lo < hi:                                           # data bytes grow with the pixels: bisect, then look around
            mid = (lo + hi) // 2
            if data_bytes(restate(random_indices(mid, mcs, seed), mcs, segment)) < target:
                lo = mid + 1
            else:
                hi = mid
        for npix in range(max(1, lo - 3), lo + 4):
            px = random_indices(npix, mcs, seed)
            if data_bytes(restate(px, mcs, segment)) == target:
                return px
    raise AssertionError(f"no input with {target} data bytes found")


def table_full_input():
    """9216 random 8-bit indices: as ONE segment the table fills and resets inside it"""
    return random_indices(9216, 8, 7)
