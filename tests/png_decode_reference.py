"""The PNG import of include/ttvdm.h ("PNG import") restated in pure Python / numpy: the chunk walk with its refusals, a serial inflate that
yields the token list and the status bits of rule 3, a tiny writer of stored, fixed and dynamic blocks from a token list (for streams no
encoder produces), the serial unfilter, and the two parallel formulations the kernels use -- pointer doubling over source words and the
anti-diagonal wavefront -- stated in numpy.  ``inflate_cases`` and ``file_cases`` are the streams and files the CPU and GPU tests share."""
import heapq
import io
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
BLOCK, CODE, DIST, SHORT, LONG, ADLER, SPAN = 1, 2, 4, 8, 16, 32, 64
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0] + [(k - 2) // 2 for k in range(2, 30)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}


# ---- the container
def chunk(tag: bytes, body: bytes, crc=None) -> bytes:
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) if crc is None else crc)


def ihdr(w, h, depth=8, color=2, interlace=0, compression=0, filt=0) -> bytes:
    return struct.pack(">IIBBBBB", w, h, depth, color, compression, filt, interlace)


def png_file(w, h, color, stream: bytes, cuts=None, extra=(), **kw) -> bytes:
    """a file around a zlib stream; ``cuts``: the IDAT payload lengths in order (the rest goes into a last chunk), ``extra``: chunks
    (tag, body) put between IHDR and the first IDAT"""
    out = [SIGNATURE, chunk(b"IHDR", ihdr(w, h, color=color, **kw))]
    out += [chunk(t, b) for t, b in extra]
    at = 0
    for n in cuts or []:
        out.append(chunk(b"IDAT", stream[at:at + n]))
        at += n
    if at < len(stream) or not cuts:
        out.append(chunk(b"IDAT", stream[at:]))
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


def zlib_header_refusal(two: bytes):
    if len(two) < 2:
        return "zlib header"
    if two[0] & 15 != 8:
        return "method 8"
    if two[0] >> 4 > 7:
        return "window"
    if two[1] & 0x20:
        return "preset dictionary"
    if ((two[0] << 8) + two[1]) % 31:
        return "check bits"
    return None


def parse(data: bytes) -> dict:
    """-> width, height, channels, color_type, spans [(file offset, bytes, frame)], idat (the default image's zlib stream), frames (per
    fcTL a dict with its fields and ``data``), plays, announced, default_is_frame; ValueError whose text holds the fragment tt_png_parse's
    text holds"""
    if len(data) < 8 or data[:8] != SIGNATURE:
        raise ValueError("signature")
    pos, first, ended = 8, True, False
    hd = dict(spans=[], frames=[], plays=None, announced=0, default_is_frame=False)
    idat, idat_open, idat_closed = bytearray(), False, False
    while pos < len(data) and not ended:
        if len(data) - pos < 12:
            raise ValueError("ends inside")
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if n > 0x7fffffff or n > len(data) - pos - 12:
            raise ValueError("ends inside")
        body = data[pos + 8:pos + 8 + n]
        if first:
            first = False
            if tag != b"IHDR":
                raise ValueError("IHDR")
            if n != 13:
                raise ValueError("IHDR of")
            if zlib.crc32(tag + body) != struct.unpack(">I", data[pos + 21:pos + 25])[0]:
                raise ValueError("CRC")
            w, h, depth, color, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if w == 0 or h == 0:
                raise ValueError("zero size")
            if color == 3:
                raise ValueError("colour type 3")
            if color not in CHANNELS:
                raise ValueError("colour type")
            if depth != 8:
                raise ValueError("bit depth")
            if comp or filt:
                raise ValueError("method")
            if lace:
                raise ValueError("interlaced")
            hd.update(width=w, height=h, channels=CHANNELS[color], color_type=color, bit_depth=depth)
        elif tag == b"IDAT":
            if idat_closed:
                raise ValueError("apart")
            if not idat_open:
                idat_open = True
                if hd["frames"]:
                    hd["default_is_frame"] = True
            hd["spans"].append((pos + 8, n, 0 if hd["default_is_frame"] else -1))
            idat += body
            if hd["default_is_frame"]:
                hd["frames"][0]["data"] += body
        else:
            idat_closed = idat_closed or idat_open
            if tag == b"IEND":
                ended = True
            elif tag == b"acTL":
                if n != 8:
                    raise ValueError("acTL")
                hd["announced"], hd["plays"] = struct.unpack(">II", body)
            elif tag == b"fcTL":
                if n != 26:
                    raise ValueError("fcTL")
                if not idat_open and hd["frames"]:
                    raise ValueError("two fcTL")
                if hd["frames"] and not (len(hd["frames"]) == 1 and hd["default_is_frame"]):
                    why = zlib_header_refusal(bytes(hd["frames"][-1]["data"][:2]))
                    if why:
                        raise ValueError(why)
                seq, fw, fh, x, y, dn, dd, dispose, blend = struct.unpack(">IIIIIHHBB", body)
                hd["frames"].append(dict(sequence=seq, width=fw, height=fh, x=x, y=y, delay_num=dn, delay_den=dd, dispose=dispose, blend=blend, data=bytearray()))
            elif tag == b"fdAT":
                if not hd["frames"] or not idat_open:
                    raise ValueError("fdAT")
                if n < 4:
                    raise ValueError("fdAT")
                hd["spans"].append((pos + 12, n - 4, len(hd["frames"]) - 1))
                hd["frames"][-1]["data"] += body[4:]
            elif not tag[0] & 0x20 and tag != b"PLTE":
                raise ValueError("unknown critical chunk")
        pos += 12 + n
    if not ended:
        raise ValueError("ends inside")
    if not idat_open:
        raise ValueError("no IDAT")
    why = zlib_header_refusal(bytes(idat[:2]))
    if why:
        raise ValueError(why)
    if hd["frames"] and not (len(hd["frames"]) == 1 and hd["default_is_frame"]):
        why = zlib_header_refusal(bytes(hd["frames"][-1]["data"][:2]))
        if why:
            raise ValueError(why)
    hd["idat"] = bytes(idat)
    return hd


# ---- canonical codes
def canonical(lengths):
    """-> {symbol: (code, length)}, codes as RFC 1951 3.2.2 numbers them (sent from the most significant bit)"""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, n in enumerate(lengths):
        if n:
            out[s] = (nxt[n], n)
            nxt[n] += 1
    return out


def kraft_left(lengths):
    """what is left of the code space in units of 2^-15 (negative: over-subscribed) and the longest length"""
    return (1 << 15) - sum(1 << (15 - n) for n in lengths if n), max([n for n in lengths if n] or [0])


def huffman_lengths(freq: dict) -> dict:
    """plain Huffman code lengths of the used symbols (one used symbol: length 1)"""
    if len(freq) == 1:
        return {s: 1 for s in freq}
    heap = [(f, s, (s,)) for s, f in sorted(freq.items())]
    heapq.heapify(heap)
    depth = {s: 0 for s in freq}
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    return depth


# ---- the writer
class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):                       # from the least significant bit
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, pair):                             # a Huffman code: from its most significant bit
        code, bits = pair
        self.put(int(format(code, f"0{bits}b")[::-1], 2), bits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bits(self):
        return 8 * len(self.out) + self.n


def length_symbol(m):
    s = max(i for i in range(29) if LEN_BASE[i] <= m) if m < 258 else 28
    return 257 + s, LEN_EXTRA[s], m - LEN_BASE[s]


def dist_symbol(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


def token_symbols(tokens):
    """tokens: ints (literals) and (length, distance) pairs -> the literal/length and the distance symbols they use, the end of block included"""
    lit, dist = {256: 1}, {}
    for t in tokens:
        if isinstance(t, tuple):
            lit[length_symbol(t[0])[0]] = lit.get(length_symbol(t[0])[0], 0) + 1
            dist[dist_symbol(t[1])[0]] = dist.get(dist_symbol(t[1])[0], 0) + 1
        else:
            lit[t] = lit.get(t, 0) + 1
    return lit, dist


CL_LENGTHS = [4] * 13 + [5] * 6                    # a complete code over all 19 code-length symbols: 13 / 16 + 6 / 32


def rle_lengths(seq):
    """a sequence of code lengths -> (symbol, extra bits, extra value) with the repeat symbols 16 / 17 / 18, greedily; runs are taken over
    the WHOLE sequence, so one may cross from the literal lengths into the distance lengths"""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                out.append((18, 7, n - 11))
                run -= n
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                out.append((16, 2, n - 3))
                run -= n
        out += [(v, 0, 0)] * run
        i = j
    return out


def run_crosses(lit_len, dist_len) -> bool:
    """a repeat symbol of ``rle_lengths`` covers the last literal/length length and the first distance length"""
    at = 0
    for s, _, extra in rle_lengths(list(lit_len) + list(dist_len)):
        n = 1 if s < 16 else extra + (3 if s < 18 else 11)
        if s >= 16 and at < len(lit_len) < at + n:
            return True
        at += n
    return False


def write_block(w: BitWriter, block: dict, final: bool):
    """block: kind "stored" (data), "fixed" (tokens) or "dynamic" (tokens; optional lit_lengths [hlit], dist_lengths [hdist], rle=False to
    send every length as itself; raw_header: (symbol, extra bits, value) triples sent as they are)"""
    kind = block["kind"]
    w.put(int(final), 1)
    w.put({"stored": 0, "fixed": 1, "dynamic": 2, "reserved": 3}[kind], 2)
    if kind == "reserved":
        return
    if kind == "stored":
        data = bytes(block["data"])
        w.align()
        w.put(len(data), 16)
        w.put(block.get("nlen", len(data) ^ 0xffff), 16)
        w.out += data
        return
    tokens = block["tokens"]
    if kind == "fixed":
        lit_len, dist_len = FIXED_LIT, FIXED_DIST
    else:
        lit_used, dist_used = token_symbols(tokens)
        lit_len = block.get("lit_lengths")
        if lit_len is None:
            depth = huffman_lengths(lit_used)
            lit_len = [depth.get(s, 0) for s in range(max(257, max(lit_used) + 1))]
        dist_len = block.get("dist_lengths")
        if dist_len is None:
            depth = huffman_lengths(dist_used) if dist_used else {0: 1}
            dist_len = [depth.get(s, 0) for s in range(max(depth) + 1)]
        assert max(lit_len) <= 15 and max(dist_len) <= 15 and 257 <= len(lit_len) <= 286 and 1 <= len(dist_len) <= 30
        w.put(len(lit_len) - 257, 5)
        w.put(len(dist_len) - 1, 5)
        w.put(19 - 4, 4)
        for s in CL_ORDER:
            w.put(CL_LENGTHS[s], 3)
        cl = canonical(CL_LENGTHS)
        seq = list(lit_len) + list(dist_len)
        header = block.get("raw_header") or (rle_lengths(seq) if block.get("rle", True) else [(v, 0, 0) for v in seq])
        for s, bits, extra in header:
            w.code(cl[s])
            w.put(extra, bits)
    lit, dist = canonical(lit_len), canonical(dist_len)
    for t in tokens:
        if isinstance(t, tuple):
            s, bits, extra = length_symbol(t[0])
            w.code(lit[s])
            w.put(extra, bits)
            s, bits, extra = dist_symbol(t[1])
            w.code(dist[s])
            w.put(extra, bits)
        elif t == "bad-literal":                      # the fixed code's symbol 286: 8 bits 11000110
            w.code((0b11000110, 8))
        else:
            w.code(lit[t])
    if block.get("eob", True):
        w.code(lit[256])


def expand(tokens, before=b"") -> bytes:
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]] if t[1] <= len(out) else 0)
        else:
            out.append(t)
    return bytes(out[len(before):])


def zlib_stream(blocks, adler=None, cmf=0x78, flg=None, trailer=True) -> bytes:
    """blocks -> a zlib stream; its Adler-32 is taken over what the blocks hold unless ``adler`` is given"""
    w = BitWriter()
    data = bytearray()
    for i, b in enumerate(blocks):
        write_block(w, b, b.get("final", i == len(blocks) - 1))
        if b["kind"] == "stored":
            data += bytes(b["data"])
        elif b["kind"] != "reserved":
            data += expand([t for t in b["tokens"] if t != "bad-literal"], bytes(data))
    w.align()
    if flg is None:
        flg = (31 - (cmf << 8) % 31) % 31
    out = bytes([cmf, flg]) + bytes(w.out)
    if trailer:
        out += struct.pack(">I", zlib.adler32(bytes(data)) if adler is None else adler)
    return out


# ---- the serial inflate: bytes, tokens and the status of rule 3
class Cut(Exception):
    """the data ended"""


class Bad(Exception):
    def __init__(self, bit):
        self.bit = bit


class BitReader:
    def __init__(self, data: bytes, pos=0):
        self.data, self.pos, self.total = data, pos, 8 * len(data)

    def peek(self, n, ahead=0):                       # bits behind the data read as zero
        at = self.pos + ahead
        return (int.from_bytes(self.data[at >> 3:(at >> 3) + 4], "little") >> (at & 7)) & ((1 << n) - 1)

    def get(self, n):
        if self.pos + n > self.total:
            raise Cut()
        v = self.peek(n)
        self.pos += n
        return v


def decode_symbol(r: BitReader, table: dict, header: bool):
    """table: {(code, length): symbol}.  Bits that are no code: CODE when the 15 bits lie inside the data, else the data ended"""
    code, bits = 0, r.peek(15)
    for n in range(1, 16):
        code = (code << 1) | ((bits >> (n - 1)) & 1)
        if (code, n) in table:
            if r.pos + n > r.total:
                raise Cut()
            r.pos += n
            return table[(code, n)]
    if r.pos + 15 > r.total:
        raise Cut()
    raise Bad(CODE)


def decoder(lengths):
    return {pair: s for s, pair in canonical(lengths).items()}


def check_set(lengths, strict: bool):
    left, longest = kraft_left(lengths)
    if left < 0 or (left > 0 and (strict or longest > 1)):
        raise Bad(CODE)


def read_codes(r: BitReader):
    nlit, ndist, ncl = r.get(5) + 257, r.get(5) + 1, r.get(4) + 4
    if nlit > 286 or ndist > 30:
        raise Bad(CODE)
    cl = [0] * 19
    for i in range(ncl):
        cl[CL_ORDER[i]] = r.get(3)
    check_set(cl, True)
    table, lens = decoder(cl), []
    while len(lens) < nlit + ndist:
        s = decode_symbol(r, table, True)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Bad(CODE)
            val, rep = lens[-1], 3 + r.get(2)
        elif s == 17:
            val, rep = 0, 3 + r.get(3)
        else:
            val, rep = 0, 11 + r.get(7)
        if len(lens) + rep > nlit + ndist:
            raise Bad(CODE)
        lens += [val] * rep
    if lens[256] == 0:
        raise Bad(CODE)
    check_set(lens[:nlit], False)
    check_set(lens[nlit:], False)
    return lens[:nlit], lens[nlit:]


def inflate(stream: bytes, expected=None) -> dict:
    """-> out (``expected`` bytes; all of them when it is None), tokens (per block a dict: kind, tokens -- ints and (length, distance)
    pairs; a stored block's data as ``data``), status (rule 3), produced"""
    out, blocks, status, clean = bytearray(), [], 0, False
    r = BitReader(stream, 16)
    try:
        why = zlib_header_refusal(stream[:2])
        if why == "zlib header":
            raise Cut()
        if why:
            raise Bad(BLOCK)
        while True:
            final, kind = r.get(1), r.get(2)
            if kind == 3:
                raise Bad(BLOCK)
            if kind == 0:
                r.pos = (r.pos + 7) & ~7
                n, c = r.get(16), r.get(16)
                if n ^ c != 0xffff:
                    raise Bad(BLOCK)
                at = r.pos >> 3
                data = stream[at:at + n]
                out += data
                blocks.append(dict(kind="stored", data=bytes(data), tokens=[]))
                r.pos += 8 * len(data)
                if len(data) < n:
                    raise Cut()
            else:
                lit_len, dist_len = (FIXED_LIT, FIXED_DIST) if kind == 1 else read_codes(r)
                lit, dist = decoder(lit_len), decoder(dist_len)
                blk = dict(kind="fixed" if kind == 1 else "dynamic", tokens=[], lit_lengths=list(lit_len), dist_lengths=list(dist_len))
                blocks.append(blk)
                while True:
                    s = decode_symbol(r, lit, False)
                    if s > 285:                                     # its bits lie inside the data: decode_symbol saw to that
                        raise Bad(CODE)
                    if s < 256:
                        out.append(s)
                        blk["tokens"].append(s)
                        continue
                    if s == 256:
                        break
                    m = LEN_BASE[s - 257] + r.peek(LEN_EXTRA[s - 257])
                    r.pos += LEN_EXTRA[s - 257]                     # whether the token ends inside the data is asked once, at its end
                    ds = decode_symbol(r, dist, False)
                    if ds > 29:
                        raise Bad(CODE)
                    d = DIST_BASE[ds] + r.peek(DIST_EXTRA[ds])
                    r.pos += DIST_EXTRA[ds]
                    if r.pos > r.total:
                        raise Cut()
                    if d > len(out):
                        status |= DIST
                    for _ in range(m):
                        out.append(out[-d] if d <= len(out) else 0)
                    blk["tokens"].append((m, d))
            if final:
                clean = True
                break
    except Cut:
        pass
    except Bad as e:
        status |= e.bit
    produced = len(out)
    if expected is None:
        expected = produced
    if produced < expected:
        status |= SHORT
    if produced > expected:
        status |= LONG
    if clean and produced == expected:
        at = (r.pos + 7) >> 3
        if at + 4 > len(stream) or struct.unpack(">I", stream[at:at + 4])[0] != zlib.adler32(bytes(out)):
            status |= ADLER
    out = bytes(out[:expected]) + bytes(max(expected - produced, 0))
    return dict(out=out, blocks=blocks, status=status, produced=produced)


def all_tokens(blocks):
    return [t for b in blocks for t in b["tokens"]]


def distances(blocks):
    return [t[1] for t in all_tokens(blocks) if isinstance(t, tuple)]


# ---- pointer doubling: the parallel formulation of the copies
def source_words(blocks, expected=None) -> np.ndarray:
    """per output byte a literal (-1 - byte) or the index of the byte it copies"""
    src = []
    for b in blocks:
        src += [-1 - v for v in b.get("data", b"")]
        for t in b["tokens"]:
            if isinstance(t, tuple):
                for _ in range(t[0]):
                    src.append(len(src) - t[1] if t[1] <= len(src) else -1)
            else:
                src.append(-1 - t)
    src = np.array(src[:expected] if expected is not None else src, dtype=np.int64)
    return src


def resolve_by_doubling(src: np.ndarray):
    """src <- src[src] for ceil(log2 n) rounds -> (the bytes, the rounds): a constant stream takes the same rounds as noise"""
    src = src.copy()
    rounds = max(int(np.ceil(np.log2(max(src.size, 2)))), 1)
    for _ in range(rounds):
        at = np.nonzero(src >= 0)[0]
        src[at] = src[src[at]]
    assert (src < 0).all()
    return (-1 - src).astype(np.uint8), rounds


# ---- the row filters
def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(stream: bytes, h, w, ch):
    """the serial unfilter -> (uint8 [h, w, ch], bit 0 set for a filter type above 4, read as type 0)"""
    rb, out, status, above = 1 + w * ch, [], 0, [0] * (w * ch)
    for y in range(h):
        kind = stream[y * rb]
        if kind > 4:
            status, kind = 1, 0
        row, cur = stream[y * rb + 1:(y + 1) * rb], [0] * (w * ch)
        for i in range(w * ch):
            a = cur[i - ch] if i >= ch else 0
            b = above[i]
            c = above[i - ch] if i >= ch else 0
            pred = 0 if kind == 0 else (a if kind == 1 else (b if kind == 2 else ((a + b) >> 1 if kind == 3 else paeth(a, b, c))))
            cur[i] = (row[i] + pred) & 255
        out.append(cur)
        above = cur
    return np.array(out, dtype=np.uint8).reshape(h, w, ch), status


def unfilter_wavefront(stream: bytes, h, w, ch):
    """the same along anti-diagonals: step t makes the pixels x = t - y of every row at once"""
    rb = 1 + w * ch
    raw = np.frombuffer(bytes(stream[:h * rb]), dtype=np.uint8).reshape(h, rb)
    kind = raw[:, 0].astype(np.int64)
    kind = np.where(kind > 4, 0, kind)[:, None]
    data = raw[:, 1:].reshape(h, w, ch).astype(np.int64)
    out = np.zeros((h + 1, w + 1, ch), dtype=np.int64)                   # a zero row above and a zero column to the left
    for t in range(w + h - 1):
        y = np.arange(max(0, t - w + 1), min(h, t + 1))
        x = t - y
        a, b, c = out[y + 1, x], out[y, x + 1], out[y, x]
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        pth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        k = kind[y]
        pred = np.select([k == 0, k == 1, k == 2, k == 3], [0 * a, a, b, (a + b) >> 1], pth)
        out[y + 1, x + 1] = (data[y, x] + pred) & 255
    return out[1:, 1:].astype(np.uint8)


def filter_rows(pixels: np.ndarray, kinds) -> bytes:
    """uint8 [h, w, ch] -> the filtered stream with row y filtered by kinds[y] (the inverse of ``unfilter``)"""
    h, w, ch = pixels.shape
    px = pixels.reshape(h, w * ch).astype(np.int64)
    out = bytearray()
    for y in range(h):
        out.append(kinds[y])
        for i in range(w * ch):
            a = px[y, i - ch] if i >= ch else 0
            b = px[y - 1, i] if y else 0
            c = px[y - 1, i - ch] if y and i >= ch else 0
            pred = (0, a, b, (a + b) >> 1, paeth(a, b, c))[kinds[y]]
            out.append(int(px[y, i] - pred) & 255)
    return bytes(out)


def decode(data: bytes):
    """one file -> (uint8 [h, w, ch], inflate status, unfilter status) of its default image"""
    hd = parse(data)
    h, w, ch = hd["height"], hd["width"], hd["channels"]
    got = inflate(hd["idat"], h * (1 + w * ch))
    px, bad = unfilter(got["out"], h, w, ch)
    return px, got["status"], bad


def pillow_pixels(data: bytes) -> np.ndarray:
    from PIL import Image
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


# ---- the streams and files the CPU and the GPU tests share
def noise(n, seed, levels=256):
    return np.random.default_rng(seed).integers(0, levels, size=n, dtype=np.uint8).tobytes()


def text(n, seed):
    """bytes with matches at many distances: words drawn from a small vocabulary"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, size=int(k), dtype=np.uint8)) for k in rng.integers(2, 9, size=40)]
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, 40))] + b" "
    return bytes(out[:n])


def compress(data, level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if not flush_every:
        return c.compress(data) + c.flush()
    out = b""
    for at in range(0, len(data), flush_every):
        out += c.compress(data[at:at + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def kinds_of(blocks):
    return {b["kind"] for b in blocks}


def encoder_cases():
    """-> [(name, stream, property)]: zlib's outputs on arbitrary bytes; ``property(blocks)`` is what the case relies on"""
    mixed = text(30000, 1) + noise(9000, 2) + bytes(7000) + text(20000, 3)
    far = noise(20000, 9) + text(3000, 4) + noise(20000, 9)[:6000]
    return [
        ("level 0: stored only", compress(mixed, 0), lambda b: kinds_of(b) == {"stored"} and len(b) >= 2),
        ("Z_FIXED", compress(mixed[:20000], 6, strategy=zlib.Z_FIXED), lambda b: kinds_of(b) == {"fixed"} and len(distances(b)) > 100),
        ("Z_HUFFMAN_ONLY", compress(mixed[:40000], 6, strategy=zlib.Z_HUFFMAN_ONLY), lambda b: "dynamic" in kinds_of(b) and not distances(b)),
        ("Z_RLE", compress(mixed, 6, strategy=zlib.Z_RLE), lambda b: set(distances(b)) == {1}),
        ("level 1", compress(mixed, 1), lambda b: "dynamic" in kinds_of(b) and len(distances(b)) > 1000),
        ("level 9", compress(far, 9), lambda b: max(distances(b)) > 16384),
        ("wbits 9", compress(mixed, 6, wbits=9), lambda b: max(distances(b)) <= 512 - 262 + 6 and len(distances(b)) > 1000),
        ("full flush every 5 bytes", compress(text(700, 5), 6, flush_every=5), lambda b: sum(1 for x in b if x["kind"] == "stored" and not x["data"]) > 100),
        ("noise then text: several blocks", compress(noise(70000, 7, 64) + text(70000, 8), 6), lambda b: len(b) >= 2),
    ]


def handbuilt_cases():
    """-> [(name, stream, property)]: streams no encoder produces"""
    rng = np.random.default_rng(11)
    lits = lambda n, lo=0, hi=256: [int(v) for v in rng.integers(lo, hi, size=n)]
    head = lits(32768)
    fifteen = [0] * 257                                # the literals 0 .. 14 and the end of block with the lengths 1 .. 15, 15
    for s in range(15):
        fifteen[s] = s + 1
    fifteen[256] = 15
    # 190 literals of 8 bits, 190 .. 192 and the end of block of 9, the length symbols 278 .. 285 of 5 bits, then 28 distance symbols of 5 bits and
    # two of 4: both sets complete, and the run of 5s runs from the literal/length lengths on into the distance lengths
    lit_c = [8] * 190 + [9] * 3 + [0] * 63 + [9] + [0] * 21 + [5] * 8
    dist_c = [5] * 28 + [4] * 2
    assert kraft_left(lit_c)[0] == 0 and kraft_left(dist_c)[0] == 0 and len(lit_c) == 286
    crossing = dict(kind="dynamic", tokens=lits(300, 0, 193) + [(131, 1), (258, 7), (115, 300)], lit_lengths=lit_c, dist_lengths=dist_c)
    cases = [
        ("length 258 at distance 1", zlib_stream([dict(kind="fixed", tokens=[65, (258, 1), 66, (258, 1)])]), lambda b: (258, 1) in all_tokens(b)),
        ("distance 32768", zlib_stream([dict(kind="dynamic", tokens=head + [(200, 32768), 7, (258, 32768)])]), lambda b: max(distances(b)) == 32768),
        ("a source in an earlier block, and a match across 32 KiB of output",
         zlib_stream([dict(kind="stored", data=bytes(head[:32700])), dict(kind="fixed", tokens=[(150, 32000), 1, 2]), dict(kind="dynamic", tokens=lits(50) + [(258, 120)])]),
         lambda b: [x["kind"] for x in b] == ["stored", "fixed", "dynamic"] and b[1]["tokens"][0] == (150, 32000)),
        ("stored blocks of 65535 and of 0 bytes", zlib_stream([dict(kind="stored", data=noise(65535, 12)), dict(kind="stored", data=b""), dict(kind="fixed", tokens=[9, (10, 1)]),
                                                               dict(kind="stored", data=b"")]), lambda b: len(b[0]["data"]) == 65535 and b[1]["data"] == b"" and b[3]["data"] == b""),
        ("15-bit codes", zlib_stream([dict(kind="dynamic", tokens=lits(400, 0, 15) + [14] * 5, lit_lengths=fifteen, dist_lengths=[1])]),
         lambda b: max(b[0]["lit_lengths"]) == 15 and 14 in b[0]["tokens"]),
        ("a single distance code", zlib_stream([dict(kind="dynamic", tokens=lits(20) + [(30, 1), 5, (9, 1)], dist_lengths=[1])]),
         lambda b: b[0]["dist_lengths"] == [1] and set(distances(b)) == {1}),
        ("HLIT = 257", zlib_stream([dict(kind="dynamic", tokens=lits(500, 0, 40))]), lambda b: len(b[0]["lit_lengths"]) == 257),
        ("a code-length run from the literal into the distance lengths", zlib_stream([crossing]),
         lambda b: run_crosses(b[0]["lit_lengths"], b[0]["dist_lengths"])),
        ("one byte", zlib_stream([dict(kind="fixed", tokens=[200])]), lambda b: all_tokens(b) == [200]),
        ("ends in a partial byte", zlib_stream([dict(kind="fixed", tokens=[1, 2, 3])]), lambda b: (3 + 3 * 8 + 7) % 8 != 0),
    ]
    return cases


def corrupt_cases():
    """-> [(name, stream, expected bytes, status)]: a stream built for every status bit of rule 3 (SPAN needs bad arrays, not bad data)"""
    good = compress(text(5000, 21), 6)
    flipped = bytearray(good)
    flipped[-1] ^= 1
    long_dist = zlib_stream([dict(kind="fixed", tokens=[1, 2, 3, (5, 4), 9])])
    over = [8] * 257                                   # 257 codes of 8 bits: over-subscribed
    incomplete = [9] * 257
    return [
        ("a reserved block type", zlib_stream([dict(kind="fixed", tokens=[1, 2]), dict(kind="reserved")]) , 10, BLOCK | SHORT),
        ("LEN / NLEN mismatch", zlib_stream([dict(kind="stored", data=b"abcdef", nlen=0x1234)]), 6, BLOCK | SHORT),
        ("a zlib header with a preset dictionary", bytes([0x78, 0x20 | (31 - (0x7820 % 31))]) + good[2:], 5000, BLOCK | SHORT),
        ("over-subscribed code lengths", zlib_stream([dict(kind="dynamic", tokens=[1, 2, 3], lit_lengths=over, dist_lengths=[1])]), 3, CODE | SHORT),
        ("incomplete code lengths", zlib_stream([dict(kind="dynamic", tokens=[1, 2, 3], lit_lengths=incomplete, dist_lengths=[1])]), 3, CODE | SHORT),
        ("a code that is not in the table", zlib_stream([dict(kind="fixed", tokens=[1, 2, "bad-literal", 3])]), 3, CODE | SHORT),
        ("a distance before the first byte", long_dist, 9, DIST),
        ("fewer bytes than expected", good, 5001, SHORT),
        ("cut in the middle", good[:len(good) // 2], 5000, SHORT),
        ("more bytes than expected", good, 4999, LONG),
        ("an Adler byte flipped", bytes(flipped), 5000, ADLER),
        ("the trailer cut", good[:-2], 5000, ADLER),
    ]


def picture(h, w, ch, seed, smooth=True):
    rng = np.random.default_rng(seed)
    if not smooth:
        return rng.integers(0, 256, size=(h, w, ch), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    planes = [(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 127 // max(w + h - 2, 1)), 255 - (xx * yy) % 256]
    out = np.stack(planes[:ch], axis=-1).astype(np.int64) + rng.integers(0, 4, size=(h, w, ch))
    return (out & 255).astype(np.uint8)


def pillow_png(pixels: np.ndarray, **kw) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels[..., 0] if pixels.shape[-1] == 1 else pixels).save(buf, format="PNG", **kw)
    return buf.getvalue()


def rechunk(data: bytes, size=1, empties=True) -> bytes:
    """the same file with its IDAT stream cut into ``size``-byte chunks, an empty chunk between every two"""
    hd = parse(data)
    cuts = []
    for _ in range(0, len(hd["idat"]), size):
        cuts += [size, 0] if empties else [size]
    return png_file(hd["width"], hd["height"], hd["color_type"], hd["idat"], cuts=[0] + cuts)


def file_cases():
    """-> [(name, bytes)]: files Pillow reads, of every mode, compression level 0 and default, several blocks, several IDAT chunks,
    1-byte IDAT chunks with empty ones between, ancillary chunks (tRNS included)"""
    out = []
    for ch, mode in ((1, "L"), (2, "LA"), (3, "RGB"), (4, "RGBA")):
        px = picture(23, 31, ch, ch)
        out.append((f"pillow {mode}", pillow_png(px)))
        out.append((f"pillow {mode} level 0", pillow_png(px, compress_level=0)))
    out.append(("256 x 384 RGB: several blocks", pillow_png(picture(256, 384, 3, 5))))
    out.append(("several IDAT chunks", pillow_png(picture(120, 200, 3, 6, smooth=False))))
    out.append(("1-byte IDAT chunks", rechunk(pillow_png(picture(9, 14, 3, 7)))))
    small = parse(pillow_png(picture(6, 5, 3, 8)))
    out.append(("ancillary chunks", png_file(5, 6, 2, small["idat"], extra=[(b"gAMA", struct.pack(">I", 45455)), (b"tRNS", bytes(6)), (b"tEXt", b"k\0v")])))
    grey = parse(pillow_png(picture(6, 5, 1, 9)))
    out.append(("grey with tRNS", png_file(5, 6, 0, grey["idat"], extra=[(b"tRNS", b"\0\7")])))
    return out



def refusal_files():
    """-> [(name, bytes, fragment of the text)]: what the parser refuses by name"""
    px = picture(4, 5, 3, 3)
    good = pillow_png(px)
    hd = parse(good)
    stream = hd["idat"]
    body = ihdr(5, 4)
    bad_crc = SIGNATURE + chunk(b"IHDR", body, crc=1) + chunk(b"IDAT", stream) + chunk(b"IEND", b"")
    no_ihdr = SIGNATURE + chunk(b"IDAT", stream) + chunk(b"IEND", b"")
    no_idat = SIGNATURE + chunk(b"IHDR", body) + chunk(b"IEND", b"")
    header = lambda cmf, flg: bytes([cmf, flg]) + stream[2:]
    out = [
        ("a bad signature", b"\x89PNX" + good[4:], "signature"),
        ("ends inside a chunk", good[:40], "ends inside"),
        ("ends before IEND", good[:-12], "ends inside"),
        ("a missing IHDR", no_ihdr, "IHDR"),
        ("a missing IDAT", no_idat, "no IDAT"),
        ("zero size", png_file(0, 4, 2, stream), "zero size"),
        ("a palette file", png_file(5, 4, 3, stream), "colour type 3"),
        ("interlaced", png_file(5, 4, 2, stream, interlace=1), "interlaced"),
        ("an unknown critical chunk", png_file(5, 4, 2, stream, extra=[(b"ABCD", b"xy")]), "unknown critical chunk"),
        ("a bad CRC on IHDR", bad_crc, "CRC"),
        ("zlib: not method 8", png_file(5, 4, 2, header(0x77, (31 - 0x7700 % 31) % 31)), "method 8"),
        ("zlib: a preset dictionary", png_file(5, 4, 2, header(0x78, 0x20 | (31 - 0x7820 % 31))), "preset dictionary"),
        ("zlib: the check bits", png_file(5, 4, 2, header(0x78, 0x02)), "check bits"),
    ]
    for depth in (1, 2, 4, 16):
        out.append((f"bit depth {depth}", png_file(5, 4, 0 if depth < 16 else 2, stream, depth=depth), "bit depth"))
    return out
