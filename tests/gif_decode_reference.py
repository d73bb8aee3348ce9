"""The GIF import of include/ttvdm.h ("GIF import", rules 1 - 5) restated in numpy / plain Python, and a small writer for handcrafted
files.  The reader: the container walked block by block, the textbook LZW decoder with a table of strings, the interlace rows, the
composition rule.  The writer: any rectangle, colour table, transparent index, disposal, interlace flag, minimum code size and sub-block
length; a greedy LZW coder with and without a deferred clear; ``pack`` for streams given code by code.  Nothing here calls the library."""
import io
import struct

import numpy as np

STATUS_CODE, STATUS_SHORT, STATUS_SPAN = 1, 2, 4
MAX_CODES = 4096


# ---- the reader
def parse(data: bytes) -> dict:
    """rule 1 -> {width, height, background, loop (None without NETSCAPE2.0), global_colors, frames: [{left, top, w, h, interlace,
    transparent (-1: none), disposal, delay, min_code_size, local, palette uint8 [256, 3], data}]}; ValueError for what the rule refuses"""
    if data[:6] not in (b"GIF87a", b"GIF89a"):
        raise ValueError("bad signature")
    width, height, packed, background, _ = struct.unpack("<HHBBB", data[6:13])
    at = 13
    table = np.zeros((256, 3), dtype=np.uint8)
    ncolors = 0
    if packed & 0x80:
        ncolors = 2 << (packed & 7)
        table[:ncolors] = np.frombuffer(data[at:at + 3 * ncolors], dtype=np.uint8).reshape(ncolors, 3)
        at += 3 * ncolors
    out = dict(width=width, height=height, background=background, loop=None, global_colors=ncolors, frames=[])
    gce = (-1, 0, 0)

    def blocks(at):
        payload = b""
        while True:
            n = data[at]
            at += 1
            if n == 0:
                return payload, at
            if at + n > len(data):
                raise ValueError("ends inside a sub-block")
            payload += data[at:at + n]
            at += n

    while at < len(data):
        kind = data[at]
        at += 1
        if kind == 0x3b:
            break
        if kind == 0x21:
            label = data[at]
            at += 1
            if label == 0xf9 and data[at] == 4:
                gp, delay, tr = struct.unpack("<BHB", data[at + 1:at + 5])
                gce = (tr if gp & 1 else -1, (gp >> 2) & 7, delay)
            elif label == 0xff and data[at:at + 12] == b"\x0bNETSCAPE2.0" and data[at + 12:at + 14] == b"\x03\x01":
                out["loop"] = struct.unpack("<H", data[at + 14:at + 16])[0]
            _, at = blocks(at)
            continue
        if kind != 0x2c:
            if out["frames"]:
                break
            raise ValueError("unknown block")
        left, top, w, h, ip = struct.unpack("<HHHHB", data[at:at + 9])
        at += 9
        fr = dict(left=left, top=top, w=w, h=h, interlace=bool(ip & 0x40), transparent=gce[0], disposal=gce[1], delay=gce[2], local=bool(ip & 0x80))
        gce = (-1, 0, 0)
        if w == 0 or h == 0 or left + w > width or top + h > height:
            raise ValueError("a rectangle of zero size or one that leaves the logical screen")
        pal = table
        if ip & 0x80:
            n = 2 << (ip & 7)
            pal = np.zeros((256, 3), dtype=np.uint8)
            pal[:n] = np.frombuffer(data[at:at + 3 * n], dtype=np.uint8).reshape(n, 3)
            at += 3 * n
        elif not ncolors:
            raise ValueError("no colour table")
        fr["palette"] = pal.copy()
        fr["min_code_size"] = data[at]
        if not 2 <= data[at] <= 8:
            raise ValueError("minimum code size")
        fr["data"], at = blocks(at + 1)
        out["frames"].append(fr)
    if not out["frames"]:
        raise ValueError("no image")
    return out


def read_codes(data: bytes, mcs: int):
    """rule 2a: the stream's codes with their places, [(code, place r, bit position)], up to the end code or the end of the data"""
    clear, nbits, pos, r, out = 1 << mcs, 8 * len(data), 0, 0, []
    value = int.from_bytes(data, "little")
    while True:
        w = min(12, (clear + 1 + r).bit_length())
        if pos + w > nbits:
            return out
        code = (value >> pos) & ((1 << w) - 1)
        out.append((code, r, pos))
        pos += w
        if code == clear + 1:
            return out
        r = 0 if code == clear else r + 1


def lzw_decode(data: bytes, mcs: int, npix: int):
    """rules 2 and 3: the textbook decoder with a table of strings -> (indices uint8 [npix], status)"""
    clear, e0 = 1 << mcs, (1 << mcs) + 2
    out, status, entries, prev = [], 0, {}, None
    for code, r, _ in read_codes(data, mcs):
        if code == clear:
            entries, prev = {}, None
            continue
        if code == clear + 1:
            break
        if code < clear:
            s = [code]
        elif code >= e0 and r >= 1 and code - e0 <= min(r - 1, MAX_CODES - 1 - e0):
            s = prev + [prev[0]] if code - e0 == r - 1 else entries[code - e0]
        else:
            s = [0]                                                # an invalid code is read as the pixel 0
            if len(out) < npix:
                status |= STATUS_CODE
        if prev is not None and e0 + r - 1 < MAX_CODES:
            entries[r - 1] = prev + [s[0]]
        out.extend(s)
        prev = s
    if len(out) < npix:
        status |= STATUS_SHORT
    px = np.zeros(npix, dtype=np.uint8)
    px[:min(npix, len(out))] = out[:npix]
    return px, status


def interlace_rows(h: int) -> list:
    """rule 4: the real row of every row in the order an interlaced image sends them"""
    return list(range(0, h, 8)) + list(range(4, h, 8)) + list(range(2, h, 4)) + list(range(1, h, 2))


def index_map(fr: dict):
    """one frame's indices [h, w] in raster order and its status"""
    px, status = lzw_decode(fr["data"], fr["min_code_size"], fr["w"] * fr["h"])
    px = px.reshape(fr["h"], fr["w"])
    if fr["interlace"]:
        real = np.empty_like(px)
        real[interlace_rows(fr["h"])] = px
        px = real
    return px, status


def compose(hd: dict, maps: list) -> np.ndarray:
    """rule 5 -> uint8 [F, H, W, 3]"""
    frames = hd["frames"]
    f0 = frames[0]
    canvas = np.empty((hd["height"], hd["width"], 3), dtype=np.uint8)
    canvas[:] = f0["palette"][f0["transparent"] if f0["transparent"] >= 0 else 0]
    out, before = [], None
    for f, fr in enumerate(frames):
        if f:
            p = frames[f - 1]
            box = (slice(p["top"], p["top"] + p["h"]), slice(p["left"], p["left"] + p["w"]))
            if p["disposal"] == 2:
                canvas[box] = p["palette"][p["transparent"] if p["transparent"] >= 0 else hd["background"]]
            elif p["disposal"] == 3:
                canvas[box] = before[box]
        before = canvas.copy()
        box = (slice(fr["top"], fr["top"] + fr["h"]), slice(fr["left"], fr["left"] + fr["w"]))
        drawn = maps[f] != fr["transparent"]
        canvas[box][drawn] = fr["palette"][maps[f]][drawn]
        out.append(canvas.copy())
    return np.stack(out)


def decode(data: bytes):
    """a whole file -> (frames uint8 [F, H, W, 3], [status per frame])"""
    hd = parse(data)
    maps = [index_map(fr) for fr in hd["frames"]]
    return compose(hd, [m for m, _ in maps]), [s for _, s in maps]


def outside_pillows_envelope(hd: dict) -> bool:
    """the two patterns in which Pillow departs from GIF89a (include/ttvdm.h, rule 5 (a) and (b)), decided on the parsed header"""
    frames = hd["frames"]
    if frames[0]["disposal"] == 3 and frames[0]["transparent"] < 0:
        return True
    last = 0
    for fr in frames:
        if fr["disposal"] == 0 and last in (2, 3):
            return True
        if fr["disposal"]:
            last = fr["disposal"]
    return False


def pillow_frames(data: bytes) -> np.ndarray:
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    out = []
    for i in range(getattr(im, "n_frames", 1)):
        im.seek(i)
        out.append(np.asarray(im.convert("RGB")).copy())
    return np.stack(out)


# ---- the writer
def pack(codes, mcs: int) -> bytes:
    """codes (clear and end codes included) -> bytes, every code at the width of its place behind the last clear code (rule 2a)"""
    clear, value, pos, r = 1 << mcs, 0, 0, 0
    for code in codes:
        w = min(12, (clear + 1 + r).bit_length())
        value |= (int(code) & ((1 << w) - 1)) << pos
        pos += w
        r = 0 if code == clear else r + 1
    return value.to_bytes((pos + 7) // 8, "little")


def lzw_codes(px, mcs: int, deferred: bool = False, clear_first: bool = True) -> list:
    """the greedy coder: a clear code at every full table, or (deferred) none -- the table stays full and the codes 12 bits wide"""
    clear, e0 = 1 << mcs, (1 << mcs) + 2
    px = [int(v) for v in np.asarray(px).reshape(-1)]
    codes = [clear] if clear_first else []
    table, nxt, prefix = {}, e0, px[0]
    for c in px[1:]:
        key = (prefix, c)
        if key in table:
            prefix = table[key]
            continue
        codes.append(prefix)
        if nxt < MAX_CODES:
            table[key] = nxt
            nxt += 1
        elif not deferred:
            codes.append(clear)
            table, nxt = {}, e0
        prefix = c
    return codes + [prefix, clear + 1]


def lzw_stream(px, mcs: int, **kw) -> bytes:
    return pack(lzw_codes(px, mcs, **kw), mcs)


def sub_blocks(data: bytes, size: int = 255) -> bytes:
    out = b""
    for at in range(0, len(data), size):
        out += bytes([len(data[at:at + size])]) + data[at:at + size]
    return out + b"\x00"


def color_table(colors) -> tuple:
    """-> (the size field, the table's bytes padded to a power of two)"""
    colors = np.asarray(colors, dtype=np.uint8).reshape(-1, 3)
    bits = max(1, int(len(colors) - 1).bit_length())
    return bits - 1, colors.tobytes() + bytes(3 * ((1 << bits) - len(colors)))


def gif_file(width: int, height: int, frames: list, global_table=None, background: int = 0, loop=0, sub_block: int = 255, trailer: bool = True,
             version: bytes = b"GIF89a") -> bytes:
    """frames: dicts with ``indices`` [h, w] (raster order) and optionally left, top, table (a local colour table), transparent, disposal,
    delay, interlace, min_code_size, deferred, stream (the LZW bytes as they are, for corrupt data), gce (False: no graphic control)"""
    out = [version]
    if global_table is not None:
        field, table = color_table(global_table)
        out += [struct.pack("<HHBBB", width, height, 0x80 | 0x70 | field, background, 0), table]
    else:
        out.append(struct.pack("<HHBBB", width, height, 0x70, background, 0))
    if loop is not None:
        out.append(b"\x21\xff\x0bNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00")
    for fr in frames:
        idx = np.asarray(fr["indices"], dtype=np.uint8)
        h, w = idx.shape
        tr = fr.get("transparent", -1)
        if fr.get("gce", True):
            out.append(b"\x21\xf9\x04" + struct.pack("<BHB", (fr.get("disposal", 0) << 2) | (tr >= 0), fr.get("delay", 5), max(tr, 0)) + b"\x00")
        flags = 0x40 if fr.get("interlace") else 0
        table = b""
        ncolors = len(global_table) if global_table is not None else 0
        if fr.get("table") is not None:
            field, table = color_table(fr["table"])
            flags |= 0x80 | field
            ncolors = len(fr["table"])
        out += [b"\x2c" + struct.pack("<HHHHB", fr.get("left", 0), fr.get("top", 0), w, h, flags), table]
        mcs = fr.get("min_code_size", max(2, int(ncolors - 1).bit_length()))
        sent = idx[interlace_rows(h)] if fr.get("interlace") else idx
        stream = fr["stream"] if "stream" in fr else lzw_stream(sent, mcs, deferred=fr.get("deferred", False))
        out += [bytes([mcs]), sub_blocks(stream, fr.get("sub_block", sub_block))]
    return b"".join(out) + (b"\x3b" if trailer else b"")


# ---- the handcrafted composition files: a 37 x 29 screen, four frames with random rectangles, global-only and alternating local tables,
# nine disposal patterns x four transparency patterns
SCREEN = (37, 29)                                  # width, height
DISPOSALS = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (1, 2, 1, 2), (1, 3, 1, 3), (2, 3, 2, 1), (1, 1, 3, 3), (0, 1, 2, 3), (3, 1, 2, 1)]
TRANSPARENCY = {"none": (-1, -1, -1, -1), "all": (2, 2, 2, 2), "later": (-1, 3, 3, 3), "odd": (-1, 1, -1, 5)}
TABLES = ("global", "alternating")


def handcrafted(tables: str, disposal, transparency, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    width, height = SCREEN
    table = rng.integers(0, 256, size=(8, 3)).astype(np.uint8)
    frames = []
    for f in range(4):
        w, h = int(rng.integers(1, width + 1)), int(rng.integers(1, height + 1))
        left, top = int(rng.integers(0, width - w + 1)), int(rng.integers(0, height - h + 1))
        local = rng.integers(0, 256, size=(16, 3)).astype(np.uint8) if tables == "alternating" and f % 2 else None
        frames.append(dict(indices=rng.integers(0, 16 if local is not None else 8, size=(h, w)), left=left, top=top, table=local,
                           transparent=transparency[f], disposal=disposal[f], delay=3 + f))
    return gif_file(width, height, frames, global_table=table, background=1)


def handcrafted_files() -> list:
    """-> [(name, bytes)]: 72 files"""
    out = []
    for ti, tables in enumerate(TABLES):
        for di, disposal in enumerate(DISPOSALS):
            for ki, (key, transparency) in enumerate(TRANSPARENCY.items()):
                out.append((f"{tables}-{''.join(map(str, disposal))}-{key}", handcrafted(tables, disposal, transparency, 1000 + 100 * ti + 10 * di + ki)))
    return out
