"""Every refusal of the GIF import (include/ttvdm.h, "GIF import"): files tt_gif_parse refuses, each with ONE fault, and for
tt_gif_decode_indices / tt_gif_compose one valid argument set (fake non-null aligned pointers) with ONE fault applied at a time; the
return code and the message (tt_last_error) are recorded.  Every refusal returns before the first HIP call, so this needs no GPU -- and
a fully valid argument set is never passed to the device entry points.  As a second line of defence the rows run in a child process
that sees no GPU (`python -m tests.gif_decode_refusals`), in the manner of tests/gif_lzw_refusals.py.  The GPU test passes the device
rows with real buffers."""
import ctypes as C
import json
import os
import struct
import sys

import numpy as np

from tests import gif_decode_reference as g

P = 0x10000          # a fake operand address; the operands sit 64 KiB apart
EINVAL, EUNSUPPORTED = -1, -2
BIG = 1 << 40

# ---- tt_gif_parse: (name, file, the code, a fragment of the message)
_T = np.arange(12, dtype=np.uint8).reshape(4, 3)
_IDX = np.arange(6).reshape(2, 3) % 4
GOOD = g.gif_file(5, 4, [dict(indices=_IDX, left=1, top=1), dict(indices=_IDX, left=2, top=2, table=_T, transparent=1, disposal=2)], global_table=_T)


def _patched(at: int, fmt: str, *values) -> bytes:
    b = bytearray(GOOD)
    b[at:at + struct.calcsize(fmt)] = struct.pack(fmt, *values)
    return bytes(b)


# where the two image descriptors stand: behind the file's head and behind frame 0, each behind its 8 bytes of graphic control
_F0 = len(g.gif_file(5, 4, [], global_table=_T, trailer=False)) + 8
_F1 = len(g.gif_file(5, 4, [dict(indices=_IDX, left=1, top=1)], global_table=_T, trailer=False)) + 8
assert GOOD[_F0] == 0x2c and GOOD[_F1] == 0x2c
FILES = [
    ("signature", b"GIF88a" + GOOD[6:], EINVAL, "bad signature"),
    ("short signature", GOOD[:4], EINVAL, "ends inside the signature"),
    ("screen", GOOD[:10], EINVAL, "ends inside the logical screen descriptor"),
    ("global table", GOOD[:20], EINVAL, "ends inside the global colour table"),
    ("descriptor", GOOD[:_F0 + 5], EINVAL, "ends inside the image descriptor of frame 0"),
    ("local table", GOOD[:_F1 + 13], EINVAL, "ends inside the local colour table of frame 1"),
    ("sub-block", GOOD[:_F0 + 13], EINVAL, "ends inside a sub-block of frame 0"),
    ("terminator", GOOD[:_F1 - 9], EINVAL, "ends inside the image data of frame 0"),
    ("extension", GOOD[:_F1 - 4], EINVAL, "ends inside an extension"),
    ("no image", GOOD[:_F0 - 8] + b"\x3b", EINVAL, "no image at all"),
    ("zero size", _patched(_F1 + 5, "<H", 0), EINVAL, "frame 1 has a rectangle of zero size"),
    ("leaves the screen", _patched(_F1 + 1, "<H", 3), EINVAL, "frame 1's rectangle (3, 2, 3 x 2) leaves the logical screen of 5 x 4"),
    ("no table", g.gif_file(5, 4, [dict(indices=_IDX, min_code_size=2)]), EINVAL, "frame 0 has no colour table"),
    ("min code size 1", _patched(_F0 + 10, "<B", 1), EINVAL, "frame 0 has a minimum code size of 1"),
    ("min code size 9", _patched(_F0 + 10, "<B", 9), EINVAL, "frame 0 has a minimum code size of 9"),
    ("unknown block", GOOD[:_F0 - 8] + b"\x99" + GOOD[_F0 - 8:], EINVAL, "unknown block 0x99"),
    # 65 536 images of one pixel behind a global table: one more than a call decodes
    ("frames", g.gif_file(1, 1, [], global_table=_T, loop=None, trailer=False) + 65536 * (b"\x2c" + struct.pack("<HHHHB", 0, 0, 1, 1, 0) + b"\x02" +
                                                                                       g.sub_blocks(g.pack([4, 1, 5], 2))) + b"\x3b",
     EUNSUPPORTED, "more than 65535 frames"),
    ("canvas", b"GIF89a" + struct.pack("<HHBBB", 5000, 5000, 0, 0, 0) + b"\x3b", EUNSUPPORTED, "a canvas of 5000 x 5000 pixels"),
]

# ---- tt_gif_decode_indices
DEC = dict(data=P, data_bytes=1000, offsets=2 * P, lengths=3 * P, npix=4 * P, mcs=5 * P, rows=6 * P, map_offsets=7 * P, n=3, maps=8 * P, maps_bytes=4096,
           status=9 * P, ws=10 * P, ws_bytes=BIG)
DEC_ORDER = ("data", "data_bytes", "offsets", "lengths", "npix", "mcs", "rows", "map_offsets", "n", "maps", "maps_bytes", "status", "ws", "ws_bytes")
DEC_ROWS = [
    (dict(data=None), EINVAL, "null data"), (dict(offsets=None), EINVAL, "null offsets"), (dict(lengths=None), EINVAL, "null lengths"),
    (dict(npix=None), EINVAL, "null npix"), (dict(mcs=None), EINVAL, "null min_code_size"), (dict(rows=None), EINVAL, "null rows"),
    (dict(map_offsets=None), EINVAL, "null map_offsets"), (dict(maps=None), EINVAL, "null maps"), (dict(status=None), EINVAL, "null status"),
    (dict(ws=None), EINVAL, "null ws"),
    (dict(n=0), EINVAL, "empty problem"), (dict(n=-2), EINVAL, "empty problem"), (dict(data_bytes=0), EINVAL, "empty problem"),
    (dict(maps_bytes=0), EINVAL, "empty problem"),
    (dict(offsets=2 * P + 4), EINVAL, "offsets is not 8-byte aligned"), (dict(map_offsets=7 * P + 4), EINVAL, "map_offsets is not 8-byte aligned"),
    (dict(lengths=3 * P + 2), EINVAL, "lengths is not 4-byte aligned"), (dict(npix=4 * P + 1), EINVAL, "npix is not 4-byte aligned"),
    (dict(mcs=5 * P + 2), EINVAL, "min_code_size is not 4-byte aligned"), (dict(rows=6 * P + 3), EINVAL, "rows is not 4-byte aligned"),
    (dict(status=9 * P + 2), EINVAL, "status is not 4-byte aligned"), (dict(ws=10 * P + 8), EINVAL, "ws is not 16-byte aligned"),
    (dict(ws_bytes="short"), EINVAL, "ws too small"), (dict(ws_bytes=0), EINVAL, "ws too small"),
    (dict(n=70000), EUNSUPPORTED, "70000 frames"), (dict(data_bytes=1 << 29), EUNSUPPORTED, "fewer than 2^29 = 536870912"),
    (dict(maps_bytes=1 << 31), EUNSUPPORTED, "fewer than 2^31 = 2147483648"),
]

# ---- tt_gif_compose
CMP = dict(maps=P, maps_bytes=4096, table=2 * P, palettes=3 * P, n=3, height=29, width=37, initial=0, out=4 * P)
CMP_ORDER = ("maps", "maps_bytes", "table", "palettes", "n", "height", "width", "initial", "out")
CMP_ROWS = [
    (dict(maps=None), EINVAL, "null maps"), (dict(table=None), EINVAL, "null table"), (dict(palettes=None), EINVAL, "null palettes"),
    (dict(out=None), EINVAL, "null out"), (dict(n=0), EINVAL, "empty problem"), (dict(height=0), EINVAL, "empty problem"),
    (dict(width=-1), EINVAL, "empty problem"), (dict(maps_bytes=0), EINVAL, "empty problem"), (dict(table=2 * P + 4), EINVAL, "table is not 8-byte aligned"),
    (dict(n=65536), EUNSUPPORTED, "65536 frames"), (dict(height=5000, width=5000), EUNSUPPORTED, "a canvas of 5000 x 5000 pixels"),
]


def row_id(fault):
    return ",".join(f"{k}={v}" for k, v in fault.items())


def parse_call(lib, data: bytes):
    from this_and_that_vdm_amd import _lib
    buf = np.frombuffer(data, dtype=np.uint8)
    hd = _lib.TtGifHeader()
    rc = lib.tt_gif_parse(buf.ctypes.data, buf.size, C.byref(hd), None, 0, None, 0)
    return [rc, lib.tt_last_error().decode() if rc else ""]


def dec_call(lib, a, stream=None):
    a = dict(a)
    if a["ws_bytes"] == "short":
        a["ws_bytes"] = lib.tt_gif_decode_ws_bytes(a["n"], a["data_bytes"]) - 1
    return [lib.tt_gif_decode_indices(*[a[k] for k in DEC_ORDER], stream), lib.tt_last_error().decode()]


def cmp_call(lib, a, stream=None):
    return [lib.tt_gif_compose(*[a[k] for k in CMP_ORDER], stream), lib.tt_last_error().decode()]


def take(lib):
    out = {"good": parse_call(lib, GOOD)}
    for name, data, _, _ in FILES:
        out["file:" + name] = parse_call(lib, data)
    for fault, _, _ in DEC_ROWS:
        assert fault, "a row without a fault would be a valid call"
        out["dec:" + row_id(fault)] = dec_call(lib, dict(DEC, **fault))
    for fault, _, _ in CMP_ROWS:
        assert fault, "a row without a fault would be a valid call"
        out["cmp:" + row_id(fault)] = cmp_call(lib, dict(CMP, **fault))
    out["sizes"] = [lib.tt_gif_decode_ws_bytes(3, 1000), lib.tt_gif_decode_ws_bytes(0, 1000), lib.tt_gif_decode_ws_bytes(3, 0), lib.tt_gif_decode_ws_bytes(70000, 1000),
                    lib.tt_gif_decode_ws_bytes(3, 1 << 29)]
    return out


def run_child():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TT_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")           # the child sees no GPU
    r = subprocess.run([sys.executable, "-m", "tests.gif_decode_refusals"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"gif decode refusals failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    print(json.dumps(take(_lib.load()), separators=(",", ":")))
