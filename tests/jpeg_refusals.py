"""Every refusal of tt_jpeg_coeffs and tt_jpeg_scan (include/ttvdm.h): one valid argument set (fake non-null aligned pointers), ONE
fault applied at a time, the return code and the message (tt_last_error) recorded.  Every refusal returns before the first HIP call, so
this needs no GPU -- and a fully valid argument set is never passed (that would launch a kernel on pointers that do not exist).  As a
second line of defence the rows run in a child process that sees no GPU (`python -m tests.jpeg_refusals`), in the manner of
tests/png_refusals.py: a row that were NOT refused would fail to launch there (TT_ELAUNCH) instead of faulting a device."""
import json
import os
import sys

P = 0x10000          # a fake operand address; the operands sit 64 KiB apart
EINVAL, EUNSUPPORTED = -1, -2
SHAPE_ROWS = [
    (dict(n=0), EINVAL, "empty problem"), (dict(n=-3), EINVAL, "empty problem"), (dict(h=0), EINVAL, "empty problem"),
    (dict(w=-2), EINVAL, "empty problem"), (dict(ch=0), EINVAL, "0 channels"), (dict(ch=2), EINVAL, "2 channels"),
    (dict(ch=4), EINVAL, "4 channels"), (dict(subsampling=1), EINVAL, "subsampling = 1"), (dict(subsampling=3), EINVAL, "subsampling = 3"),
    (dict(h=30000, w=30000), EUNSUPPORTED, "a frame of 2700000000 bytes"),
    (dict(h=20000, w=20000), EUNSUPPORTED, "a scan bound of"),
    (dict(n=65536), EUNSUPPORTED, "more than one grid covers"),
]
COEFFS = dict(frames=P, n=3, h=13, w=37, ch=3, quality=75, subsampling=2, coeffs=2 * P, counts=3 * P)
COEFFS_ORDER = ("frames", "n", "h", "w", "ch", "quality", "subsampling", "coeffs", "counts")
COEFFS_ROWS = SHAPE_ROWS + [
    (dict(frames=None), EINVAL, "null frames"), (dict(coeffs=None), EINVAL, "null coeffs"),
    (dict(quality=0), EINVAL, "quality = 0"), (dict(quality=101), EINVAL, "quality = 101"),
    (dict(coeffs=2 * P + 8), EINVAL, "coeffs is not 16-byte aligned"), (dict(counts=3 * P + 4), EINVAL, "counts is not 16-byte aligned"),
]
# 13 x 37 in 4:2:0: 3 MCUs of 6 blocks: a bound of 18 x 432 + 2 -> 7792 bytes a frame
SCAN = dict(coeffs=P, n=3, h=13, w=37, ch=3, subsampling=2, tables=2 * P, ntables=1, out=3 * P, cap=3 * 7792, lengths=4 * P, ws=5 * P, ws_bytes=1 << 20)
SCAN_ORDER = ("coeffs", "n", "h", "w", "ch", "subsampling", "tables", "ntables", "out", "cap", "lengths", "ws", "ws_bytes")
SCAN_ROWS = SHAPE_ROWS + [
    (dict(coeffs=None), EINVAL, "null coeffs"), (dict(tables=None), EINVAL, "null tables"), (dict(out=None), EINVAL, "null out"),
    (dict(lengths=None), EINVAL, "null lengths"), (dict(ws=None), EINVAL, "null ws"),
    (dict(ntables=2), EINVAL, "ntables = 2"), (dict(ntables=0), EINVAL, "ntables = 0"),
    (dict(coeffs=P + 8), EINVAL, "coeffs is not 16-byte aligned"), (dict(tables=2 * P + 4), EINVAL, "tables is not 16-byte aligned"),
    (dict(out=3 * P + 1), EINVAL, "out is not 16-byte aligned"), (dict(lengths=4 * P + 2), EINVAL, "lengths is not 4-byte aligned"),
    (dict(ws=5 * P + 8), EINVAL, "ws is not 16-byte aligned"),
    (dict(cap=3 * 7792 - 1), EINVAL, "cap too small"), (dict(cap=0), EINVAL, "cap too small"), (dict(ws_bytes=100), EINVAL, "ws too small"),
]
FAMILIES = {"coeffs": ("tt_jpeg_coeffs", COEFFS, COEFFS_ORDER, COEFFS_ROWS), "scan": ("tt_jpeg_scan", SCAN, SCAN_ORDER, SCAN_ROWS)}


def row_id(family, fault):
    return family + ":" + ",".join(f"{k}={v}" for k, v in fault.items())


def take(lib):
    out = {}
    assert lib.tt_jpeg_scan_bound(13, 37, 3, 2) == 7792
    for family, (entry, valid, order, rows) in FAMILIES.items():
        for fault, _, _ in rows:
            assert fault, "a row without a fault would be a valid call"
            a = dict(valid, **fault)
            out[row_id(family, fault)] = [getattr(lib, entry)(*[a[k] for k in order], None), lib.tt_last_error().decode()]
    return out


def run_child():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TT_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")           # the child sees no GPU
    r = subprocess.run([sys.executable, "-m", "tests.jpeg_refusals"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"jpeg refusals failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    print(json.dumps(take(_lib.load()), separators=(",", ":")))
