"""Every refusal of tt_gif_lzw_frames (include/ttvdm.h, "GIF LZW on the device"): one valid argument set (fake non-null aligned
pointers), ONE fault applied at a time, the return code and the message (tt_last_error) recorded; and what the two size functions
answer for the same faults (0).  Every refusal returns before the first HIP call, so this needs no GPU -- and a fully valid argument
set is never passed (that would launch kernels on pointers that do not exist).  As a second line of defence the rows run in a child
process that sees no GPU (`python -m tests.gif_lzw_refusals`), in the manner of tests/gif_refusals.py: a row that were NOT refused would
fail to launch there (TT_ELAUNCH) instead of faulting a device.  The GPU test passes the same rows with real device buffers."""
import json
import os
import sys

P = 0x10000          # a fake operand address; the operands sit 64 KiB apart
EINVAL, EUNSUPPORTED = -1, -2
BIG = 1 << 40        # a cap and a workspace that are never the fault
ARGS = dict(indices=P, n=3, npix=384, mcs=2 * P, nmcs=3, segment=100, out=3 * P, cap=BIG, lengths=4 * P, status=5 * P, ws=6 * P, ws_bytes=BIG)
ORDER = ("indices", "n", "npix", "mcs", "nmcs", "segment", "out", "cap", "lengths", "status", "ws", "ws_bytes")
SEGMENT_MAX = 65536
# (fault, the code, a fragment of the message)
ROWS = [
    (dict(indices=None), EINVAL, "null indices"), (dict(mcs=None), EINVAL, "null min_code_size"), (dict(out=None), EINVAL, "null out"),
    (dict(lengths=None), EINVAL, "null lengths"), (dict(status=None), EINVAL, "null status"), (dict(ws=None), EINVAL, "null ws"),
    (dict(n=0), EINVAL, "empty problem"), (dict(n=-1), EINVAL, "empty problem"), (dict(npix=0), EINVAL, "empty problem"),
    (dict(npix=-7), EINVAL, "empty problem"),
    (dict(nmcs=2), EINVAL, "nmcs = 2"), (dict(nmcs=0), EINVAL, "nmcs = 0"),
    (dict(segment=-1), EINVAL, "segment = -1"), (dict(segment=SEGMENT_MAX + 1), EINVAL, f"segment = {SEGMENT_MAX + 1}"),
    (dict(out=3 * P + 8), EINVAL, "out is not 16-byte aligned"), (dict(ws=6 * P + 4), EINVAL, "ws is not 16-byte aligned"),
    (dict(lengths=4 * P + 2), EINVAL, "lengths is not 4-byte aligned"), (dict(status=5 * P + 1), EINVAL, "status is not 4-byte aligned"),
    (dict(mcs=2 * P + 2), EINVAL, "min_code_size is not 4-byte aligned"),
    (dict(cap="short"), EINVAL, "cap too small"), (dict(cap=0), EINVAL, "cap too small"),
    (dict(ws_bytes="short"), EINVAL, "ws too small"), (dict(ws_bytes=0), EINVAL, "ws too small"),
    (dict(n=70000, nmcs=1), EUNSUPPORTED, "70000 frames"),
    (dict(npix=400_000_000, segment=0), EUNSUPPORTED, "fewer than 2^29 = 536870912"),
    (dict(n=60000, nmcs=1, npix=1 << 20, segment=1), EUNSUPPORTED, "fewer than 2^31 = 2147483648"),
]
# faults that the size functions see too (they take n, npix, segment): both answer 0
SIZE_FAULTS = [dict(npix=0), dict(npix=-7), dict(segment=-1), dict(segment=SEGMENT_MAX + 1), dict(npix=400_000_000, segment=0)]


def row_id(fault):
    return ",".join(f"{k}={v}" for k, v in fault.items())


def resolve(lib, a):
    """'short': one byte less than the size function asks for"""
    a = dict(a)
    if a["cap"] == "short":
        a["cap"] = a["n"] * lib.tt_gif_lzw_frames_bound(a["npix"], a["segment"]) - 1
    if a["ws_bytes"] == "short":
        a["ws_bytes"] = lib.tt_gif_lzw_frames_ws_bytes(a["n"], a["npix"], a["segment"]) - 1
    return a


def call(lib, a, stream=None):
    return [lib.tt_gif_lzw_frames(*[a[k] for k in ORDER], stream), lib.tt_last_error().decode()]


def take(lib):
    out = {}
    for fault, _, _ in ROWS:
        assert fault, "a row without a fault would be a valid call"
        out[row_id(fault)] = call(lib, resolve(lib, dict(ARGS, **fault)))
    for fault in SIZE_FAULTS:
        a = dict(ARGS, **fault)
        out["sizes:" + row_id(fault)] = [lib.tt_gif_lzw_frames_bound(a["npix"], a["segment"]), lib.tt_gif_lzw_frames_ws_bytes(a["n"], a["npix"], a["segment"])]
    out["sizes:n=0"] = [1, lib.tt_gif_lzw_frames_ws_bytes(0, 384, 100)]
    out["sizes:valid"] = [lib.tt_gif_lzw_frames_bound(384, 100), lib.tt_gif_lzw_frames_ws_bytes(3, 384, 100)]
    return out


def run_child():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TT_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")           # the child sees no GPU
    r = subprocess.run([sys.executable, "-m", "tests.gif_lzw_refusals"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"gif lzw refusals failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    print(json.dumps(take(_lib.load()), separators=(",", ":")))
