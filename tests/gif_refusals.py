"""Every refusal of tt_color_hist and tt_palette_map (include/ttvdm.h): one valid argument set (fake non-null aligned pointers), ONE
fault applied at a time, the return code and the message (tt_last_error) recorded.  Every refusal returns before the first HIP call, so
this needs no GPU -- and a fully valid argument set is never passed (that would launch a kernel on pointers that do not exist).  As a
second line of defence the rows run in a child process that sees no GPU (`python -m tests.gif_refusals`), in the manner of
tests/frame_metrics_refusals.py: a row that were NOT refused would fail to launch there (TT_ELAUNCH) instead of faulting a device."""
import ctypes
import json
import os
import sys

P = 0x10000          # a fake operand address; the operands sit 64 KiB apart
EINVAL, EUNSUPPORTED = -1, -2
HIST = dict(frames=P, n=3, h=13, w=37, ch=3, nhist=3, hist=2 * P)
HIST_ORDER = ("frames", "n", "h", "w", "ch", "nhist", "hist")
# (fault, the code, a fragment of the message)
HIST_ROWS = [
    (dict(frames=None), EINVAL, "null frames"), (dict(hist=None), EINVAL, "null hist"),
    (dict(n=0), EINVAL, "empty problem"), (dict(h=0), EINVAL, "empty problem"), (dict(w=-2), EINVAL, "empty problem"),
    (dict(ch=4), EINVAL, "4 channels"), (dict(ch=1), EINVAL, "1 channels"),
    (dict(nhist=2), EINVAL, "2 histograms for 3 frames"), (dict(nhist=0), EINVAL, "0 histograms"),
    (dict(hist=2 * P + 8), EINVAL, "hist is not 16-byte aligned"),
    (dict(h=4105, w=4105), EUNSUPPORTED, "16851025 pixels per histogram"),                       # one frame beyond (2^32 - 1) / 255
    (dict(n=5, nhist=1, h=2048, w=2048), EUNSUPPORTED, "20971520 pixels per histogram"),          # ... and all frames together
    (dict(n=70000, nhist=70000, h=2, w=2), EUNSUPPORTED, "70000 histograms"),
]
MAP = dict(frames=P, n=3, h=13, w=37, ch=3, palettes=2 * P, npal=3, ncolors=(256, 1, 17), indices=3 * P, sse=4 * P, stats=5 * P)
MAP_ORDER = ("frames", "n", "h", "w", "ch", "palettes", "npal", "ncolors", "indices", "sse", "stats")
MAP_ROWS = [
    (dict(frames=None), EINVAL, "null frames"), (dict(palettes=None), EINVAL, "null palettes"), (dict(ncolors=None), EINVAL, "null ncolors"),
    (dict(indices=None), EINVAL, "null indices"), (dict(sse=None), EINVAL, "null sse"),
    (dict(n=0), EINVAL, "empty problem"), (dict(h=-1), EINVAL, "empty problem"), (dict(w=0), EINVAL, "empty problem"),
    (dict(ch=4), EINVAL, "4 channels"), (dict(ch=2), EINVAL, "2 channels"),
    (dict(npal=2, ncolors=(4, 4)), EINVAL, "2 palettes for 3 frames"),
    (dict(ncolors=(256, 0, 17)), EINVAL, "ncolors[1] = 0"), (dict(ncolors=(257, 1, 17)), EINVAL, "ncolors[0] = 257"),
    (dict(ncolors=(256, 1, -5)), EINVAL, "ncolors[2] = -5"),
    (dict(palettes=2 * P + 2), EINVAL, "palettes is not 4-byte aligned"), (dict(sse=4 * P + 4), EINVAL, "sse is not 8-byte aligned"),
    (dict(stats=5 * P + 4), EINVAL, "stats is not 16-byte aligned"),
    (dict(n=1025, npal=1025, ncolors=(2,) * 1025), EUNSUPPORTED, "1025 palettes"),
    (dict(n=70000, npal=1, ncolors=(2,), h=2, w=2), EUNSUPPORTED, "70000 frames"),
    (dict(n=5, npal=1, ncolors=(9,), h=2048, w=2048), EUNSUPPORTED, "20971520 pixels per palette"),
]


def row_id(family, fault):
    return family + ":" + ",".join(f"{k}={v if not isinstance(v, tuple) or len(v) < 8 else len(v)}" for k, v in fault.items())


def take(lib):
    out = {}
    for fault, _, _ in HIST_ROWS:
        assert fault, "a row without a fault would be a valid call"
        a = dict(HIST, **fault)
        out[row_id("hist", fault)] = [lib.tt_color_hist(*[a[k] for k in HIST_ORDER], None), lib.tt_last_error().decode()]
    for fault, _, _ in MAP_ROWS:
        assert fault
        a = dict(MAP, **fault)
        if a["ncolors"] is not None:
            a["ncolors"] = (ctypes.c_int32 * len(a["ncolors"]))(*a["ncolors"])
        out[row_id("map", fault)] = [lib.tt_palette_map(*[a[k] for k in MAP_ORDER], None), lib.tt_last_error().decode()]
    return out


def run_child():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TT_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")           # the child sees no GPU
    r = subprocess.run([sys.executable, "-m", "tests.gif_refusals"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"gif refusals failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    print(json.dumps(take(_lib.load()), separators=(",", ":")))
