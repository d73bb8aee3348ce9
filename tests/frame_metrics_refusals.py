"""Every refusal of tt_frame_metrics and tt_frames_pool2 (include/ttvdm.h): one valid argument set (fake non-null aligned pointers), ONE
fault applied at a time, the return code and the message (tt_last_error) recorded.  Every refusal returns before the first HIP call, so
this needs no GPU -- and a fully valid argument set is never passed (that would launch a kernel on pointers that do not exist).  As a
second line of defence the rows run in a child process that sees no GPU (`python -m tests.frame_metrics_refusals`), in the manner of
tests/attention_refusals.py: a row that were NOT refused would fail to launch there (TT_ELAUNCH) instead of faulting a device."""
import json
import os
import sys

P = 0x10000          # a fake operand address; the operands sit 64 KiB apart
SSE_ONLY = 1
METRICS = dict(a=P, b=2 * P, kind=1, n=2, h=32, w=48, ch=3, data_range=255.0, flags=0, rec=3 * P, ws=4 * P, ws_bytes=1 << 20)
METRICS_ORDER = ("a", "b", "kind", "n", "h", "w", "ch", "data_range", "flags", "rec", "ws", "ws_bytes")
# (fault, a fragment of the message)
METRICS_ROWS = [
    (dict(a=None), "null a"), (dict(b=None), "null b"), (dict(rec=None), "null rec"),
    (dict(n=0), "empty problem"), (dict(n=-3), "empty problem"),
    (dict(ch=0), "channels"), (dict(ch=5), "channels"),
    (dict(kind=2), "kind 2"), (dict(kind=-1), "kind -1"),
    (dict(h=10), "no 11 x 11 window"), (dict(w=10), "no 11 x 11 window"), (dict(h=3, w=5), "no 11 x 11 window"),
    (dict(data_range=0.0), "data_range"), (dict(data_range=-1.0), "data_range"), (dict(data_range=float("inf")), "data_range"),
    (dict(data_range=float("nan")), "data_range"),
    (dict(flags=2), "unknown flags"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=2 * 2 * 3 * 96 - 1), "workspace"), (dict(ws=4 * P + 4), "ws is not 8-byte aligned"),
    (dict(rec=3 * P + 4), "rec is not 8-byte aligned"),
    (dict(kind=0, data_range=1.0, a=P + 2), "4-byte elements"),
    (dict(flags=SSE_ONLY, h=3, w=5, ws=None), "workspace"),               # the flag admits the small frame: the next check refuses
]
POOL = dict(src=P, kind=1, n=2, h=32, w=48, ch=3, dst=2 * P)
POOL_ORDER = ("src", "kind", "n", "h", "w", "ch", "dst")
POOL_ROWS = [
    (dict(src=None), "null src"), (dict(dst=None), "null dst"), (dict(kind=3), "kind 3"), (dict(n=0), "empty problem"),
    (dict(h=31), "must be even"), (dict(w=47), "must be even"), (dict(ch=0), "channels"), (dict(ch=5), "channels"),
    (dict(dst=2 * P + 2), "4-byte aligned"), (dict(kind=0, src=P + 1), "4-byte aligned"),
]


def row_id(family, fault):
    return family + ":" + ",".join(f"{k}={v}" for k, v in fault.items())


def take(lib):
    out = {}
    for fault, _ in METRICS_ROWS:
        assert fault, "a row without a fault would be a valid call"
        m = dict(METRICS, **fault)
        out[row_id("metrics", fault)] = [lib.tt_frame_metrics(*[m[k] for k in METRICS_ORDER], None), lib.tt_last_error().decode()]
    for fault, _ in POOL_ROWS:
        assert fault
        p = dict(POOL, **fault)
        out[row_id("pool2", fault)] = [lib.tt_frames_pool2(*[p[k] for k in POOL_ORDER], None), lib.tt_last_error().decode()]
    # the workspace query answers 0 for what the entry point refuses, and the stated size otherwise (host arithmetic only)
    out["ws_bytes"] = [lib.tt_frame_metrics_ws_bytes(2, 32, 48, 0), lib.tt_frame_metrics_ws_bytes(2, 3, 5, 0),
                       lib.tt_frame_metrics_ws_bytes(2, 3, 5, SSE_ONLY), lib.tt_frame_metrics_ws_bytes(0, 32, 48, 0),
                       lib.tt_frame_metrics_ws_bytes(1, 26, 27, 0), lib.tt_frame_metrics_ws_bytes(3, 256, 384, 0)]
    return out


def run_child():
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TT_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")           # the child sees no GPU
    r = subprocess.run([sys.executable, "-m", "tests.frame_metrics_refusals"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"frame metrics refusals failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    print(json.dumps(take(_lib.load()), separators=(",", ":")))
