"""Every refusal of tt_png_filter, tt_png_tokens and tt_png_emit (include/ttvdm.h): one valid argument set (fake non-null aligned
pointers), ONE fault applied at a time, the return code and the message (tt_last_error) recorded.  Every refusal returns before the
first HIP call, so this needs no GPU -- and a fully valid argument set is never passed (that would launch a kernel on pointers that do
not exist).  As a second line of defence the rows run in a child process that sees no GPU (`python -m tests.png_refusals`), in the
manner of tests/gif_refusals.py: a row that were NOT refused would fail to launch there (TT_ELAUNCH) instead of faulting a device."""
import json
import os
import sys

P = 0x10000          # a fake operand address; the operands sit 64 KiB apart
EINVAL, EUNSUPPORTED = -1, -2
SHAPE_ROWS = [
    (dict(n=0), EINVAL, "empty problem"), (dict(n=-3), EINVAL, "empty problem"), (dict(h=0), EINVAL, "empty problem"),
    (dict(w=-2), EINVAL, "empty problem"), (dict(ch=0), EINVAL, "0 channels"), (dict(ch=5), EINVAL, "5 channels"),
    (dict(h=40000, w=40000, ch=4), EUNSUPPORTED, "a filtered stream of 6400040000 bytes"),
    (dict(n=2 ** 31 - 1, h=2), EUNSUPPORTED, "more than one grid covers"),
]
FILTER = dict(frames=P, n=3, h=13, w=37, ch=3, filter=5, filtered=2 * P)
FILTER_ORDER = ("frames", "n", "h", "w", "ch", "filter", "filtered")
FILTER_ROWS = SHAPE_ROWS + [
    (dict(frames=None), EINVAL, "null frames"), (dict(filtered=None), EINVAL, "null filtered"),
    (dict(filter=-1), EINVAL, "filter = -1"), (dict(filter=6), EINVAL, "filter = 6"),
    (dict(filtered=2 * P + 8), EINVAL, "filtered is not 16-byte aligned"),
]
TOKENS = dict(filtered=P, n=3, h=13, w=37, ch=3, records=2 * P)
TOKENS_ORDER = ("filtered", "n", "h", "w", "ch", "records")
TOKENS_ROWS = SHAPE_ROWS + [
    (dict(filtered=None), EINVAL, "null filtered"), (dict(records=None), EINVAL, "null records"),
    (dict(filtered=P + 4), EINVAL, "filtered is not 16-byte aligned"), (dict(records=2 * P + 4), EINVAL, "records is not 16-byte aligned"),
]
EMIT = dict(filtered=P, n=3, h=13, w=37, ch=3, tables=2 * P, headers=3 * P, out=4 * P, out_bytes=5000, cap=5000)
EMIT_ORDER = ("filtered", "n", "h", "w", "ch", "tables", "headers", "out", "out_bytes", "cap")
EMIT_ROWS = SHAPE_ROWS + [
    (dict(filtered=None), EINVAL, "null filtered"), (dict(tables=None), EINVAL, "null tables"), (dict(headers=None), EINVAL, "null headers"),
    (dict(out=None), EINVAL, "null out"),
    (dict(filtered=P + 8), EINVAL, "filtered is not 16-byte aligned"), (dict(tables=2 * P + 4), EINVAL, "tables is not 16-byte aligned"),
    (dict(headers=3 * P + 4), EINVAL, "headers is not 16-byte aligned"), (dict(out=4 * P + 1), EINVAL, "out is not 16-byte aligned"),
    (dict(out_bytes=0), EINVAL, "out_bytes = 0"), (dict(cap=4999), EINVAL, "cap too small"), (dict(cap=0), EINVAL, "cap too small"),
]
FAMILIES = {"filter": ("tt_png_filter", FILTER, FILTER_ORDER, FILTER_ROWS), "tokens": ("tt_png_tokens", TOKENS, TOKENS_ORDER, TOKENS_ROWS),
            "emit": ("tt_png_emit", EMIT, EMIT_ORDER, EMIT_ROWS)}


def row_id(family, fault):
    return family + ":" + ",".join(f"{k}={v}" for k, v in fault.items())


def take(lib):
    out = {}
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
    r = subprocess.run([sys.executable, "-m", "tests.png_refusals"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"png refusals failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    print(json.dumps(take(_lib.load()), separators=(",", ":")))
