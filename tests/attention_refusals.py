"""Every refusal of tt_attention and tt_temporal_attention: one valid argument set per family (plain, fused query projection, v_rows,
fp8; fake non-null 16-byte-aligned pointers), ONE fault applied at a time, one row per TT_FAIL of the two entry points, the return code
and the message (tt_last_error) recorded.  Every refusal returns before the first HIP call, so this needs no GPU -- and a fully valid argument set is never passed
(that would launch a kernel on pointers that do not exist).  As a second line of defence the rows run in a child process that sees no
GPU (`python -m tests.attention_refusals`): a row that were NOT refused would fail to launch there (TT_ELAUNCH) instead of faulting a device.

tests/test_attention_refusals_cpu.py compares the child's answers with tests/golden/attention_refusals.json, which
tests/golden/make_attention_refusals.py writes from another build of the library (TT_LIBTTVDM)."""
import json
import os
import sys

TT_BF16, TT_F16, TT_F32 = 0, 1, 2
P = 0x10000          # a fake operand address; the operands sit 64 KiB apart

PLAIN = dict(q=P, ldq=128, k=2 * P, ldk=128, vt=3 * P, ldvt=128, out=4 * P, ldo=128, nseq=2, lq=64, heads=2, head_dim=64, mask=0, lk=64,
             k_seq_stride=64, v_seq_stride=64, frames=1, ctx_batches=1, dtype=TT_BF16, batch0=0, fp8=0)
FAMILIES = {
    "plain": PLAIN,
    "qproj": dict(PLAIN, q=None, mask=1, frames=2, ctx_batches=2, ldvt=256, qx=5 * P, ldqx=128, wq=6 * P, ldwq=128, bq=7 * P, qc=128, ln_eps=1e-5),
    "vrows": dict(PLAIN, v_rows=1),
    "fp8": dict(PLAIN, fp8=1),
}
# (family, fault): one per TT_FAIL of tt_attention, in the entry point's order, plus the other arms of the null check
ATTENTION_ROWS = [
    ("plain", dict(k=None)), ("plain", dict(q=None)), ("plain", dict(vt=None)), ("plain", dict(out=None)),
    ("qproj", dict(head_dim=128)), ("qproj", dict(mask=0)), ("qproj", dict(dtype=TT_F32)),
    ("qproj", dict(qc=100)), ("qproj", dict(wq=None)), ("qproj", dict(ln_eps=0.0)),
    ("qproj", dict(bq=7 * P + 4)),
    ("plain", dict(head_dim=96)),
    ("plain", dict(lq=0)),
    ("plain", dict(mask=3)),
    ("qproj", dict(frames=0)),
    ("qproj", dict(batch0=2)),
    ("plain", dict(lk=65)),
    ("qproj", dict(mask=2, v_seq_stride=72)),
    ("plain", dict(dtype=7)),
    ("fp8", dict(dtype=TT_F32)),
    ("plain", dict(ldk=129)),
    ("plain", dict(out=4 * P + 2)),
    ("vrows", dict(head_dim=128)),
    ("plain", dict(ldvt=64)),
    ("vrows", dict(ldvt=64)),
    ("plain", dict(ldk=1 << 30)),
    ("qproj", dict(ldqx=1 << 30)),
]
TEMPORAL = dict(qkv=P, ldqkv=384, out=2 * P, ldo=128, batch=1, frames=14, hw=5, heads=2, head_dim=64, dtype=TT_BF16)
TEMPORAL_ROWS = [dict(qkv=None), dict(out=None), dict(head_dim=96), dict(frames=0), dict(frames=33), dict(dtype=7), dict(ldqkv=385), dict(out=2 * P + 2)]


def row_id(family, fault):
    return family + ":" + ",".join(f"{k}={v}" for k, v in fault.items())


def take(lib):
    from this_and_that_vdm_amd._lib import TtAttnArgs
    import ctypes as C
    out = {}
    for family, fault in ATTENTION_ROWS:
        assert fault, "a row without a fault would be a valid call"
        a = TtAttnArgs()
        for k, v in dict(FAMILIES[family], **fault).items():
            setattr(a, k, v)
        out[row_id(family, fault)] = [lib.tt_attention(C.byref(a), None), lib.tt_last_error().decode()]
    for fault in TEMPORAL_ROWS:
        assert fault
        t = dict(TEMPORAL, **fault)
        code = lib.tt_temporal_attention(t["qkv"], t["ldqkv"], t["out"], t["ldo"], t["batch"], t["frames"], t["hw"], t["heads"], t["head_dim"], t["dtype"], None)
        out[row_id("temporal", fault)] = [code, lib.tt_last_error().decode()]
    return out


def run_child(lib_path=None):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TT_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")           # the child sees no GPU
    if lib_path:
        env["TT_LIBTTVDM"] = lib_path
    r = subprocess.run([sys.executable, "-m", "tests.attention_refusals"], cwd=root, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"attention refusals failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.splitlines()[-1])


if __name__ == "__main__":
    from this_and_that_vdm_amd import _lib
    print(json.dumps(take(_lib.load()), separators=(",", ":")))
