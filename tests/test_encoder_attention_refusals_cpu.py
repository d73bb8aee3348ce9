"""Every refusal of tt_encoder_attention: one valid argument set (fake non-null 16-byte-aligned pointers), ONE fault applied per case, the
return code and the tt_last_error text checked.  Every refusal returns before the first HIP call, so nothing is launched and no GPU is
needed; a fully valid argument set is never passed (as in tests/attention_refusals.py)."""
import ctypes as C

import pytest

from this_and_that_vdm_amd import _lib

TT_BF16, TT_F16, TT_F32 = 0, 1, 2
TT_EINVAL, TT_EUNSUPPORTED = -1, -2
P = 0x10000
VALID = dict(q=P, ldq=480, k=P + 320, ldk=480, v=P + 640, ldv=480, out=4 * P, ldo=160, nseq=2, l=17, heads=2, head_dim=80, causal=0,
             k_seq_stride=17, v_seq_stride=17, dtype=TT_BF16)
VALID_F32 = dict(VALID, dtype=TT_F32, v=3 * P, ldv=40, v_seq_stride=20)

CASES = [
    ("null q", VALID, dict(q=None), TT_EINVAL, "null operand"),
    ("null k", VALID, dict(k=None), TT_EINVAL, "null operand"),
    ("null v", VALID, dict(v=None), TT_EINVAL, "null operand"),
    ("null out", VALID, dict(out=None), TT_EINVAL, "null operand"),
    ("no sequences", VALID, dict(nseq=0), TT_EINVAL, "empty problem"),
    ("no tokens", VALID, dict(l=0), TT_EINVAL, "empty problem"),
    ("no heads", VALID, dict(heads=0), TT_EINVAL, "empty problem"),
    ("head_dim 96", VALID, dict(head_dim=96), TT_EUNSUPPORTED, "head_dim 96 (64 or 80)"),
    ("head_dim 128", VALID, dict(head_dim=128), TT_EUNSUPPORTED, "head_dim 128 (64 or 80)"),
    ("bad dtype", VALID, dict(dtype=7), TT_EINVAL, "bad dtype"),
    ("causal 2", VALID, dict(causal=2), TT_EINVAL, "causal 2"),
    ("row stride off a chunk", VALID, dict(ldk=484), TT_EINVAL, "16-byte chunks"),
    ("fp32 v^T sequence stride off a chunk", VALID_F32, dict(v_seq_stride=18), TT_EINVAL, "16-byte chunks"),
    ("base pointer off a chunk", VALID, dict(k=P + 324), TT_EINVAL, "16-byte boundaries"),
    ("out pointer off a chunk", VALID, dict(out=4 * P + 2), TT_EINVAL, "16-byte boundaries"),
    ("k sequence stride < l", VALID, dict(k_seq_stride=16), TT_EINVAL, "l exceeds sequence stride"),
    ("v sequence stride < l", VALID_F32, dict(v_seq_stride=16), TT_EINVAL, "l exceeds sequence stride"),
    ("row stride < row", VALID, dict(ldo=152), TT_EINVAL, "row stride smaller than the row"),
    ("fp32 v^T row shorter than the keys", VALID_F32, dict(ldv=36), TT_EINVAL, "row stride smaller than the row"),
    ("K beyond 2 GiB", VALID, dict(ldk=1 << 30), TT_EUNSUPPORTED, "larger than 2 GiB"),
]


@pytest.fixture(scope="module")
def lib():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("what,base,fault,code,text", CASES, ids=[c[0] for c in CASES])
def test_refusal(lib, what, base, fault, code, text):
    assert fault, "a case without a fault would be a valid call"
    a = _lib.TtEncAttnArgs()
    for k, v in dict(base, **fault).items():
        setattr(a, k, v)
    assert lib.tt_encoder_attention(C.byref(a), None) == code
    msg = lib.tt_last_error().decode()
    assert msg.startswith("tt_encoder_attention:") and text in msg, msg


def test_null_args(lib):
    assert lib.tt_encoder_attention(None, None) == TT_EINVAL


def test_struct_size_matches_the_header():
    import os
    import subprocess
    import tempfile
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = '#include <stdio.h>\n#include "ttvdm.h"\nint main(){printf("%zu\\n", sizeof(TtEncAttnArgs));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(repo, "include"), c, "-o", exe])
        assert int(subprocess.check_output([exe])) == C.sizeof(_lib.TtEncAttnArgs)
