"""tt_gesture_maps without a GPU: every refusal of the entry point (one valid argument set with fake aligned pointers, ONE fault per
case, the code and the tt_last_error text checked; all refusals return before the first HIP call and a fully valid set is never
passed, as in tests/test_encoder_attention_refusals_cpu.py), the host-side record building, and the closed form the kernel is built to
against the host rasteriser."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import gesture_cases as gc
from this_and_that_vdm_amd import _lib
from this_and_that_vdm_amd import gesture_map as gm

TT_BF16, TT_F16, TT_F32 = 0, 1, 2
TT_EINVAL, TT_EUNSUPPORTED = -1, -2
P = 0x10000
TWO = ((0, 1, 30, 20, 1), (0, 5, 50, 33, 0))            # (map, frame, x, y, first)
VALID = dict(points=TWO, npoints=2, nmaps=1, frames=6, org_h=48, org_w=72, out_h=32, out_w=40, dilate=1, flip=0, dst=P, dtype=TT_F16,
             ws=2 * P, ws_bytes=2 * (32 + 40) * 8)

CASES = [
    ("null dst", dict(dst=None), TT_EINVAL, "null dst"),
    ("null points", dict(points=None), TT_EINVAL, "null points"),
    ("negative npoints", dict(npoints=-1), TT_EINVAL, "npoints -1"),
    ("no maps", dict(nmaps=0), TT_EINVAL, "0 map(s)"),
    ("no frames", dict(frames=0), TT_EINVAL, "0 frame(s)"),
    ("out_h 0", dict(out_h=0), TT_EINVAL, "output size 0 x 40"),
    ("out_w -1", dict(out_w=-1), TT_EINVAL, "output size 32 x -1"),
    ("org_h 0", dict(org_h=0), TT_EINVAL, "original size 0 x 72"),
    ("org_w 0", dict(org_w=0), TT_EINVAL, "original size 48 x 0"),
    ("map out of range", dict(points=((0, 1, 30, 20, 1), (1, 5, 50, 33, 0))), TT_EINVAL, "point 1 names map 1, frame 5"),
    ("negative map", dict(points=((-1, 1, 30, 20, 1),), npoints=1), TT_EINVAL, "point 0 names map -1"),
    ("frame out of range", dict(points=((0, 6, 30, 20, 1),), npoints=1), TT_EINVAL, "point 0 names map 0, frame 6"),
    ("negative frame", dict(points=((0, -1, 30, 20, 1),), npoints=1), TT_EINVAL, "frame -1"),
    ("first 2", dict(points=((0, 1, 30, 20, 2),), npoints=1), TT_EINVAL, "first 2"),
    ("dilate 2", dict(dilate=2), TT_EINVAL, "dilate 2"),
    ("flip -1", dict(flip=-1), TT_EINVAL, "flip -1"),
    ("bad dtype", dict(dtype=7), TT_EINVAL, "bad dtype"),
    ("dst off a 16-byte boundary", dict(dst=P + 8), TT_EINVAL, "16-byte boundary"),
    ("65 points", dict(points=tuple((0, i % 6, i, i, 0) for i in range(65)), npoints=65, ws_bytes=1 << 20), TT_EUNSUPPORTED, "65 points"),
    ("original axis too long", dict(org_w=(1 << 24) + 1), TT_EUNSUPPORTED, "an axis may be at most 16777216"),
    ("frame beyond 32-bit indices", dict(out_h=1 << 15, out_w=1 << 15), TT_EUNSUPPORTED, "32-bit frame indices"),
    ("null workspace", dict(ws=None), TT_EINVAL, "workspace"),
    ("workspace too small", dict(ws_bytes=2 * (32 + 40) * 8 - 1), TT_EINVAL, "= 1152 bytes"),
    ("workspace off a 16-byte boundary", dict(ws=2 * P + 8), TT_EINVAL, "workspace"),
]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


@pytest.mark.parametrize("what,fault,code,text", CASES, ids=[c[0] for c in CASES])
def test_refusal(lib, what, fault, code, text):
    assert fault, "a case without a fault would be a valid call"
    a = dict(VALID, **fault)
    pts = a["points"]
    recs = None if pts is None else (_lib.TtGesturePoint * len(pts))(*[_lib.TtGesturePoint(*p) for p in pts])
    got = lib.tt_gesture_maps(recs, a["npoints"], a["nmaps"], a["frames"], a["org_h"], a["org_w"], a["out_h"], a["out_w"], a["dilate"],
                              a["flip"], a["dst"], a["dtype"], a["ws"], a["ws_bytes"], None)
    msg = lib.tt_last_error().decode()
    assert got == code, (got, msg)
    assert msg.startswith("tt_gesture_maps:") and text in msg, msg


def test_ws_bytes_and_record_layout(lib):
    assert lib.tt_gesture_maps_ws_bytes(2, 32, 40) == 2 * 72 * 8
    assert lib.tt_gesture_maps_ws_bytes(0, 32, 40) == 0
    assert lib.tt_gesture_maps_ws_bytes(64, 256, 448) == 64 * 704 * 8
    assert C.sizeof(_lib.TtGesturePoint) == 20


# ---- point_records / GesturePoints
def test_point_records_truncate_and_mark_the_first():
    recs = gm.point_records([(0, 71.9, 47.9), (2, -50.0, 200.0), (1, "3.99", "-0.5")], 6)
    assert recs == [(0, 0, 71, 47, 1), (0, 2, -50, 200, 0), (0, 1, 3, 0, 0)]


def test_point_records_frame_indices_follow_numpy_indexing():
    F = 5
    assert gm.point_records([(-1, 1, 2)], F) == [(0, F - 1, 1, 2, 1)]
    assert gm.point_records([(-F, 1, 2)], F) == [(0, 0, 1, 2, 1)]
    for bad in (F, -F - 1):
        with pytest.raises(IndexError):
            gm.point_records([(0, 1, 2), (bad, 1, 2)], F)
        with pytest.raises(IndexError):                   # the host path raises the same error for the same list
            gm.rasterise_points([(0, 1, 2), (bad, 1, 2)], (4, 4), 8, 8, F, dilate=False)


def test_point_records_map_indices_of_a_list():
    a = gm.GesturePoints(((0, 30, 20), (5, 50, 33)), (48, 72))
    b = gm.GesturePoints(((1, 10, 30),), (48, 72))
    recs = [r for m, g in enumerate([a, b]) for r in gm.point_records(g.points, 6, m)]
    assert recs == [(0, 0, 30, 20, 1), (0, 5, 50, 33, 0), (1, 1, 10, 30, 1)]      # `first` restarts with every map
    assert a.dilate is True and a.flip is False and a.org_hw == (48, 72)
    with pytest.raises(Exception):
        a.flip = True                                     # frozen


def test_gesture_points_from_dir(tmp_path):
    import PIL.Image
    PIL.Image.new("RGB", (72, 48)).save(tmp_path / "im_0.jpg")
    (tmp_path / "data.txt").write_text("0 30.5 20.25\n5 50 33\n")
    gp = gm.GesturePoints.from_dir(str(tmp_path), flip=True)
    assert gp == gm.GesturePoints(((0, 30.5, 20.25), (5, 50.0, 33.0)), (48, 72), True, True)
    assert gm.point_records(gp.points, 6) == [(0, 0, 30, 20, 1), (0, 5, 50, 33, 0)]


def test_get_thisthat_sam_default_is_the_host_path(tmp_path):
    import PIL.Image
    PIL.Image.new("RGB", (72, 48)).save(tmp_path / "im_0.jpg")
    (tmp_path / "data.txt").write_text("0 30 20\n5 50 33\n")
    cfg = dict(video_seq_length=6, conditioning_channels=3, height=32, width=40, dilate=True, motion_bucket_id=None)
    cond, bucket, frames, coords = gm.get_thisthat_sam(cfg, str(tmp_path))
    assert isinstance(cond, np.ndarray) and cond.dtype == np.float32 and bucket == 200
    assert np.array_equal(cond, gc.host("interior")) and frames == [0, 5] and coords == [(20, 30), (33, 50)]


# ---- the specification the kernel is built to, independent of the kernel
@pytest.mark.parametrize("name", list(gc.CASES))
def test_closed_form_matches_the_host_rasteriser(name):
    """1 - d_c ry[y] rx[x] in numpy fp64 against rasterise_points, every element.  Bound: the host's three fp32 roundings,
    3 A^2 u = 2.5e-7 (tests/gesture_cases.py), stated as 3e-7; measured 1.0e-7 at the most."""
    pts, org, out, f, dilate, flip = gc.CASES[name]
    want = gc.host(name).astype(np.float64)
    got = gc.closed_form(pts, org, out, f, dilate, flip)
    err = float(np.abs(got - want).max())
    print(f"closed form vs host, {name}: max |err| = {err:.3e}")
    assert gc.HOST_BOUND <= 3e-7
    assert err <= 3e-7, err
    named = {r[1] for r in gm.point_records(pts, f)}
    for fr in range(f):
        if fr not in named:
            assert not got[fr].any() and not want[fr].any()
