"""GPU: tt_gesture_maps against the HOST rasteriser (gesture_map.rasterise_points) on every element of the ten cases of
tests/gesture_cases.py, in fp32, fp16 and bf16; several maps in one call; no points at all; a captured and replayed call.

fp32 bound: gesture_cases.BOUND32 = 6 A^2 u = 5.0e-7 absolute (host 3 A^2 u + kernel 3 A^2 u, derived there from the number formats;
at or below the 1e-6 the specification requires).  16-bit bound: BOUND32 + ulp(host value) / 2 in that format (the kernel stores the
round-to-nearest-even of its fp32 value).  Frames no point names must be exact zeros."""
import numpy as np
import pytest
import torch

from tests import gesture_cases as gc
from this_and_that_vdm_amd import gesture_map as gm

pytestmark = pytest.mark.gpu
DTYPES = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops
    return ops


def _check(out: torch.Tensor, name: str, dtype_name: str, what: str):
    pts, org, hw, f, dilate, flip = gc.CASES[name]
    want = gc.host(name).astype(np.float64)
    got = out.float().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    bound = np.full_like(want, gc.BOUND32)
    if dtype_name != "float32":
        bound = bound + 0.5 * gc.ulp(gc.host(name), *gc.FORMATS[dtype_name])
    err = np.abs(got - want)
    print(f"{what} {name} {dtype_name}: max |err| = {err.max():.3e}, worst err / bound = {(err / bound).max():.3f}")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (name, dtype_name, float(err.max()), int((err > bound).sum()))
    named = {r[1] for r in gm.point_records(pts, f)}
    for fr in range(f):
        if fr not in named:
            assert not want[fr].any() and (got[fr] == 0.0).all() and not np.signbit(got[fr]).any(), (name, fr)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("name", list(gc.CASES))
def test_case_matches_the_host_rasteriser(ops, name, dtype_name):
    pts, org, hw, f, dilate, flip = gc.CASES[name]
    gp = gm.GesturePoints(pts, org, dilate, flip)
    out = gm.rasterise_points_device(gp, hw[0], hw[1], f, "cuda", DTYPES[dtype_name])
    assert out.shape == (f, 3, hw[0], hw[1]) and out.dtype == DTYPES[dtype_name] and out.is_cuda
    _check(out, name, dtype_name, "device vs host")
    # the same call into a buffer full of NaNs: every element is written by the kernel
    buf = torch.full((1, f, 3, hw[0], hw[1]), float("nan"), dtype=DTYPES[dtype_name], device="cuda")
    ops.gesture_maps(gm.point_records(pts, f), 1, f, org, hw, dilate, flip, DTYPES[dtype_name], "cuda", out=buf)
    assert torch.equal(buf[0], out)


def test_no_dilate_overshoots_like_the_host(ops):
    pts, org, hw, f, dilate, flip = gc.CASES["no_dilate"]
    out = gm.rasterise_points_device(gm.GesturePoints(pts, org, dilate, flip), hw[0], hw[1], f, "cuda")
    assert float(out.min()) < -0.05 and float(out.max()) > 1.05            # no clamping of the resize's overshoot


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_two_maps_in_one_call(ops, dtype_name):
    dt = DTYPES[dtype_name]
    p1, org, hw, f, _, _ = gc.CASES["interior"]
    p6 = gc.CASES["flip"][0]
    a, b = gm.GesturePoints(p1, org), gm.GesturePoints(p6, org)
    both = gm.rasterise_points_device([a, b], hw[0], hw[1], f, "cuda", dt)              # same size / dilate / flip: ONE call, nmaps = 2
    assert both.shape == (2, f, 3, hw[0], hw[1])
    for got, g in zip(both, (a, b)):
        assert torch.equal(got, gm.rasterise_points_device(g, hw[0], hw[1], f, "cuda", dt))
    _check(both[0], "interior", dtype_name, "map 0 of two")
    # cases 1 and 6 as they are (case 6 is flipped): each map is bitwise its own single-map call, and within the bound of the host
    b_flip = gm.GesturePoints(p6, org, True, True)
    mixed = gm.rasterise_points_device([a, b_flip], hw[0], hw[1], f, "cuda", dt)
    assert mixed.shape == (2, f, 3, hw[0], hw[1])
    assert torch.equal(mixed[0], both[0])
    assert torch.equal(mixed[1], gm.rasterise_points_device(b_flip, hw[0], hw[1], f, "cuda", dt))
    _check(mixed[1][:2], "flip", dtype_name, "map 1 of two")
    assert not mixed[1][2:].any()


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_no_points_gives_all_zeros(ops, dtype_name):
    buf = torch.full((2, 3, 3, 24, 57), float("nan"), dtype=DTYPES[dtype_name], device="cuda")
    out = ops.gesture_maps([], 2, 3, (67, 101), (24, 57), True, False, DTYPES[dtype_name], "cuda", out=buf)
    assert out is buf and not out.any() and not torch.signbit(out).any()


def test_captured_call_replays_bitwise(ops):
    pts, org, hw, f, dilate, flip = gc.CASES["odd_w57"]
    recs = gm.point_records(pts, f)
    eager = ops.gesture_maps(recs, 1, f, org, hw, dilate, flip, torch.float16, "cuda")
    buf = torch.full_like(eager, float("nan"))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                             # the stream's workspace exists before the capture
        ops.gesture_maps(recs, 1, f, org, hw, dilate, flip, torch.float16, "cuda", out=buf)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.gesture_maps(recs, 1, f, org, hw, dilate, flip, torch.float16, "cuda", out=buf)
    for _ in range(2):
        buf.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf, eager)
