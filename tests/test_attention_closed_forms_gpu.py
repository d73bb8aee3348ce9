"""GPU: every attention route (tt_attention: attn_kernel with masks 0 / 1 / 2, the fused query projection, row-major V, fp32 exact and
split16; attn_pipe_kernel; attn8_kernel; tt_temporal_attention's two kernels; tt_encoder_attention) on the closed-form operands of
tests/attention_closed_forms.py (its docstring has the three families F1 / F2 / F3 and the derivation of every bound term): every element
of every output against its expectation, and the layout contracts on F1 and F2 -- poisoned padding between lk and the sequence strides,
q / qx / out as strided row views with sentinel rows in between, launches of batch sub-ranges with batch0 -- each giving the bits of the
plain run.  Every tt_attention case asserts the kernel instance it claims to test (ops.PROFILE: tt_attention_kernel's answer)."""
import time

import pytest
import torch

from tests import attention_closed_forms as cf

pytestmark = pytest.mark.gpu

ROUTES = cf.routes()
RATIOS = {}                         # (family, kernel, types) -> largest err/bound seen (printed when the module ends)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from this_and_that_vdm_amd import ops as o
    t0 = time.time()
    yield o
    print(f"\n[closed forms] module time {time.time() - t0:.1f} s; worst err/bound per family and route (F2 in 16-bit storage is bit for bit: 0):")
    for k, v in sorted(RATIOS.items()):
        print(f"[closed forms]   {k}: {v:.3g}")


def _route_key(P):
    if P.entry == "temporal":
        kernel = "tattn_mfma_kernel" if P.mfma else "tattn_kernel"
    else:
        kernel = P.kernel.split("<")[0]
        if P.entry == "attention" and kernel == "attn_kernel":
            kernel += "".join(s for s, on in ((" mask 1/2", P.mask != 0), (" QP", P.qproj), (" VR", P.v_rows), (" split16", P.split)) if on)
    return f"{P.family} {kernel} {P.ptype}" + (f" -> {P.dt}" if P.ptype == "fp8" else "")


def _run(ops, P):
    """one launch, every element checked; -> the output rows"""
    if P.family == "F2":
        cf.assert_margin(P)            # on the CPU, fp64, from the storage values: what "bit for bit" rests on
    if P.family == "F3" and P.ptype == "fp8":
        cf.assert_fp8_range(P)
    got, wide, name = cf.run(ops, P)
    if P.entry == "attention":
        assert name == P.kernel, f"{P.name}: launched {name}, the case is built for {P.kernel}"
    ratio, msg = cf.check(P, got)
    key = _route_key(P)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    assert msg is None, msg
    if P.cb > 1:
        keep = torch.ones(wide.shape[0], dtype=torch.bool)
        keep[P.cls::P.cb] = False
        assert bool((wide[keep].double() == cf.SENTINEL).all()), f"{P.name}: a row between the view's rows was written"
    return got


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r.id)
def test_closed_forms(ops, route):
    full = {}
    for fam in route.families:
        P = route.make(fam)
        plain = full[fam] = _run(ops, P)
        if fam == "F3":
            continue
        Pp = route.make(fam, poison=True)
        assert torch.equal(_run(ops, Pp), plain), f"{Pp.name}: the bits differ from the plain run's"
        if route.views:
            for cb, cls in ((2, 1), (3, 2)):
                Pv = route.make(fam, cb=cb, cls=cls)
                assert torch.equal(_run(ops, Pv), plain), f"{Pv.name}: the bits differ from the plain run's"
    if route.batch0:
        for b0 in (1, 2):
            for fam in ("F1", "F2"):
                P = route.make(fam, batch0=b0)
                rows = full[fam][b0 * P.kw["frames"] * P.kw["lq"]:]
                assert torch.equal(_run(ops, P), rows), f"{P.name}: the bits differ from the full launch's rows"
