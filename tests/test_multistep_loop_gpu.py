"""GPU: the fused denoise loop with the DPM-Solver++ 2M step (DenoiseLoop.begin(multistep=...)) against the oracle's loop body
(oracle.scheduler.denoise_loop) driven by tests/multistep_reference.OracleMultistepScheduler.  tiny_vgl, F = 4, 8 x 16 latents, 5
context tokens, 6 steps -- steps 1..4 are second order, 0 and 5 first order.  Limits are those of tests/test_denoise_loop_gpu.py:
TT_F32 inside the north-star tolerance on every element, fp16 storage rel-L2 <= 3e-3 and cos >= 0.99999 (the CFG-3 case: scaled by
the weight its combination gives the networks' error, see there).  Also: graph replay == eager
launches, no history leaking between requests (the buffer is poisoned with NaN first), split-CFG branches, order 1 == the Euler loop,
independence of the requests of one call, a control-guidance window whose UNet-only graph is first captured mid-request, the
use_instructpix2pix batch, and the range audit's two new sites."""
import functools

import pytest
import torch

from tests.multistep_reference import OracleMultistepScheduler
from tests.parity_common import assert_north_star, build_pair, err_stats

pytestmark = pytest.mark.gpu

STEPS = 6
IGS = 1.5


@functools.lru_cache(maxsize=None)
def _pair(dtype):
    return build_pair("tiny_vgl", dtype, "cuda:0", True)


@functools.lru_cache(maxsize=None)
def _inputs(seed=3):
    from this_and_that_vdm_amd.utils.synthetic import synthetic_inputs
    return synthetic_inputs(2, 4, 8, 16, ctx_tokens=5, ctx_dim=64, seed=seed)


@functools.lru_cache(maxsize=None)
def _sched(order=2):
    from this_and_that_vdm_amd.svd import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(solver_order=order)
    s.set_timesteps(STEPS)
    return s


def _kw(seed=3, with_cn=True, order=2):
    """begin() arguments of one request; order None: the Euler loop (no ``multistep``)"""
    inp, s = _inputs(seed), _sched(order or 2)
    kw = dict(latents=inp["latents"], image_latents=inp["image_latents"], encoder_hidden_states=inp["encoder_hidden_states"],
              added_time_ids=inp["added_time_ids"], guidance_scale=inp["guidance_scale"], sigmas=s.sigmas, timesteps=s.timesteps,
              controlnet_cond=inp["gesture_latents"] if with_cn else None)
    if order is not None:
        kw["multistep"] = s.multistep_coefficients
    return kw


def _kw2(seeds, order=2):
    """two requests in one call: batched tensors class by class (element c * R + r)"""
    a, b = (_kw(s, True, order) for s in seeds)
    by_class = lambda k: torch.cat([a[k][0:1], b[k][0:1], a[k][1:2], b[k][1:2]])
    kw = dict(a, latents=torch.cat([a["latents"], b["latents"]]), image_latents=by_class("image_latents"),
              encoder_hidden_states=by_class("encoder_hidden_states"), added_time_ids=by_class("added_time_ids"),
              guidance_scale=torch.cat([a["guidance_scale"], b["guidance_scale"] + 0.5]),
              controlnet_cond=torch.stack([a["controlnet_cond"], b["controlnet_cond"]]))
    return kw


def _run(dtype, kw, with_cn=True, graph=True, split_cfg=False):
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    p_unet, p_cn, _, _ = _pair(dtype)
    loop = DenoiseLoop(p_unet, p_cn if with_cn else None, use_graph=graph, split_cfg=split_cfg).begin(**kw)
    out = loop.run().clone()
    torch.cuda.synchronize()
    return out, loop


@functools.lru_cache(maxsize=None)
def _oracle(dtype, with_cn, kind="plain"):
    """the reference's loop body with the 2M scheduler, computed once per case and shared"""
    from oracle.scheduler import denoise_loop
    _, _, o_unet, o_cn = _pair(dtype)
    inp = _inputs()
    args = (inp["latents"], inp["image_latents"], inp["encoder_hidden_states"], inp["added_time_ids"])
    kw = {}
    if kind == "ip2p":
        args = (inp["latents"],) + _ip2p_constants()
        kw = dict(use_instructpix2pix=True, image_guidance_scale=IGS)
    with torch.no_grad():
        return denoise_loop(o_unet, o_cn if with_cn else None, OracleMultistepScheduler(), *args, inp["gesture_latents"],
                            inp["guidance_scale"], num_inference_steps=STEPS, conditioning_scale=1.0, **kw)


def _ip2p_constants():
    inp = _inputs()
    img, ctx = inp["image_latents"][1:], inp["encoder_hidden_states"][1:]
    return (torch.cat([img, img, torch.zeros_like(img)]), torch.cat([ctx, torch.zeros_like(ctx), torch.zeros_like(ctx)]),
            inp["added_time_ids"][:1].repeat(3, 1))


def _check(got, ref, dtype, what, scale=1.0):
    """scale: how much more of the networks' fp16 error the case's CFG combination lets through than the CFG-2 combination the two
    fp16 limits were set for -- rel-L2 grows with it, 1 - cos with its square"""
    s = err_stats(got, ref)
    print(f"{what} ({dtype}):", s)
    if dtype == torch.float32:
        assert_north_star(got.reshape(ref.shape), ref, what)
    else:
        assert s["rel_l2"] <= 3e-3 * scale and s["cos"] >= 1.0 - 1e-5 * scale * scale, (what, s)


def _ip2p_scale(guidance):
    """v = u + g (cd - u) carries the three predictions' errors with weight |1 - g| + g; v = u + g (cd - u) + s (cd - e1) with
    |1 - g| + g + 2 s.  The ratio of the two, root-mean-square over the frames' guidance ramp: 1.84 for g = 1 .. 3 over 4 frames and
    s = 1.5."""
    g = guidance.flatten().double()
    two = (1.0 - g).abs() + g
    return float(((two + 2.0 * IGS).pow(2).mean() / two.pow(2).mean()).sqrt())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("with_cn", [True, False])
@torch.no_grad()
def test_fused_multistep_loop_matches_oracle_loop(with_cn, dtype):
    kw = _kw(with_cn=with_cn)
    c = kw["multistep"]
    assert float(c[0]) == 0.0 and float(c[STEPS - 1]) == 0.0 and bool((c[1:STEPS - 1] > 0).all())      # steps 1..4 are second order
    graph, loop = _run(dtype, kw, with_cn, graph=True)
    eager, _ = _run(dtype, kw, with_cn, graph=False)
    assert torch.equal(graph, eager), "graph replay must equal eager launches"
    _check(graph, _oracle(dtype, with_cn), dtype, "6-step 2M fused loop vs the oracle loop")
    if dtype == torch.float16:
        split, _ = _run(dtype, kw, with_cn, split_cfg=True)
        assert torch.equal(split, graph), "split-CFG branches must reproduce the joint launch"
        euler, _ = _run(dtype, _kw(with_cn=with_cn, order=None), with_cn)
        assert not torch.equal(euler, graph)                        # the sampler is live
        # the history holds the last step's data prediction; that step's sigma_next is 0, so it is the result up to fp32 rounding
        torch.testing.assert_close(loop.x0_hist.reshape(graph.shape), graph, rtol=1e-5, atol=1e-6)


@torch.no_grad()
def test_history_does_not_leak_between_requests():
    """A, B, A on one loop object whose history buffer starts as NaN and is never cleared: step 0 does not read it"""
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    p_unet, p_cn, _, _ = _pair(torch.float16)
    loop = DenoiseLoop(p_unet, p_cn, use_graph=True)
    loop.begin(**_kw(3))                                            # allocates the buffer ...
    loop.x0_hist.fill_(float("nan"))                                # ... which every later begin() leaves as it finds it
    hist = loop.x0_hist
    first = loop.begin(**_kw(3)).run().clone()
    assert loop.x0_hist is hist and bool(torch.isfinite(first).all())
    other = loop.begin(**_kw(4)).run().clone()
    again = loop.begin(**_kw(3)).run().clone()
    assert loop.x0_hist is hist
    assert torch.equal(again, first) and not torch.equal(other, first)
    fresh, _ = _run(torch.float16, _kw(3))
    assert torch.equal(fresh, first)


@torch.no_grad()
def test_order_1_is_the_euler_loop():
    """R = 2: both loops end in request-form kernels with identical statements -- bitwise.  R = 1: the Euler loop ends in the older
    single-request kernel, which is not contraction-free; that pair is held to the oracle tolerance."""
    dtype = torch.float16
    m2, loop = _run(dtype, _kw2((3, 4), order=1))
    assert float(loop.coef_tab.abs().max()) == 0.0
    e2, _ = _run(dtype, _kw2((3, 4), order=None))
    assert torch.equal(m2, e2)
    m1, _ = _run(dtype, _kw(3, order=1))
    e1, _ = _run(dtype, _kw(3, order=None))
    _check(m1, e1, dtype, "order-1 multistep loop vs the Euler loop, R = 1")


@torch.no_grad()
def test_requests_of_one_call_are_independent():
    dtype = torch.float16
    a, _ = _run(dtype, _kw2((3, 4)))
    b, _ = _run(dtype, _kw2((3, 5)))
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    eager, _ = _run(dtype, _kw2((3, 4)), graph=False)
    assert torch.equal(eager, a)


@torch.no_grad()
def test_control_guidance_window_captures_the_unet_only_graph_mid_request(monkeypatch):
    """controlnet_keep = [1, 1, 0, 0, 1, 1]: the UNet-only graph is first captured at step 2, a second-order step whose replay reads the
    data prediction of step 1 -- a capture whose warm-up pass left its own in the history would differ from eager launches."""
    import oracle.scheduler as osched
    dtype = torch.float16
    keep = [1.0, 1.0, 0.0, 0.0, 1.0, 1.0]
    kw = dict(_kw(3), controlnet_keep=keep)
    graph, _ = _run(dtype, kw, graph=True)
    eager, _ = _run(dtype, kw, graph=False)
    assert torch.equal(graph, eager), "two-graph replay must equal eager launches"
    full, _ = _run(dtype, _kw(3))
    assert not torch.equal(full, graph)
    # the oracle's loop body takes its keep list from controlnet_keep(n, start, end), which cannot express a hole: hand it this one
    monkeypatch.setattr(osched, "controlnet_keep", lambda n, *a, **k: list(keep))
    _, _, o_unet, o_cn = _pair(dtype)
    inp = _inputs()
    ref = osched.denoise_loop(o_unet, o_cn, OracleMultistepScheduler(), inp["latents"], inp["image_latents"], inp["encoder_hidden_states"],
                              inp["added_time_ids"], inp["gesture_latents"], inp["guidance_scale"], num_inference_steps=STEPS)
    _check(graph, ref, dtype, "windowed 2M loop (graph) vs the oracle loop")
    _check(eager, ref, dtype, "windowed 2M loop (eager) vs the oracle loop")


@torch.no_grad()
def test_instructpix2pix_multistep_loop_matches_oracle_loop():
    """The CFG-3 combination weighs the networks' fp16 error 1.84 times as heavily as the CFG-2 one (_ip2p_scale), so the fp16 limits
    of the CFG-2 cases are scaled by that: rel-L2 <= 5.5e-3, 1 - cos <= 3.4e-5 (tests/test_denoise_loop_gpu.py holds the Euler loop's
    CFG-3 case to 1e-2 and 1e-4).  Measured: rel-L2 3.07e-3, cos 0.9999953."""
    dtype = torch.float16
    il3, ehs3, ids3 = _ip2p_constants()
    kw = dict(_kw(3), image_latents=il3, encoder_hidden_states=ehs3, added_time_ids=ids3, image_guidance_scale=IGS)
    graph, _ = _run(dtype, kw)
    eager, _ = _run(dtype, kw, graph=False)
    assert torch.equal(graph, eager)
    scale = _ip2p_scale(_inputs()["guidance_scale"])
    assert 1.8 < scale < 1.9
    _check(graph, _oracle(dtype, True, "ip2p"), dtype, "use_instructpix2pix 2M loop vs the oracle loop", scale)


@torch.no_grad()
def test_range_audit_lists_both_outputs_and_changes_no_bit():
    from this_and_that_vdm_amd import audit
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    dtype = torch.float16
    p_unet, p_cn, _, _ = _pair(dtype)
    plain, _ = _run(dtype, _kw(3))
    loop = DenoiseLoop(p_unet, p_cn, use_graph=True)
    with audit.RangeAudit() as a:
        audit.watch(p_unet, "unet")
        audit.watch(p_cn, "controlnet")
        out = loop.begin(**_kw(3)).run().clone()
        rep = a.report()
    assert torch.equal(out, plain)
    ops_seen = {s.split("/")[1].split("#")[0] for s in rep.sites()}
    assert {"cfg_multistep_step", "cfg_multistep_x0"} <= ops_seen and "cfg_euler_step" not in ops_seen, sorted(ops_seen)
    for op in ("cfg_multistep_step", "cfg_multistep_x0"):
        rows = [r for r in rep.rows if r["site"].split("/")[1].split("#")[0] == op]
        assert len(rows) == 1 and rows[0]["record"]["count"] == STEPS * out.numel(), (op, rows)


def test_begin_refuses_coefficients_that_do_not_fit():
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    p_unet, p_cn, _, _ = _pair(torch.float16)
    kw = _kw(3)
    with pytest.raises(ValueError, match="5 coefficients for 6 steps"):
        DenoiseLoop(p_unet, p_cn).begin(**dict(kw, multistep=kw["multistep"][:5]))
    with pytest.raises(ValueError, match=r"multistep\[0\] must be 0"):
        DenoiseLoop(p_unet, p_cn).begin(**dict(kw, multistep=kw["multistep"].flip(0)[1:].repeat(2)[:6]))
