"""GPU: several independent requests in one DenoiseLoop (latents [R,F,4,h,w], batch element c * R + r).

Semantics under test: every request of a batched call is what a call of its own gives.  The oracle loop (oracle.scheduler.denoise_loop,
the reference's loop body) is therefore run ONCE PER REQUEST with that request's inputs and the batched result is compared slice by
slice, with the single-request test's limits (tests/test_denoise_loop_gpu.py): TT_F32 inside the north-star tolerance on every
element, fp16 storage rel-L2 <= 3e-3 and cos >= 0.99999.  Shapes are that test's: tiny_vgl, F = 4, 8 x 16 latents, 5 context tokens,
4 steps.  Also: a request's result does not depend on its neighbour (bitwise), graph replay == eager launches, and the two R-request
entry points of the C ABI against plain torch statements (fp32 arithmetic in the same order: bit for bit)."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests.parity_common import assert_north_star, build_pair, err_stats

pytestmark = pytest.mark.gpu

F_, H_, W_, S_, D_, STEPS = 4, 8, 16, 5, 64, 4
IGS = 1.5                                   # image_guidance_scale of the use_instructpix2pix cases (exact in fp32)


@functools.lru_cache(maxsize=None)
def _pair(dtype):
    return build_pair("tiny_vgl", dtype, "cuda:0", True)


@functools.lru_cache(maxsize=None)
def _request(seed: int, kind: str):
    """CPU fp32 inputs of ONE request; every tensor differs between seeds (latents, image latents, contexts, gesture latents,
    time ids, guidance ramp).  kind: cfg2z (CFG 2, all-zero uncond context and image latents: what the pipeline builds),
    cfg2nz (CFG 2, every context non-zero), ip2p (CFG 3 in the reference's order), nocfg (CFG batch 1)."""
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ln = lambda t: torch.nn.functional.layer_norm(t, (S_, D_))
    lat = rn(1, F_, 4, H_, W_) * math.sqrt(700.0 ** 2 + 1)
    img, img_u = rn(1, F_, 4, H_, W_), rn(1, F_, 4, H_, W_) * 0.5
    ctx, ctx_u = ln(rn(1, S_, D_)), ln(rn(1, S_, D_))
    ges = rn(F_, 4, H_, W_)
    z = torch.zeros_like
    il, ehs = {"cfg2z": ([z(img), img], [z(ctx), ctx]), "cfg2nz": ([img_u, img], [ctx_u, ctx]),
               "ip2p": ([img, img, z(img)], [ctx, z(ctx), z(ctx)]), "nocfg": ([img], [ctx])}[kind]
    ids = torch.tensor([[6.0, 100.0 + 20.0 * seed, 0.1]])
    guidance = None if kind == "nocfg" else torch.linspace(1.0, 2.0 + seed % 3, F_).reshape(1, F_, 1, 1, 1)
    return dict(latents=lat, image_latents=il, encoder_hidden_states=ehs, added_time_ids=[ids] * len(il), gesture_latents=ges,
                guidance_scale=guidance)


def _batched(seeds, kind, shared_gesture=False):
    """the requests' tensors in the reference's batch order: CFG class by CFG class (torch.cat([neg, cond]) of batched tensors)"""
    reqs = [_request(s, kind) for s in seeds]
    ncls = len(reqs[0]["image_latents"])
    by_class = lambda name: torch.cat([r[name][c] for c in range(ncls) for r in reqs])
    return dict(latents=torch.cat([r["latents"] for r in reqs]), image_latents=by_class("image_latents"),
                encoder_hidden_states=by_class("encoder_hidden_states"), added_time_ids=by_class("added_time_ids"),
                guidance_scale=None if kind == "nocfg" else torch.cat([r["guidance_scale"] for r in reqs]),
                controlnet_cond=reqs[0]["gesture_latents"] if shared_gesture else torch.stack([r["gesture_latents"] for r in reqs]))


@functools.lru_cache(maxsize=None)
def _oracle(dtype, seed, kind, with_cn, window=False, gesture_seed=None):
    """the reference loop body on ONE request (computed once per distinct request and shared by the tests)"""
    from oracle.scheduler import EulerDiscreteScheduler as OSched, denoise_loop
    _, _, o_unet, o_cn = _pair(dtype)
    o_cn = o_cn if with_cn else None
    r = _request(seed, kind)
    ges = _request(seed if gesture_seed is None else gesture_seed, kind)["gesture_latents"]
    il, ehs, ids = (torch.cat(r[k]) for k in ("image_latents", "encoder_hidden_states", "added_time_ids"))
    with torch.no_grad():
        if kind == "nocfg":                     # denoise_loop always splits a CFG batch: the same body without one
            sched = OSched()
            sched.set_timesteps(STEPS)
            lat = r["latents"]
            for t in sched.timesteps:
                x = torch.cat([sched.scale_model_input(lat, t), il], dim=2)
                down = mid = None
                if o_cn is not None:
                    down, mid = o_cn(x, t, ehs, ids, controlnet_cond=ges, conditioning_scale=1.0, guess_mode=False)
                eps = o_unet(x, t, ehs, ids, down_block_additional_residuals=down, mid_block_additional_residual=mid)
                lat = sched.step(eps, t, lat)
            return lat
        kw = dict(control_guidance_start=0.25, control_guidance_end=0.75) if window else {}
        if kind == "ip2p":
            kw.update(use_instructpix2pix=True, image_guidance_scale=IGS)
        return denoise_loop(o_unet, o_cn, OSched(), r["latents"], il, ehs, ids, ges, r["guidance_scale"], num_inference_steps=STEPS,
                            conditioning_scale=1.0, **kw)


def _begin_kw(seeds, kind, with_cn, shared_gesture=False):
    from this_and_that_vdm_amd.svd.scheduling_euler_discrete import EulerDiscreteScheduler
    sched = EulerDiscreteScheduler()
    sched.set_timesteps(STEPS)
    kw = _batched(seeds, kind, shared_gesture)
    if not with_cn:
        kw["controlnet_cond"] = None
    if kind == "ip2p":
        kw["image_guidance_scale"] = IGS
    return dict(kw, sigmas=sched.sigmas, timesteps=sched.timesteps)


def _run(dtype, seeds, kind, with_cn, graph=True, shared_gesture=False, **extra):
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    p_unet, p_cn, _, _ = _pair(dtype)
    loop = DenoiseLoop(p_unet, p_cn if with_cn else None, use_graph=graph).begin(**_begin_kw(seeds, kind, with_cn, shared_gesture), **extra)
    out = loop.run().clone()
    torch.cuda.synchronize()
    return out, loop


def _check(got, ref, dtype, what):
    s = err_stats(got, ref)
    print(f"{what} ({dtype}):", s)
    if dtype == torch.float32:
        assert_north_star(got.reshape(ref.shape), ref, what)
    else:
        assert s["rel_l2"] <= 3e-3 and s["cos"] >= 0.99999, (what, s)


CASES = {                       # name: (request seeds, kind, with ControlNet)
    "r2_vgl": ((0, 1), "cfg2z", True),                    # all-zero uncond contexts: the zero-context shortcut paths
    "r2_vl": ((0, 1), "cfg2z", False),
    "r3_cfg2": ((0, 1, 2), "cfg2z", True),                # odd R with an even CFG batch
    "r2_ip2p": ((0, 1), "ip2p", True),                    # C = 3, hw = 128 is no multiple of 3: the general Q3 path
    "r2_nocfg": ((0, 1), "nocfg", True),
    "r2_all_contexts_nonzero": ((0, 1), "cfg2nz", True),  # the general paths
}


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", sorted(CASES))
@torch.no_grad()
def test_every_request_matches_its_own_oracle_loop(case, dtype):
    seeds, kind, with_cn = CASES[case]
    got, _ = _run(dtype, seeds, kind, with_cn)
    assert got.shape == (len(seeds), F_, 4, H_, W_)
    for i, seed in enumerate(seeds):
        _check(got[i:i + 1], _oracle(dtype, seed, kind, with_cn), dtype, f"{case}: request {i} of {len(seeds)} vs its own oracle loop")


@torch.no_grad()
def test_shared_gesture_latents_serve_every_request():
    """controlnet_cond [F,4,h,w] (the reference's shape) is the gesture map of every request"""
    dtype = torch.float16
    got, _ = _run(dtype, (0, 1), "cfg2z", True, shared_gesture=True)
    _check(got[0:1], _oracle(dtype, 0, "cfg2z", True), dtype, "shared gesture: request 0")
    _check(got[1:2], _oracle(dtype, 1, "cfg2z", True, gesture_seed=0), dtype, "shared gesture: request 1 (request 0's map)")


@pytest.mark.parametrize("kind", ["cfg2z", "cfg2nz"])
@torch.no_grad()
def test_a_request_does_not_depend_on_its_neighbour(kind):
    """R = 2 twice with request 0 fixed and the other request's latents, image latents, contexts, gesture latents, time ids and guidance
    replaced by other non-zero values (which contexts are all-zero stays as it is: that is launch structure).  Bitwise: a context or a
    GroupNorm segment leaking across requests changes bits."""
    a, _ = _run(torch.float16, (0, 1), kind, True)
    b, _ = _run(torch.float16, (0, 2), kind, True)
    assert torch.equal(a[0], b[0]), "request 0 changed with its neighbour"
    assert not torch.equal(a[1], b[1])


@torch.no_grad()
def test_graph_replay_equals_eager_launches_and_is_reused():
    eager, _ = _run(torch.float16, (0, 1), "cfg2z", True, graph=False)
    first, loop = _run(torch.float16, (0, 1), "cfg2z", True, graph=True)
    assert torch.equal(first, eager), "graph replay must equal eager launches"
    graph = loop._graph
    assert graph is not None
    again = loop.begin(**_begin_kw((0, 1), "cfg2z", True)).run().clone()
    assert loop._graph is graph, "a second begin() with the same shapes must reuse the captured graph"
    assert torch.equal(again, first)
    # other requests through the same graph (static buffers are refilled), then one request on the same loop object: a new graph
    other = loop.begin(**_begin_kw((2, 0), "cfg2z", True)).run().clone()
    assert loop._graph is graph and torch.equal(other[1], _run(torch.float16, (2, 0), "cfg2z", True, graph=False)[0][1])
    one = loop.begin(**_begin_kw((0,), "cfg2z", True)).run().clone()
    assert one.shape == (1, F_, 4, H_, W_) and loop._graph is not graph


@torch.no_grad()
def test_control_guidance_window_matches_per_request_oracle():
    """controlnet_keep = [0, 1, 1, 0]: the UNet-only graph serves the first and last step (reference :611-617).  Limits of the
    single-request window test (tests/test_denoise_loop_gpu.py): rel-L2 <= 1e-2, cos >= 0.9999."""
    from oracle.scheduler import controlnet_keep
    keep = controlnet_keep(STEPS, 0.25, 0.75)
    assert keep == [0.0, 1.0, 1.0, 0.0]
    got, loop = _run(torch.float16, (0, 1), "cfg2z", True, controlnet_keep=keep)
    assert loop._graph is not None and loop._graph_off is not None
    eager, _ = _run(torch.float16, (0, 1), "cfg2z", True, graph=False, controlnet_keep=keep)
    assert torch.equal(got, eager)
    for i in range(2):
        s = err_stats(got[i:i + 1], _oracle(torch.float16, i, "cfg2z", True, window=True))
        print(f"windowed loop, request {i} vs oracle:", s)
        assert s["rel_l2"] <= 1e-2 and s["cos"] >= 0.9999, s
    assert not torch.equal(got, _run(torch.float16, (0, 1), "cfg2z", True)[0])


@torch.no_grad()
def test_guess_mode_without_cfg_and_latent_replacement_per_request():
    """guess_mode (logspace residual scales) is live at R = 2 without CFG and refused with CFG; overwriting ONE request's latents between
    two steps (what the pipeline does with a callback's return value) changes that request only."""
    from this_and_that_vdm_amd.svd.denoise import DenoiseLoop
    p_unet, p_cn, _, _ = _pair(torch.float16)
    plain, _ = _run(torch.float16, (0, 1), "nocfg", True)
    guess, _ = _run(torch.float16, (0, 1), "nocfg", True, guess_mode=True)
    assert not torch.equal(plain[0], guess[0]) and not torch.equal(plain[1], guess[1])
    single = DenoiseLoop(p_unet, p_cn).begin(**_begin_kw((1,), "nocfg", True), guess_mode=True).run().clone()
    s = err_stats(guess[1:2], single)
    assert s["rel_l2"] <= 3e-3 and s["cos"] >= 0.99999, s
    with pytest.raises(NotImplementedError, match="guess_mode"):
        DenoiseLoop(p_unet, p_cn).begin(**_begin_kw((0, 1), "cfg2z", True), guess_mode=True)
    with pytest.raises(NotImplementedError, match="split_cfg"):
        DenoiseLoop(p_unet, p_cn, split_cfg=True).begin(**_begin_kw((0, 1), "cfg2z", True))
    ref, _ = _run(torch.float16, (0, 1), "cfg2z", True)
    loop = DenoiseLoop(p_unet, p_cn).begin(**_begin_kw((0, 1), "cfg2z", True))
    loop.step()
    cur = loop.result()
    assert cur.shape == (2, F_, 4, H_, W_)
    new = cur.clone()
    new[1] *= 0.5
    loop.latents.copy_(new.reshape(loop.latents.shape))
    out = loop.run().clone()
    assert torch.equal(out[0], ref[0]) and not torch.equal(out[1], ref[1])


def test_more_batch_elements_than_the_cap_are_refused_before_any_launch():
    from this_and_that_vdm_amd.svd import denoise
    p_unet, p_cn, _, _ = _pair(torch.float16)
    cap = denoise.MAX_BATCH
    assert cap >= 8                                         # R = 4 with CFG 2 must fit
    for nr, c in ((cap + 1, 1), (cap // 2 + 1, 2)):
        loop = denoise.DenoiseLoop(p_unet, p_cn)
        b = nr * c
        with pytest.raises(ValueError, match=f"cap is {cap}"):
            # CPU tensors: nothing of them may reach a kernel
            loop.begin(latents=torch.zeros(nr, F_, 4, H_, W_), image_latents=torch.zeros(b, F_, 4, H_, W_),
                       encoder_hidden_states=torch.zeros(b, S_, D_), added_time_ids=torch.zeros(b, 3),
                       guidance_scale=torch.ones(1, F_, 1, 1, 1) if c > 1 else None, sigmas=torch.ones(STEPS + 1),
                       timesteps=torch.ones(STEPS), controlnet_cond=torch.zeros(F_, 4, H_, W_))
        assert loop._key is None and not loop._static
    with pytest.raises(ValueError, match="CFG batch"):
        denoise.DenoiseLoop(p_unet, p_cn).begin(**dict(_begin_kw((0, 1, 2), "cfg2z", True), latents=torch.zeros(4, F_, 4, H_, W_)))
    with pytest.raises(ValueError, match="guidance_scale"):
        denoise.DenoiseLoop(p_unet, p_cn).begin(**dict(_begin_kw((0, 1), "cfg2z", True), guidance_scale=torch.ones(3, F_, 1, 1, 1)))
    with pytest.raises(ValueError, match="controlnet_cond"):
        denoise.DenoiseLoop(p_unet, p_cn).begin(**dict(_begin_kw((0, 1), "cfg2z", True), controlnet_cond=torch.zeros(3, F_, 4, H_, W_)))


# ---- the two entry points against plain torch (fp32, same order of operations: bit for bit) -------------------------------------------
R3, F3, H3, W3 = 3, 3, 3, 5                                  # h * w = 15: odd


def _glue_inputs(cfg):
    g = torch.Generator().manual_seed(77 + cfg)
    lat = torch.randn(R3, F3, 4, H3, W3, generator=g) * 300.0
    img = torch.randn(R3 * cfg, F3, 4, H3, W3, generator=g)
    cond = torch.randn(R3, F3, 4, H3, W3, generator=g)
    eps = torch.randn(R3 * cfg, F3, 4, H3, W3, generator=g)
    sig = torch.tensor([700.0, 123.456, 17.25, 0.0])
    return lat, img, cond, eps, sig


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("cfg", [1, 2, 3])
def test_prep_model_input_requests_equals_torch(cfg, dtype):
    from this_and_that_vdm_amd import ops
    lat, img, cond, _, sig = _glue_inputs(cfg)
    step, cpad = 1, 16
    sg = sig[step]
    c_in = 1.0 / torch.sqrt(sg * sg + 1.0)
    for cond_t in (None, cond[1], cond):                   # no gesture latents, shared [F,4,h,w], per request [R,F,4,h,w]
        x = ops.prep_model_input_requests(lat.cuda(), img.cuda(), None if cond_t is None else cond_t.cuda(), sig.cuda(), step, R3, cfg,
                                          F3, H3, W3, cpad, dtype)
        got = x.cpu().view(cfg, R3, F3, H3, W3, cpad)       # batch element c * R + r
        want = torch.zeros(cfg, R3, F3, 4 * 3, H3, W3)
        want[:, :, :, 0:4] = (lat * c_in)[None]
        want[:, :, :, 4:8] = img.view(cfg, R3, F3, 4, H3, W3)
        if cond_t is not None:
            want[:, :, :, 8:12] = (cond_t if cond_t.dim() == 5 else cond_t[None].expand(R3, -1, -1, -1, -1))[None]
        assert torch.equal(got[..., :12], want.permute(0, 1, 2, 4, 5, 3).to(dtype)), (cfg, dtype, None if cond_t is None else cond_t.dim())
        assert float(got[..., 12:].float().abs().max()) == 0.0
        if dtype == torch.float32:
            # the scheduler's own statement divides by sqrt(sigma^2 + 1) instead of multiplying by its reciprocal: <= 1 ulp apart
            ref = lat / ((sg ** 2 + 1) ** 0.5)
            g0 = got[0, ..., :4].permute(0, 1, 4, 2, 3)
            lo, hi = torch.nextafter(ref, torch.full_like(ref, -math.inf)), torch.nextafter(ref, torch.full_like(ref, math.inf))
            assert bool(((g0 >= lo) & (g0 <= hi)).all())


@pytest.mark.parametrize("cfg", [1, 2, 3])
def test_cfg_euler_step_requests_equals_torch(cfg):
    from this_and_that_vdm_amd import ops
    lat, _, _, eps, sig = _glue_inputs(cfg)
    step = 1
    sg, sn = sig[step], sig[step + 1]
    c_out, c_skip = -sg / torch.sqrt(sg * sg + 1.0), 1.0 / (sg * sg + 1.0)
    e = eps.view(cfg, R3, F3, 4, H3, W3)
    eps_tok = eps.permute(0, 1, 3, 4, 2).reshape(-1, 4).contiguous().cuda()
    g_all = torch.linspace(1.0, 3.0, F3).reshape(1, F3)
    g_req = torch.stack([torch.linspace(1.0, 2.0 + r, F3) for r in range(R3)])
    for guidance in ((None,) if cfg == 1 else (g_all, g_req)):
        if cfg == 1:
            v = e[0]
        else:
            g = guidance.reshape(-1, F3, 1, 1, 1)
            if cfg == 2:
                u, cd = e[0], e[1]
                v = u + g * (cd - u)
            else:
                e1, cd, u = e[0], e[1], e[2]
                v = u + g * (cd - u) + IGS * (cd - e1)
        x0 = v * c_out + lat * c_skip
        want = lat + (lat - x0) / sg * (sn - sg)
        got = lat.clone().cuda()
        ops.cfg_euler_step_requests(eps_tok, got, None if guidance is None else guidance.cuda(), sig.cuda(), step, R3, cfg, F3, H3, W3,
                                    IGS if cfg == 3 else None)
        assert torch.equal(got.cpu(), want), (cfg, None if guidance is None else tuple(guidance.shape))
    if cfg == 3:
        with pytest.raises(ValueError):
            ops.cfg_euler_step_requests(eps_tok, lat.clone().cuda(), g_all.cuda(), sig.cuda(), step, R3, 3, F3, H3, W3)


def test_entry_points_refuse_bad_arguments_with_tt_einval():
    from this_and_that_vdm_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")      # refused before any launch: never read or written
    p = buf.data_ptr()
    EINVAL = -1

    def prep(lat=p, img=p, cond=None, per=0, sig=p, step=0, nr=2, cfg=2, f=2, h=2, w=2, cpad=8, x=p, dtype=2):
        return lib.tt_prep_model_input_requests(lat, img, cond, per, sig, step, nr, cfg, f, h, w, cpad, x, dtype, None)

    def euler(eps=p, ld=4, lat=p, g=p, per=0, igs=0.0, sig=p, step=0, nr=2, cfg=2, f=2, h=2, w=2):
        return lib.tt_cfg_euler_step_requests(eps, ld, lat, g, per, C.c_float(igs), sig, step, nr, cfg, f, h, w, None)

    bad_prep = [dict(lat=None), dict(img=None), dict(sig=None), dict(x=None), dict(nr=0), dict(cfg=0), dict(cfg=4), dict(f=0), dict(h=0),
                dict(w=-1), dict(step=-1), dict(cpad=4), dict(cpad=12), dict(cond=p, cpad=8), dict(per=2), dict(dtype=3)]
    for kw in bad_prep:
        assert prep(**kw) == EINVAL, kw
        assert b"tt_prep_model_input_requests" in lib.tt_last_error()
    bad_euler = [dict(eps=None), dict(lat=None), dict(sig=None), dict(nr=0), dict(cfg=0), dict(cfg=4), dict(f=0), dict(h=0), dict(w=0),
                 dict(ld=3), dict(step=-1), dict(per=2), dict(cfg=3, g=None)]
    for kw in bad_euler:
        assert euler(**kw) == EINVAL, kw
        assert b"tt_cfg_euler_step_requests" in lib.tt_last_error()
    assert float(buf.abs().max()) == 0.0
