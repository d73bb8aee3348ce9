"""CPU: DPMSolverMultistepScheduler (DPM-Solver++ 2M on the SVD schedule) -- the schedule is the Euler class's bit for bit, the step
coefficients, order 1 == Euler bit for bit, order 2 against the paper's formula in fp64 under a derived per-element bound, the
convergence order on an analytic Gaussian denoiser, from_config, and the refusals of tt_cfg_multistep_step_requests (answered before
any launch, so the library needs no device for them)."""
import ctypes as C
import json
import math
import os
import re

import pytest
import torch

from tests.multistep_reference import (coefficients, gaussian_denoiser_run, gaussian_exact, published_step, published_x0)
from this_and_that_vdm_amd.svd import DPMSolverMultistepScheduler, EulerDiscreteScheduler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.mark.parametrize("n", [1, 2, 3, 25])
def test_schedule_is_the_euler_schedule_bit_for_bit(n):
    e, m = EulerDiscreteScheduler(), DPMSolverMultistepScheduler()
    assert torch.equal(torch.as_tensor(e.init_noise_sigma), torch.as_tensor(m.init_noise_sigma))
    e.set_timesteps(n)
    m.set_timesteps(n)
    assert m.sigmas.dtype == torch.float32 and torch.equal(e.sigmas, m.sigmas) and torch.equal(e.timesteps, m.timesteps)
    assert torch.equal(torch.as_tensor(e.init_noise_sigma), torch.as_tensor(m.init_noise_sigma))
    x = torch.randn(2, 3, 4, generator=torch.Generator().manual_seed(n)) * 700.0
    assert torch.equal(e.scale_model_input(x, e.timesteps[0]), m.scale_model_input(x, m.timesteps[0]))
    assert DPMSolverMultistepScheduler.order == 1 and m.num_inference_steps == n


@pytest.mark.parametrize("n", [1, 2, 3, 25])
def test_multistep_coefficients(n):
    m = DPMSolverMultistepScheduler()
    m.set_timesteps(n)
    c = m.multistep_coefficients
    assert c.shape == (n,) and c.dtype == torch.float32
    assert float(c[0]) == 0.0 and float(c[n - 1]) == 0.0
    sig = [float(s) for s in m.sigmas]                                       # the fp32 sigmas as doubles
    for i in range(1, n - 1):
        want = torch.tensor(math.log(sig[i] / sig[i + 1]) / (2.0 * math.log(sig[i - 1] / sig[i])), dtype=torch.float64).to(torch.float32)
        assert float(c[i]) == float(want) and float(c[i]) > 0.0, i
    if n <= 2:
        assert float(c.abs().max()) == 0.0
    assert torch.equal(c, coefficients(m.sigmas))
    m1 = DPMSolverMultistepScheduler(solver_order=1)
    m1.set_timesteps(n)
    assert m1.multistep_coefficients.shape == (n,) and float(m1.multistep_coefficients.abs().max()) == 0.0
    for bad in (0, 3, "2", True):
        with pytest.raises(NotImplementedError, match="solver_order"):
            DPMSolverMultistepScheduler(solver_order=bad)


def test_order_1_step_is_the_euler_step_bit_for_bit():
    g = torch.Generator().manual_seed(7)
    e, m = EulerDiscreteScheduler(), DPMSolverMultistepScheduler(solver_order=1)
    e.set_timesteps(6)
    m.set_timesteps(6)
    xe = xm = torch.randn(2, 3, 4, 5, 7, generator=g) * e.init_noise_sigma
    for t in e.timesteps:
        v = torch.randn(xe.shape, generator=g)
        oe, om = e.step(v, t, xe), m.step(v, t, xm)
        assert torch.equal(oe.prev_sample, om.prev_sample) and torch.equal(oe.pred_original_sample, om.pred_original_sample)
        assert torch.equal(om[0], oe.prev_sample)
        xe, xm = oe.prev_sample, om.prev_sample
    assert bool(torch.isfinite(xm).all())


def _step_bound(v, x, x0, hist, sigma, sigma_next, c):
    """Per-element bound on |fp32 step - exact step| for one update whose inputs (v, x, hist, sigma, sigma_next) are the fp32 values
    the step received.  u = 2^-24; every fp32 operation returns its exact result times (1 + d), |d| <= u; first order in u, with a
    factor 1.01 over the whole for the O(u^2) terms.  Magnitudes are taken from the fp64 values.

      c_out = -s / sqrt(s*s + 1)      square, add, sqrt (halves what it is given, adds u), divide:   relative 3u
      c_skip = 1 / (s*s + 1)          square, add, divide:                                          relative 3u
      t1 = v * c_out                  relative 4u
      t2 = x * c_skip                 relative 4u   (the host step divides x by (s*s + 1) instead: relative 3u, covered)
      x0 = t1 + t2                    E0 = 5u (|t1| + |t2|)
      diff = x0 - hist                E0 + u A,                      A = |x0| + |hist|
      prod = c * diff                 |c| (E0 + u A) + 2u |c| A      (c itself is the exact ratio rounded to fp32: relative u)
      D = x0 + prod                   E_D = E0 (1 + |c|) + 3u |c| A + u (|x0| + |c| A)
      s1 = x - D                      E_D + u B,                     B = |x| + |D|,  |D| <= |x0| + |c| A
      q = s1 / s                      (E_D + 2u B) / s
      dt = s_next - s                 relative u
      m = q * dt                      rho (E_D + 2u B) + 2u rho B,   rho = |s_next - s| / s
      x' = x + m                      E = rho E_D + 5u rho B + u |x|
    The fp64 side's own rounding (2^-53 relative, on values of at most a few thousand) is below 1e-12 and is ignored."""
    sq = sigma * sigma + 1.0
    t1, t2 = v.double().abs() * sigma / math.sqrt(sq), x.double().abs() / sq
    e0 = 5.0 * U * (t1 + t2)
    a = x0.abs() + hist.double().abs()
    ca = abs(c)
    e_d = e0 * (1.0 + ca) + 3.0 * U * ca * a + U * (x0.abs() + ca * a)
    b = x.double().abs() + x0.abs() + ca * a
    rho = abs(sigma_next - sigma) / sigma
    return 1.01 * (rho * e_d + 5.0 * U * rho * b + U * x.double().abs())


def test_order_2_step_matches_the_published_form_within_the_derived_bound():
    """Six steps from |x| ~ 700; every step's fp32 result against the paper's update evaluated in fp64 on the very inputs the step
    received (its fp32 latents, model output and previous data prediction), under _step_bound -- derived above from the unit roundoff
    and the operation count, before the first run.  The bound is tight enough to tell the samplers apart: on a second-order step the
    first-order update lies outside it."""
    g = torch.Generator().manual_seed(3)
    m = DPMSolverMultistepScheduler()
    n = 6
    m.set_timesteps(n)
    x = torch.randn(2, 3, 4, 5, 7, generator=g) * m.init_noise_sigma
    assert 500.0 < float(x.abs().mean()) < 700.0 and float(x.abs().max()) > 1400.0
    sig = [float(s) for s in m.sigmas]
    hist = None
    second = 0
    for i, t in enumerate(m.timesteps):
        v = torch.randn(x.shape, generator=g)
        out = m.step(v, t, x)
        x0 = published_x0(v, x, sig[i])
        two = 1 <= i <= n - 2
        want = published_step(x, x0, hist, sig[i], sig[i + 1], sig[i - 1] if two else None, second_order=two)
        c = float(m.multistep_coefficients[i])
        assert (c != 0.0) == two
        h0 = hist if two else torch.zeros_like(x)
        bound = _step_bound(v, x, x0, h0, sig[i], sig[i + 1], c)
        err = (out.prev_sample.double() - want).abs()
        print(f"step {i}: max err {float(err.max()):.3e}  max err/bound {float((err / bound).max()):.3f}  |x| max {float(x.abs().max()):.1f}")
        assert bool((err <= bound).all()), (i, float((err / bound).max()))
        assert bool(((out.pred_original_sample.double() - x0).abs() <= 1.01 * 5.0 * U * (v.double().abs() + x.double().abs())).all())
        if two:
            second += 1
            euler = published_step(x, x0, None, sig[i], sig[i + 1], second_order=False)
            assert float(((euler - want).abs() > bound).double().mean()) > 0.99
        hist, x = out.pred_original_sample, out.prev_sample
    assert second == 4
    with pytest.raises(RuntimeError, match="out of order"):
        m.set_timesteps(n)
        m._init_step_index(m.timesteps[2])
        m.step(v, m.timesteps[2], x)


CASES = [(0.3, 0.2), (0.3, 0.8), (-0.5, 2.0)]


@pytest.fixture(scope="module")
def convergence():
    """RMS error against the exact end point of the probability-flow ODE, {(mu, s): {sampler: {N: err}}}"""
    out = {}
    for k, (mu, s) in enumerate(CASES):
        x_t = mu + math.sqrt(s * s + 700.0 ** 2) * torch.randn(4096, generator=torch.Generator().manual_seed(20 + k))
        exact = gaussian_exact(x_t, mu, s)
        res = {"euler": {}, "2m": {}}
        for n in (12, 25, 50):
            for name, sched in (("euler", EulerDiscreteScheduler()), ("2m", DPMSolverMultistepScheduler())):
                got = gaussian_denoiser_run(sched, n, mu, s, x_t)
                res[name][n] = float((got.double() - exact).pow(2).mean().sqrt())
        print(f"(mu, s) = ({mu}, {s}):", "  ".join(f"N={n} euler {res['euler'][n]:.2e} / 2M {res['2m'][n]:.2e}" for n in (12, 25, 50)),
              f"  25/50 ratio euler {res['euler'][25] / res['euler'][50]:.2f}  2M {res['2m'][25] / res['2m'][50]:.2f}")
        out[(mu, s)] = res
    return out


@pytest.mark.parametrize("case", CASES)
def test_convergence_on_the_analytic_gaussian_denoiser(convergence, case):
    """Solver accuracy on a toy with a closed-form answer; it says nothing about pictures from trained weights."""
    r = convergence[case]
    for n in (12, 25, 50):
        assert r["2m"][n] < r["euler"][n], (case, n, r)
    assert r["2m"][25] < r["euler"][50], (case, r)
    assert r["2m"][25] / r["2m"][50] >= 3.0, (case, r)
    assert r["euler"][25] / r["euler"][50] < 2.5, (case, r)


def test_from_config_round_trip(tmp_path):
    e = EulerDiscreteScheduler(sigma_max=500.0)
    m = DPMSolverMultistepScheduler.from_config(e.config)                  # the diffusers idiom, from a FrozenDict
    assert isinstance(m, DPMSolverMultistepScheduler) and m.config.solver_order == 2 and m.config.lower_order_final is True
    assert all(m.config[k] == v for k, v in e.config.items()) and m.config.sigma_max == 500.0
    back = EulerDiscreteScheduler.from_config(m.config)                    # ... and back: the keys Euler does not take are ignored
    assert type(back) is EulerDiscreteScheduler and dict(back.config) == dict(e.config)
    again = DPMSolverMultistepScheduler.from_config(dict(m.config, solver_order=1, lower_order_final=False))
    assert again.config.solver_order == 1 and again.config.lower_order_final is False
    path = tmp_path / "scheduler_config.json"
    path.write_text(json.dumps(dict(e.config, _class_name="DPMSolverMultistepScheduler", _diffusers_version="0.25.1", trained_betas=None,
                                    algorithm_type="dpmsolver++", solver_order=2)))
    j = DPMSolverMultistepScheduler.from_config(str(path))
    assert dict(j.config) == dict(m.config)
    j.set_timesteps(5)
    m.set_timesteps(5)
    assert torch.equal(j.sigmas, m.sigmas) and torch.equal(j.multistep_coefficients, m.multistep_coefficients)
    for bad in (dict(solver_order=3), dict(beta_schedule="linear"), dict(use_karras_sigmas=False), dict(prediction_type="epsilon"),
                dict(trained_betas=[0.1, 0.2])):
        with pytest.raises(NotImplementedError):
            DPMSolverMultistepScheduler.from_config(dict(e.config, **bad))


def test_entry_point_is_declared_bound_and_refuses_bad_arguments():
    """Header and binding agree; every refusal is TT_EINVAL with the entry point's name in tt_last_error, decided before a launch, so the
    library answers without a device (the operands are then made-up addresses; with a device, a zeroed buffer that stays zero)."""
    from this_and_that_vdm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.tt_abi_version() == 11
    name = "tt_cfg_multistep_step_requests"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "ttvdm.h")).read(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} not declared in ttvdm.h"
    params = [p.strip() for p in m.group(1).split(",")]
    args = _lib.SIGNATURES[name][1]
    assert len(params) == len(args) == 16
    for p, a in zip(params, args):
        want = _lib._vp if "*" in p or "tt_stream_t" in p else {"int32_t": _lib._i32, "int64_t": _lib._i64, "float": _lib._f32}[p.split()[0]]
        assert a is want, (p, a)
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda") if torch.cuda.is_available() else None     # where there is a device, a
    p = 0x1000 if buf is None else buf.data_ptr()                                                         # real buffer no row may touch

    def call(eps=p, ld=4, lat=p, hist=p, g=p, per=0, igs=0.0, sig=p, step=0, coef=p, nr=2, cfg=2, f=2, h=2, w=2):
        return lib.tt_cfg_multistep_step_requests(eps, ld, lat, hist, g, per, C.c_float(igs), sig, step, coef, nr, cfg, f, h, w, None)

    bad = [dict(eps=None), dict(lat=None), dict(hist=None), dict(sig=None), dict(coef=None), dict(nr=0), dict(cfg=0), dict(cfg=4),
           dict(f=0), dict(h=0), dict(w=0), dict(ld=3), dict(step=-1), dict(per=2), dict(cfg=3, g=None)]
    for kw in bad:
        assert call(**kw) == -1, kw                                     # TT_EINVAL
        assert name.encode() in lib.tt_last_error(), kw
    assert buf is None or float(buf.abs().max()) == 0.0


def test_ops_wrapper_names_the_counts():
    from this_and_that_vdm_amd import ops
    z = torch.zeros
    f, h, w = 3, 4, 6
    with pytest.raises(ValueError, match="guidance holds 9 values"):
        ops.cfg_multistep_step_requests(z(8, 4), z(2, f, 4, h, w), z(2, f, 4, h, w), z(3, f), z(3), 0, z(1), 2, 2, f, h, w)
    with pytest.raises(ValueError, match="image_guidance_scale"):
        ops.cfg_multistep_step_requests(z(8, 4), z(2, f, 4, h, w), z(2, f, 4, h, w), z(1, f), z(3), 0, z(1), 2, 3, f, h, w)
    with pytest.raises(ValueError, match="x0_hist"):
        ops.cfg_multistep_step_requests(z(8, 4), z(2, f, 4, h, w), z(1, f, 4, h, w), z(1, f), z(3), 0, z(1), 2, 2, f, h, w)
    with pytest.raises(ValueError, match="coef holds 2 values"):
        ops.cfg_multistep_step_requests(z(8, 4), z(2, f, 4, h, w), z(2, f, 4, h, w), z(1, f), z(3), 0, z(2), 2, 2, f, h, w)
