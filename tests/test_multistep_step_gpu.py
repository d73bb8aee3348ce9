"""GPU: tt_cfg_multistep_step_requests against the torch fp32 statement of its arithmetic (tests/multistep_reference.kernel_step),
bit for bit: requests 1..3 x CFG batch 1..3, an odd token count (F = 3, 5 x 7), eps rows of stride 8 whose unused columns hold NaN,
guidance absent / [F] / [R,F], coefficient 0 and 0.37.  The history after the call is x0; with coefficient 0 a NaN-filled history is
never read and the latents are tt_cfg_euler_step_requests' bits; one case is larger than one pass of the capped grid."""
import pytest
import torch

from tests.multistep_reference import kernel_step

pytestmark = pytest.mark.gpu

F_, H_, W_ = 3, 5, 7
IGS = 1.5
STEP = 2


def _sigmas():
    from this_and_that_vdm_amd.svd import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(6)
    return s.sigmas


def _inputs(r, cfg, f=F_, h=H_, w=W_, seed=0):
    g = torch.Generator().manual_seed(100 * r + 10 * cfg + seed)
    sig = _sigmas()
    lat = torch.randn(r, f, 4, h, w, generator=g) * float(sig[STEP])
    hist = torch.randn(r, f, 4, h, w, generator=g)
    eps = torch.randn(cfg, r, f, 4, h, w, generator=g)
    return lat, hist, eps, sig


def _tokens(eps, ld):
    """[C,R,F,4,h,w] -> token rows [C*R*F*h*w, ld] of batch element c * R + r; the columns past the four channels hold NaN"""
    rows = eps.permute(0, 1, 2, 4, 5, 3).reshape(-1, 4)
    out = torch.full((rows.shape[0], ld), float("nan"))
    out[:, :4] = rows
    return out.cuda()


def _guidances(r, cfg):
    if cfg == 1:
        return [None]
    g_all = torch.linspace(1.0, 3.0, F_).reshape(1, F_)
    g_req = torch.stack([torch.linspace(1.0, 2.0 + k, F_) for k in range(r)])
    return [g_all, g_req]


@pytest.mark.parametrize("c", [0.0, 0.37])
@pytest.mark.parametrize("cfg", [1, 2, 3])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_step_equals_the_torch_statement_bit_for_bit(r, cfg, c):
    from this_and_that_vdm_amd import ops
    lat, hist, eps, sig = _inputs(r, cfg)
    tok = _tokens(eps, 8)
    assert tok.stride(0) == 8 and bool(torch.isnan(tok[:, 4:]).all())
    coef = torch.tensor([c], dtype=torch.float32)
    for guidance in _guidances(r, cfg):
        g5 = None if guidance is None else guidance.reshape(-1, F_, 1, 1, 1)
        want, x0 = kernel_step(eps, lat, hist, g5, IGS, sig[STEP], sig[STEP + 1], coef[0])
        got = lat.clone().cuda()
        h_dev = (torch.full_like(hist, float("nan")) if c == 0.0 else hist.clone()).cuda()
        ops.cfg_multistep_step_requests(tok, got, h_dev, None if guidance is None else guidance.cuda(), sig.cuda(), STEP, coef.cuda(), r, cfg,
                                        F_, H_, W_, IGS if cfg == 3 else None)
        what = (r, cfg, c, None if guidance is None else tuple(guidance.shape))
        assert torch.equal(h_dev.cpu(), x0), what                         # the history is this step's data prediction
        assert torch.equal(got.cpu(), want), what
        if c == 0.0:
            assert bool(torch.isfinite(got).all()), what                  # the NaN history was not read
            euler = lat.clone().cuda()
            ops.cfg_euler_step_requests(tok, euler, None if guidance is None else guidance.cuda(), sig.cuda(), STEP, r, cfg, F_, H_, W_,
                                        IGS if cfg == 3 else None)
            assert torch.equal(got, euler), what
        else:
            e_want, _ = kernel_step(eps, lat, hist, g5, IGS, sig[STEP], sig[STEP + 1], torch.tensor(0.0))
            assert not torch.equal(want, e_want)                          # the coefficient is live
    if cfg == 3:
        with pytest.raises(ValueError):
            ops.cfg_multistep_step_requests(tok, lat.clone().cuda(), hist.clone().cuda(), _guidances(r, cfg)[0].cuda(), sig.cuda(), STEP,
                                            coef.cuda(), r, 3, F_, H_, W_)


def test_more_elements_than_one_pass_of_the_grid():
    """the launch caps its grid at 2048 blocks of 256 threads = 524288 elements per pass: 3 x 419 x 419 = 526683 take a second pass,
    with a ragged end"""
    from this_and_that_vdm_amd import ops
    h = w = 419
    assert F_ * h * w > 2048 * 256
    lat, hist, eps, sig = _inputs(1, 1, h=h, w=w)
    coef = torch.tensor([0.37], dtype=torch.float32)
    want, x0 = kernel_step(eps, lat, hist, None, IGS, sig[STEP], sig[STEP + 1], coef[0])
    got, h_dev = lat.clone().cuda(), hist.clone().cuda()
    ops.cfg_multistep_step_requests(_tokens(eps, 4), got, h_dev, None, sig.cuda(), STEP, coef.cuda(), 1, 1, F_, h, w)
    assert torch.equal(got.cpu(), want) and torch.equal(h_dev.cpu(), x0)
