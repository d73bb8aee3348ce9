"""Shared statements of the DPM-Solver++ 2M update (a plain module, not a conftest; it holds no text of the reference project):

* published_step(): fp64, in the form the paper prints it (Lu et al., "DPM-Solver++", the multistep second-order data-prediction
  update) with alpha = 1, lambda = -ln sigma: e^{-h} and 1/(2r) -- written from the formula, not from the kernel's statements;
* kernel_step(): the torch fp32 statement of tt_cfg_multistep_step_requests, line for line (include/ttvdm.h);
* coefficients(): c_i = h_i / (2 h_{i-1}) recomputed in fp64 from fp32 sigmas;
* OracleMultistepScheduler: what oracle.scheduler.denoise_loop drives (set_timesteps, timesteps, scale_model_input, step -> tensor),
  so the oracle's loop body runs the new sampler as it stands;
* gaussian_denoiser_run(): the probability-flow ODE on an analytic Gaussian denoiser, whose end point is known in closed form."""
import math

import torch

from oracle.scheduler import EulerDiscreteScheduler as _OracleEuler


def coefficients(sigmas: torch.Tensor, solver_order: int = 2) -> torch.Tensor:
    """fp32 [N] from fp32 sigmas [N + 1] (the last one 0): 0 at i = 0 and i = N - 1, h_i / (2 h_{i-1}) in fp64 elsewhere"""
    s = [float(v) for v in sigmas.detach().cpu().to(torch.float32)]
    n = len(s) - 1
    c = [0.0] * n
    if solver_order == 2:
        for i in range(1, n - 1):
            c[i] = math.log(s[i] / s[i + 1]) / (2.0 * math.log(s[i - 1] / s[i]))
    return torch.tensor(c, dtype=torch.float64).to(torch.float32)


def published_x0(v: torch.Tensor, x: torch.Tensor, sigma: float) -> torch.Tensor:
    """fp64 data prediction of SVD's v-prediction parametrisation: x0 = c_skip x + c_out v"""
    return x.double() / (sigma * sigma + 1.0) - v.double() * sigma / math.sqrt(sigma * sigma + 1.0)


def published_step(x, x0, x0_prev, sigma: float, sigma_next: float, sigma_prev=None, second_order: bool = True):
    """fp64.  lambda = -ln sigma, h = lambda_next - lambda, r = h_prev / h, alpha = 1:
        D  = (1 + 1/(2r)) x0 - (1/(2r)) x0_prev          (second order; first order: D = x0)
        x' = (sigma_next / sigma) x - (e^{-h} - 1) D
    sigma_next == 0: h is infinite, e^{-h} = 0, x' = D."""
    x, x0 = x.double(), x0.double()
    e_mh = 0.0 if sigma_next == 0.0 else math.exp(-(math.log(sigma) - math.log(sigma_next)))
    d = x0
    if second_order:
        h = math.log(sigma) - math.log(sigma_next)
        h_prev = math.log(sigma_prev) - math.log(sigma)
        r = h_prev / h
        d = (1.0 + 1.0 / (2.0 * r)) * x0 - (1.0 / (2.0 * r)) * x0_prev.double()
    return (sigma_next / sigma) * x - (e_mh - 1.0) * d


def kernel_step(eps, lat, hist, guidance, image_guidance, sg, sn, c):
    """eps fp32 [C,R,F,4,h,w] (CFG class by class), lat / hist fp32 [R,F,4,h,w], guidance None or broadcastable [R|1,F,1,1,1],
    sg / sn / c fp32 0-dim tensors.  Returns (new latents, new history); hist is not touched when c == 0."""
    cfg = eps.shape[0]
    if cfg == 3:
        e1, cd, u = eps[0], eps[1], eps[2]
        v = u + guidance * (cd - u) + image_guidance * (cd - e1)
    elif cfg == 2:
        u, cd = eps[0], eps[1]
        v = u + guidance * (cd - u)
    else:
        v = eps[0]
    c_out, c_skip = -sg / torch.sqrt(sg * sg + 1.0), 1.0 / (sg * sg + 1.0)
    x0 = v * c_out + lat * c_skip
    d = x0 + c * (x0 - hist) if float(c) != 0.0 else x0
    return lat + (lat - d) / sg * (sn - sg), x0


class OracleMultistepScheduler(_OracleEuler):
    """the oracle's Euler scheduler with its step() extended by the extrapolated data prediction; step() returns a tensor"""

    def __init__(self, solver_order: int = 2, **cfg):
        super().__init__(**cfg)
        self.solver_order = solver_order
        self.coefs = self._prev_x0 = None

    def set_timesteps(self, num_inference_steps, device=None):
        super().set_timesteps(num_inference_steps, device=device)
        self.coefs = coefficients(self.sigmas, self.solver_order)
        self._prev_x0 = None

    def step(self, model_output, timestep, sample):
        if self._step_index is None:
            self._init_step_index(timestep)
        sample = sample.to(torch.float32)
        i = self._step_index
        sigma = self.sigmas[i]
        pred_x0 = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
        c = float(self.coefs[i])
        d = pred_x0 + c * (pred_x0 - self._prev_x0) if c != 0.0 else pred_x0
        self._prev_x0 = pred_x0
        prev = (sample + (sample - d) / sigma * (self.sigmas[i + 1] - sigma)).to(model_output.dtype)
        self._step_index += 1
        return prev


def gaussian_denoiser_run(scheduler, n: int, mu: float, s: float, x_t: torch.Tensor) -> torch.Tensor:
    """Data ~ N(mu, s^2): the ideal denoiser is x0(x, sigma) = mu + s^2 / (s^2 + sigma^2) (x - mu).  Runs ``scheduler`` (the product
    classes' interface: step().prev_sample) for n steps from x_t at sigma_0, feeding it that denoiser as the v-prediction the step
    consumes (x0 = c_skip x + c_out v  =>  v = (x0 - c_skip x) / c_out, formed in fp64 and rounded to fp32).  The exact end point of the
    probability-flow ODE is gaussian_exact()."""
    scheduler.set_timesteps(n)
    x = x_t.clone()
    for i, t in enumerate(scheduler.timesteps):
        sg = float(scheduler.sigmas[i])
        xd = x.double()
        x0 = mu + s * s / (s * s + sg * sg) * (xd - mu)
        v = ((x0 - xd / (sg * sg + 1.0)) / (-sg / math.sqrt(sg * sg + 1.0))).to(torch.float32)
        x = scheduler.step(v, t, x).prev_sample
    return x


def gaussian_exact(x_t: torch.Tensor, mu: float, s: float, sigma_max: float = 700.0) -> torch.Tensor:
    return mu + (x_t.double() - mu) * s / math.sqrt(s * s + sigma_max * sigma_max)
