"""DPMSolverMultistepScheduler for the SVD pipelines: DPM-Solver++ multistep, second order ("2M"; Lu et al., "DPM-Solver++: Fast
Solver for Guided Sampling of Diffusion Probabilistic Models", 2022) in the sigma parametrisation alpha = 1, lambda = -ln sigma -- what
diffusers' DPMSolverMultistepScheduler computes with algorithm_type "dpmsolver++", solver_type "midpoint", final_sigmas_type "zero" on
a Karras schedule.  One network evaluation per step, like Euler; the only state is the previous step's data prediction x0.

The schedule is EulerDiscreteScheduler's, bit for bit (this class inherits set_timesteps' arithmetic, init_noise_sigma and
scale_model_input), so ``pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)`` changes the update rule
and nothing else.  The pipelines never call step(): they hand ``multistep_coefficients`` to DenoiseLoop.begin(multistep=...), and the
per-step tensor math runs in tt_cfg_multistep_step_requests (arithmetic and derivation: include/ttvdm.h).  step() is the same update
on the host, for callers that drive a loop of their own.

What this buys is solver accuracy per network evaluation, shown on an analytic denoiser (tests).  Picture quality at fewer
steps on trained This&That weights has not been evaluated by anyone."""
from __future__ import annotations

import math

import torch

from .scheduling_euler_discrete import EulerDiscreteScheduler, EulerDiscreteSchedulerOutput


class DPMSolverMultistepScheduler(EulerDiscreteScheduler):
    order = 1           # network evaluations per step

    def __init__(self, num_train_timesteps: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012,
                 beta_schedule: str = "scaled_linear", prediction_type: str = "v_prediction",
                 interpolation_type: str = "linear", use_karras_sigmas: bool = True, sigma_min: float = 0.002,
                 sigma_max: float = 700.0, timestep_spacing: str = "leading", timestep_type: str = "continuous",
                 steps_offset: int = 1, solver_order: int = 2, lower_order_final: bool = True):
        """The Euler class's arguments (defaults = SVD's shipped scheduler_config.json) and ``solver_order`` 1 or 2.
        ``lower_order_final`` is accepted for config compatibility: sigma_N = 0 makes the final step first order whatever it says."""
        if solver_order not in (1, 2) or isinstance(solver_order, bool):
            raise NotImplementedError(f"solver_order {solver_order!r}: 1 (Euler's update) or 2 (DPM-Solver++ 2M)")
        super().__init__(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
                         prediction_type=prediction_type, interpolation_type=interpolation_type, use_karras_sigmas=use_karras_sigmas,
                         sigma_min=sigma_min, sigma_max=sigma_max, timestep_spacing=timestep_spacing, timestep_type=timestep_type,
                         steps_offset=steps_offset)
        self.config = type(self.config)(self.config, solver_order=int(solver_order), lower_order_final=bool(lower_order_final))
        self.multistep_coefficients = None          # fp32 [N]: c_i of every step, valid after set_timesteps
        self._x0_prev = None

    def set_timesteps(self, num_inference_steps: int, device=None):
        """EulerDiscreteScheduler.set_timesteps, then the step coefficients c_i = h_i / (2 h_{i-1}), h_i = ln(sigma_i / sigma_{i+1}),
        for 1 <= i <= N-2 -- fp64 from the fp32 sigmas, rounded to fp32 -- and 0 at i = 0 (no history) and i = N-1 (sigma_N = 0).
        Resets the history."""
        super().set_timesteps(num_inference_steps, device=device)
        n = int(num_inference_steps)
        sig = [float(s) for s in self.sigmas.cpu()]          # fp32 values, exactly, as Python doubles
        c = [0.0] * n
        if self.config.solver_order == 2:
            for i in range(1, n - 1):
                c[i] = math.log(sig[i] / sig[i + 1]) / (2.0 * math.log(sig[i - 1] / sig[i]))
        self.multistep_coefficients = torch.tensor(c, dtype=torch.float64).to(torch.float32).to(device=device)
        self._x0_prev = None

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, return_dict: bool = True, **_):
        """One update in torch fp32, statement by statement what tt_cfg_multistep_step_requests does after the CFG combination -- except
        that x0 is formed as EulerDiscreteScheduler.step forms it (sample / (sigma^2 + 1); the kernels multiply by the reciprocal, at
        most an ulp away), so that a step with coefficient 0 is that class's step bit for bit."""
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        sample = sample.to(torch.float32)
        sigma, sigma_next = self.sigmas[i], self.sigmas[i + 1]
        x0 = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + sample / (sigma ** 2 + 1)
        c = self.multistep_coefficients[i]
        d = x0
        if float(c) != 0.0:
            if self._x0_prev is None:
                raise RuntimeError("step() out of order: a second-order step needs the data prediction of the step before it")
            d = x0 + c * (x0 - self._x0_prev)
        self._x0_prev = x0
        prev = (sample + (sample - d) / sigma * (sigma_next - sigma)).to(model_output.dtype)
        self._step_index += 1
        if not return_dict:
            return (prev,)
        return EulerDiscreteSchedulerOutput(prev_sample=prev, pred_original_sample=x0)
