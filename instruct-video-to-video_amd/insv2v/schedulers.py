"""DDIM / DDPM schedules as the reference configures them (pl_trainer/inference/inference.py:26-51;
diffusers 0.21.4 DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False) and
DDPMScheduler(clip_sample=False), 'leading' spacing, scaled_linear betas).

Only the per-step SCALAR coefficients are computed on the host (fp32, same operation order as
diffusers); the tensor update runs in insv2v_cfg_step:
    x0   = (x_t - sqrt(1-a_t) eps) / sqrt(a_t)
    prev = c_x0 * x0 + c_eps * eps + c_xt * x_t + c_noise * noise

DPMSolverMultistepScheduler (DPM-Solver++ 2M, Lu et al. 2022, data-prediction form; ODE and SDE) adds one term, c_hist times the x0
prediction of the previous executed step (insv2v_cfg_step_ms).

``strength_to_start`` maps an edit strength in (0, 1] to the number of executed steps / ``start_time`` of a partial edit.
"""
import math

import numpy as np
import torch


class _Schedule:
    def __init__(self, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", num_train_timesteps=1000, **unused):
        if beta_schedule != "scaled_linear":
            raise NotImplementedError(beta_schedule)
        self.num_train_timesteps = num_train_timesteps
        self.betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, dim=0)
        self.num_inference_steps = None
        self.timesteps = None

    def _end_alpha(self):
        """The cumulative alpha a step lands at once prev < 0 (each scheduler's own end point)."""
        return self.final_alpha_cumprod

    def known_coefficients(self, t):
        """-> (k_src, k_noise) = (sqrt(a_prev), sqrt(1 - a_prev)), a_prev the cumulative alpha the output of step ``t`` lives at: what a
        masked step re-noises the source latent with (``known = k_src * z + k_noise * n``, DESIGN.md "Masked and partial edits").
        Computed in float64, handed over as fp32-valued python floats."""
        prev = int(t) - self.num_train_timesteps // self.num_inference_steps
        a_prev = float(self.alphas_cumprod[prev].double()) if prev >= 0 else float(torch.as_tensor(self._end_alpha()).double())
        return float(np.float32(math.sqrt(a_prev))), float(np.float32(math.sqrt(1.0 - a_prev)))

    def start_coefficients(self, t):
        """-> (sqrt(a_t), sqrt(1 - a_t)) as fp32-valued floats: the level a partial edit (strength < 1) starts from at timestep ``t``."""
        a_t = float(self.alphas_cumprod[int(t)].double())
        return float(np.float32(math.sqrt(a_t))), float(np.float32(math.sqrt(1.0 - a_t)))

    def _leading(self, n, offset):
        ratio = self.num_train_timesteps // n
        return torch.from_numpy((np.arange(0, n) * ratio).round()[::-1].copy().astype(np.int64) + offset)


class DDIMScheduler(_Schedule):
    stochastic = False

    def __init__(self, set_alpha_to_one=False, steps_offset=1, clip_sample=False, **kw):
        super().__init__(**kw)
        if clip_sample:
            raise NotImplementedError("clip_sample")
        self.steps_offset = steps_offset
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]

    def set_timesteps(self, n):
        self.num_inference_steps = n
        self.timesteps = self._leading(n, self.steps_offset)

    def coefficients(self, t):
        """-> dict(sqrt_a, sqrt_1ma, coef=(c_x0, c_eps, c_xt, c_noise)) as python floats."""
        prev = t - self.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
        return dict(sqrt_a=float(a_t ** 0.5), sqrt_1ma=float((1 - a_t) ** 0.5),
                    coef=(float(a_prev ** 0.5), float((1 - a_prev) ** 0.5), 0.0, 0.0))


class DDPMScheduler(_Schedule):
    stochastic = True

    def __init__(self, clip_sample=False, **kw):
        super().__init__(**kw)
        if clip_sample:
            raise NotImplementedError("clip_sample")

    def set_timesteps(self, n):
        self.num_inference_steps = n
        self.timesteps = self._leading(n, 0)

    def _end_alpha(self):
        return 1.0

    def coefficients(self, t):
        prev = t - self.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev] if prev >= 0 else torch.tensor(1.0)
        b_t, b_prev = 1 - a_t, 1 - a_prev
        cur_a = a_t / a_prev
        cur_b = 1 - cur_a
        c_noise = 0.0
        if t > 0:
            c_noise = float(torch.clamp(b_prev / b_t * cur_b, min=1e-20) ** 0.5)
        return dict(sqrt_a=float(a_t ** 0.5), sqrt_1ma=float(b_t ** 0.5),
                    coef=(float((a_prev ** 0.5 * cur_b) / b_t), 0.0, float(cur_a ** 0.5 * b_prev / b_t), c_noise))


class DPMSolverMultistepScheduler(_Schedule):
    """DPM-Solver++ multistep, data-prediction form, orders 1 and 2 (2M), as the ODE solver ("dpmsolver++") or its SDE variant
    ("sde-dpmsolver++"), with lower_order_final.

    Time grid and end point are THIS PROJECT'S DDIMScheduler's: 'leading' spacing, steps_offset=1, and alpha_bar_prev = alpha_bar[0]
    once prev < 0.  ``timesteps`` therefore equals DDIM's and order 1 of the ODE form IS DDIM, which ties the sampler to the goldens of
    the unmodified reference.  The grid is a stated choice of this project, not a pin against diffusers' DPMSolverMultistepScheduler
    (diffusers is not available where this was built; its default end point differs).

    With alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma), h = lambda_prev - lambda_t, h_last = lambda_t - lambda of the
    previous executed step, r = h_last / h and E = expm1(-h), the update prev = c_xt x_t + c_x0 x0 + c_hist x0_last + c_noise n has
        ODE  c_xt = sigma_prev / sigma_t            c_x0 = -alpha_prev E (1 + 1/(2r))              c_hist = +alpha_prev E / (2r)          c_noise = 0
        SDE  c_xt = sigma_prev / sigma_t e^-h       c_x0 = alpha_prev (1 - e^-2h) (1 + 1/(2r))     c_hist = -alpha_prev (1 - e^-2h) / (2r)  c_noise = sigma_prev sqrt(1 - e^-2h)
    and order 1 is the same without the 1/(2r) terms.  Order 1 is taken on the first executed step (no history: also the first step
    after start_time > 0), with solver_order=1, and on the last step when lower_order_final and num_inference_steps < 15.
    The scalars are computed in float64 and handed to the kernel as fp32."""

    multistep = True

    def __init__(self, solver_order=2, algorithm_type="dpmsolver++", lower_order_final=True, steps_offset=1, **kw):
        super().__init__(**kw)
        if solver_order not in (1, 2):
            raise NotImplementedError(f"solver_order {solver_order}")
        if algorithm_type not in ("dpmsolver++", "sde-dpmsolver++"):
            raise NotImplementedError(algorithm_type)
        self.solver_order = solver_order
        self.algorithm_type = algorithm_type
        self.lower_order_final = lower_order_final
        self.steps_offset = steps_offset
        self.stochastic = algorithm_type == "sde-dpmsolver++"
        self.final_alpha_cumprod = self.alphas_cumprod[0]

    def set_timesteps(self, n):
        self.num_inference_steps = n
        self.timesteps = self._leading(n, self.steps_offset)

    def _alpha_sigma_lambda(self, a):
        a = float(a)
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        return alpha, sigma, math.log(alpha / sigma)

    def coefficients(self, t, t_last=None):
        """t_last: the timestep of the previous EXECUTED step of this trajectory, None on its first step.
        -> dict(sqrt_a, sqrt_1ma, coef=(c_x0, 0, c_xt, c_noise), c_hist) as python floats; c_hist multiplies that step's x0."""
        prev = t - self.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev] if prev >= 0 else self.final_alpha_cumprod
        _, sigma_t, lam_t = self._alpha_sigma_lambda(a_t)
        alpha_p, sigma_p, lam_p = self._alpha_sigma_lambda(a_prev)
        h = lam_p - lam_t
        last = self.lower_order_final and self.num_inference_steps < 15 and t == int(self.timesteps[-1])
        second = self.solver_order == 2 and t_last is not None and not last
        g = 0.0   # 1 / (2r)
        if second:
            g = h / (2.0 * (lam_t - self._alpha_sigma_lambda(self.alphas_cumprod[t_last])[2]))
        if self.stochastic:
            w = -math.expm1(-2.0 * h)   # 1 - e^-2h
            c_xt, c_x0, c_hist, c_noise = sigma_p / sigma_t * math.exp(-h), alpha_p * w * (1.0 + g), -alpha_p * w * g, sigma_p * math.sqrt(w)
        else:
            e = math.expm1(-h)
            c_xt, c_x0, c_hist, c_noise = sigma_p / sigma_t, -alpha_p * e * (1.0 + g), alpha_p * e * g, 0.0
        f32 = lambda v: float(np.float32(v))
        return dict(sqrt_a=float(a_t ** 0.5), sqrt_1ma=float((1 - a_t) ** 0.5), coef=(f32(c_x0), 0.0, f32(c_xt), f32(c_noise)),
                    c_hist=f32(c_hist) if second else 0.0)


def strength_to_start(strength, steps):
    """Edit strength s in (0, 1] -> (n_exec, start_time): n_exec = min(steps, max(1, floor(s * steps + 0.5))) steps are executed, from
    ``timesteps[start_time]`` = ``timesteps[steps - n_exec]`` on.  s == 1.0 is the full trajectory from pure noise."""
    s = float(strength)
    if not (0.0 < s <= 1.0):   # (also refuses NaN)
        raise ValueError(f"strength must be in (0, 1], not {strength!r}")
    n_exec = min(int(steps), max(1, int(math.floor(s * steps + 0.5))))
    return n_exec, int(steps) - n_exec
