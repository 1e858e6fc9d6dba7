"""Float64 restatement of DPM-Solver++ multistep (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion
Probabilistic Models", data-prediction form, orders 1 and 2M, ODE and SDE) for the tests of insv2v.schedulers.DPMSolverMultistepScheduler.

Written from the paper's update in its D0 / D1 form, not from the product's coefficient table, on the time grid the product states:
DDIM's 'leading' timesteps with offset 1 and alpha_bar_prev = alpha_bar[0] once prev < 0.  ``RefScheduler`` has the surface
oracle.pipelines drives (``timesteps``, ``alphas_cumprod``, a stateful ``step()``), so the GPU tests assign it to ``pipe.scheduler``.
"""
import math

import numpy as np
import torch


def alphas_cumprod(beta_start=0.00085, beta_end=0.012, n=1000):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, n, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def leading_timesteps(n, train=1000, offset=1):
    return [int(k * (train // n)) + offset for k in range(n)][::-1]


class StepOutput:
    def __init__(self, prev_sample, pred_original_sample):
        self.prev_sample = prev_sample
        self.pred_original_sample = pred_original_sample


class RefScheduler:
    """Stateful float64 sampler.  ``noises``: the SDE form's variance noise per executed step (tensors or arrays shaped like the sample)."""

    def __init__(self, n, solver_order=2, sde=False, lower_order_final=True, noises=None):
        self.alphas_cumprod = alphas_cumprod()
        self.ac = self.alphas_cumprod.double().numpy()
        self.num_inference_steps = n
        self.ratio = 1000 // n
        self.timesteps = torch.tensor(leading_timesteps(n), dtype=torch.int64)
        self.order, self.sde, self.lower_order_final, self.noises = solver_order, sde, lower_order_final, noises
        self.reset()

    def reset(self):
        self.x0_last, self.t_last, self.k = None, None, 0

    def _asl(self, t):
        a = self.ac[t] if t >= 0 else self.ac[0]
        alpha, sigma = math.sqrt(a), math.sqrt(1.0 - a)
        return alpha, sigma, math.log(alpha) - math.log(sigma)

    def step64(self, eps, t, x, noise=None):
        """One step on float64 arrays; -> (prev, x0)."""
        alpha_t, sigma_t, lam_t = self._asl(t)
        alpha_s, sigma_s, lam_s = self._asl(t - self.ratio)   # s: the time stepped to
        x0 = (x - sigma_t * eps) / alpha_t
        h = lam_s - lam_t
        final = self.lower_order_final and self.num_inference_steps < 15 and t == int(self.timesteps[-1])
        d0, d1 = x0, None
        if self.order == 2 and self.x0_last is not None and not final:
            r = (lam_t - self._asl(self.t_last)[2]) / h
            d1 = (x0 - self.x0_last) / r
        if not self.sde:
            prev = sigma_s / sigma_t * x - alpha_s * math.expm1(-h) * d0
            if d1 is not None:
                prev = prev - 0.5 * alpha_s * math.expm1(-h) * d1
        else:
            w = 1.0 - math.exp(-2.0 * h)
            prev = sigma_s / sigma_t * math.exp(-h) * x + alpha_s * w * d0 + sigma_s * math.sqrt(w) * noise
            if d1 is not None:
                prev = prev + 0.5 * alpha_s * w * d1
        self.x0_last, self.t_last = x0, t
        self.k += 1
        return prev, x0

    def step(self, model_output, t, sample):
        """The call oracle.pipelines makes: fp32 tensors in and out, the arithmetic in float64."""
        noise = None
        if self.sde:
            noise = torch.as_tensor(self.noises[self.k]).double().reshape(sample.shape)
        prev, x0 = self.step64(model_output.double(), int(t), sample.double(), noise)
        return StepOutput(prev.to(sample.dtype), x0.to(sample.dtype))


# ---- the closed-form case: data N(mu, s^2) -------------------------------------------------------------------------------------------
MU, S = 1.0, 0.25


def gauss_eps(x, alpha, sigma, mu=MU, s=S):
    """The exact noise prediction for data N(mu, s^2) at (alpha, sigma)."""
    return sigma * (x - alpha * mu) / (alpha * alpha * s * s + sigma * sigma)


def gauss_marginal(z, alpha, sigma, mu=MU, s=S):
    """The probability-flow solution through z: x = alpha mu + sqrt(alpha^2 s^2 + sigma^2) z."""
    return alpha * mu + math.sqrt(alpha * alpha * s * s + sigma * sigma) * z


def gauss_trajectory(z, n, solver_order):
    """Float64 restatement run from the marginal at timesteps[0] to the end point; -> (x_end, exact x_end)."""
    ref = RefScheduler(n, solver_order=solver_order)
    a, sg, _ = ref._asl(int(ref.timesteps[0]))
    x = gauss_marginal(z, a, sg)
    for t in ref.timesteps.tolist():
        a, sg, _ = ref._asl(t)
        x, _ = ref.step64(gauss_eps(x, a, sg), t, x)
    a, sg, _ = ref._asl(-1)
    return x, gauss_marginal(z, a, sg)


def rel_rms(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / np.sqrt((b ** 2).mean()))
