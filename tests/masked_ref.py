"""Float64 restatement of masked ("edit here") and partial ("edit this much") sampling, for the tests of insv2v_cfg_step_mask, the
schedulers' ``known_coefficients`` and the drivers' ``mask`` / ``strength`` controls.

Definition ("Masked and partial edits").  z: the scaled source latent; n: a fixed noise tensor shaped like the clip [F,4,h,w];
m: a latent-resolution mask [F,h,w] in [0,1], 1 = edit, 0 = keep, broadcast over the 4 channels; a_prev: the cumulative alpha the
step's output lives at.  After the scheduler update of every step

    known      = sqrt(a_prev) z + sqrt(1 - a_prev) n
    latent_out = m prev + (1 - m) known

while the x0 prediction (and so a multistep scheduler's history) stays the model's own.  a_prev is each scheduler's own end point:
alphas_cumprod[prev], and once prev < 0 alphas_cumprod[0] for DDIM / DPM-Solver++ and 1.0 for DDPM.  Strength s in (0, 1] runs the last
n_exec = min(steps, max(1, floor(s steps + 0.5))) steps, from sqrt(a_t) z + sqrt(1 - a_t) n at t = timesteps[steps - n_exec].

Written from that definition on top of tests/multistep_ref.py (its RefScheduler at order 1 of the ODE form is DDIM on this grid), not
from the product's code.  ``MaskedScheduler`` has the surface oracle.pipelines drives, so the GPU tests assign it to ``pipe.scheduler``.
"""
import math

import torch

import multistep_ref as mr


def strength_plan(steps, s):
    """-> (n_exec, start_time)."""
    n_exec = min(steps, max(1, math.floor(s * steps + 0.5)))
    return n_exec, steps - n_exec


def a_prev64(kind, n, t, ac=None):
    """The cumulative alpha (float64) the output of step t of an n-step grid lives at.  kind: "ddim", "ddpm", "dpmsolver++",
    "sde-dpmsolver++"."""
    ac = mr.alphas_cumprod().double().numpy() if ac is None else ac
    prev = t - 1000 // n
    if prev >= 0:
        return float(ac[prev])
    return 1.0 if kind == "ddpm" else float(ac[0])


def known_coefficients(kind, n, t):
    a = a_prev64(kind, n, t)
    return math.sqrt(a), math.sqrt(1.0 - a)


def timesteps(kind, n):
    return mr.leading_timesteps(n, offset=0 if kind == "ddpm" else 1)


def blend(prev, z, n, m, k_src, k_noise):
    """latent_out of the definition; arrays or tensors in float64, m [F,h,w] against [F,4,h,w] (or with a leading batch of 1)."""
    m = m[..., None, :, :]
    return m * prev + (1 - m) * (k_src * z + k_noise * n)


def start_latent(kind, n, s, z, noise):
    """(start_time, initial latent) of strength s: the noise itself at s == 1.0."""
    _, st = strength_plan(n, s)
    if s == 1.0:
        return st, noise
    ac = mr.alphas_cumprod().double().numpy()
    a = float(ac[timesteps(kind, n)[st]])
    return st, math.sqrt(a) * z + math.sqrt(1.0 - a) * noise


class Ddpm64:
    """DDPM ancestral step (fixed_small variance, 'leading' spacing without offset, end point alpha_bar = 1) in float64."""

    def __init__(self, n, noises=None):
        self.alphas_cumprod = mr.alphas_cumprod()
        self.ac = self.alphas_cumprod.double().numpy()
        self.num_inference_steps, self.ratio, self.noises = n, 1000 // n, noises
        self.timesteps = torch.tensor(timesteps("ddpm", n), dtype=torch.int64)
        self.k = 0

    def step64(self, eps, t, x, noise=None):
        prev = t - self.ratio
        a_t, a_p = float(self.ac[t]), float(self.ac[prev]) if prev >= 0 else 1.0
        b_t, b_p = 1 - a_t, 1 - a_p
        cur_a = a_t / a_p
        x0 = (x - math.sqrt(b_t) * eps) / math.sqrt(a_t)
        out = math.sqrt(a_p) * (1 - cur_a) / b_t * x0 + math.sqrt(cur_a) * b_p / b_t * x
        if t > 0:
            out = out + math.sqrt(max(b_p / b_t * (1 - cur_a), 1e-20)) * noise
        self.k += 1
        return out, x0


def inner_scheduler(kind, n, noises=None):
    if kind == "ddpm":
        return Ddpm64(n, noises)
    return mr.RefScheduler(n, solver_order=1 if kind == "ddim" else 2, sde=kind == "sde-dpmsolver++", noises=noises)


class MaskedScheduler:
    """A float64 sampler (``inner_scheduler``) followed by the blend.  z, noise [1,F,4,h,w] and mask [1,F,h,w] tensors (or None: no
    blend, the inner sampler alone).  ``noises``: the variance noise per executed step of a stochastic sampler."""

    def __init__(self, kind, n, z=None, noise=None, mask=None, noises=None):
        self.kind, self.n = kind, n
        self.inner = inner_scheduler(kind, n, noises)
        self.noises = noises
        self.alphas_cumprod, self.timesteps, self.num_inference_steps = self.inner.alphas_cumprod, self.inner.timesteps, n
        self.z, self.noise, self.mask = (None if v is None else torch.as_tensor(v).double() for v in (z, noise, mask))

    def step64(self, eps, t, x, var_noise=None):
        prev, x0 = self.inner.step64(eps, t, x, var_noise)
        if self.mask is not None:
            prev = blend(prev, self.z.reshape(x.shape), self.noise.reshape(x.shape), self.mask.reshape(x.shape[:-3] + x.shape[-2:]),
                         *known_coefficients(self.kind, self.n, t))
        return prev, x0

    def step(self, model_output, t, sample, **unused):
        """The call oracle.pipelines makes: fp32 tensors in and out, the arithmetic in float64."""
        var = None
        if self.noises is not None and self.noises[self.inner.k] is not None:
            var = torch.as_tensor(self.noises[self.inner.k]).double().reshape(sample.shape)
        prev, x0 = self.step64(model_output.double(), int(t), sample.double(), var)
        return mr.StepOutput(prev.to(sample.dtype), x0.to(sample.dtype))


def trajectory(kind, n, eps_fn, z, noise, mask, strength=1.0, noises=None):
    """The whole masked / partial trajectory on float64 arrays with a synthetic model eps_fn(x, t); -> (final latent, list of x0)."""
    s = MaskedScheduler(kind, n, z, noise, mask, noises)
    st, x = start_latent(kind, n, strength, torch.as_tensor(z).double(), torch.as_tensor(noise).double())
    x0s = []
    for t in s.timesteps.tolist()[st:]:
        var = None if noises is None or noises[s.inner.k] is None else torch.as_tensor(noises[s.inner.k]).double()
        x, x0 = s.step64(eps_fn(x, t), t, x, var)
        x0s.append(x0)
    return x, x0s
