"""Float64 / integer restatement of the per-pixel edit strength, for the tests of insv2v_strength_release,
insv2v_cfg_step_release, the pipelines' ``release=`` and the drivers' ``strength_map=``.  Built on tests/masked_ref.py, which is not edited.

Definition.  S: a strength image [T,H,W] fp32 in [0,1]; steps = num_ddim_steps.

    s_c        = the value of latent cell c: the 8x8 pairwise fp32 mean (mode "mean") or the maximum (mode "max") of its pixels - bit for
                 bit what insv2v_mask_to_latent gives
    n_exec(s)  = 0 if s <= 0 or s is NaN, else min(steps, max(1, floor(s * steps + 0.5)))     (s * steps + 0.5 formed in double)
    release_c  = steps - n_exec(s_c)                                                         int32 in [0, steps]
    G          = 0 where S <= 0 or NaN, elsewhere M (the image mask) or 1                     image resolution

and behind the scheduler update of step j - the GLOBAL index in scheduler.timesteps -

    m_eff      = m if release_c <= j else 0            (m: the latent mask at the cell, 1 without a mask)
    latent_out = m_eff prev + (1 - m_eff) (k_src src + k_noise known_noise)

with pred_x0 and eps_out the model's own.  Written from that definition, not from the product's code.

The second half of the file holds the inputs the GPU tests use (``step_case``, ``smap_case``, ``pipe_release``) and a float64 model of the
step with the misreadings the CPU tests plant into it (``step64``), so that the CPU file shows on the GPU file's exact inputs that each
misreading is caught."""
import math

import numpy as np
import torch

import masked_ref as kr


# ---------------------------------------------------------------------------------------------------------------- the release map
def _tree8(v, mode):
    """Pairwise over the last axis of length 8, in the array's own precision: ((0+1)+(2+3))+((4+5)+(6+7)), or the maximum the same way
    (fmax: a NaN loses against a number, as fmaxf)."""
    op = np.fmax if mode == "max" else np.add
    return op(op(op(v[..., 0], v[..., 1]), op(v[..., 2], v[..., 3])), op(op(v[..., 4], v[..., 5]), op(v[..., 6], v[..., 7])))


def cell_values(S, mode):
    """fp32 [N,H,W] -> fp32 [N,H/8,W/8]: per cell the pairwise sum of each pixel row, then of the 8 row sums, times 1/64 (exact) - the
    sum tests/test_masked_gpu.py's ``_np_reduce`` takes in float64, here in fp32 and in the kernel's order, so the bits are the kernel's."""
    S = np.asarray(S, dtype=np.float32)
    n, H, W = S.shape
    cells = S.reshape(n, H // 8, 8, W // 8, 8).transpose(0, 1, 3, 2, 4)   # [n, h, w, row, column]
    with np.errstate(invalid="ignore"):
        v = _tree8(_tree8(cells, mode), mode)
    return v.astype(np.float32) if mode == "max" else (v * np.float32(0.015625)).astype(np.float32)


def n_exec(s, steps, clamp_one=True):
    """Executed steps of fp32 cell strengths ``s`` (any shape): the double formula.  ``clamp_one=False`` plants the misreading without
    the max(1, .)."""
    s = np.asarray(s, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        q = np.floor(s.astype(np.float64) * float(steps) + 0.5)
        q = np.minimum(float(steps), np.maximum(1.0, q) if clamp_one else q)
        return np.where(s > 0, q, 0.0).astype(np.int32)   # s > 0 is False for NaN (and for -0.0)


def release_plan(S, steps, mode, clamp_one=True):
    """Strength image fp32 [N,H,W] -> release map int32 [N,H/8,W/8]."""
    return release_of_cells(cell_values(S, mode), steps, clamp_one)


def release_of_cells(s_c, steps, clamp_one=True):
    return (np.int32(steps) - n_exec(s_c, steps, clamp_one)).astype(np.int32)


def gate(S, M=None, from_cell=None):
    """G fp32 [N,H,W].  ``from_cell`` (a mode) plants the misreading that decides per cell instead of per pixel."""
    S = np.asarray(S, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        on = S > 0
        if from_cell is not None:
            on = np.repeat(np.repeat(cell_values(S, from_cell) > 0, 8, axis=1), 8, axis=2)
    return np.where(on, np.float32(1.0) if M is None else np.asarray(M, dtype=np.float32), np.float32(0.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the step
def effective_mask(m, release, j, like):
    """m_eff [.., F,h,w] float64: m (None: ones) where release <= j, else 0."""
    release = torch.as_tensor(np.asarray(release)).to(torch.int64)
    m = torch.ones(release.shape, dtype=torch.float64) if m is None else torch.as_tensor(m).double().reshape(release.shape)
    return torch.where(release <= j, m, torch.zeros_like(m))


def blend(prev, z, n, m, release, j, k_src, k_noise):
    """latent_out of the definition: float64 tensors, m / release [F,h,w] against [F,4,h,w] (or with a leading batch of 1)."""
    return kr.blend(prev, z, n, effective_mask(m, release, j, prev), k_src, k_noise)


class ReleasedScheduler(kr.MaskedScheduler):
    """masked_ref's float64 sampler followed by the gated blend; the step's global index is the position of t in ``timesteps``.  Has the
    surface oracle.pipelines drives.  ``local_from``: plants the misreading that counts the executed steps instead (j - local_from)."""

    def __init__(self, kind, n, z, noise, mask, release, noises=None, local_from=0):
        super().__init__(kind, n, z, noise, mask, noises)
        self.release, self.local_from = np.asarray(release), local_from
        self._ts = self.timesteps.tolist()

    def step64(self, eps, t, x, var_noise=None):
        prev, x0 = self.inner.step64(eps, t, x, var_noise)
        j = self._ts.index(int(t)) - self.local_from
        rel = self.release.reshape(x.shape[:-3] + x.shape[-2:])
        prev = blend(prev, self.z.reshape(x.shape), self.noise.reshape(x.shape), None if self.mask is None else self.mask.reshape(rel.shape), rel, j,
                     *kr.known_coefficients(self.kind, self.n, t))
        return prev, x0


def trajectory(kind, n, eps_fn, z, noise, mask, release, strength=1.0, noises=None, local_index=False, all_latents=False):
    """The whole released trajectory on float64 tensors with a synthetic model eps_fn(x, t); -> (final latent, list of x0[, latents]).
    ``strength`` decides which steps run, from the noised source below 1.0, as in masked_ref.trajectory; ``noises``: per EXECUTED step."""
    st, x = kr.start_latent(kind, n, strength, torch.as_tensor(z).double(), torch.as_tensor(noise).double())
    s = ReleasedScheduler(kind, n, z, noise, mask, release, noises, local_from=st if local_index else 0)
    x0s, xs = [], []
    for t in s.timesteps.tolist()[st:]:
        var = None if noises is None or noises[s.inner.k] is None else torch.as_tensor(noises[s.inner.k]).double()
        x, x0 = s.step64(eps_fn(x, t), t, x, var)
        x0s.append(x0)
        xs.append(x)
    return (x, x0s, xs) if all_latents else (x, x0s)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
F, H, W = 3, 5, 7   # 4 h w = 140: two 128-thread workgroups, the second partial; an odd w shows a row / column swap


def f32(v):
    return float(np.float32(v))


COEF = (f32(0.83), f32(0.05), f32(0.41), f32(0.3))
SA, S1 = f32(0.8), f32(0.6)
KS, KN = f32(0.93), f32(0.37)
TC, IC = 7.5, 1.5
RELEASE_VALUES = (0, 1, 2, 5)
STEPS_LAUNCHED = (0, 1, 2, 4)


def _rnd(key, shape, kind="normal"):
    from insv2v import synth
    return synth.synth_input(f"strength_map.{key}", tuple(shape), kind=kind)


def step_release():
    """int32 [F,h,w] with the values 0, 1, 2, 5 in a pattern that differs per frame (and per row)."""
    f, y, x = np.meshgrid(np.arange(F), np.arange(H), np.arange(W), indexing="ij")
    return torch.from_numpy(np.asarray(RELEASE_VALUES, dtype=np.int32)[(x + 2 * y + 3 * f + (f * y) % 3) % 4])


def step_case(nbranch, R):
    """The operands of one insv2v_cfg_step_release launch as CPU tensors (fp32, the release map int32)."""
    lat, hist, noise = _rnd("lat", (F, 4, H, W)), _rnd("hist", (F, 4, H, W)), _rnd("noise", (F, 4, H, W))
    ref, dq = _rnd(f"ref{R}", (R, 4, H, W)), _rnd(f"dq{R}", (F - R, 4, H, W))
    e = _rnd("eps3", (3, F, 4, H, W)) if nbranch == 3 else _rnd("eps0", (F, 4, H, W))
    eps_in = e.permute(0, 1, 3, 4, 2).contiguous() if nbranch == 3 else e
    mask = (_rnd("mask", (F, H, W), "uniform") + 0.5).clamp(0.0, 1.0).contiguous()   # soft, with exact zeros and ones
    return dict(lat=lat, hist=hist, noise=noise, ref=ref, dq=dq, e=e, eps_in=eps_in, mask=mask, src=_rnd("src", (F, 4, H, W)),
                kn=_rnd("kn", (F, 4, H, W)), release=step_release())


MISREADINGS = ("lt", "gate_x0", "ignore_mask", "channel_index")


def step64(o, *, nbranch, correct, c_hist, noise, step, masked=True, misreading=None):
    """Float64 model of one launch: CFG combine, correction, update (the statement of tests/test_multistep_gpu.py's ``_step_ref64``),
    then the gated blend.  -> (eps, x0, latent_out).  ``misreading``: one of MISREADINGS, planted."""
    e, lat = o["e"].double(), o["lat"].double()
    if nbranch == 3:
        e = e[0] + IC * (e[1] - e[0]) + TC * (e[2] - e[1])
    if correct:
        ref = o["ref"].double()
        R = ref.shape[0]
        d = (lat[:R] - SA * ref) / S1 - e[:R]
        q = d.mean(0, keepdim=True) if correct == 1 else o["dq"].double()
        e = torch.cat([e[:R] + d, e[R:] + q], 0)
    x0 = (lat - S1 * e) / SA
    prev = COEF[0] * x0 + COEF[1] * e + COEF[2] * lat
    if c_hist != 0.0:
        prev = prev + c_hist * o["hist"].double()
    if noise is not None:
        prev = prev + COEF[3] * torch.as_tensor(noise).double()
    rel = o["release"].to(torch.int64)
    m = o["mask"].double() if masked else torch.ones(rel.shape, dtype=torch.float64)
    known = KS * o["src"].double() + KN * o["kn"].double()
    if misreading == "channel_index":   # release read at [f,c,y,x] of a [F,h,w] array (wrapped here; the kernel would read past its end)
        flat = rel.reshape(-1)
        idx = torch.arange(F * 4 * H * W).reshape(F, 4, H, W) % flat.numel()
        open_ = flat[idx] <= step
    else:
        open_ = ((rel < step) if misreading == "lt" else (rel <= step))[:, None].expand(F, 4, H, W)
    m4 = (torch.ones_like(m) if misreading == "ignore_mask" else m)[:, None].expand(F, 4, H, W)
    m_eff = torch.where(open_, m4, torch.zeros_like(m4))
    out = m_eff * prev + (1 - m_eff) * known
    if misreading == "gate_x0":
        x0 = m_eff * x0 + (1 - m_eff) * o["src"].double()
    return e, x0, out


def smap_case(N, HH, WW, steps):
    """A strength image fp32 [N,HH,WW] (numpy) that holds, spread over cells of a random map in [0,1]: the values 0, -0.0, NaN, 1, k/steps
    and one fp32 step either side of (k + 0.5)/steps as whole cells, a cell with a single non-zero pixel and a cell of 64 distinct values -
    and, with it, a soft image mask of the same shape."""
    S = _rnd(f"smap.{N}.{HH}.{WW}", (N, HH, WW), "uniform").abs().clamp(0.0, 1.0).numpy().astype(np.float32)
    S[S < 0.2] = 0.0                                        # a fifth of the pixels is untouched: the gate is not trivially one
    cells = [(n, y, x) for n in range(N) for y in range(HH // 8) for x in range(WW // 8)]
    ks = sorted({0, steps // 2, steps - 1})                 # (three k of each kind: the maps have 30 cells, 20 steps would ask for 86)
    ties = [np.float32((k + 0.5) / steps) for k in ks]
    special = [np.float32(0.0), np.float32(-0.0), np.float32(np.nan), np.float32(1.0)] + [np.float32((k + 1) / steps) for k in ks]
    for v in ties:
        special += [np.nextafter(v, np.float32(0.0), dtype=np.float32), v, np.nextafter(v, np.float32(2.0), dtype=np.float32)]
    single = np.zeros((8, 8), dtype=np.float32)
    single[5, 3] = 0.3                                      # mean 0.3 / 64: n_exec 1 only through the max(1, .); the gate is one pixel
    distinct = (np.arange(64, dtype=np.float32).reshape(8, 8) + 1) / np.float32(97.0)
    blocks = [single, distinct] + [np.full((8, 8), v, dtype=np.float32) for v in special]
    if len(cells) < len(blocks):                            # a small image takes as many as it has cells: the single pixel or the 64 values first
        blocks = blocks[steps % 2:]
    for (n, y, x), b in zip(cells, blocks):
        S[n, 8 * y:8 * y + 8, 8 * x:8 * x + 8] = b
    M = (_rnd(f"smap.mask.{N}.{HH}.{WW}", (N, HH, WW), "uniform") + 0.5).clamp(0.0, 1.0).numpy().astype(np.float32)
    return S, M


def pipe_release(F_, h, w, steps, mid):
    """int32 [1,F,h,w] with the three levels 0 (free from the first step), ``mid`` and ``steps`` (never released), in blocks that differ per frame."""
    f, y, x = np.meshgrid(np.arange(F_), np.arange(h), np.arange(w), indexing="ij")
    return torch.from_numpy(np.asarray((0, mid, steps), dtype=np.int32)[(x // 3 + y // 2 + f) % 3])[None]


START_TIME_CASE = dict(steps=10, start_time=3, mid=6)   # a release value between start_time and steps: shows the loop's i used for j


def eps_model(x, t):
    """A synthetic pointwise model for the float64 trajectories."""
    return torch.tanh(x) * 0.7 + 0.1 + 1e-4 * t


def rel_rms(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())
