"""Float64 restatement of the mask estimate: THE definition ``InferenceIP2PVideo.estimate_mask`` and the kernels of
csrc/automask.hip are tested against.  numpy only; nothing here touches the GPU.

For a video latent z [T,4,h,w], its condition cond = z / scale_factor, and n draws:
  1  timestep     i0 = strength_to_start(mask_strength, steps)[1], t = timesteps[i0], (ka, kb) = start_coefficients(t);
                  draw d of a chunk sees x_d = ka z + kb N_d                                                   (``noised``)
  2  chunks       consecutive chunks of frames_in_batch frames, no overlap, the last one may be shorter        (``chunks``)
  3  raw map      raw[t,y,x] = 1/(4 n) sum_d sum_c |eps3 - eps2|                                               (``raw_map``)
  4  mean         mu = mean(raw) over the WHOLE video
  5  zero case    mu == 0: soft = 0 everywhere, an empty mask; no NaN, no division
  6  normalise    soft0 = min(raw, r mu) / (r mu), r = clamp_ratio
  7  smooth       (optional) temporal binomial [1,2,1]/4 over the frames of the whole video, edge frames replicated, then the spatial
                  3x3 binomial [1,2,1] x [1,2,1] / 16, edges replicated
  8  threshold    bin = soft > threshold, strict
  9  dilate       mask_latent = max over the (2 dilate + 1)^2 SPATIAL square of bin, zeros outside the frame
  10 image mask   mask [T,8h,8w] = mask_latent with every cell replicated 8x8                                  (``finish``)

``mutate=`` plants one wrong reading of the definition at a time (``FINISH_MUTATIONS`` / ``RAW_MUTATIONS``): tests/test_automask_cpu.py
shows that the inputs of the GPU tests tell every one of them from the definition.  The inputs of the GPU tests are generated here
(``raw_input``, ``eps_input``) so that the CPU test examines exactly what the GPU test runs.
"""
import itertools

import numpy as np

DEFAULTS = dict(n_maps=4, mask_strength=0.5, clamp_ratio=3.0, threshold=0.5, smooth=True, dilate=1)
BAND = 1e-5   # a cell whose soft value is within BAND of the threshold may fall on either side in fp32

FINISH_MUTATIONS = ("temporal_zero_pad", "spatial_zero_pad", "ge", "dilate_first", "per_frame_mean", "per_chunk_mean", "dilate_across_frames")
RAW_MUTATIONS = ("no_quarter", "no_n", "eps3_minus_eps1")


def chunks(T, frames_in_batch):
    """[(start, stop)] of the consecutive chunks."""
    return [(s, min(s + frames_in_batch, T)) for s in range(0, T, frames_in_batch)]


def noised(z, noise, ka, kb):
    return ka * np.asarray(z, np.float64) + kb * np.asarray(noise, np.float64)


def raw_map(eps, mutate=None):
    """eps [n,3,F,4,h,w] (the three branch predictions of n draws, reference layout) -> raw [F,h,w]."""
    eps = np.asarray(eps, np.float64)
    n = eps.shape[0]
    d = np.abs(eps[:, 2] - eps[:, 0 if mutate == "eps3_minus_eps1" else 1]).sum(axis=(0, 2))
    if mutate != "no_quarter":
        d = d / 4.0
    if mutate != "no_n":
        d = d / n
    return d


def _pad(a, axis, zero):
    pad = [(0, 0)] * a.ndim
    pad[axis] = (1, 1)
    return np.pad(a, pad, mode="constant") if zero else np.pad(a, pad, mode="edge")


def _binomial(a, axis, zero=False):
    p = _pad(a, axis, zero)
    n = a.shape[axis]
    sl = lambda o: tuple(slice(o, o + n) if ax == axis else slice(None) for ax in range(a.ndim))
    return (p[sl(0)] + 2.0 * p[sl(1)] + p[sl(2)]) / 4.0


def smooth3(soft0, mutate=None):
    s = _binomial(soft0, 0, zero=mutate == "temporal_zero_pad")
    s = _binomial(s, 1, zero=mutate == "spatial_zero_pad")
    return _binomial(s, 2, zero=mutate == "spatial_zero_pad")


def dilate_max(a, d, frames=False):
    """max over the (2d+1)^2 spatial square (``frames``: also over 2d+1 frames - a planted error), zeros outside."""
    if d == 0:
        return a.copy()
    T, h, w = a.shape
    dt = d if frames else 0
    p = np.pad(a, ((dt, dt), (d, d), (d, d)), mode="constant")
    out = np.zeros_like(a)
    for k, i, j in itertools.product(range(2 * dt + 1), range(2 * d + 1), range(2 * d + 1)):
        out = np.maximum(out, p[k:k + T, i:i + h, j:j + w])
    return out


def finish(raw, clamp_ratio=3.0, threshold=0.5, smooth=True, dilate=1, mutate=None, chunk=2):
    """Steps 4-10 -> dict(mu, soft, bin, mask_latent, mask), float64 (the 0 / 1 maps too)."""
    raw = np.asarray(raw, np.float64)
    T, h, w = raw.shape
    if mutate == "per_frame_mean":
        mu = raw.mean(axis=(1, 2), keepdims=True)
    elif mutate == "per_chunk_mean":
        mu = np.concatenate([np.full((b - a, 1, 1), raw[a:b].mean()) for a, b in chunks(T, chunk)], 0)
    else:
        mu = np.full((1, 1, 1), raw.mean())
    cap = clamp_ratio * mu
    ok = cap > 0
    soft = np.where(ok, np.minimum(raw, cap) / np.where(ok, cap, 1.0), 0.0)
    if smooth:
        soft = smooth3(soft, mutate)
    if mutate == "dilate_first":   # (max commutes with a threshold, so the masks agree: what this error changes is the soft map it reports)
        soft = dilate_max(soft, dilate)
        b = (soft > threshold).astype(np.float64)
        ml = b
    else:
        b = ((soft >= threshold) if mutate == "ge" else (soft > threshold)).astype(np.float64)
        ml = dilate_max(b, dilate, frames=mutate == "dilate_across_frames")
    return dict(mu=float(raw.mean()), soft=soft, bin=b, mask_latent=ml, mask=np.repeat(np.repeat(ml, 8, axis=1), 8, axis=2))


def mask_to_latent(mask, mode):
    """numpy restatement of ops.mask_to_latent: [T,8h,8w] -> [T,h,w], the mean or the max of every 8x8 cell."""
    T, H, W = mask.shape
    c = mask.reshape(T, H // 8, 8, W // 8, 8)
    return c.max(axis=(2, 4)) if mode == "max" else c.mean(axis=(2, 4))


def near_threshold(soft, threshold, dilate):
    """Cells whose mask_latent may legitimately differ in fp32: within ``dilate`` (Chebyshev, spatial) of a cell with
    |soft - threshold| <= BAND.  -> (number of such band cells, boolean map of the excluded cells)."""
    band = (np.abs(soft - threshold) <= BAND).astype(np.float64)
    return int(band.sum()), dilate_max(band, dilate) > 0


# ---- the inputs of the GPU tests --------------------------------------------------------------------------------------------------------
FINISH_SHAPES = [(T, h, w) for T in (1, 2, 3, 16) for h, w in ((1, 1), (5, 7), (33, 47))]
FINISH_FLAGS = [(s, d, th) for s in (True, False) for d in (0, 1, 2) for th in (0.3, 0.5)]
EPS_CASES = [(s, n) for s in ((1, 1, 1), (3, 5, 7), (2, 9, 13)) for n in (1, 3, 8)]   # ((F,h,w), n)


def _synth(key, shape, kind="normal"):
    from insv2v import synth
    return synth.synth_input("automask." + key, tuple(shape), kind=kind)


def raw_input(T, h, w):
    """A non-negative map with a heavy tail and structure in space and time (fp32 tensor): a log-normal field, three times larger on a
    block of frames / rows / columns - so that both thresholds cut through it, whole frames differ, and the edges matter."""
    r = (0.9 * _synth(f"raw.{T}.{h}.{w}", (T, h, w))).exp()
    r[T // 3:T // 3 + max(1, T // 2), : max(1, h // 2), w // 3:] *= 3.0
    return r.float().contiguous()


def eps_input(F, h, w, n):
    """[n,3,F,4,h,w] fp32 (reference layout)."""
    return _synth(f"eps.{F}.{h}.{w}.{n}", (n, 3, F, 4, h, w)).float().contiguous()


def exact_raw():
    """1 on a rectangle that holds exactly a quarter of the cells of a 2x8x8 map, 0 elsewhere: mu = 1/4, r mu = 3/4, soft0 in {0, 1}, and
    binomial smoothing stays dyadic - every fp32 intermediate is exact.  The corners of the smoothed rectangle are exactly 9/16."""
    r = np.zeros((2, 8, 8), np.float32)
    r[:, 2:6, 2:6] = 1.0
    return r


EXACT_FLAGS = [(s, d, th) for s in (True, False) for d in (0, 1, 2) for th in (0.5, 0.5625)]
