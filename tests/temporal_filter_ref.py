"""Float64 restatement of the temporal filter that stabilizes an edit along the source video's optical flow (DESIGN.md section 21;
csrc/temporal_filter.hip holds the kernel, insv2v/temporal_filter.py the host side).  Nothing of the product is imported here.  This
file is the contract.

All frames are [T,3,H,W].  E is the edit, in whatever range it is in; A is the guide, the source video, read as
a = clamp(x * scale + shift, 0, 1) (``SIGNED`` for frames in [-1, 1]).  Parameters: ``radius`` R in 1 .. 4, ``sigma`` > 0 (on [0, 1]
data), ``strength`` s in (0, 1].  For frame t the neighbour offsets are k in (-R .. -1, 1 .. R), in that order; G_{t,k} [2,H,W] is the flow
defined on frame t pointing into frame t + k, U_{t,k} [H,W] its validity (0 or 1; 0 wherever t + k is outside the video).
Per pixel x and neighbour k with U_{t,k}(x) = 1:

    p   = x + G_{t,k}(x);   S(.) = the border-clamped lerp sample at p (clamped) of tests/masktrack_ref.py: ``_taps`` / ``_sample`` as they are
    d2  = (1/3) sum_c (a_t[c](x) - S(a_{t+k}[c]))^2
    w_k = s exp(-d2 / (2 sigma^2))

and per pixel and channel

    out_t[c](x) = E_t[c](x) + (sum_k w_k (S(E_{t+k}[c]) - E_t[c](x))) / (1 + sum_k w_k)

the sums over the valid k in the order above.  A neighbour with U = 0 is SKIPPED, not multiplied by 0: a NaN in a frame nothing valid
reaches cannot leak.  The residual form is deliberate: a pixel without a valid neighbour, and a video that is constant along its
trajectories, come back as out == E bit for bit, through the division.

``filter_video(..., dtype=np.float32)`` restates the kernel's operation order in float32 (without FMA contraction, numpy's exp for the
device's): a = x * scale + shift clamped, the three squares added in channel order and divided by 3, arg = d2 * float32(-1 / (2 sigma^2))
(the factor formed in float64 and rounded once), w = s * exp(arg), num += w * (S - E), den += w, q = num / (1 + den), out = E + q
rounded once to the output dtype.  It only calibrates the bound.

Bound of the kernel, per element, against float64 (never against the kernel):
    4 x the restatement's worst |float32 - float64| on the case's inputs    (4: FMA contraction and the device's expf)
    + sum_k 2^-22 (2 + |arg_k|) w_k |S_k - E_t| / (1 + sum w)               (the rounding of the exponential's argument: arg carries a few
                                                                            roundings of relative 2^-24, exp turns an absolute error of
                                                                            the argument into a relative error of the weight, and a
                                                                            relative error of w_k moves the output by at most this share)
    floored at one rounding of the output dtype (half a unit in the last place of the reference value).
The inputs are seeded by name, so the CPU and the GPU file see the same arrays."""
import functools
import zlib

import numpy as np

import masktrack_ref as mr

SIGNED = (0.5, 0.5)   # the affine of frames in [-1, 1]
ONE = (1.0, 0.0)
DEFAULTS = dict(radius=2, sigma=0.1, strength=1.0)
MARGIN = 4.0
CASES = [(2, 2, 2, 1), (3, 16, 24, 1), (5, 17, 33, 2), (9, 40, 56, 4)]   # (T, H, W, R)
DTYPES = ("f16", "f32")
CASE_SIGMA, CASE_STRENGTH = 0.1, 0.75
MUTATIONS = ("edit_weight", "neg_flow", "t_minus_k", "zero_pad", "nearest", "no_centre", "mul_zero", "no_affine", "chan_sum")
MUTATION_CASES = [CASES[2], CASES[3]]
MIN_DEPARTURE = 10.0   # a planted misreading must miss the reference by at least this many bounds


def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def offsets_of(radius):
    return tuple(range(-radius, 0)) + tuple(range(1, radius + 1))


def stored(a, dtype):
    """The array as the operand holds it: rounded to float16 or float32, returned as float64 (exact)."""
    return np.asarray(a).astype(np.float16 if dtype == "f16" else np.float32).astype(np.float64)


def affine(x, scale_shift, dtype=np.float64):
    s, h = (dtype(v) for v in scale_shift)
    with np.errstate(invalid="ignore"):
        v = np.asarray(x).astype(dtype) * s + h
        return np.where(np.isnan(v), v, np.minimum(np.maximum(v, dtype(0)), dtype(1)))


def rounding(ref, dt):
    """One rounding of the output dtype at the reference value: half a unit in the last place."""
    ref = np.abs(np.asarray(ref, np.float64))
    return np.maximum(ref * 2.0 ** -11, 2.0 ** -25) if dt == "f16" else np.maximum(ref * 2.0 ** -24, 2.0 ** -150)


# ------------------------------------------------------------------------------------------------------------------ the definition
def filter_video(E, A, G, U, offsets, sigma=0.1, strength=1.0, guide_affine=SIGNED, dtype=np.float64, out_dtype=None, mutate=None):
    """E, A [T,3,H,W] as stored, G [K,T,2,H,W], U [K,T,H,W] -> dict(out [T,3,H,W], terms [T,H,W] = the bound's derived term (float64 only),
    n_valid [T,H,W]).  ``out_dtype`` ("f16" / "f32"): the float32 restatement rounds its result to it."""
    assert mutate is None or mutate in MUTATIONS
    f = dtype
    E = np.asarray(E).astype(f)
    a = np.asarray(A).astype(f) if mutate == "no_affine" else affine(A, guide_affine, f)
    wsrc = E if mutate == "edit_weight" else a
    T, _, H, W = E.shape
    G, U = np.asarray(G).astype(f), np.asarray(U)
    if mutate == "neg_flow":
        G = -G
    ys, xs = (v.astype(f) for v in np.mgrid[0:H, 0:W])
    neg_inv = f(np.float32(-1.0 / (2.0 * float(sigma) ** 2))) if f is np.float32 else None
    s = f(strength)
    out, terms, count = np.empty_like(E), np.zeros((T, H, W)), np.zeros((T, H, W), np.int64)
    for t in range(T):
        num, den = np.zeros((3, H, W), f), np.zeros((H, W), f)
        per_k = []
        for i, k in enumerate(offsets):
            tn = t - k if mutate == "t_minus_k" else t + k
            if not 0 <= tn < T:
                continue
            v = U[i, t] > 0.5
            if not v.any() and mutate != "mul_zero":
                continue
            tp = mr._taps(xs + G[i, t, 0], ys + G[i, t, 1], H, W, f, clamp=mutate != "zero_pad")
            smp = lambda P: mr._sample(P, tp, mutate == "nearest")   # noqa: E731
            with np.errstate(invalid="ignore", over="ignore"):
                d = [wsrc[t, c] - smp(wsrc[tn, c]) for c in range(3)]
                d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if mutate != "chan_sum":
                    d2 = d2 / f(3)
                arg = d2 * neg_inv if neg_inv is not None else -d2 / f(2.0 * float(sigma) ** 2)
                w = s * np.exp(arg)
                diff = np.stack([smp(E[tn, c]) - E[t, c] for c in range(3)])
                if mutate == "mul_zero":      # the misreading: every neighbour is read and weighed by U
                    w = w * v.astype(f)
                    num, den = num + w * diff, den + w
                else:                         # the definition: an invalid neighbour contributes nothing, whatever it holds
                    num, den = num + np.where(v, w * diff, f(0)), den + np.where(v, w, f(0))
            count[t] += v
            per_k.append((np.where(v, np.abs(arg), 0.0), np.where(v, w, 0.0), np.where(v, np.abs(diff).max(0), 0.0)))
        with np.errstate(invalid="ignore"):
            if mutate == "no_centre":     # the misreading: the neighbours' weighted mean replaces the pixel
                q = np.where(den > 0, num / np.where(den > 0, den, f(1)), f(0))
            else:
                q = num / (f(1) + den)
            out[t] = np.where(q == 0, E[t], E[t] + q)
        if f is np.float64:
            for aa, ww, dd in per_k:
                with np.errstate(invalid="ignore"):
                    terms[t] += 2.0 ** -22 * (2.0 + aa) * ww * dd / (1.0 + den)
    if out_dtype is not None:
        out = stored(out, out_dtype).astype(f)
    return dict(out=out, terms=terms, n_valid=count)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _texture(rng, H, W, amp, cells):
    return mr._smooth(rng, H, W, amp, cells=cells)


def reach(G, U, offsets, T, H, W):
    """(taps [T,H,W], centre [T,H,W]) of bool: the pixels some VALID neighbour's four clamped taps read, and the pixels that have a
    valid neighbour (whose own guide value is then used)."""
    taps, centre = np.zeros((T, H, W), bool), np.zeros((T, H, W), bool)
    ys, xs = (v.astype(np.float64) for v in np.mgrid[0:H, 0:W])
    for i, k in enumerate(offsets):
        for t in range(T):
            if not 0 <= t + k < T:
                continue
            v = U[i, t] > 0.5
            tp = mr._taps(xs + G[i, t, 0], ys + G[i, t, 1], H, W, np.float64)
            for yy, xx in zip(tp["y"], tp["x"]):
                taps[t + k][yy[v], xx[v]] = True
            centre[t] |= v
    return taps, centre


@functools.lru_cache(maxsize=None)
def case_inputs(T, H, W, R, dt):
    """One GPU case: E, A [T,3,H,W] as stored (A a little beyond [-1, 1] so the clamp acts; the guide smooth enough that the photometric
    weights spread over (0, 1]), smooth seeded G [K,T,2,H,W] of a few pixels, U [K,T,H,W] with holes, whole out-of-video slabs and - from
    8 x 8 up - a rectangle of the middle frame that NO valid neighbour reaches; ``nan_A`` / ``nan_E``: where a NaN may be planted (A: no
    valid tap and no valid neighbour of its own; E: no valid tap - its own output pixel is then NaN, and only that one)."""
    rng = _rng(f"temporal_filter.case.{T}.{H}.{W}.{R}.{dt}")
    offs = offsets_of(R)
    K = len(offs)
    amp = min(3.0, min(H, W) / 8.0)
    G = np.stack([[np.stack([mr._smooth(rng, H, W, amp) + 0.3 * amp * np.sign(k), mr._smooth(rng, H, W, amp) - 0.2 * amp * np.sign(k)])
                   for _ in range(T)] for k in offs]).astype(np.float32).astype(np.float64)
    U = (rng.uniform(0, 1, (K, T, H, W)) > 0.15).astype(np.float64)
    for i, k in enumerate(offs):
        for t in range(T):
            if not 0 <= t + k < T:
                U[i, t] = 0.0
            elif H >= 8:
                y0, x0 = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
                U[i, t, y0:y0 + max(3, H // 4), x0:x0 + max(3, W // 4)] = 0.0
    base = [_texture(rng, H, W, 0.8, 8) for _ in range(3)]
    A = 1.05 * np.stack([[base[c] + _texture(rng, H, W, 0.12, 5) + rng.uniform(-0.03, 0.03, (H, W)) for c in range(3)] for _ in range(T)])
    E = np.stack([[0.8 * base[(c + 1) % 3] + _texture(rng, H, W, 0.15, 3) + rng.uniform(-0.05, 0.05, (H, W)) + 0.1 * ((t * 5) % 3 - 1)
                   for c in range(3)] for t in range(T)])
    if H >= 8:   # a dead rectangle in the middle frame: every neighbour with a tap in it, and every neighbour OF it, is invalid
        t0, y0, y1, x0, x1 = T // 2, H // 3, H // 3 + max(3, H // 4), W // 3, W // 3 + max(3, W // 4)
        ys, xs = (v.astype(np.float64) for v in np.mgrid[0:H, 0:W])
        for i, k in enumerate(offs):
            U[i, t0, y0:y1, x0:x1] = 0.0
            t = t0 - k
            if 0 <= t < T:
                tp = mr._taps(xs + G[i, t, 0], ys + G[i, t, 1], H, W, np.float64)
                hit = np.zeros((H, W), bool)
                for yy, xx in zip(tp["y"], tp["x"]):
                    hit |= (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
                U[i, t][hit] = 0.0
    taps, centre = reach(G, U, offs, T, H, W)
    return dict(E=stored(E, dt), A=stored(A, dt), G=G, U=U, offsets=offs, nan_A=~taps & ~centre, nan_E=~taps)


def planted(X, where):
    """X [T,3,H,W] with NaN in all three channels wherever ``where`` [T,H,W]."""
    X = X.copy()
    X[np.broadcast_to(where[:, None], X.shape)] = np.nan
    return X


def reference(E, A, G, U, offsets, sigma, strength, guide_affine, dt):
    """The float64 result on these inputs, the float32 restatement's worst departure from it and the kernel's per-element bound."""
    ref = filter_video(E, A, G, U, offsets, sigma, strength, guide_affine)
    r32 = filter_video(E, A, G, U, offsets, sigma, strength, guide_affine, dtype=np.float32, out_dtype=dt)
    assert np.isfinite(ref["out"]).all() and np.isfinite(r32["out"]).all()
    worst = float(np.abs(r32["out"].astype(np.float64) - ref["out"]).max())
    bound = np.maximum(MARGIN * worst + ref["terms"][:, None], rounding(ref["out"], dt))
    return dict(out=ref["out"], bound=bound, worst=worst, terms=ref["terms"], n_valid=ref["n_valid"])


@functools.lru_cache(maxsize=None)
def case_reference(T, H, W, R, dt, sigma=CASE_SIGMA, strength=CASE_STRENGTH):
    """``reference`` of a GPU case, NaN planted in A - computed once, shared by the tests."""
    inp = case_inputs(T, H, W, R, dt)
    A = planted(inp["A"], inp["nan_A"])
    return dict(reference(inp["E"], A, inp["G"], inp["U"], inp["offsets"], sigma, strength, SIGNED, dt), A=A)


# ------------------------------------------------------------------------------------------------------------------ the closed forms
# The flicker case of the GPU file: an integer-translating source, E_t = A_t + delta_t (units of 2^-6), every value exact in float16.
FLICKER = dict(T=6, H=24, W=32, shift=(2, 1), deltas=np.array([0, 16, 4, 24, 8, 20]) / 64.0, radius=2, strength=1.0, sigma=0.1)


def translation_video(T, H, W, shift, deltas=None, seed="temporal_filter.exact"):
    """A random image (multiples of 2^-6 in [1/4, 1/2]: [0, 1] data, the affine is the identity) translated by the integer ``shift`` =
    (dx, dy) per frame: frame t shows canvas[o - t shift + x], so ``fwd[t] = +shift`` and ``bwd[t] = -shift``; plus the per-frame
    constant ``deltas[t]`` on the edit.  -> dict(A, E [T,3,H,W], fwd, bwd [T-1,2,H,W])."""
    rng = _rng(f"{seed}.{T}.{H}.{W}")
    dx, dy = shift
    m = (T - 1) * max(abs(dx), abs(dy)) + 1
    canvas = rng.integers(16, 33, (3, H + 2 * m, W + 2 * m)) / 64.0
    A = np.stack([canvas[:, m - t * dy:m - t * dy + H, m - t * dx:m - t * dx + W] for t in range(T)])
    deltas = np.zeros(T) if deltas is None else np.asarray(deltas, np.float64)
    fwd = np.broadcast_to(np.array([dx, dy], np.float64)[None, :, None, None], (T - 1, 2, H, W)).copy()
    return dict(A=A, E=A + deltas[:, None, None, None], fwd=fwd, bwd=-fwd)


def translation_neighbours(T, H, W, shift, radius):
    """G and U of an integer translation, as ``neighbour_flows`` must chain them: G_{t,k} = k shift, valid where every link of the chain
    stays inside the frame (monotone along a straight line: where x + k shift does), invalid outside the video."""
    offs = offsets_of(radius)
    dx, dy = shift
    ys, xs = np.mgrid[0:H, 0:W]
    G, U = np.zeros((len(offs), T, 2, H, W)), np.zeros((len(offs), T, H, W))
    for i, k in enumerate(offs):
        for t in range(T):
            if 0 <= t + k < T:
                G[i, t, 0], G[i, t, 1] = k * dx, k * dy
                U[i, t] = (xs + k * dx >= 0) & (xs + k * dx < W) & (ys + k * dy >= 0) & (ys + k * dy < H)
    return G, U, offs


def flicker_closed_form(deltas, radius, strength):
    """delta'_t = delta_t + s sum_k (delta_{t+k} - delta_t) / (1 + s n_t), n_t = the number of in-video neighbours: what a pixel whose
    whole window is valid carries after the filter when every weight is exactly s."""
    d = np.asarray(deltas, np.float64)
    T = len(d)
    out = np.empty(T)
    for t in range(T):
        nb = [t + k for k in offsets_of(radius) if 0 <= t + k < T]
        out[t] = d[t] + strength * sum(d[j] - d[t] for j in nb) / (1.0 + strength * len(nb))
    return out


def interior(T, H, W, shift, radius):
    """[H,W] bool: the pixels whose trajectory stays inside the frame for every offset within +-radius (at any frame)."""
    ys, xs = np.mgrid[0:H, 0:W]
    ok = np.ones((H, W), bool)
    for k in offsets_of(radius):
        ok &= (xs + k * shift[0] >= 0) & (xs + k * shift[0] < W) & (ys + k * shift[1] >= 0) & (ys + k * shift[1] < H)
    return ok
