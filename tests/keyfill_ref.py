"""Float64 restatement of the kernel that fills the frames between edited key frames along the source video's optical flow (DESIGN.md
section 24; csrc/keyfill.hip holds the kernel, insv2v/keyfill.py the host side).  Nothing of the product is imported here.  This file is
the contract.

A [T,3,H,W] is the source video: its raw values are used for the residual and the result, a = clamp(x * scale + shift, 0, 1) (``SIGNED``
for frames in [-1, 1]) for the photometric weight.  E [Tk,3,H,W] holds the edited key frames; key slot j is frame key_frame[j] of A.  Entry
i of the frame table is the in-between frame t = frames[i] with up to two sides, s = 0 (the previous key) and s = 1 (the next): slots[i][s]
(-1: no such side), weights[i][s] = tw_s >= 0 (tw_0 + tw_1 = 1 over the existing sides), the flow G_s = G[i, s] [2,H,W] defined on frame
t and pointing into the key's frame, and its validity U_s = U[i, s] [H,W].  A side is ACTIVE at pixel x when its slot is >= 0 and
U_s(x) > 1/2; an inactive side is SKIPPED, not multiplied by 0: a NaN in its G or in the taps it would reach cannot leak.  Per active side

    p      = x + G_s(x);   S(.) = the border-clamped lerp sample at p (clamped) of tests/masktrack_ref.py: ``_taps`` / ``_sample`` as they are
    d2_s   = (1/3) sum_c (a_t[c](x) - S(a_key[c]))^2
    w_s    = tw_s exp(-d2_s / (2 sigma^2))
    r_s[c] = S(E_key[c] - A_key[c])            mode "residual" (A raw: exactly 0 where the edit equals the source in all four taps)
    r_s[c] = S(E_key[c]) - A_t[c](x)           mode "warp"

and with Wsum = the sum of w_s over the active sides

    Wsum > 0:   out[c] = A_t[c](x) + (sum_s w_s r_s[c]) / Wsum,   conf(x) = Wsum
    otherwise:  out[c] = A_t[c](x) + sum over the EXISTING sides of tw'_s r0_s[c],   conf(x) = 0      (a hole: no active side, or every
                weight underflowed; r0_s = the same quantity at x itself, no flow read; tw' = tw renormalised over the existing sides)

and out = A_t[c](x) itself when the added term is 0.

``fill_video(..., dtype=np.float32)`` restates the kernel's operation order in float32 (without FMA contraction, numpy's exp for the
device's): a = x * scale + shift clamped, the three squares added in channel order and divided by 3, arg = d2 * float32(-1 / (2 sigma^2))
(the factor formed in float64 and rounded once), w = tw * exp(arg), num += w * r and Wsum += w in side order from 0, q = num / Wsum,
out = A + q rounded once to the output dtype.  It only calibrates the bound.

Bound of the kernel, per element, against float64 (never against the kernel):
    4 x the restatement's worst |float32 - float64| on the case's inputs    (4: FMA contraction and the device's expf, as section 21)
    + sum_s 2^-22 (2 + |arg_s|) (w_s / Wsum) |r_s[c] - q[c]|                (the rounding of the exponential's argument: arg carries a few
                                                                            roundings of relative 2^-24, exp turns an absolute error of
                                                                            the argument into a relative error delta_s of the weight,
                                                                            and d q / d w_s = (r_s - q) / Wsum for the NORMALISED
                                                                            quotient q = sum w r / sum w: a pixel with one active side
                                                                            does not depend on its weight at all)
    floored at one rounding of the output dtype (half a unit in the last place of the reference value).
conf = Wsum has the same 4 x term, + sum_s 2^-22 (2 + |arg_s|) w_s, floored at one fp32 rounding.
The inputs are seeded by name, so the CPU and the GPU file see the same arrays."""
import functools
import zlib

import numpy as np

import masktrack_ref as mr

SIGNED = (0.5, 0.5)   # the affine of frames in [-1, 1]
ONE = (1.0, 0.0)
MODES = ("residual", "warp")
MARGIN = 4.0
CASE_SIGMA = 0.1
DTYPES = ("f16", "f32")
# (H, W, T, keys): 2 x 2 with ONE key and a single one-sided frame; 5 x 7; 3 x 300 (a 256-thread block straddles rows); 17 x 33 with three
# irregular keys, a frame before the first and one after the last (one-sided) and two-sided frames at unequal distances; n = 65 frames
# (two launches: 64 + 1)
CASES = [(2, 2, 2, (0,)), (5, 7, 5, (0, 4)), (3, 300, 5, (0, 4)), (17, 33, 8, (1, 4, 6)), (5, 7, 67, (0, 66))]
MUTATIONS = ("tw_swap", "edit_weight", "neg_flow", "res_sign", "no_norm", "norm_plus_one", "mul_zero", "fallback_warped", "no_affine",
             "affine_residual", "chan_sum", "nearest", "zero_pad", "mode_swap")
MUTATION_CASES = [CASES[2], CASES[3]]
MIN_DEPARTURE = 10.0   # a planted misreading must miss the reference by at least this many bounds
MAX_ARG = 80.0         # -arg = d2 / (2 sigma^2) stays below it on the active sides of a case: Wsum never underflows there


def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def stored(a, dtype):
    """The array as the operand holds it: rounded to float16 or float32, returned as float64 (exact)."""
    with np.errstate(invalid="ignore"):
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


def sides_of(T, keys):
    """(frames, slots, weights) of every in-between frame of a video of T frames with the key frames ``keys`` (increasing):
    tw_0 = (b - t) / (b - a), tw_1 = (t - a) / (b - a); a frame before the first or after the last key has one side with weight 1."""
    frames, slots, weights = [], [], []
    for t in range(T):
        if t in keys:
            continue
        prv = max((j for j, k in enumerate(keys) if k < t), default=-1)
        nxt = min((j for j, k in enumerate(keys) if k > t), default=-1)
        frames.append(t)
        slots.append((prv, nxt))
        if prv < 0 or nxt < 0:
            weights.append((1.0 if prv >= 0 else 0.0, 1.0 if nxt >= 0 else 0.0))
        else:
            a, b = keys[prv], keys[nxt]
            weights.append(((b - t) / (b - a), (t - a) / (b - a)))
    return frames, slots, weights


# ------------------------------------------------------------------------------------------------------------------ the definition
def fill_video(A, E, key_frame, frames, slots, weights, G, U, sigma=0.1, mode="residual", guide_affine=SIGNED, dtype=np.float64, out_dtype=None,
               mutate=None):
    """A [T,3,H,W], E [Tk,3,H,W] as stored, G [n,2,2,H,W], U [n,2,H,W] -> dict(out [n,3,H,W] (the rows of ``frames``), conf [n,H,W],
    terms [n,3,H,W] and conf_terms [n,H,W] = the bounds' derived terms (float64 only), n_active [n,H,W], max_arg = the largest
    d2 / (2 sigma^2) of an active side).  ``out_dtype`` ("f16" / "f32"): the float32 restatement rounds its result to it."""
    assert mode in MODES and (mutate is None or mutate in MUTATIONS)
    f = dtype
    if mutate == "mode_swap":
        mode = MODES[1 - MODES.index(mode)]
    Ar, E = np.asarray(A).astype(f), np.asarray(E).astype(f)
    a = Ar if mutate == "no_affine" else affine(A, guide_affine, f)
    wkey = (E if mutate == "no_affine" else affine(E, guide_affine, f)) if mutate == "edit_weight" else None   # (the misreading: the weight on E)
    Ares = a if mutate == "affine_residual" else Ar
    _, _, H, W = Ar.shape
    n = len(frames)
    G, U = np.asarray(G).astype(f), np.asarray(U)
    if mutate == "neg_flow":
        G = -G
    ys, xs = (v.astype(f) for v in np.mgrid[0:H, 0:W])
    neg_inv = f(np.float32(-1.0 / (2.0 * float(sigma) ** 2))) if f is np.float32 else None
    out, conf = np.empty((n, 3, H, W), f), np.zeros((n, H, W), f)
    terms, conf_terms, count, max_arg = np.zeros((n, 3, H, W)), np.zeros((n, H, W)), np.zeros((n, H, W), np.int64), 0.0
    for i, t in enumerate(frames):
        num, wsum = np.zeros((3, H, W), f), np.zeros((H, W), f)
        exist = [s for s in (0, 1) if slots[i][s] >= 0]
        tws = sum(float(weights[i][s]) for s in exist)
        per_side, warped = [], {}
        for s in exist:
            slot = slots[i][s]
            kf = key_frame[slot]
            v = U[i, s] > 0.5
            if not v.any() and mutate not in ("mul_zero", "fallback_warped"):
                continue
            with np.errstate(invalid="ignore"):   # (a NaN of G at an inactive pixel: its taps are computed and thrown away below)
                tp = mr._taps(xs + G[i, s, 0], ys + G[i, s, 1], H, W, f, clamp=mutate != "zero_pad")
            smp = lambda P: mr._sample(P, tp, mutate == "nearest")   # noqa: E731
            tw = f(weights[i][1 - s] if mutate == "tw_swap" else weights[i][s])
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                d = [a[t, c] - smp(wkey[slot, c] if wkey is not None else a[kf, c]) for c in range(3)]
                d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                if mutate != "chan_sum":
                    d2 = d2 / f(3)
                arg = d2 * neg_inv if neg_inv is not None else -d2 / f(2.0 * float(sigma) ** 2)
                w = tw * np.exp(arg)
                if mode == "residual":
                    res = np.stack([smp(E[slot, c] - Ares[kf, c]) for c in range(3)])
                else:
                    res = np.stack([smp(E[slot, c]) - Ar[t, c] for c in range(3)])
                if mutate == "res_sign":
                    res = -res
                warped[s] = res
                if mutate == "mul_zero":      # the misreading: every existing side is read and weighed by U
                    w = np.where(np.isnan(G[i, s, 0]), f(np.nan), w * v.astype(f))   # (0 * what a NaN flow reaches)
                    num, wsum = num + w * res, wsum + w
                else:                         # the definition: an inactive side contributes nothing, whatever it holds
                    num, wsum = num + np.where(v, w * res, f(0)), wsum + np.where(v, w, f(0))
            count[i] += v
            if v.any():
                max_arg = max(max_arg, float(np.abs(arg)[v].max()))
            per_side.append((np.where(v, np.abs(arg), 0.0), np.where(v, w, 0.0), np.where(v, res, 0.0)))
        has = wsum > 0
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            den = f(1) if mutate == "no_norm" else (f(1) + wsum if mutate == "norm_plus_one" else np.where(has, wsum, f(1)))
            q = num / den
            qf = np.zeros((3, H, W), f)       # the hole: the keys blended at x itself, tw renormalised over the existing sides
            for s in exist:
                slot = slots[i][s]
                kf = key_frame[slot]
                r0 = E[slot] - Ares[kf] if mode == "residual" else E[slot] - Ar[t]
                if mutate == "fallback_warped" and s in warped:
                    r0 = warped[s]
                if mutate == "res_sign":
                    r0 = -r0
                twn = f(np.float32(float(weights[i][s]) / tws)) if f is np.float32 else float(weights[i][s]) / tws
                qf = qf + twn * r0
            q = np.where(has, q, qf)
            out[i] = np.where(q == 0, Ar[t], Ar[t] + q)
        conf[i] = np.where(has, wsum, f(0))
        if f is np.float64:
            for aa, ww, rr in per_side:
                with np.errstate(invalid="ignore", divide="ignore"):
                    delta = 2.0 ** -22 * (2.0 + aa)
                    terms[i] += np.where(has, delta * ww / np.where(has, wsum, 1.0) * np.abs(rr - q), 0.0)
                    conf_terms[i] += delta * ww
    if out_dtype is not None:
        out = stored(out, out_dtype).astype(f)
    return dict(out=out, conf=conf, terms=terms, conf_terms=conf_terms, n_active=count, max_arg=max_arg)


def fill_pixel_loop(A, E, key_frame, frames, slots, weights, G, U, sigma, mode, guide_affine, sampler):
    """The same definition written one pixel at a time, with ``sampler(plane [H,W], px, py) -> float`` for S(.) (the CPU file passes
    ``torch.nn.functional.grid_sample``): an independent restatement to hold ``fill_video`` against.  -> (out [n,3,H,W], conf [n,H,W])."""
    A, E = np.asarray(A, np.float64), np.asarray(E, np.float64)
    g = affine(A, guide_affine)
    _, _, H, W = A.shape
    out, conf = np.empty((len(frames), 3, H, W)), np.zeros((len(frames), H, W))
    for i, t in enumerate(frames):
        for y in range(H):
            for x in range(W):
                num, wsum = np.zeros(3), 0.0
                for s in (0, 1):
                    slot = slots[i][s]
                    if slot < 0 or not U[i, s, y, x] > 0.5:
                        continue
                    kf = key_frame[slot]
                    px, py = x + G[i, s, 0, y, x], y + G[i, s, 1, y, x]
                    d2 = sum((g[t, c, y, x] - sampler(g[kf, c], px, py)) ** 2 for c in range(3)) / 3.0
                    w = weights[i][s] * np.exp(-d2 / (2.0 * sigma ** 2))
                    if mode == "residual":
                        r = np.array([sampler(E[slot, c], px, py) - sampler(A[kf, c], px, py) for c in range(3)])
                    else:
                        r = np.array([sampler(E[slot, c], px, py) - A[t, c, y, x] for c in range(3)])
                    num, wsum = num + w * r, wsum + w
                if wsum > 0:
                    q, conf[i, y, x] = num / wsum, wsum
                else:
                    exist = [s for s in (0, 1) if slots[i][s] >= 0]
                    tws = sum(weights[i][s] for s in exist)
                    q = np.zeros(3)
                    for s in exist:
                        slot = slots[i][s]
                        ref = A[key_frame[slot], :, y, x] if mode == "residual" else A[t, :, y, x]
                        q = q + weights[i][s] / tws * (E[slot, :, y, x] - ref)
                out[i, :, y, x] = A[t, :, y, x] + q
    return out, conf


# ------------------------------------------------------------------------------------------------------------------ inputs
def _reach(key_frame, frames, slots, G, U, Tk, H, W):
    """[Tk,H,W] bool: the pixels of every key slot that some ACTIVE side's four clamped taps read, or that a pixel without any active
    side reads in place (the hole's fallback)."""
    reach = np.zeros((Tk, H, W), bool)
    ys, xs = (v.astype(np.float64) for v in np.mgrid[0:H, 0:W])
    for i in range(len(frames)):
        act = [(slots[i][s] >= 0) & (U[i, s] > 0.5) for s in (0, 1)]
        hole = ~(act[0] | act[1])
        for s in (0, 1):
            if slots[i][s] < 0:
                continue
            reach[slots[i][s]] |= hole
            tp = mr._taps(xs + np.nan_to_num(G[i, s, 0]), ys + np.nan_to_num(G[i, s, 1]), H, W, np.float64)
            for yy, xx in zip(tp["y"], tp["x"]):
                reach[slots[i][s]][yy[act[s]], xx[act[s]]] = True
    return reach


@functools.lru_cache(maxsize=None)
def case_inputs(H, W, T, keys, edt, adt):
    """One GPU case: A [T,3,H,W] (a little beyond [-1, 1] so the clamp acts; smooth enough in time that the photometric weights spread
    over (0, 1]) and E [Tk,3,H,W] = the keys of A plus an edit of a few tenths, as stored in ``adt`` / ``edt``; smooth seeded G
    [n,2,2,H,W] of a few pixels; U [n,2,H,W] with holes, a whole invalid side (frame 1, side 0, from two frames up) and - from 5 x 7 up -
    a rectangle of the middle frame NO active side covers (the fallback).  NaN is planted in G wherever the side is inactive, and in the
    key frames of A and in E wherever neither an active side's tap nor a hole's fallback reads."""
    rng = _rng(f"keyfill.case.{H}.{W}.{T}.{keys}.{edt}.{adt}")
    keys = list(keys)
    frames, slots, weights = sides_of(T, keys)
    n, Tk = len(frames), len(keys)
    amp = min(3.0, min(H, W) / 4.0)
    G = np.stack([[np.stack([mr._smooth(rng, H, W, amp) + 0.3 * amp * (2 * s - 1), mr._smooth(rng, H, W, amp) - 0.2 * amp * (2 * s - 1)])
                   for s in (0, 1)] for _ in range(n)]).astype(np.float32).astype(np.float64)
    U = (rng.uniform(0, 1, (n, 2, H, W)) > 0.15).astype(np.float64)
    if n >= 2:
        U[1, 0] = 0.0
    if H >= 5:
        y0, x0 = H // 3, W // 3
        U[n // 2, :, y0:y0 + max(2, H // 4), x0:x0 + max(2, W // 4)] = 0.0
    for i in range(n):
        for s in (0, 1):
            if slots[i][s] < 0:
                U[i, s] = rng.integers(0, 2, (H, W))   # whatever a side that does not exist holds, it is not read
    base = [mr._smooth(rng, H, W, 0.8, cells=8) for _ in range(3)]
    drift = [mr._smooth(rng, H, W, 0.1, cells=5) for _ in range(3)]
    A = 1.05 * np.stack([[base[c] + (t / max(T - 1, 1) - 0.5) * drift[c] + mr._smooth(rng, H, W, 0.05, cells=5) + rng.uniform(-0.03, 0.03, (H, W))
                          for c in range(3)] for t in range(T)])
    edit = np.stack([[mr._smooth(rng, H, W, 0.35, cells=3) + 0.15 * (j % 3 - 1) + rng.uniform(-0.05, 0.05, (H, W)) for _ in range(3)] for j in range(Tk)])
    A = stored(A, adt)
    E = stored(A[keys] + edit, edt)
    active = np.stack([[(slots[i][s] >= 0) & (U[i, s] > 0.5) for s in (0, 1)] for i in range(n)])
    reach = _reach(keys, frames, slots, G, U, Tk, H, W)
    G = np.where(np.broadcast_to(active[:, :, None], G.shape), G, np.nan)
    for j, k in enumerate(keys):
        A[k][np.broadcast_to(~reach[j][None], A[k].shape)] = np.nan
        E[j][np.broadcast_to(~reach[j][None], E[j].shape)] = np.nan
    return dict(A=A, E=E, G=G, U=U, key_frame=keys, frames=frames, slots=slots, weights=weights,
                planted=dict(G=int(np.isnan(G).sum()), A=int(np.isnan(A).sum()), E=int(np.isnan(E).sum())))


def reference(inp, sigma, mode, guide_affine, edt):
    """The float64 result on these inputs, the float32 restatement's worst departure from it and the kernel's per-element bounds."""
    args = (inp["A"], inp["E"], inp["key_frame"], inp["frames"], inp["slots"], inp["weights"], inp["G"], inp["U"], sigma, mode, guide_affine)
    ref = fill_video(*args)
    r32 = fill_video(*args, dtype=np.float32, out_dtype=edt)
    assert np.isfinite(ref["out"]).all() and np.isfinite(r32["out"]).all(), "a planted NaN reached the reference"
    assert np.array_equal(ref["conf"] > 0, r32["conf"] > 0), "float32 and float64 disagree on where Wsum underflows"
    worst = float(np.abs(r32["out"].astype(np.float64) - ref["out"]).max())
    worst_conf = float(np.abs(r32["conf"].astype(np.float64) - ref["conf"]).max())
    bound = np.maximum(MARGIN * worst + ref["terms"], rounding(ref["out"], edt))
    conf_bound = np.maximum(MARGIN * worst_conf + ref["conf_terms"], rounding(ref["conf"], "f32"))
    return dict(out=ref["out"], conf=ref["conf"], bound=bound, conf_bound=conf_bound, worst=worst, worst_conf=worst_conf, terms=ref["terms"],
                n_active=ref["n_active"], max_arg=ref["max_arg"])


@functools.lru_cache(maxsize=None)
def case_reference(H, W, T, keys, edt, adt, mode):
    """``reference`` of a GPU case - computed once, shared by the tests."""
    ref = reference(case_inputs(H, W, T, keys, edt, adt), CASE_SIGMA, mode, SIGNED, edt)
    assert ref["max_arg"] < MAX_ARG
    return ref


def translation_case(H=6, W=9, shift0=(2, 1), shift1=(-1, 2), seed="keyfill.exact"):
    """T = 3, keys 0 and 2, frame 1 in between with tw = (1/2, 1/2).  The keys' sources are frame 1 translated by integers (key s shows
    A_1(x + shift_s)), so G_s = -shift_s, d2 = 0 wherever the trajectory stays inside the frame (U_s = 1 exactly there) and w_s = 1/2.
    Every value is a multiple of 2^-6 in [1/4, 1/2] ([0, 1] data: the affine is the identity), the edit adds multiples of 2^-6 within
    +-1/4: all sums below are exact in float16.  -> dict(A [3,3,H,W], E [2,3,H,W], G, U, key_frame, frames, slots, weights, want
    [1,3,H,W] = the closed form: A_1 + the mean of the valid sides' translated residuals, and in a hole the mean of the keys' residuals
    at x itself)."""
    rng = _rng(f"{seed}.{H}.{W}")
    m = 4
    canvas = rng.integers(16, 33, (3, H + 2 * m, W + 2 * m)) / 64.0
    cut = lambda dx, dy: canvas[:, m + dy:m + dy + H, m + dx:m + dx + W]   # noqa: E731
    A = np.stack([cut(*shift0), cut(0, 0), cut(*shift1)])
    R = rng.integers(-16, 17, (2, 3, H, W)) / 64.0
    ys, xs = np.mgrid[0:H, 0:W]
    G, U = np.zeros((1, 2, 2, H, W)), np.zeros((1, 2, H, W))
    moved = np.zeros((2, 3, H, W))
    for s, (dx, dy) in enumerate((shift0, shift1)):
        G[0, s, 0], G[0, s, 1] = -dx, -dy
        U[0, s] = (xs - dx >= 0) & (xs - dx < W) & (ys - dy >= 0) & (ys - dy < H)
        moved[s] = R[s][:, np.clip(ys - dy, 0, H - 1), np.clip(xs - dx, 0, W - 1)]
    v = U[0] > 0.5
    count = v.sum(0)
    blend = np.where(count > 0, (v[0] * moved[0] + v[1] * moved[1]) / np.maximum(count, 1), (R[0] + R[1]) / 2)
    return dict(A=A, E=A[[0, 2]] + R, G=G, U=U, key_frame=[0, 2], frames=[1], slots=[(0, 1)], weights=[(0.5, 0.5)], want=(A[1] + blend)[None],
                conf=(count / 2.0)[None])


# The case whose weights ALL underflow: the in-between frame differs from both keys by about 0.4 on the guide everywhere, so
# d2 / (2 sigma^2) > 1e4 at sigma = 1e-3 - exp gives exactly 0 in float32 and in float64 - and every pixel takes the fallback with conf 0.
UNDERFLOW = dict(H=5, W=7, T=3, keys=(0, 2), sigma=1e-3)


@functools.lru_cache(maxsize=None)
def underflow_inputs(dt):
    c = UNDERFLOW
    rng = _rng(f"keyfill.underflow.{dt}")
    H, W, T = c["H"], c["W"], c["T"]
    frames, slots, weights = sides_of(T, list(c["keys"]))
    A = rng.uniform(-0.02, 0.02, (T, 3, H, W)) + np.array([0.6, -0.2, 0.6])[:, None, None, None]   # per FRAME: the keys high, frame 1 low
    E = A[list(c["keys"])] + rng.uniform(-0.3, 0.3, (2, 3, H, W))
    G = rng.uniform(-1.5, 1.5, (1, 2, 2, H, W)).astype(np.float32).astype(np.float64)
    return dict(A=stored(A, dt), E=stored(E, dt), G=G, U=np.ones((1, 2, H, W)), key_frame=list(c["keys"]), frames=frames, slots=slots, weights=weights)
