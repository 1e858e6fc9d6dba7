"""Float64 restatement of the pixel-space scores (csrc/pixel_score.hip holds the kernels, insv2v/pixel_score.py the
host side).  Nothing of the product is imported here.

All values v below are a frame's values after the affine map  v = clamp(x * scale + shift, 0, 1)  (data_range 1).

Flow warp error of the pair (t, t+1), b = fwd[t] defined on frame t and pointing into t+1, c = bwd[t] (or None), per pixel x:
    p, inb, pc and the sample S(.) as in tests/masktrack_ref.py (border clamp, lerps) - its ``_taps`` / ``_sample`` are used as they are
    cons  = true without c; else with cf = S(c), d = b + cf:   |d|^2 <= alpha (|b|^2 + |cf|^2) + beta
    valid = inb and cons
    err   = (1/3) sum_c (A_t[c](x) - S(A_{t+1}[c]))^2
    sums  = (sum valid w_t err, sum valid w_t, count of valid);   warp_error = sums[0] / sums[1]

Fidelity of frame t, w = the region weight (1 without one), se = (1/3) sum_c (x - y)^2:
    sums 0..4 = sum se, sum w se, sum (1-w) se, sum w, sum (1-w)                       each on its own - no subtraction
    SSIM: Gaussian window, 11 taps, sigma 1.5, exp(-k^2 / 2 sigma^2) normalised to sum 1, separable, inside the frame only (centres
          5 <= y <= H-6, 5 <= x <= W-6), K1 = 0.01, K2 = 0.03, population (co)variances, per channel
          ((2 mx my + C1)(2 sxy + C2)) / ((mx^2 + my^2 + C1)(sx^2 + sy^2 + C2)),  s = the mean of the three channels
    sums 5..9 = sum s, sum wc s, sum (1-wc) s, sum wc, sum (1-wc)                       wc = w at the window CENTRE
    mse = sum se / (H W), psnr = 10 log10(1 / mse) (inf for 0), ssim = sum s / centres; inside / outside: the weighted sums over their
    weight sums, nan when that is 0.

``*_f32`` functions restate the kernels' operation order in float32 (without FMA contraction); they only calibrate the bounds:

    per element   |kernel - float64| <= MARGIN * max(worst |float32 restatement - float64| of the case, FLOOR)
    per sum       |kernel - float64| <= MARGIN * max(sum of the weighted |float32 restatement - float64|, FLOOR * sum of the weights) + summation term

MARGIN = 4 is for what the compiler may do differently from the restatement: contract a * b + c into one FMA, and add in another tree.
The sum bound takes the L1 error of the restatement, not the error of its sum: the kernel's element errors are of the same size but need
not cancel the same way.  FLOOR: a measured error below the roundings that are always there would claim too much (an all-equal case
measures 0, yet ``2 mx my`` and ``mx^2 + my^2`` may contract differently) - 2^-23 for an SSIM value (<= 1 in magnitude; its division,
the channel sum and the division by 3 round at least three times, to within 2^-24 each, on top of those of numerator and denominator),
and for err / se 4 roundings relative to the value itself, 2^-22 err, which is 0 where the value is exactly 0: the bit-exact cases stay
bit-exact.  Summation: n 2^-53 sum |terms| (the partial sums are float64 in any order).
The inputs are seeded by name, so the CPU and the GPU file see the same arrays."""
import functools
import zlib

import numpy as np

import masktrack_ref as mr

ALPHA, BETA = mr.ALPHA, mr.BETA
MARGIN = 4.0
FLOOR_SSIM = 2.0 ** -23
FLOOR_REL_ERR = 2.0 ** -22
TILE = (16, 64)   # the fidelity kernel's tile of SSIM centres (rows, columns): insv2v_frame_fidelity_tile; the GPU file asserts it
RADIUS, SIGMA, K1, K2 = 5, 1.5, 0.01, 0.03
SIGNED = (0.5, 0.5)   # the affine of frames in [-1, 1]
_TH, _TW = TILE
# (T, H, W, dtype of X, dtype of Y): one window; one more centre in either direction; exactly one tile, one centre fewer, one more in each
# direction (a second tile row / column of a single centre); two tiles and a bit in both, odd width; T = 1 and 3
FIDELITY_CASES = [(1, 11, 11, "f32", "f32"), (3, 11, 12, "f16", "f16"), (1, 12, 11, "f32", "f16"),
                  (1, _TH + 10, _TW + 10, "f32", "f32"), (3, _TH + 9, _TW + 9, "f16", "f32"), (1, _TH + 11, _TW + 10, "f32", "f32"),
                  (1, _TH + 10, _TW + 11, "f16", "f16"), (3, 2 * _TH + 13, 2 * _TW + 17, "f32", "f16")]
WARP_CASES = [(2, 2, 2, "f32"), (2, 3, 5, "f16"), (4, 17, 23, "f32"), (4, 64, 96, "f16"), (2, 64, 96, "f32")]   # (T, H, W, dtype)
SSIM_MUTATIONS = ("sample_cov", "uniform7", "sigma1", "same_pad", "k2", "range2", "w_corner", "grey")
WARP_MUTATIONS = ("zero_pad", "neg_fwd", "pair_shift", "no_cons", "lt", "nearest", "all_pixels", "chan_sum")
MUTATION_FIDELITY_CASE = FIDELITY_CASES[-1]
MUTATION_WARP_CASE = WARP_CASES[3]
FIDELITY_KEYS = ("se", "se_in", "se_out", "w_in", "w_out", "ssim", "ssim_in", "ssim_out", "wc_in", "wc_out")


def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


def stored(a, dtype):
    """The array as the operand holds it: rounded to float16 or float32, returned as float64 (exact)."""
    return np.asarray(a).astype(np.float16 if dtype == "f16" else np.float32).astype(np.float64)


def affine(x, scale_shift, dtype=np.float64):
    s, h = (dtype(v) for v in scale_shift)
    return np.minimum(np.maximum(np.asarray(x).astype(dtype) * s + h, dtype(0)), dtype(1))


# ------------------------------------------------------------------------------------------------------------------ SSIM and squared error
def gauss(sigma=SIGMA, radius=RADIUS):
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * sigma * sigma))
    return g / g.sum()


def _filt(P, g):
    """The separable window over the last two axes, inside the frame only: a row pass, then a column pass, each a sum in tap order."""
    n, H, W = len(g), P.shape[-2], P.shape[-1]
    R = sum(g[j] * P[..., :, j:W - n + 1 + j] for j in range(n))
    return sum(g[j] * R[..., j:H - n + 1 + j, :] for j in range(n))


def ssim_map(X, Y, mutate=None):
    """The definition: X, Y [3,H,W] float64 values in [0,1] -> the SSIM map [H-10,W-10] (the mean of the three channels)."""
    assert mutate is None or mutate in SSIM_MUTATIONS
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    L = 2.0 if mutate == "range2" else 1.0
    C1, C2 = (K1 * L) ** 2, ((0.01 if mutate == "k2" else K2) * L) ** 2
    if mutate == "grey":
        X, Y = X.mean(0, keepdims=True), Y.mean(0, keepdims=True)
    g = gauss(1.0) if mutate == "sigma1" else gauss()
    if mutate == "uniform7":
        g = np.where(np.abs(np.arange(-RADIUS, RADIUS + 1)) <= 3, 1.0 / 7.0, 0.0)
    if mutate == "same_pad":
        X, Y = (np.pad(a, ((0, 0), (RADIUS, RADIUS), (RADIUS, RADIUS))) for a in (X, Y))
    mx, my = _filt(X, g), _filt(Y, g)
    sx2, sy2, sxy = _filt(X * X, g) - mx * mx, _filt(Y * Y, g) - my * my, _filt(X * Y, g) - mx * my
    if mutate == "sample_cov":
        n = float(len(g) ** 2)
        sx2, sy2, sxy = (v * n / (n - 1.0) for v in (sx2, sy2, sxy))
    s = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx2 + sy2 + C2))
    return s.mean(0)   # (with "same_pad" a map of the frame's size: the definition's centres are its inner part)


def ssim_map_f32(X, Y):
    """The kernel's operation order in float32: the moments of x - 1/2 and y - 1/2 (the variances are the same, their cancellation
    error is smaller), mu = m + 1/2, the channels added in order and divided by 3."""
    f = np.float32
    a, b = np.asarray(X).astype(f) - f(0.5), np.asarray(Y).astype(f) - f(0.5)
    g = gauss().astype(f)
    m = [_filt(p, g) for p in (a, b, a * a, b * b, a * b)]
    mx, my = m[0] + f(0.5), m[1] + f(0.5)
    sx2, sy2, sxy = m[2] - m[0] * m[0], m[3] - m[1] * m[1], m[4] - m[0] * m[1]
    C1, C2 = f(0.01) * f(0.01), f(0.03) * f(0.03)
    s = ((f(2) * mx * my + C1) * (f(2) * sxy + C2)) / ((mx * mx + my * my + C1) * (sx2 + sy2 + C2))
    return ((s[0] + s[1]) + s[2]) / f(3)


def se_map(X, Y, dtype=np.float64):
    d = np.asarray(X).astype(dtype) - np.asarray(Y).astype(dtype)
    return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / dtype(3)


def fidelity_sums(se, s, w=None, mutate=None):
    """The ten sums of one frame from its squared-error map [H,W] and SSIM map [H-10,W-10], in float64."""
    se, s = np.asarray(se, np.float64), np.asarray(s, np.float64)
    H, W = se.shape
    w = np.ones((H, W)) if w is None else np.asarray(w, np.float64)
    if mutate == "same_pad":
        wc = w
    elif mutate == "w_corner":
        wc = w[:H - 2 * RADIUS, :W - 2 * RADIUS]
    else:
        wc = w[RADIUS:H - RADIUS, RADIUS:W - RADIUS]
    return np.array([se.sum(), (w * se).sum(), ((1 - w) * se).sum(), w.sum(), (1 - w).sum(),
                     s.sum(), (wc * s).sum(), ((1 - wc) * s).sum(), wc.sum(), (1 - wc).sum()])


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(a, np.float64) / np.asarray(b, np.float64)


def _psnr(mse):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -10.0 * np.log10(mse)


def fidelity_metrics(sums, H, W, region=True, n_centres=None):
    """The host-side conventions: the ten sums [..., 10] of frames of H x W -> dict of mse / psnr / ssim (and _inside / _outside)."""
    q = dict(zip(FIDELITY_KEYS, np.moveaxis(np.asarray(sums, np.float64), -1, 0)))
    mse = q["se"] / (H * W)
    out = dict(mse=mse, psnr=_psnr(mse), ssim=q["ssim"] / (n_centres or (H - 2 * RADIUS) * (W - 2 * RADIUS)))
    if region:
        for side in ("in", "out"):
            m = _div(q["se_" + side], q["w_" + side])
            out.update({f"mse_{side}side": m, f"psnr_{side}side": _psnr(m), f"ssim_{side}side": _div(q["ssim_" + side], q["wc_" + side])})
    return out


def fidelity_frame(X, Y, w, x_affine=SIGNED, y_affine=SIGNED, mutate=None):
    """One frame, X / Y [3,H,W] as stored -> (the ten float64 sums, their bounds for the kernel)."""
    forgot = mutate == "range2"   # the affine forgotten: SSIM on the raw values with data_range 2
    Xv, Yv = (np.asarray(X, np.float64), np.asarray(Y, np.float64)) if forgot else (affine(X, x_affine), affine(Y, y_affine))
    se, s = se_map(affine(X, x_affine), affine(Y, y_affine)), ssim_map(Xv, Yv, mutate)
    sums = fidelity_sums(se, s, w, mutate)
    if mutate is not None:
        return sums, None
    f = np.float32
    X32, Y32 = affine(X, x_affine, f), affine(Y, y_affine, f)
    e_se = np.abs(se_map(X32, Y32, f).astype(np.float64) - se)
    e_s = np.abs(ssim_map_f32(X32, Y32).astype(np.float64) - s)
    ones_se, ones_s = np.ones_like(se), np.ones_like(s)
    l1 = fidelity_sums(np.maximum(e_se, FLOOR_REL_ERR * se), np.maximum(e_s, FLOOR_SSIM), w)   # the weighted element bounds, summed
    mag = fidelity_sums(se, np.abs(s), w)
    n = np.array([se.size] * 5 + [s.size] * 5)
    bound = MARGIN * l1 + n * 2.0 ** -53 * mag
    bound[[3, 4, 8, 9]] = (n * 2.0 ** -53 * fidelity_sums(ones_se, ones_s, w))[[3, 4, 8, 9]]   # weight sums: summation only
    return sums, dict(bound=bound, worst_se=float(e_se.max()), worst_ssim=float(e_s.max()))


# ------------------------------------------------------------------------------------------------------------------ warp error
def warp_pair(A0, A1, b, c, alpha=ALPHA, beta=BETA, dtype=np.float64, mutate=None):
    """A0, A1 [3,H,W] values in [0,1], b / c [2,H,W] -> dict(err [H,W] (0 where invalid), valid [H,W] bool) in ``dtype``."""
    assert mutate is None or mutate in WARP_MUTATIONS
    A0, A1, b = (np.asarray(a).astype(dtype) for a in (A0, A1, b))
    if mutate == "neg_fwd":
        b = -b
    H, W = b.shape[1:]
    ys, xs = (a.astype(dtype) for a in np.mgrid[0:H, 0:W])
    px, py = xs + b[0], ys + b[1]
    inb = (px >= 0) & (px <= dtype(W - 1)) & (py >= 0) & (py <= dtype(H - 1))
    zero_pad, nearest = mutate == "zero_pad", mutate == "nearest"
    t = mr._taps(px, py, H, W, dtype, clamp=not zero_pad)
    cons = np.ones((H, W), bool)
    if c is not None and mutate != "no_cons":
        c = np.asarray(c).astype(dtype)
        tc = mr._taps(px, py, H, W, dtype)
        cfx, cfy = mr._sample(c[0], tc), mr._sample(c[1], tc)
        dx, dy = b[0] + cfx, b[1] + cfy
        lhs, rhs = dx * dx + dy * dy, dtype(alpha) * ((b[0] * b[0] + b[1] * b[1]) + (cfx * cfx + cfy * cfy)) + dtype(beta)
        cons = lhs < rhs if mutate == "lt" else lhs <= rhs
    valid = cons if zero_pad else inb & cons   # zero padding: every pixel is compared, against zeros outside the frame
    d = [A0[ch] - mr._sample(A1[ch], t, nearest) for ch in range(3)]
    s = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    err = s if mutate == "chan_sum" else s / dtype(3)
    return dict(err=np.where(valid, err, dtype(0)), valid=valid)


def warp_sums(err, valid, w=None, mutate=None):
    err, valid = np.asarray(err, np.float64), np.asarray(valid, bool)
    w = np.ones(err.shape) if w is None else np.asarray(w, np.float64)
    weight = w.sum() if mutate == "all_pixels" else (w * valid).sum()
    return np.array([(w * valid * err).sum(), weight, float(valid.sum())])


def warp_video(A, fwd, bwd=None, region=None, alpha=ALPHA, beta=BETA, affine_map=SIGNED, dtype=np.float64, mutate=None):
    """A [T,3,H,W] as stored -> dict(sums [T-1,3], warp_error [T-1], err [T-1,H,W], valid [T-1,H,W])."""
    V = affine(A, affine_map, dtype)
    T = V.shape[0]
    pairs = []
    for t in range(T - 1):
        t0, t1 = (min(t + 1, T - 1), min(t + 2, T - 1)) if mutate == "pair_shift" else (t, t + 1)
        pairs.append(warp_pair(V[t0], V[t1], fwd[t], None if bwd is None else bwd[t], alpha, beta, dtype, mutate))
    err, valid = np.stack([p["err"] for p in pairs]), np.stack([p["valid"] for p in pairs])
    sums = np.stack([warp_sums(err[t], valid[t], None if region is None else region[t], mutate) for t in range(T - 1)])
    return dict(sums=sums, warp_error=_div(sums[:, 0], sums[:, 1]), err=err, valid=valid)


def warp_excluded(b, c, alpha=ALPHA, beta=BETA):
    """The pixels whose ``valid`` the comparison leaves out: a decision margin of the float64 definition under masktrack_ref's guards."""
    H, W = b.shape[1:]
    return mr.excluded(mr.margins(np.zeros((2, H, W)), np.ones((H, W)), b, c, alpha, beta))


# ------------------------------------------------------------------------------------------------------------------ inputs
def _texture(rng, H, W, cells=5):
    """A smooth field in about [-1, 1] plus fine noise."""
    return mr._smooth(rng, H, W, 0.9, cells=cells) + rng.uniform(-0.2, 0.2, (H, W))


def region_input(key, T, H, W):
    """[T,H,W] float32-exact weights in [0,1]: a soft blob with flat 0 and flat 1 areas, moving a little from frame to frame."""
    rng = _rng(f"pixel_score.region.{key}.{T}.{H}.{W}")
    out = []
    for _ in range(T):
        s = 0.5 + 1.5 * mr._smooth(rng, H, W, 1.0, cells=6)
        out.append(np.clip(s, 0.0, 1.0))
    return np.stack(out).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def fidelity_inputs(T, H, W, xdt, ydt):
    """X, Y [T,3,H,W] as stored (values a little beyond [-1,1] so the clamp acts), region [T,H,W]; Y = X with a change that is large
    inside the region and small outside."""
    rng = _rng(f"pixel_score.fidelity.{T}.{H}.{W}.{xdt}.{ydt}")
    X = 1.1 * np.stack([[_texture(rng, H, W) for _ in range(3)] for _ in range(T)])
    w = region_input("fid", T, H, W)
    change = np.stack([[0.4 * _texture(rng, H, W, cells=3) for _ in range(3)] for _ in range(T)])
    Y = X + change * (0.1 + 0.9 * w[:, None]) + 0.05
    return dict(X=stored(X, xdt), Y=stored(Y, ydt), w=w)


@functools.lru_cache(maxsize=None)
def fidelity_reference(T, H, W, xdt, ydt, with_region=True):
    """(sums [T,10], bounds [T,10], worst element errors of the float32 restatement) of a case - computed once, shared by the tests."""
    inp = fidelity_inputs(T, H, W, xdt, ydt)
    rows = [fidelity_frame(inp["X"][t], inp["Y"][t], inp["w"][t] if with_region else None) for t in range(T)]
    return (np.stack([r[0] for r in rows]), np.stack([r[1]["bound"] for r in rows]),
            max(r[1]["worst_se"] for r in rows), max(r[1]["worst_ssim"] for r in rows))


@functools.lru_cache(maxsize=None)
def warp_inputs(T, H, W, dt):
    """A [T,3,H,W] as stored, fwd / bwd [T-1,2,H,W] float32-exact (smooth flows of a few pixels, bwd about -fwd resampled plus noise and
    planted inconsistent rectangles, as masktrack_ref.step_inputs), region [T,H,W]."""
    rng = _rng(f"pixel_score.warp.{T}.{H}.{W}.{dt}")
    amp = min(3.0, min(H, W) / 8.0)
    ys, xs = (a.astype(np.float64) for a in np.mgrid[0:H, 0:W])
    fwd, bwd = [], []
    for _ in range(T - 1):
        b = np.stack([mr._smooth(rng, H, W, amp) + 0.4 * amp, mr._smooth(rng, H, W, amp) - 0.3 * amp])
        t = mr._taps(xs - b[0], ys - b[1], H, W, np.float64)
        c = -np.stack([mr._sample(b[0], t), mr._sample(b[1], t)]) + rng.uniform(-0.05, 0.05, (2, H, W))
        for _ in range(2 if H >= 8 else 0):
            y0, x0 = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
            c[:, y0:y0 + max(3, H // 5), x0:x0 + max(3, W // 5)] += np.array([3.0, -2.0])[:, None, None]
        fwd.append(b), bwd.append(c)
    A = 1.05 * np.stack([[_texture(rng, H, W) for _ in range(3)] for _ in range(T)])
    f32 = lambda a: np.stack(a).astype(np.float32).astype(np.float64)   # noqa: E731
    return dict(A=stored(A, dt), fwd=f32(fwd), bwd=f32(bwd), w=region_input("warp", T, H, W))


@functools.lru_cache(maxsize=None)
def warp_reference(T, H, W, dt, with_bwd=True, with_region=True):
    """The float64 result of a case, the excluded pixels, and the bounds: per element of err (on pixels both sides call valid) and per
    sum 0 (when the valid sets agree)."""
    inp = warp_inputs(T, H, W, dt)
    bwd, w = (inp["bwd"] if with_bwd else None), (inp["w"] if with_region else None)
    ref = warp_video(inp["A"], inp["fwd"], bwd, w)
    r32 = warp_video(inp["A"], inp["fwd"], bwd, w, dtype=np.float32)
    both = ref["valid"] & r32["valid"]
    e = np.where(both, np.abs(r32["err"].astype(np.float64) - ref["err"]), 0.0)
    worst = float(e.max())
    elem = MARGIN * np.maximum(worst, FLOOR_REL_ERR * ref["err"])   # [T-1,H,W]
    ex = np.stack([warp_excluded(inp["fwd"][t], None if bwd is None else bwd[t]) for t in range(T - 1)])
    return dict(ref=ref, excluded=ex, elem_bound=elem, worst=worst, share=float(ex.mean()))


# ------------------------------------------------------------------------------------------------------------------ the exact cases
# (H, W, per-pair displacements (dx, dy), per-frame constants delta in units of 2^-8, dtype, planted inconsistent rectangle (t, y0, y1, x0, x1))
EXACT_CASES = [(9, 13, [(1, 0), (2, -1), (0, 1)], None, "f32", None), (9, 13, [(1, 0), (2, -1), (0, 1)], [0, 12, 4, 32], "f16", None),
               (12, 17, [(-2, 1), (1, 1)], [8, 0, 20], "f32", (1, 4, 7, 5, 9)), (5, 7, [(-1, 2)], [0, 64], "f16", None)]


def translation_video(H, W, disps, deltas=None, bad_rect=None, seed="pixel_score.exact"):
    """A random image (multiples of 2^-8 in [1/4, 1/2]) translated by the integer ``disps[t]`` between frames t and t+1, plus the per-frame
    constant ``deltas[t]`` * 2^-8 (all values stay inside [0, 1], the affine is the identity): fwd[t] = +d, bwd[t] = -d.  Everything is
    exact in float16 and float32, so the expectation is integer arithmetic: err = ((delta_{t+1} - delta_t) 2^-8)^2 at every valid pixel,
    valid = the pixel's target lies in the frame - (H - |dy|)(W - |dx|) pixels - and, with ``bad_rect`` (bwd[t] made inconsistent on
    [y0,y1) x [x0,x1)), is not in the rectangle."""
    rng = _rng(f"{seed}.{H}.{W}")
    T = len(disps) + 1
    d = np.asarray(disps, np.int64).reshape(T - 1, 2)
    pos = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(-d, 0)])   # frame t shows canvas[o + pos_t + x]
    m = int(np.abs(pos).max()) + 1
    canvas = rng.integers(64, 129, (3, H + 2 * m, W + 2 * m)) / 256.0
    deltas = np.zeros(T) if deltas is None else np.asarray(deltas, np.float64)
    A = np.stack([canvas[:, m + pos[t, 1]:m + pos[t, 1] + H, m + pos[t, 0]:m + pos[t, 0] + W] + deltas[t] / 256.0 for t in range(T)])
    fwd = np.broadcast_to(d.astype(np.float64)[:, :, None, None], (T - 1, 2, H, W)).copy()
    bwd = -fwd
    ys, xs = np.mgrid[0:H, 0:W]
    valid, valid_plain = [], []
    for t in range(T - 1):
        sx, sy = xs + d[t, 0], ys + d[t, 1]
        v = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        valid_plain.append(v.copy())
        if bad_rect is not None and bad_rect[0] == t:
            _, y0, y1, x0, x1 = bad_rect
            bwd[t][:, y0:y1, x0:x1] += 5.0
            v &= ~((sy >= y0) & (sy < y1) & (sx >= x0) & (sx < x1))
        valid.append(v)
    err = np.array([((deltas[t + 1] - deltas[t]) / 256.0) ** 2 for t in range(T - 1)])
    return dict(A=A, fwd=fwd, bwd=bwd, valid=np.stack(valid), valid_plain=np.stack(valid_plain), err=err, disps=d)
