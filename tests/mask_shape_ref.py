"""The definition of a shaped mask (insv2v_mask_shape; include/insv2v_hip.h) in numpy: integers for the distance
transform and the two hard decisions, float64 for the ramp.  Nothing here imports the product.

  inside    = m > tau (strict; a NaN is outside)
  D2_out(x) = squared Euclidean distance to the nearest inside pixel of the frame, D2_in(x) to the nearest outside pixel; the frame
              border is not outside; every D2 > R^2, and a frame without the set, gives FAR = (R + 1)^2
  s         = sqrt(D2_out) on outside pixels, 1 - sqrt(D2_in) on inside pixels
  shaped    = 1 where s <= g, else 0 where s >= g + f, else u = (g + f - s) / f -> u or u^2 (3 - 2 u), kept inside [2^-126, 1 - 2^-24]
  support   = shaped > 0

``grow`` and ``feather`` are fp32 numbers (what the C entry receives); everything after that is float64.
"""
import math
from fractions import Fraction

import numpy as np

MAX = 32
PROFILES = ("linear", "smooth")
RAMP_LO, RAMP_HI = 2.0 ** -126, 1.0 - 2.0 ** -24


def params(grow, feather):
    """(g, f, g + f) in float64 from the fp32 values of grow and feather."""
    g, f = float(np.float32(grow)), float(np.float32(feather))
    return g, f, g + f


def check_limits(grow, feather):
    g, f, h = params(grow, feather)
    if not (math.isfinite(g) and math.isfinite(f)) or not (-MAX <= g <= MAX and 0 <= f <= MAX and h >= -MAX):
        raise ValueError(f"grow {grow} / feather {feather} outside the limits")


def radius(grow, feather):
    """(R, FAR): the smallest search radius that decides every pixel, and what a distance beyond it is reported as."""
    g, f, h = params(grow, feather)
    R = int(math.ceil(max(h, 1.0 - g, 1.0)))
    return R, (R + 1) ** 2


def thresholds_exact(grow, feather):
    """The four integer thresholds from exact rational arithmetic on the fp32 values of grow and feather:
    out_one = floor(g^2) (g >= 0), out_zero = ceil((g+f)^2) (g + f > 0), in_one = ceil((1-g)^2) (g < 1), in_zero = floor((1-g-f)^2)
    (g + f <= 1); -1 / 0 where the comparison holds for no / every D2 >= 0."""
    g, f = Fraction(float(np.float32(grow))), Fraction(float(np.float32(feather)))
    h = g + f
    return dict(out_one=math.floor(g * g) if g >= 0 else -1,
                out_zero=math.ceil(h * h) if h > 0 else 0,
                in_one=math.ceil((1 - g) ** 2) if g < 1 else 0,
                in_zero=math.floor((1 - h) ** 2) if h <= 1 else -1)


def inside_set(m, threshold=0.5):
    with np.errstate(invalid="ignore"):
        return np.asarray(m, dtype=np.float32) > np.float32(threshold)   # NaN > tau is False


def _vertical(hit, cap):
    """Per pixel the distance (in rows, capped at ``cap``) to the nearest True of its column in ``hit`` [H,W]."""
    H = hit.shape[0]
    v = np.full(hit.shape, cap, dtype=np.int64)
    for dy in range(0, min(cap, H)):
        sh = np.zeros_like(hit)
        sh[dy:] |= hit[:H - dy]
        sh[:H - dy] |= hit[dy:]
        v = np.where(sh & (v == cap), dy, v)
    return v


def squared_distance(hit, R):
    """[H,W] bool -> int64 squared Euclidean distance to the nearest True, FAR = (R+1)^2 beyond R or when there is none."""
    H, W = hit.shape
    far = (R + 1) ** 2
    v2 = _vertical(hit, R + 1) ** 2
    d = np.full((H, W), far, dtype=np.int64)
    for dx in range(-R, R + 1):
        if abs(dx) >= W:
            continue
        lo, hi = max(0, -dx), min(W, W - dx)     # x with 0 <= x + dx < W
        d[:, lo:hi] = np.minimum(d[:, lo:hi], dx * dx + v2[:, lo + dx:hi + dx])
    return np.where(d > R * R, far, d)


def distances(m, threshold, R):
    """m [T,H,W] -> (inside bool, D2_out, D2_in int64)."""
    ins = inside_set(m, threshold)
    d2o = np.stack([squared_distance(f, R) for f in ins])
    d2i = np.stack([squared_distance(~f, R) for f in ins])
    return ins, d2o, d2i


def signed_distance(ins, d2o, d2i):
    return np.where(ins, 1.0 - np.sqrt(d2i.astype(np.float64)), np.sqrt(d2o.astype(np.float64)))


def mask_shape(m, grow=0.0, feather=0.0, threshold=0.5, profile="smooth"):
    """m [T,H,W] -> dict(shaped float64, support float64 0/1, d2_out, d2_in int64, inside, one, zero, ramp bool, s float64).  The hard
    decisions are those on s in float64; ``decide_on_integers`` states them on D2 and the tests show the two agree."""
    check_limits(grow, feather)
    if profile not in PROFILES:
        raise ValueError(profile)
    g, f, h = params(grow, feather)
    R, far = radius(grow, feather)
    ins, d2o, d2i = distances(m, threshold, R)
    s = signed_distance(ins, d2o, d2i)
    one = s <= g
    zero = ~one & (s >= h)
    ramp = ~one & ~zero
    shaped = one.astype(np.float64)
    if ramp.any():
        u = (h - s[ramp]) / f
        val = u if profile == "linear" else u * u * (3.0 - 2.0 * u)
        shaped[ramp] = np.clip(val, RAMP_LO, RAMP_HI)
    return dict(shaped=shaped, support=(shaped > 0).astype(np.float64), d2_out=d2o, d2_in=d2i, inside=ins, one=one, zero=zero, ramp=ramp, s=s)


def decide_on_integers(ins, d2o, d2i, th):
    """(one, zero) from the integer maps and a dict of the four thresholds (the planner's, or ``thresholds_exact``)."""
    one = np.where(ins, d2i >= th["in_one"], d2o <= th["out_one"])
    zero = ~one & np.where(ins, d2i <= th["in_zero"], d2o >= th["out_zero"])
    return one, zero


def ramp_fp32(ins, d2o, d2i, ramp, grow, feather, profile):
    """The ramp restated in fp32 in the kernel's operation order (no FMA contraction, numpy's correctly rounded sqrt and division):
    s from sqrt of the integer, u = (gf - s) / f with gf = fp32(g + f), then u * u * (3 - 2 u), clamped -> fp32 values on ``ramp``."""
    g, f, h = params(grow, feather)
    gf, f32 = np.float32(h), np.float32(f)
    one, two, three = np.float32(1), np.float32(2), np.float32(3)
    s = np.where(ins, one - np.sqrt(d2i.astype(np.float32)), np.sqrt(d2o.astype(np.float32))).astype(np.float32)[ramp]
    u = (gf - s) / f32
    val = u if profile == "linear" else (u * u) * (three - two * u)
    return np.clip(val, np.float32(RAMP_LO), np.float32(RAMP_HI)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the GPU file's cases
SQRT2 = float(np.float32(math.sqrt(2.0)))   # fp32(sqrt 2) < sqrt 2: a pixel at squared distance 2 is NOT reached
TAU = 0.5
# (name, T, H, W, grow, feather, profile)
CASES = [
    ("1x1_inside", 1, 1, 1, 0.0, 0.0, "smooth"),
    ("1x1_outside", 1, 1, 1, 3.0, 2.0, "smooth"),
    ("row", 2, 1, 37, 2.5, 4.0, "smooth"),
    ("column", 2, 37, 1, 2.5, 4.0, "smooth"),
    ("R_beyond_frame", 3, 9, 13, 20.0, 12.0, "smooth"),
    ("shrink_smooth", 3, 17, 33, -2.0, 3.0, "smooth"),
    ("shrink_linear", 3, 17, 33, -2.0, 3.0, "linear"),
    ("feather_max_smooth", 3, 17, 33, 0.0, 32.0, "smooth"),
    ("feather_max_linear", 3, 17, 33, 0.0, 32.0, "linear"),
    ("sqrt2_hard", 3, 17, 33, SQRT2, 0.0, "smooth"),
    ("row_tiles", 2, 40, 521, 32.0, 32.0, "smooth"),
    ("special_frames", 5, 64, 96, 4.0, 8.0, "smooth"),
]


def _blobs(rng, H, W, n):
    """A frame of background values below tau with n blobs above it (rectangles and single pixels), a few pixels exactly at tau beside them
    (strictly: outside) and soft values on both sides of tau."""
    m = rng.uniform(0.0, 0.45, size=(H, W))
    for _ in range(n):
        h, w = int(rng.integers(1, max(2, H // 2 + 1))), int(rng.integers(1, max(2, W // 3 + 1)))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        m[y:y + h, x:x + w] = rng.uniform(0.55, 1.0, size=(h, w))
        m[y, x] = 1.0
        if x + w < W:
            m[y, x + w] = TAU
        if y + h < H:
            m[y + h, x] = TAU
    return m


def case_input(name):
    """The fp32 mask [T,H,W] of a case; the same array on every call."""
    _, T, H, W, g, f, _ = next(c for c in CASES if c[0] == name)
    rng = np.random.default_rng(100000 * T + 1000 * H + W)
    if name == "1x1_inside":
        return np.ones((1, 1, 1), np.float32)
    if name == "1x1_outside":
        return np.full((1, 1, 1), 0.25, np.float32)
    if name == "row_tiles":   # R = 64: single pixels and a rectangle on both sides of the row tiles' boundaries (256, 512) and on all four borders
        m = rng.uniform(0.0, 0.45, size=(T, H, W))
        for t, y, x in ((0, 0, 0), (0, 39, 255), (0, 20, 512), (0, 10, 520), (1, 39, 0), (1, 0, 256), (1, 5, 511), (1, 39, 520), (1, 0, 400)):
            m[t, y, x] = 1.0
        m[1, 8:31, 230:290] = 0.8      # an interior up to 11 pixels deep across the boundary at 256
        m[0, 30:40, 500:521] = 0.7     # and one that touches the bottom and right borders across the boundary at 512
        m[1, 20, 256] = TAU            # a hole exactly at tau inside the rectangle
        return m.astype(np.float32)
    if name == "special_frames":
        m = np.stack([_blobs(rng, H, W, 4) for _ in range(T)])
        m[0] = 0.2                                      # empty
        m[1] = 0.9                                      # full
        m[2, 5:20, 40:70] = np.nan                      # NaN: outside, also in the middle of ...
        m[2, 10:50, 10:60] = np.where(np.isnan(m[2, 10:50, 10:60]), np.nan, 0.75)   # ... a blob
        m[2, 30:34, 20:30] = TAU                        # exactly tau: outside
        m[3] = 0.1
        m[3, H - 1, W - 1] = 0.6                        # a single inside pixel in a corner
        return m.astype(np.float32)
    n = 1 if H * W < 64 else 3
    m = np.stack([_blobs(rng, H, W, n) for _ in range(T)])
    if name.startswith(("shrink", "feather_max", "sqrt2")):
        m[0, 3:13, 8:22] = 0.9      # thick enough to survive a shrink by 2
        m[0, 7, 14] = 0.3           # with a hole
    return m.astype(np.float32)


def case_reference(name):
    """(input, the reference's dict) of a case."""
    _, T, H, W, g, f, profile = next(c for c in CASES if c[0] == name)
    m = case_input(name)
    return m, mask_shape(m, g, f, TAU, profile)


def ramp_bound(r, grow, feather, profile):
    """The bound on |kernel - float64| over the ramp of a reference result: 4 x the worst departure of the fp32 restatement in the kernel's
    operation order on these inputs (the factor covers FMA contraction and the device's sqrtf), floored at one fp32 rounding of a value
    below 1.  -> (bound, the restatement's worst departure)."""
    if not r["ramp"].any():
        return 2.0 ** -24, 0.0
    worst = float(np.abs(ramp_fp32(r["inside"], r["d2_out"], r["d2_in"], r["ramp"], grow, feather, profile).astype(np.float64) - r["shaped"][r["ramp"]]).max())
    return max(4.0 * worst, 2.0 ** -24), worst
