"""The definition of the region edit (csrc/region.hip are the kernels, insv2v/region.py the host side), float64 numpy.

Resampling is the separable antialiased resampling ``torch.nn.functional.interpolate(..., antialias=True, align_corners=False)`` computes
on the CPU, applied to the CROP: per axis, with ``n_in`` source and ``n_out`` destination samples, ``scale = n_in / n_out``,
``s = max(scale, 1)``, and for destination index i: ``c = scale (i + 0.5)``, ``xmin = max(int(c - support s + 0.5), 0)``,
``xsize = min(int(c + support s + 0.5), n_in) - xmin``, weights ``f((j + xmin - c + 0.5) / s)`` for j < xsize, divided by their sum.
``bicubic`` is the cubic convolution with A = -0.5 (support 2), ``bilinear`` the triangle (support 1).  ``test_region_cpu.py`` pins this
restatement to ``interpolate`` in float64; after that it is the reference of the GPU tests.

Every planted misreading of the definition is a switch (``MISREADINGS``); the CPU tests require that the test inputs tell each from the
definition by more than the GPU tolerance (``need_gap``), so an input that cannot distinguish one fails there."""
import math

import numpy as np

CUBIC_A = -0.5
SUPPORT = {"bicubic": 2.0, "bilinear": 1.0}
MISREADINGS = ("a075", "no_antialias", "frame_clip", "unnormalised", "align_corners", "ramp_at_border", "no_down_clamp", "mask_twice", "ge_threshold")
EPS32 = 2.0 ** -24


def cubic(t, A=CUBIC_A, factored=False):
    """The cubic convolution kernel as interpolate writes it; ``factored``: its outer piece as A (t - 1) (t - 2)^2 - the same polynomial
    without the cancellation among terms of size 16, which is how the kernels (and the fp32 emulation) evaluate it."""
    t = np.abs(t)
    if factored:
        return np.where(t < 1.0, ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0, np.where(t < 2.0, (t - 1.0) * (t - 2.0) * (t - 2.0) * A, 0.0))
    return np.where(t < 1.0, ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0, np.where(t < 2.0, (((t - 5.0) * t + 8.0) * t - 4.0) * A, 0.0))


def triangle(t):
    t = np.abs(t)
    return np.where(t < 1.0, 1.0 - t, 0.0)


def axis_taps(n_in, n_out, kind, wrong=None, dtype=np.float64, lo=0, hi=None):
    """Per destination index: (xmin, weights) along one axis.  ``lo`` / ``hi`` (misreading ``frame_clip`` only): the box inside an axis of
    ``hi`` samples - the taps are then clipped at the frame and ``xmin`` may be negative or reach beyond ``n_in``."""
    A = -0.75 if wrong == "a075" else CUBIC_A
    f = (lambda t: cubic(t, A, dtype is np.float32)) if kind == "bicubic" else triangle
    sup = SUPPORT[kind]
    out = []
    for i in range(n_out):
        if wrong == "align_corners":
            scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
            c = scale * i + 0.5
        else:
            scale = n_in / n_out
            c = scale * (i + 0.5)
        s = 1.0 if wrong == "no_antialias" else max(scale, 1.0)
        first, last = (-lo, hi - lo) if wrong == "frame_clip" else (0, n_in)
        xmin = max(int(c - sup * s + 0.5), first)
        xsize = min(int(c + sup * s + 0.5), last) - xmin
        t = ((np.arange(xsize) + xmin - c + 0.5) / s).astype(dtype)
        w = f(t).astype(dtype)
        if wrong != "unnormalised":
            total = dtype(0)
            for v in w:                       # the sum in tap order, as interpolate forms it
                total = dtype(total + v)
            w = (w / total).astype(dtype)
        out.append((xmin, w))
    return out


def _apply(x, taps, axis, dtype):
    """One separable pass along ``axis`` (-1 or -2), each output a sum in tap order."""
    x = np.moveaxis(x, axis, -1)
    out = np.zeros(x.shape[:-1] + (len(taps),), dtype)
    for i, (xmin, w) in enumerate(taps):
        acc = np.zeros(x.shape[:-1], dtype)
        for j, wj in enumerate(w):
            acc = (acc + wj * x[..., xmin + j]).astype(dtype)
        out[..., i] = acc
    return np.moveaxis(out, -1, axis)


def resample(x, box, size, kind, wrong=None, dtype=np.float64):
    """x [..., H, W], box (x0, y0, x1, y1), size (w, h) -> [..., h, w]: the horizontal pass, then the vertical one (the kernels' order)."""
    x0, y0, x1, y1 = box
    w, h = size
    H, W = x.shape[-2:]
    if wrong == "frame_clip":
        tx, ty = axis_taps(x1 - x0, w, kind, wrong, dtype, x0, W), axis_taps(y1 - y0, h, kind, wrong, dtype, y0, H)
        tx, ty = [(m + x0, wt) for m, wt in tx], [(m + y0, wt) for m, wt in ty]
        return _apply(_apply(x.astype(dtype), tx, -1, dtype), ty, -2, dtype)
    crop = x[..., y0:y1, x0:x1].astype(dtype)
    return _apply(_apply(crop, axis_taps(x1 - x0, w, kind, wrong, dtype), -1, dtype), axis_taps(y1 - y0, h, kind, wrong, dtype), -2, dtype)


def abs_weight_sum(x, box, size, kind):
    """sum |w_y| |w_x| |x| per destination element: what the fp32 error bound scales with."""
    x0, y0, x1, y1 = box
    w, h = size
    ab = lambda taps: [(m, np.abs(wt)) for m, wt in taps]   # noqa: E731
    crop = np.abs(x[..., y0:y1, x0:x1].astype(np.float64))
    return _apply(_apply(crop, ab(axis_taps(x1 - x0, w, kind)), -1, np.float64), ab(axis_taps(y1 - y0, h, kind)), -2, np.float64)


def footprint(n_in, n_out, kind):
    """Per destination index the half-open range of source indices with a tap (whatever its weight)."""
    return [(m, m + len(w)) for m, w in axis_taps(n_in, n_out, kind)]


def mask_bbox(mask, threshold=0.5, wrong=None):
    """mask [T, H, W] -> int32 [T + 1, 4]: per frame and over all frames the half-open box (x0, y0, x1, y1) of ``mask > threshold``
    (strict; a NaN is outside); an empty frame gives (W, H, 0, 0)."""
    T, H, W = mask.shape
    inside = (mask >= threshold) if wrong == "ge_threshold" else (mask > threshold)
    out = np.zeros((T + 1, 4), np.int32)
    for t in range(T + 1):
        m = inside[t] if t < T else inside.any(0)
        ys, xs = np.nonzero(m)
        out[t] = (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) if len(xs) else (W, H, 0, 0)
    return out


def ramp(frame_hw, box, blend, wrong=None):
    """[bh, bw]: min(1, (d + 0.5) / blend), d = the distance in pixels to the nearest box edge that is not also a frame border; 1 for
    blend = 0 and for a box that is the whole frame."""
    H, W = frame_hw
    x0, y0, x1, y1 = box
    bh, bw = y1 - y0, x1 - x0
    if blend == 0:
        return np.ones((bh, bw))
    border = wrong == "ramp_at_border"
    inf = np.full((bh, bw), np.inf)
    xs, ys = np.arange(bw)[None, :] + np.zeros((bh, 1)), np.arange(bh)[:, None] + np.zeros((1, bw))
    d = np.minimum(np.minimum(xs if (x0 > 0 or border) else inf, (bw - 1 - xs) if (x1 < W or border) else inf),
                   np.minimum(ys if (y0 > 0 or border) else inf, (bh - 1 - ys) if (y1 < H or border) else inf))
    return np.minimum(1.0, (d + 0.5) / blend)


def down_src(source, box, size, wrong=None, dtype=np.float64):
    d = resample(source, box, size, "bicubic", dtype=dtype)
    return d if wrong == "no_down_clamp" else np.clip(d, -1.0, 1.0)


def paste(source, edit_w, down, box, mode="residual", blend=8, mask_w=None, wrong=None, dtype=np.float64):
    """source [n, C, H, W], edit_w / down [n, C, h, w], mask_w [n, h, w] or None -> the pasted frames [n, C, H, W]."""
    x0, y0, x1, y1 = box
    n, C, H, W = source.shape
    h, w = edit_w.shape[-2:]
    full, bsize = (0, 0, w, h), (x1 - x0, y1 - y0)
    out = source.astype(dtype).copy()
    src = out[..., y0:y1, x0:x1].copy()
    r = ramp((H, W), box, blend, wrong).astype(dtype)
    if mode == "residual":
        operand = (edit_w.astype(dtype) - down.astype(dtype)).astype(dtype)
        up = resample(operand, full, bsize, "bicubic", dtype=dtype)
        if wrong == "mask_twice" and mask_w is not None:
            up = up * np.clip(resample(mask_w, full, bsize, "bilinear", dtype=dtype), 0.0, 1.0)[:, None]
        res = src + r * up
    else:
        up = resample(edit_w, full, bsize, "bicubic", dtype=dtype)
        M = r if mask_w is None else r * np.clip(resample(mask_w, full, bsize, "bilinear", dtype=dtype), 0.0, 1.0)[:, None]
        res = src + M * (up - src)
    out[..., y0:y1, x0:x1] = np.clip(res, -1.0, 1.0).astype(dtype)
    return out


def measured_k(x, box, size, kind):
    """The worst ratio |fp32 emulation - float64| / (2^-24 sum |w_y||w_x||x|) over the elements of one case (0 where the scale is 0)."""
    a, b = resample(x, box, size, kind, dtype=np.float32).astype(np.float64), resample(x, box, size, kind)
    scale = EPS32 * abs_weight_sum(x, box, size, kind)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, np.abs(a - b) / scale, 0.0)
    return float(r.max())


def need_gap(name, ref, other, tol):
    """The habit of the other reference files: an input that cannot tell a misreading from the definition by more than the GPU
    tolerance fails here, on the CPU."""
    gap = float(np.max(np.abs(np.asarray(ref, np.float64) - np.asarray(other, np.float64))))
    assert gap > tol, f"the inputs cannot tell the misreading {name!r} from the definition: gap {gap:.3e} <= tolerance {tol:.3e}"
    return gap


# ---------------------------------------------------------------------------------------------------------------- the plan (integers)
def region_plan(frame_hw, size, bbox=None, box=None, pad=0.25):
    """The restatement of ``insv2v.region.region_plan`` the CPU test pins the module against: (x0, y0, x1, y1) only."""
    H, W = frame_hw
    w, h = size
    if box is not None:
        return tuple(box)
    if bbox is None:
        return (0, 0, W, H)
    x0, y0, x1, y1 = bbox
    g = math.ceil(pad * max(x1 - x0, y1 - y0))
    x0, y0, x1, y1 = x0 - g, y0 - g, x1 + g, y1 + g
    bw, bh = x1 - x0, y1 - y0
    if bw * h < bh * w:
        need = -(-bh * w // h)
        x0 -= (need - bw) // 2
        x1 = x0 + need
    elif bh * w < bw * h:
        need = -(-bw * h // w)
        y0 -= (need - bh) // 2
        y1 = y0 + need
    if x1 - x0 >= W:
        x0, x1 = 0, W
    if y1 - y0 >= H:
        y0, y1 = 0, H
    dx, dy = max(0, -x0) - max(0, x1 - W), max(0, -y0) - max(0, y1 - H)
    return (x0 + dx, y0 + dy, x1 + dx, y1 + dy)


# ---------------------------------------------------------------------------------------------------------------- the shared test inputs
SRC_SHAPE = (2, 3, 45, 70)       # the resample source [n, C, H, W]
TILE_W, TILE_H = 64, 16          # the kernels' destination tile (csrc/region.hip): sizes on either side of it are cases below
# (name, box (x0, y0, x1, y1), size (w, h)): boxes at the four corners, in the middle and the whole frame; destinations 24 x 16 and
# 8 x 8; one destination on each side of the tile edge; ratios 8, non-integer, 1, 1/3 and 1/8
RESAMPLE_CASES = [
    ("whole_24x16", (0, 0, 70, 45), (24, 16)),
    ("top_left_ratio_8", (0, 0, 64, 40), (8, 8)),
    ("bottom_right_equal_size", (46, 29, 70, 45), (24, 16)),
    ("top_right_ratio_third", (62, 0, 70, 8), (24, 24)),
    ("bottom_left_8x8", (0, 37, 21, 45), (8, 8)),
    ("middle_non_integer", (13, 9, 58, 38), (24, 16)),
    ("tile_minus_1", (0, 0, 70, 45), (TILE_W - 1, TILE_H - 1)),
    ("tile_exact", (0, 0, 70, 45), (TILE_W, TILE_H)),
    ("tile_plus_1", (0, 0, 70, 45), (TILE_W + 1, TILE_H + 1)),
    ("middle_ratio_eighth", (30, 20, 33, 22), (24, 16)),
]
PASTE_SHAPE = (2, 3, 37, 53)     # the paste source: sides that are no multiples of 8
PASTE_SIZE = (24, 16)            # the working clip (w, h)
PASTE_BOXES = {"two_borders": (0, 0, 30, 20), "middle": (9, 6, 45, 31),
               # boxes SMALLER than the working clip (the paste down-samples: its two larger stagings): ratios 2 and 4
               "half": (20, 15, 32, 23), "quarter": (20, 15, 26, 19)}
# The measured constant of the error bound K 2^-24 sum |w_y||w_x||x|: the worst ratio of the fp32 emulation above to the float64
# definition over RESAMPLE_CASES with both filters is 6.71 (test_region_cpu.py recomputes it and fails if it is larger); the tests use 4 x
# that, which also covers the kernels' fma contraction and the different rounding of the weights' argument.
K_MEASURED, K_FACTOR = 6.8, 4.0


def uniform(name, shape, lo=-1.0, hi=1.0):
    """Seeded fp32 values, a function of the name."""
    seed = int.from_bytes(name.encode(), "little") % (2 ** 32)
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


def resample_bound(x, box, size, kind):
    """Per element: K 2^-24 sum |w_y||w_x||x| plus one ulp of the result (fp32)."""
    ref = resample(x, box, size, kind)
    return K_FACTOR * K_MEASURED * EPS32 * abs_weight_sum(x, box, size, kind) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def paste_bound(source, edit_w, down, box, mode, mask_w=None):
    """Per element of the frame (0 outside the box) the fp32 bound of the paste.  K = K_FACTOR K_MEASURED as for the resample.
    residual: the operand edit - down is itself an fp32 rounding per tap (+1 on K); the ramp's division, its product with the resampled
    residual, the sum with the source and the clip's store are four more roundings of values no larger than |up| + |src| + 1.
    replace: the resampled edit and the resampled mask each carry their resample bound, the mask's scaled by |up - src|; the clamp, the
    two products, the difference, the sum and the store are six roundings of such values."""
    x0, y0, x1, y1 = box
    h, w = edit_w.shape[-2:]
    full, bsize, K = (0, 0, w, h), (x1 - x0, y1 - y0), K_FACTOR * K_MEASURED
    src = np.abs(source[..., y0:y1, x0:x1].astype(np.float64))
    if mode == "residual":
        op = edit_w.astype(np.float64) - down.astype(np.float64)
        up = np.abs(resample(op, full, bsize, "bicubic"))
        b = (K + 1) * EPS32 * abs_weight_sum(op, full, bsize, "bicubic") + 4 * EPS32 * (up + src + 1)
    else:
        up = resample(edit_w, full, bsize, "bicubic")
        am = 0.0 if mask_w is None else abs_weight_sum(mask_w, full, bsize, "bilinear")[:, None]
        b = K * EPS32 * (abs_weight_sum(edit_w, full, bsize, "bicubic") + am * np.abs(up - source[..., y0:y1, x0:x1])) + 6 * EPS32 * (np.abs(up) + src + 1)
    out = np.zeros(source.shape)
    out[..., y0:y1, x0:x1] = b
    return out


def paste_inputs(name, zero_half=False, constant=None):
    """(source, edit_w, down, mask_w) of a paste case, fp32: a source in [-1, 1], a working clip ``down`` and an edit that differs from it
    by up to 0.5 (``constant``: by exactly that; ``zero_half``: not at all in the right half of the working clip), and a mask that is
    soft on the left, exactly 0 in the right half."""
    n, C, H, W = PASTE_SHAPE
    w, h = PASTE_SIZE
    source = uniform(name + ".source", PASTE_SHAPE)
    down = uniform(name + ".down", (n, C, h, w), -0.75, 0.75)
    delta = np.full((n, C, h, w), constant, np.float32) if constant is not None else uniform(name + ".delta", (n, C, h, w), -0.5, 0.5)
    if zero_half:
        delta[..., w // 2:] = 0.0
    mask_w = uniform(name + ".mask", (n, h, w), -0.2, 1.2)
    mask_w[..., w // 2:] = 0.0
    return source, (down + delta).astype(np.float32), down, mask_w
