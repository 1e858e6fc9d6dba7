"""The definition of the region edit that follows the object (csrc/region.hip are the kernels,
insv2v/region_track.py the host side), float64 numpy, on top of ``region_ref`` (section 26).

A track is n boxes (x0, y0, x1, y1) of doubles, half-open in continuous pixel coordinates: pixel j covers [j, j + 1), its centre is
j + 0.5.  A frame's COVER is [floor(x0), ceil(x1)) x [floor(y0), ceil(y1)).

Resample (box -> n_out samples), per axis: e = x1 - x0, X0 = floor(x0), n_in = ceil(x1) - X0, scale = e / n_out, s = max(scale, 1),
c = (x0 - X0) + scale (i + 0.5) in cover coordinates; tap range and weights as in ``region_ref.axis_taps`` with this c and this n_in: the
taps are clipped at the COVER.  Paste (n_w working samples -> the cover's pixels): scale' = n_w / e, s = max(scale', 1),
c = scale' (X + 0.5 - x0), taps clipped to [0, n_w); ramp = clamp(d / blend, 0, 1), d = the signed distance from the pixel's centre to
the nearest box edge that is not a frame border (x0 == 0, x1 == W, y0 == 0, y1 == H exactly); blend == 0: 1 where the centre lies inside
the half-open box, else 0; no such edge: 1.  A pixel under a ramp of 0 keeps the source.

Every planted misreading is a switch (``MISREADINGS``); ``test_region_track_cpu.py`` requires that the GPU file's inputs tell each from
the definition by more than the GPU tolerance (``region_ref.need_gap``)."""
import math

import numpy as np

import region_ref as rr

MISREADINGS = ("floor_box", "no_half_pixel", "cover_scale", "frame_clip", "frame0_box", "plane_index", "ramp_from_cover", "paste_from_cover",
               "smooth_unnormalised", "no_containment")
EPS32 = rr.EPS32
TRACK_SUBPIXEL = 256


def cover(box):
    x0, y0, x1, y1 = box
    return math.floor(x0), math.floor(y0), math.ceil(x1), math.ceil(y1)


def _taps(centres, s, n_in, kind, dtype, first=0, last=None):
    """Per centre c (in the coordinates of an axis of ``n_in`` samples): (xmin, weights), the expressions of ``region_ref.axis_taps``."""
    f = (lambda t: rr.cubic(t, rr.CUBIC_A, dtype is np.float32)) if kind == "bicubic" else rr.triangle
    sup, last, out = rr.SUPPORT[kind], (n_in if last is None else last), []
    for c in centres:
        xmin = max(int(c - sup * s + 0.5), first)
        xsize = max(min(int(c + sup * s + 0.5), last) - xmin, 0)
        t = ((np.arange(xsize) + xmin - c + 0.5) / s).astype(dtype)
        w = f(t).astype(dtype)
        total = dtype(0)
        for v in w:
            total = dtype(total + v)
        with np.errstate(divide="ignore", invalid="ignore"):
            w = (w / total).astype(dtype)
        out.append((xmin, w))
    return out


def down_taps(lo, hi, n_out, kind, wrong=None, dtype=np.float64, limit=None):
    """The taps of one axis of the resample in FRAME coordinates: the box [lo, hi) -> n_out samples (``limit``: the frame's size, the
    misreading ``frame_clip`` only)."""
    X0, X1 = math.floor(lo), math.ceil(hi)
    n_in, e, off = X1 - X0, hi - lo, lo - X0
    scale = (n_in if wrong == "cover_scale" else e) / n_out
    if wrong == "floor_box":
        off = 0.0
    half = 0.0 if wrong == "no_half_pixel" else 0.5
    centres = [off + scale * (i + half) for i in range(n_out)]
    first, last = (-X0, limit - X0) if wrong == "frame_clip" else (0, n_in)
    return [(m + X0, w) for m, w in _taps(centres, max(scale, 1.0), n_in, kind, dtype, first, last)]


def up_taps(lo, hi, n_w, kind, wrong=None, dtype=np.float64):
    """The taps of one axis of the paste, per pixel of the cover of [lo, hi), in the coordinates of the working image of n_w samples."""
    X0, X1 = math.floor(lo), math.ceil(hi)
    scale = n_w / (hi - lo)
    origin = float(X0) if wrong == "paste_from_cover" else lo
    centres = [scale * (X + 0.5 - origin) for X in range(X0, X1)]
    return _taps(centres, max(scale, 1.0), n_w, kind, dtype)


def _apply2(x, tx, ty, dtype):
    """The horizontal pass, then the vertical one, of the rows and columns the taps touch (``region_ref._apply``: sums in tap order)."""
    xa, xb = min(m for m, _ in tx), max(m + len(w) for m, w in tx)
    ya, yb = min(m for m, _ in ty), max(m + len(w) for m, w in ty)
    crop = x[..., ya:yb, xa:xb].astype(dtype)
    return rr._apply(rr._apply(crop, [(m - xa, w) for m, w in tx], -1, dtype), [(m - ya, w) for m, w in ty], -2, dtype)


def _box_of(boxes, n, c, C, wrong):
    if wrong == "frame0_box":
        return boxes[0]
    if wrong == "plane_index":
        return boxes[(n * C + c) % len(boxes)]
    return boxes[n]


def resample_track(x, boxes, size, kind, wrong=None, dtype=np.float64, clamp=None):
    """x [n, C, H, W], boxes n x (x0, y0, x1, y1), size (w, h) -> [n, C, h, w]."""
    n, C, H, W = x.shape
    w, h = size
    out = np.zeros((n, C, h, w), dtype)
    for i in range(n):
        for c in range(C):
            x0, y0, x1, y1 = _box_of(boxes, i, c, C, wrong)
            out[i, c] = _apply2(x[i, c], down_taps(x0, x1, w, kind, wrong, dtype, W), down_taps(y0, y1, h, kind, wrong, dtype, H), dtype)
    return np.clip(out, *clamp) if clamp is not None else out


def abs_weight_sum_track(x, boxes, size, kind):
    """sum |w_y| |w_x| |x| per destination element: what the fp32 error bound scales with."""
    n, C, H, W = x.shape
    w, h = size
    ab = lambda taps: [(m, np.abs(wt)) for m, wt in taps]   # noqa: E731
    out = np.zeros((n, C, h, w))
    for i in range(n):
        x0, y0, x1, y1 = boxes[i]
        out[i] = _apply2(np.abs(x[i].astype(np.float64)), ab(down_taps(x0, x1, w, kind)), ab(down_taps(y0, y1, h, kind)), np.float64)
    return out


def measured_k(x, boxes, size, kind):
    """The worst ratio |fp32 emulation - float64| / (2^-24 sum |w_y||w_x||x|) over the elements of one case."""
    a, b = resample_track(x, boxes, size, kind, dtype=np.float32).astype(np.float64), resample_track(x, boxes, size, kind)
    scale = EPS32 * abs_weight_sum_track(x, boxes, size, kind)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(scale > 0, np.abs(a - b) / scale, 0.0)
    return float(r.max())


# The constant of the error bound K 2^-24 sum |w_y||w_x||x| (section 26's form): the worst ratio of the fp32 emulation above to the
# float64 definition over RESAMPLE_CASES with both filters (test_region_track_cpu.py recomputes it and fails if it is larger); the GPU
# tests use K_FACTOR x that, which also covers the kernels' fma contraction.  Measured from the emulation on the CPU, never from the kernel.
K_MEASURED, K_FACTOR = 7.8, 4.0


def resample_bound(x, boxes, size, kind):
    ref = resample_track(x, boxes, size, kind)
    return K_FACTOR * K_MEASURED * EPS32 * abs_weight_sum_track(x, boxes, size, kind) + np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def ramp_track(frame_hw, box, blend, wrong=None):
    """[cover h, cover w]: the ramp over the pixels of the box's cover."""
    H, W = frame_hw
    x0, y0, x1, y1 = box
    X0, Y0, X1, Y1 = cover(box)
    left, right, top, bottom = x0 != 0, x1 != W, y0 != 0, y1 != H
    if wrong == "ramp_from_cover":
        x0, y0, x1, y1 = X0, Y0, X1, Y1
    cx, cy = np.arange(X0, X1)[None, :] + 0.5 + np.zeros((Y1 - Y0, 1)), np.arange(Y0, Y1)[:, None] + 0.5 + np.zeros((1, X1 - X0))
    inf = np.full(cx.shape, np.inf)
    d = np.minimum(np.minimum(cx - x0 if left else inf, x1 - cx if right else inf), np.minimum(cy - y0 if top else inf, y1 - cy if bottom else inf))
    inside = ((cx >= x0) | (not left)) & ((cx < x1) | (not right)) & ((cy >= y0) | (not top)) & ((cy < y1) | (not bottom))
    if blend == 0:
        return inside.astype(np.float64)
    return np.where(np.isinf(d), 1.0, np.clip(d / blend, 0.0, 1.0))


def paste_track(source, edit_w, down, boxes, mode="residual", blend=8, mask_w=None, wrong=None, dtype=np.float64):
    """source [n, C, H, W], edit_w / down [n, C, h, w], mask_w [n, h, w] or None -> the pasted frames [n, C, H, W]: frame i in its own
    box, only the box's cover written."""
    n, C, H, W = source.shape
    h, w = edit_w.shape[-2:]
    out = source.astype(dtype).copy()
    for i in range(n):
        for c in range(C):
            box = _box_of(boxes, i, c, C, wrong)
            x0, y0, x1, y1 = box
            X0, Y0, X1, Y1 = cover(box)
            tx, ty = up_taps(x0, x1, w, "bicubic", wrong, dtype), up_taps(y0, y1, h, "bicubic", wrong, dtype)
            src = out[i, c, Y0:Y1, X0:X1].copy()
            r = ramp_track((H, W), box, blend, wrong).astype(dtype)
            with np.errstate(invalid="ignore"):
                if mode == "residual":
                    operand = (edit_w[i, c].astype(dtype) - down[i, c].astype(dtype)).astype(dtype)
                    add = r * _apply2(operand, tx, ty, dtype)
                else:
                    M = r
                    if mask_w is not None:
                        mx, my = up_taps(x0, x1, w, "bilinear", wrong, dtype), up_taps(y0, y1, h, "bilinear", wrong, dtype)
                        M = r * np.clip(_apply2(mask_w[i], mx, my, dtype), 0.0, 1.0)
                    add = M * (_apply2(edit_w[i, c], tx, ty, dtype) - src)
            add = np.where(r == 0, 0.0, add).astype(dtype)      # under a ramp of 0 the source stays (what was resampled may be 0 / 0)
            res = np.where(add == 0, src, src + add)
            out[i, c, Y0:Y1, X0:X1] = np.where(np.isnan(res), res, np.clip(res, -1.0, 1.0)).astype(dtype)
    return out


def paste_bound(source, edit_w, down, boxes, mode, mask_w=None):
    """``region_ref.paste_bound`` per frame over its cover (0 outside): the same count of roundings - the ramp is one division as there."""
    n, C, H, W = source.shape
    h, w = edit_w.shape[-2:]
    K, out = K_FACTOR * K_MEASURED, np.zeros(source.shape)
    for i in range(n):
        x0, y0, x1, y1 = boxes[i]
        X0, Y0, X1, Y1 = cover(boxes[i])
        src = source[i, :, Y0:Y1, X0:X1].astype(np.float64)
        tx, ty = up_taps(x0, x1, w, "bicubic"), up_taps(y0, y1, h, "bicubic")
        ab = lambda taps: [(m, np.nan_to_num(np.abs(wt))) for m, wt in taps]   # noqa: E731
        clean = lambda taps: [(m, np.nan_to_num(wt)) for m, wt in taps]   # noqa: E731
        if mode == "residual":
            op = edit_w[i].astype(np.float64) - down[i].astype(np.float64)
            up = np.abs(_apply2(op, clean(tx), clean(ty), np.float64))
            b = (K + 1) * EPS32 * _apply2(np.abs(op), ab(tx), ab(ty), np.float64) + 4 * EPS32 * (up + np.abs(src) + 1)
        else:
            up = _apply2(edit_w[i].astype(np.float64), clean(tx), clean(ty), np.float64)
            am = 0.0
            if mask_w is not None:
                am = _apply2(np.abs(mask_w[i].astype(np.float64)), ab(up_taps(x0, x1, w, "bilinear")), ab(up_taps(y0, y1, h, "bilinear")), np.float64)[None]
            b = K * EPS32 * (_apply2(np.abs(edit_w[i].astype(np.float64)), ab(tx), ab(ty), np.float64) + am * np.abs(up - src)) + 6 * EPS32 * (np.abs(up) + np.abs(src) + 1)
        out[i, :, Y0:Y1, X0:X1] = b
    return out


# ---------------------------------------------------------------------------------------------------------------- the plan (numbers)
def track_plan(frame_hw, size, bboxes, pad=0.25, smooth=2.0, wrong=None):
    """The restatement of ``insv2v.region_track.track_plan`` the CPU test pins the module against: the boxes only."""
    H, W = frame_hw
    w, h = size
    live = [t for t, b in enumerate(bboxes) if b[2] > b[0] and b[3] > b[1]]
    if not live:
        raise ValueError("empty")
    bw0, bh0 = max(bboxes[t][2] - bboxes[t][0] for t in live), max(bboxes[t][3] - bboxes[t][1] for t in live)
    sx0, sy0, sx1, sy1 = rr.region_plan((H, W), (w, h), bbox=(0, 0, bw0, bh0), pad=pad)
    T, axes = len(bboxes), []
    for lo, hi, B, limit in ((0, 2, sx1 - sx0, W), (1, 3, sy1 - sy0, H)):
        raw = np.interp(np.arange(T), live, [(bboxes[t][lo] + bboxes[t][hi]) / 2 for t in live])   # linear between, held at the ends
        cs = raw.copy()
        if smooth > 0:
            R = math.ceil(3 * smooth)
            for t in range(T):
                ks = np.arange(max(0, t - R), min(T, t + R + 1))
                g = np.exp(-(ks - t) ** 2 / (2.0 * smooth * smooth))
                full = np.exp(-np.arange(-R, R + 1) ** 2 / (2.0 * smooth * smooth)).sum()
                cs[t] = (g * raw[ks]).sum() / (full if wrong == "smooth_unnormalised" else g.sum())
        origins = []
        for t in range(T):
            o = round((cs[t] - B / 2) * TRACK_SUBPIXEL) / TRACK_SUBPIXEL
            if t in live and wrong != "no_containment":
                o = max(min(o, bboxes[t][lo]), bboxes[t][hi] - B)
            origins.append(float(min(max(o, 0), limit - B)))
        axes.append((origins, B))
    return [(x, y, x + axes[0][1], y + axes[1][1]) for x, y in zip(axes[0][0], axes[1][0])]


# ---------------------------------------------------------------------------------------------------------------- the shared test inputs
SRC_SHAPE = (3, 2, 75, 110)      # the resample source [n, C, H, W]
TILE_W, TILE_H = rr.TILE_W, rr.TILE_H


def moved(box, shifts):
    """One box per shift (dx, dy): the box moved, its size kept."""
    return [(box[0] + dx, box[1] + dy, box[2] + dx, box[3] + dy) for dx, dy in shifts]


SHIFTS = [(0.0, 0.0), (0.37109375, 1.2109375), (-3.62890625, 2.05078125)]
# (name, boxes - one per frame -, size (w, h), clamp).  Vertical ratios: <= 1.1 (the smallest staging), <= 3 (the middle one), above (the largest).
RESAMPLE_CASES = [
    ("tile_minus_1", moved((10.25, 5.5, 90.75, 60.125), SHIFTS), (TILE_W - 1, TILE_H - 1), None),            # staging: the largest (3.6)
    ("tile_exact", moved((10.25, 5.5, 90.75, 45.5), SHIFTS), (TILE_W, TILE_H), None),                        # the middle one (2.5)
    ("tile_plus_1", moved((10.25, 5.5, 90.75, 22.625), SHIFTS), (TILE_W + 1, TILE_H + 1), None),             # the smallest (1.007)
    ("subpixel_shift_ratio_1", moved((20.5, 10.25, 44.5, 26.25), [(0.0, 0.0), (0.25, 0.125), (0.66015625, 0.90234375)]), (24, 16), None),
    ("ratio_8_x_third_y", moved((4.3125, 30.6875, 68.3125, 38.6875), SHIFTS), (8, 24), None),
    ("ratio_2p67_x_eighth_y", moved((8.4375, 20.71875, 72.4375, 23.71875), SHIFTS), (24, 24), None),
    ("ratio_eighth_x_8_y", moved((50.1875, 4.40625, 53.1875, 68.40625), SHIFTS), (24, 8), None),
    ("x0_is_0_y1_is_H", [(0.0, 44.5, 45.25, 75.0), (0.0, 43.25, 45.25, 75.0), (0.0, 50.125, 40.5, 75.0)], (24, 16), None),   # sizes differ per frame
    ("cover_touches_border", [(0.25, 0.5, 50.75, 40.5), (60.3125, 40.1875, 109.625, 74.6875), (0.75, 34.25, 109.25, 74.75)], (40, 24), None),
    ("clamped", moved((10.25, 5.5, 90.75, 45.5), SHIFTS), (24, 16), (-0.5, 0.5)),
]
CHUNK_SHAPE, CHUNK_SIZE = (65, 1, 20, 24), (16, 8)      # 65 frames: two launches, frames 63 and 64 either side of the boundary
CHUNK_BOXES = [(1.0 + 0.0625 * t, 0.5 + 0.03125 * t, 13.0 + 0.125 * t, 10.5 + 0.0625 * t) for t in range(65)]
PASTE_SHAPE = (3, 2, 37, 53)
PASTE_SIZE = (24, 16)
PASTE_BOXES = {"middle": moved((9.25, 6.5, 45.25, 30.5), SHIFTS),
               "two_borders": [(0.0, 0.0, 30.5, 20.25), (0.0, 0.0, 31.125, 20.75), (22.5, 16.75, 53.0, 37.0)],
               # boxes SMALLER than the working clip (the paste down-samples: its two larger stagings): ratios 2 and 4
               "half": moved((20.3125, 15.1875, 32.3125, 23.1875), SHIFTS), "quarter": moved((20.3125, 15.1875, 26.3125, 19.1875), SHIFTS)}


def paste_inputs(name, constant=None, zero_half=False):
    """``region_ref.paste_inputs`` for the three frames of ``region_track_ref.PASTE_SHAPE``."""
    n, C, H, W = PASTE_SHAPE
    w, h = PASTE_SIZE
    source = rr.uniform(name + ".source", PASTE_SHAPE)
    down = rr.uniform(name + ".down", (n, C, h, w), -0.75, 0.75)
    delta = np.full((n, C, h, w), constant, np.float32) if constant is not None else rr.uniform(name + ".delta", (n, C, h, w), -0.5, 0.5)
    if zero_half:
        delta[..., w // 2:] = 0.0
    mask_w = rr.uniform(name + ".mask", (n, h, w), -0.2, 1.2)
    mask_w[..., w // 2:] = 0.0
    return source, (down + delta).astype(np.float32), down, mask_w
