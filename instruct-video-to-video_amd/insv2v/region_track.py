"""A region edit that follows the object: one real-valued box per frame (csrc/region.hip are the kernels,
tests/region_track_ref.py the float64 definition).

``edit_region`` edits ONE box per unit, the union of the mask over all frames.  For anything that moves that is the wrong box: the object
is a small part of the working clip and the edit runs at a fraction of the resolution the feature exists to provide.  ``track=`` gives
every frame its own box of one fixed size that travels with the object - by fractions of a pixel, because an integer box that follows a
smooth motion steps by whole pixels and the whole working clip would shake by 1 / ratio of a working pixel from frame to frame.

  check_track            the parameters of ``track=`` (``TRACK_KEYS``), completed with their defaults
  track_plan             a pure function of numbers: per-frame bounding boxes -> per-frame boxes of one size
  given_track            the same dict for boxes the caller gives (``track=dict(boxes=[...])``), validated
  crop_to_working_track  every frame's box at working size: ``ops.region_resample_track``
  paste_back_track       the working-resolution edit laid over each frame's own box: ``ops.region_paste_track``

``insv2v.region.edit_region(..., track=True)`` and the ``track`` key of ``edit_regions``' units are the drivers.  ``smooth=2.0`` is a
starting value, NOT tuned here (as every default of sections 18 - 26).  As for a static box, ``strength_map="mask"`` passes through to the
inner edit and a tensor ``strength_map`` raises ValueError there (``region._check_strength_map``): it is not resampled along the track."""
import math

import torch

from . import ops
from .region import MAX_RATIO, REGION_DEFAULTS, _check_frames, _check_mask, _check_size, _device, _is_num, _mask_box

TRACK_KEYS = ("smooth", "boxes")
TRACK_DEFAULTS = dict(smooth=2.0, boxes=None)
TRACK_SUBPIXEL = 256   # origins are multiples of 1 / 256 pixel: x0 + Bw is exact in double


def check_track(track=True):
    """``track``: True (the defaults) or a dict with keys among ``TRACK_KEYS`` -> the complete dict.  ``smooth``: the sigma in frames of
    the Gaussian the centres are smoothed with (0: none); ``boxes``: None (planned from the per-frame mask) or one (x0, y0, x1, y1) of
    finite numbers per frame.  ValueError otherwise; nothing is launched."""
    if track is True:
        track = {}
    if not isinstance(track, dict) or set(track) - set(TRACK_KEYS):
        raise ValueError(f"track must be True or a dict with keys among {TRACK_KEYS}, got {track!r}")
    t = dict(TRACK_DEFAULTS, **track)
    if not _is_num(t["smooth"]) or not math.isfinite(t["smooth"]) or not 0 <= t["smooth"] <= 64:
        raise ValueError(f"track: smooth must be a number of frames in [0, 64], not {t['smooth']!r}")
    if t["boxes"] is not None:
        b = t["boxes"].tolist() if torch.is_tensor(t["boxes"]) else t["boxes"]
        if not isinstance(b, (list, tuple)) or len(b) == 0 or not all(isinstance(r, (list, tuple)) and len(r) == 4 and all(_is_num(v) and math.isfinite(v) for v in r) for r in b):
            raise ValueError("track: boxes must be one (x0, y0, x1, y1) of finite numbers per frame")
        t["boxes"] = [tuple(float(v) for v in r) for r in b]
    return t


def _ratio_check(Bw, Bh, w, h):
    if Bw > MAX_RATIO * w or w > MAX_RATIO * Bw or Bh > MAX_RATIO * h or h > MAX_RATIO * Bh:
        raise ValueError(f"track: a box of {Bw:g}x{Bh:g} pixels and a working size of {w}x{h} differ by more than a factor of {MAX_RATIO} along an "
                         f"axis (ratios {Bw / w:.3g} and {Bh / h:.3g}, allowed [1/{MAX_RATIO}, {MAX_RATIO}]): choose another size")


def _travel(boxes):
    cx, cy = [(b[0] + b[2]) / 2 for b in boxes], [(b[1] + b[3]) / 2 for b in boxes]
    return max(math.hypot(x - cx[0], y - cy[0]) for x, y in zip(cx, cy))


def _fill_empty(values):
    """Linear interpolation in time over the None entries between the nearest values; at the ends the nearest value is held."""
    known = [t for t, v in enumerate(values) if v is not None]
    out = []
    for t, v in enumerate(values):
        if v is None:
            before, after = [k for k in known if k < t], [k for k in known if k > t]
            if before and after:
                a, b = before[-1], after[0]
                v = values[a] + (values[b] - values[a]) * (t - a) / (b - a)
            else:
                v = values[before[-1]] if before else values[after[0]]
        out.append(v)
    return out


def _smooth(values, sigma):
    """A Gaussian over time of ``sigma`` frames, radius ceil(3 sigma); at the ends the window is truncated and renormalised."""
    if sigma == 0:
        return list(values)
    R, T, out = math.ceil(3 * sigma), len(values), []
    for t in range(T):
        ks = range(max(0, t - R), min(T, t + R + 1))
        ws = [math.exp(-(k - t) ** 2 / (2.0 * sigma * sigma)) for k in ks]
        out.append(sum(wt * values[k] for wt, k in zip(ws, ks)) / sum(ws))
    return out


def track_plan(frame_hw, size, bboxes, pad=0.25, smooth=2.0):
    """Per-frame boxes of ONE size that follow the object.  A pure function of numbers: no GPU, no library beyond ``math``.

    ``bboxes``: T integer boxes (x0, y0, x1, y1) as ``mask_bbox`` gives them per frame, (W, H, 0, 0) - any box without pixels - for an
    empty frame.  (1) One size: the largest width and the largest height over the non-empty frames go through ``region_plan``'s steps 1 -
    3 (grow by ``ceil(pad max)``, widen to the aspect of ``size``, take the whole frame in a dimension the box then exceeds) -> integers
    (Bw, Bh), checked against the ratio limit.  (2) Raw centres: those of the non-empty bboxes; empty frames are interpolated linearly in
    time between the nearest non-empty ones, the nearest value is held at the ends.  (3) Smoothing: a Gaussian of ``sigma = smooth``
    frames, radius ``ceil(3 smooth)``, truncated and renormalised at the ends of the unit; ``smooth = 0`` keeps the raw centres.  (4) The
    origins are rounded to multiples of 1 / ``TRACK_SUBPIXEL`` pixel.  (5) Containment: a non-empty frame's box is shifted by the smallest
    amount that puts its own bbox inside it.  (6) Every box is shifted inside the frame.  The shifts of (5) and (6) end on integers, so
    they keep (4), and (6) keeps (5) because the bboxes lie inside the frame.

    Returns dict(boxes - T tuples of floats -, size, frame=(H, W), ratio, anisotropy, union - the static box ``region_plan`` takes for the
    union of the bboxes -, travel - the largest distance in pixels of a box's centre from the first frame's).  Guaranteed for the
    delivered numbers: every box inside the frame, every width exactly Bw and height exactly Bh, every non-empty bbox inside its box.
    ValueError: no non-empty frame, a bbox outside the frame, a bad ``size``, a ratio outside [1/8, 8]."""
    H, W = (int(v) for v in frame_hw)
    w, h = (int(v) for v in size)
    _check_size((w, h))
    if H < 1 or W < 1:
        raise ValueError(f"track: a frame of {W}x{H} has no pixels")
    bboxes = [tuple(int(v) for v in b) for b in bboxes]
    live = [b for b in bboxes if b[2] > b[0] and b[3] > b[1]]
    if not live:
        raise ValueError(f"track: the mask is empty in every one of the {len(bboxes)} frames (no pixel above the threshold): there is nothing to follow")
    for b in live:
        if b[0] < 0 or b[1] < 0 or b[2] > W or b[3] > H:
            raise ValueError(f"track: the mask's bounding box {b} is not inside the {W}x{H} frame")
    bw0, bh0 = max(b[2] - b[0] for b in live), max(b[3] - b[1] for b in live)
    sized = _mask_box(H, W, w, h, (0, 0, bw0, bh0), pad)
    Bw, Bh = sized[2] - sized[0], sized[3] - sized[1]
    _ratio_check(Bw, Bh, w, h)
    union = _mask_box(H, W, w, h, (min(b[0] for b in live), min(b[1] for b in live), max(b[2] for b in live), max(b[3] for b in live)), pad)
    is_live = [b[2] > b[0] and b[3] > b[1] for b in bboxes]
    boxes_axis = []
    for lo, hi, B, limit in ((0, 2, Bw, W), (1, 3, Bh, H)):
        centres = _smooth(_fill_empty([(b[lo] + b[hi]) / 2 if ok else None for b, ok in zip(bboxes, is_live)]), smooth)
        origins = []
        for c, b, ok in zip(centres, bboxes, is_live):
            o = round((c - B / 2) * TRACK_SUBPIXEL) / TRACK_SUBPIXEL
            if ok:
                o = max(min(o, float(b[lo])), float(b[hi] - B))
            origins.append(min(max(o, 0.0), float(limit - B)))
        boxes_axis.append(origins)
    boxes = [(x, y, x + Bw, y + Bh) for x, y in zip(*boxes_axis)]
    return dict(boxes=boxes, size=(w, h), frame=(H, W), ratio=(Bw / w, Bh / h), anisotropy=(Bw / w) / (Bh / h), union=union, travel=_travel(boxes))


def given_track(frame_hw, size, boxes):
    """The plan dict for boxes the caller gives: T boxes of finite numbers, each non-empty and inside the frame, all of one width and one
    height (the zoom is constant along a unit), within the ratio limit.  ValueError otherwise."""
    H, W = (int(v) for v in frame_hw)
    w, h = (int(v) for v in size)
    _check_size((w, h))
    boxes = [tuple(float(v) for v in b) for b in boxes]
    for b in boxes:
        if len(b) != 4 or not all(math.isfinite(v) for v in b):
            raise ValueError(f"track: the box {b} must be four finite numbers (x0, y0, x1, y1)")
        if not (b[2] > b[0] and b[3] > b[1]):
            raise ValueError(f"track: the box {b} is empty")
        if b[0] < 0 or b[1] < 0 or b[2] > W or b[3] > H:
            raise ValueError(f"track: the box {b} is not inside the {W}x{H} frame")
    Bw, Bh = boxes[0][2] - boxes[0][0], boxes[0][3] - boxes[0][1]
    if any(b[2] - b[0] != Bw or b[3] - b[1] != Bh for b in boxes):
        raise ValueError(f"track: the boxes must share one width and one height ({Bw:g}x{Bh:g} in the first frame): a box that changes size along the track is not covered")
    _ratio_check(Bw, Bh, w, h)
    return dict(boxes=boxes, size=(w, h), frame=(H, W), ratio=(Bw / w, Bh / h), anisotropy=(Bw / w) / (Bh / h), union=None, travel=_travel(boxes))


def unit_track_plan(frames, mask, mask_key, params, track, fn, dev):
    """The track plan of one unit (``region.edit_region`` / ``edit_regions``) and the mask that is cropped with the frames.  Every
    refusal happens before the first launch."""
    _check_frames(frames, fn)
    T, frame_hw = frames.shape[1], tuple(frames.shape[-2:])
    if params["box"] is not None:
        raise ValueError(f"{fn}: region['box'] fixes one box for the unit and track= moves it: give one of them (explicit boxes go in track=dict(boxes=[...]))")
    if isinstance(mask, str) and mask != "auto":
        raise ValueError(f"mask must be a tensor, None or the string \"auto\", not {mask!r}")
    if torch.is_tensor(mask):
        _check_mask(mask, frames.shape, fn)
    if track["boxes"] is not None:
        if len(track["boxes"]) != T:
            raise ValueError(f"{fn}: track['boxes'] has {len(track['boxes'])} boxes for {T} frames: one per frame")
        plan = given_track(frame_hw, params["size"], track["boxes"])
    else:
        if isinstance(mask, str) or mask_key is not None:
            raise ValueError(f"{fn}: mask=\"auto\" and mask_key= produce their mask inside the working-resolution edit, so there is nothing to follow: "
                             "pass track=dict(boxes=[(x0, y0, x1, y1), ...]), one box per frame")
        if not torch.is_tensor(mask):
            raise ValueError(f"{fn}: track= follows a per-frame mask [1,{T},H,W]; without one pass track=dict(boxes=[...])")
        if mask.shape[1] != T:
            raise ValueError(f"{fn}: a still mask {tuple(mask.shape)} does not move, so there is nothing to follow over {T} frames: pass a per-frame "
                             f"mask [1,{T},H,W] or track=dict(boxes=[...])")
        m = mask[0].to(device=dev, dtype=torch.float32)
        rows = ops.mask_bbox(m, threshold=float(params["threshold"])).cpu().tolist()    # one launch, one read-back of 16 (T + 1) bytes
        plan = track_plan(frame_hw, params["size"], rows[:T], pad=params["pad"], smooth=track["smooth"])
    return dict(plan, mode=params["mode"], blend=params["blend"]), (mask if torch.is_tensor(mask) else None)


@torch.no_grad()
def crop_to_working_track(frames, mask, plan, device=None):
    """``crop_to_working`` with the plan's per-frame ``boxes``: (``down_src`` [1,T,3,h,w], ``mask_w`` [1,T,h,w] or None).  A still mask
    [1,1,H,W] is cropped once per frame - every frame looks at it through its own box."""
    _check_frames(frames, "crop_to_working_track")
    if tuple(frames.shape[-2:]) != tuple(plan["frame"]) or frames.shape[1] != len(plan["boxes"]):
        raise ValueError(f"crop_to_working_track: frames {tuple(frames.shape)} are not the plan's {len(plan['boxes'])} frames of {plan['frame'][1]}x{plan['frame'][0]}")
    dev = _device(frames, device)
    down = ops.region_resample_track(frames[0].to(device=dev, dtype=torch.float32), plan["boxes"], plan["size"], mode="bicubic", clamp=(-1.0, 1.0))[None]
    mask_w = None
    if mask is not None:
        _check_mask(mask, frames.shape, "crop_to_working_track")
        m = mask[0].to(device=dev, dtype=torch.float32)[:, None].expand(frames.shape[1], 1, *frames.shape[-2:])   # (a still mask: frame stride 0)
        mask_w = ops.region_resample_track(m, plan["boxes"], plan["size"], mode="bilinear")[:, 0][None]
    return down, mask_w


@torch.no_grad()
def paste_back_track(frames, edit_w, down_src, plan, mask_w=None, device=None):
    """``paste_back`` with the plan's per-frame ``boxes``: the source everywhere except in each frame's own box."""
    _check_frames(frames, "paste_back_track")
    T, (w, h) = frames.shape[1], plan["size"]
    if T != len(plan["boxes"]):
        raise ValueError(f"paste_back_track: {T} frames for the plan's {len(plan['boxes'])} boxes")
    for name, t in (("edit_w", edit_w), ("down_src", down_src)):
        if not torch.is_tensor(t) or tuple(t.shape) != (1, T, 3, h, w):
            raise ValueError(f"paste_back_track: {name} {tuple(getattr(t, 'shape', ()))} must be [1,{T},3,{h},{w}], the plan's working clip")
    mode, blend = plan.get("mode", REGION_DEFAULTS["mode"]), plan.get("blend", REGION_DEFAULTS["blend"])
    dev = _device(edit_w, device)
    out = frames[0].to(device=dev, dtype=torch.float32).clone()
    as_w = lambda t: t[0].to(device=dev, dtype=torch.float32).contiguous()   # noqa: E731
    m = None
    if mode == "replace" and mask_w is not None:
        if tuple(mask_w.shape) not in ((1, T, h, w), (1, 1, h, w)):
            raise ValueError(f"paste_back_track: mask_w {tuple(mask_w.shape)} must be [1,{T},{h},{w}] or [1,1,{h},{w}]")
        m = as_w(mask_w)
    ops.region_paste_track(out, as_w(edit_w), as_w(down_src), plan["boxes"], mode=mode, blend=blend, mask_w=m)
    return out[None]
