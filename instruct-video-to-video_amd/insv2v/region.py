"""Editing a region at full resolution: crop, edit at the model's size, paste back (csrc/region.hip are the
kernels, tests/region_ref.py the float64 definition).

Every other editing feature works at the model's working resolution: a 1920 x 1080 clip comes back at 384 x 384, or all of its pixels go
through the UNet far from the resolution it was trained at.  ``edit_region`` is the "only masked" of the image inpainting tools: it takes
the box around the mask, resamples it to the working size (antialiased bicubic for frames, bilinear for masks - the operator of
``torch.nn.functional.interpolate(antialias=True)`` applied to the crop), runs an ORDINARY ``edit_video`` on that clip, resamples what
the edit changed back to the source's resolution and lays it over the untouched source.

  check_region     the parameters of ``region=`` (``REGION_KEYS``), completed with their defaults
  region_plan      a pure function of integers: the box of a frame that is edited, from the mask's bounding box or a given box
  crop_to_working  the box of frames and mask at working size: ``ops.region_resample``
  paste_back       the working-resolution edit laid over the full-resolution source: ``ops.region_paste``
  edit_region      plan, crop, ``edit_video`` on the working clip, paste
  edit_regions     the same around ``edit_videos``: sources of different size share one stacked run

``track=`` of the two drivers (``region_track.py``) gives every frame its own real-valued box that follows the
object, in place of the one box per unit; ``track=None`` is everything described here.

The drivers are wrappers, not a new per-unit keyword: the inner edit is by construction an ordinary edit of an ordinary clip, so
``mask_shape=``, ``stabilize=``, ``keyframes=``, ``strength=``, seeds and stacking keep working, with their guarantees, at working
resolution.  Consequences: flow dicts passed through (``mask_flows``, ``stabilize_flows``, ``key_flows``, ``flows_per_window``) and
``cond`` / ``enc_noise`` / ``init_noises`` belong to the WORKING clip; ``mask="auto"`` and ``mask_key=`` produce their mask inside the
inner edit, so the box cannot be derived from them: pass ``box=(x0, y0, x1, y1)`` or ``box="frame"``.  ``strength_map="mask"`` (DESIGN.md
section 28) passes through - the map is then the resampled mask; a tensor ``strength_map`` raises ValueError, static or tracked: it
would have to be resampled to the working clip like the mask, which is not built.

``mode="residual"`` (the default) carries up what the edit CHANGED, ``edit_w - down_src``, and the source keeps its own detail - the
reasoning of ``keyframes=``'s default; a residual that is exactly zero (outside a hard working-resolution mask, wherever the edit changed
nothing) stays zero through the filter, so the pixel is the source's, bit for bit.  ``mode="replace"`` blends the resampled edit in under
the resampled mask.  ``size=(384, 384)``, ``pad=0.25``, ``blend=8`` and ``threshold=0.5`` are starting values, NOT tuned here: there is
no checkpoint and no footage to tune them on (as sections 18 - 24)."""
import math

import torch

from . import ops

REGION_KEYS = ("size", "box", "pad", "mode", "blend", "threshold")
REGION_MODES = ("residual", "replace")
REGION_DEFAULTS = dict(size=(384, 384), box=None, pad=0.25, mode="residual", blend=8, threshold=0.5)
MAX_RATIO = 8   # per axis, box / working size and its inverse: what bounds the kernels' LDS staging


def _is_num(v):
    return not isinstance(v, bool) and isinstance(v, (int, float))


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, int)


def _is_box(v):
    return isinstance(v, (list, tuple)) and len(v) == 4 and all(_is_int(c) for c in v)


def check_region(region=True):
    """``region``: True (the defaults) or a dict with keys among ``REGION_KEYS`` -> the complete dict.  ValueError for values the region
    edit cannot run with (nothing is launched).  ``size`` is (W, H) of the working clip; ``box`` None (the box around the mask, the whole
    frame without one), (x0, y0, x1, y1) or "frame"."""
    if region is True:
        region = {}
    if not isinstance(region, dict) or set(region) - set(REGION_KEYS):
        raise ValueError(f"region must be True or a dict with keys among {REGION_KEYS}, got {region!r}")
    r = dict(REGION_DEFAULTS, **region)
    size = r["size"]
    if not isinstance(size, (list, tuple)) or len(size) != 2 or not all(_is_int(v) for v in size):
        raise ValueError(f"region: size must be (W, H), two integers, not {size!r}")
    _check_size(tuple(size))
    if r["box"] is not None and r["box"] != "frame" and not _is_box(r["box"]):
        raise ValueError(f"region: box must be None, \"frame\" or four integers (x0, y0, x1, y1), not {r['box']!r}")
    if not _is_num(r["pad"]) or not math.isfinite(r["pad"]) or not 0 <= r["pad"] <= 4:
        raise ValueError(f"region: pad must be a number in [0, 4] (a fraction of the mask's longer side), not {r['pad']!r}")
    if r["mode"] not in REGION_MODES:
        raise ValueError(f"region: mode must be 'residual' or 'replace', not {r['mode']!r}")
    if not _is_num(r["blend"]) or not math.isfinite(r["blend"]) or r["blend"] < 0:
        raise ValueError(f"region: blend must be a finite number of pixels >= 0, not {r['blend']!r}")
    if not _is_num(r["threshold"]) or not math.isfinite(r["threshold"]):
        raise ValueError(f"region: threshold must be a finite number, not {r['threshold']!r}")
    r["size"] = tuple(size)
    r["box"] = tuple(r["box"]) if _is_box(r["box"]) else r["box"]
    return r


def _check_size(size):
    w, h = size
    if w <= 0 or h <= 0 or w % 8 or h % 8:
        raise ValueError(f"region: the working size {w}x{h} must be positive multiples of 8 (one latent cell per 8x8 pixels)")


def _mask_box(H, W, w, h, bbox, pad):
    """Steps (1) - (4) of ``region_plan`` for a bounding box inside the frame (integers in, integers out); ``track_plan`` sizes its
    boxes with the same steps."""
    x0, y0, x1, y1 = bbox
    g = math.ceil(pad * max(x1 - x0, y1 - y0))
    x0, y0, x1, y1 = x0 - g, y0 - g, x1 + g, y1 + g
    bw, bh = x1 - x0, y1 - y0
    if bw * h < bh * w:      # too narrow for the aspect w : h
        need = -(-bh * w // h)
        x0 -= (need - bw) // 2
        x1 = x0 + need
    elif bh * w < bw * h:    # too flat
        need = -(-bw * h // w)
        y0 -= (need - bh) // 2
        y1 = y0 + need
    if x1 - x0 >= W:
        x0, x1 = 0, W
    if y1 - y0 >= H:
        y0, y1 = 0, H
    dx, dy = max(0, -x0) - max(0, x1 - W), max(0, -y0) - max(0, y1 - H)
    return x0 + dx, y0 + dy, x1 + dx, y1 + dy


def region_plan(frame_hw, size, bbox=None, box=None, pad=0.25):
    """The box of a frame of ``frame_hw`` = (H, W) pixels that is edited at the working ``size`` = (w, h).  A pure function of integers:
    no GPU, no library.

    ``box`` (x0, y0, x1, y1), half-open: validated - non-empty, inside the frame - and taken as it is.  Else ``bbox``, the mask's bounding
    box: (1) every side grows by ``ceil(pad * max(bw, bh))``; (2) the shorter side widens symmetrically until the box has the aspect of
    ``size``; (3) where a side then exceeds the frame, the whole frame is taken in that dimension - the anisotropy is reported, not
    refused; (4) the box is shifted inside the frame.  With neither, the whole frame.  The full-resolution frame needs no multiple of 8.

    Returns dict(box, size, frame=(H, W), ratio=(bw / w, bh / h), anisotropy=ratio_x / ratio_y).  ValueError, naming the sizes: an empty
    mask, a ``size`` that is not positive multiples of 8, a box outside the frame, a per-axis ratio outside [1/8, 8]."""
    H, W = (int(v) for v in frame_hw)
    w, h = (int(v) for v in size)
    _check_size((w, h))
    if H < 1 or W < 1:
        raise ValueError(f"region: a frame of {W}x{H} has no pixels")
    if box is not None:
        x0, y0, x1, y1 = (int(v) for v in box)
        if x1 <= x0 or y1 <= y0:
            raise ValueError(f"region: the box ({x0}, {y0}, {x1}, {y1}) is empty")
        if x0 < 0 or y0 < 0 or x1 > W or y1 > H:
            raise ValueError(f"region: the box ({x0}, {y0}, {x1}, {y1}) is not inside the {W}x{H} frame")
    elif bbox is not None:
        x0, y0, x1, y1 = (int(v) for v in bbox)
        if x1 <= x0 or y1 <= y0:
            raise ValueError(f"region: the mask is empty in the {W}x{H} frame (no pixel above the threshold): there is no box to edit")
        if x0 < 0 or y0 < 0 or x1 > W or y1 > H:
            raise ValueError(f"region: the mask's bounding box ({x0}, {y0}, {x1}, {y1}) is not inside the {W}x{H} frame")
        x0, y0, x1, y1 = _mask_box(H, W, w, h, (x0, y0, x1, y1), pad)
    else:
        x0, y0, x1, y1 = 0, 0, W, H
    bw, bh = x1 - x0, y1 - y0
    if bw > MAX_RATIO * w or w > MAX_RATIO * bw or bh > MAX_RATIO * h or h > MAX_RATIO * bh:
        raise ValueError(f"region: a box of {bw}x{bh} pixels and a working size of {w}x{h} differ by more than a factor of {MAX_RATIO} along an "
                         f"axis (ratios {bw / w:.3g} and {bh / h:.3g}, allowed [1/{MAX_RATIO}, {MAX_RATIO}]): choose another size or box")
    return dict(box=(x0, y0, x1, y1), size=(w, h), frame=(H, W), ratio=(bw / w, bh / h), anisotropy=(bw / w) / (bh / h))


def _check_frames(frames, fn):
    if not torch.is_tensor(frames) or frames.dim() != 5 or frames.shape[0] != 1 or frames.shape[2] != 3 or not frames.is_floating_point():
        raise ValueError(f"{fn}: frames must be a floating-point [1,T,3,H,W] tensor in [-1, 1], not {tuple(getattr(frames, 'shape', ()))}")


def _check_mask(mask, frames_shape, fn):
    _, T, _, H, W = frames_shape
    if not torch.is_tensor(mask) or not mask.is_floating_point() or mask.dim() != 4 or mask.shape[0] != 1 or mask.shape[1] not in (1, T) \
            or tuple(mask.shape[2:]) != (H, W):
        raise ValueError(f"{fn}: mask {tuple(getattr(mask, 'shape', ()))} must be a floating-point [1,{T},{H},{W}] or [1,1,{H},{W}] for frames {tuple(frames_shape)}")


def _device(t, device):
    return torch.device(device) if device is not None else (t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device()))


@torch.no_grad()
def crop_to_working(frames, mask, plan, device=None):
    """``frames`` [1,T,3,H,W] in [-1, 1] and ``mask`` ([1,T,H,W], [1,1,H,W] or None) -> (``down_src`` [1,T,3,h,w], ``mask_w`` [1,T or
    1,h,w] or None), fp32 on the device: the plan's box at the plan's size.  ``down_src = clamp(bicubic, -1, 1)`` - the cubic overshoots
    and the inner edit's composite clips, so without the clamp "edit == source outside the mask" would stop being exact; ``mask_w`` is
    the bilinear (triangle) resampling."""
    _check_frames(frames, "crop_to_working")
    if tuple(frames.shape[-2:]) != tuple(plan["frame"]):
        raise ValueError(f"crop_to_working: frames {tuple(frames.shape)} are not the plan's {plan['frame'][1]}x{plan['frame'][0]} frame")
    dev = _device(frames, device)
    down = ops.region_resample(frames[0].to(device=dev, dtype=torch.float32), plan["box"], plan["size"], mode="bicubic", clamp=(-1.0, 1.0))[None]
    mask_w = None
    if mask is not None:
        _check_mask(mask, frames.shape, "crop_to_working")
        m = mask[0].to(device=dev, dtype=torch.float32)[:, None]                       # [Tm,1,H,W]
        mask_w = ops.region_resample(m, plan["box"], plan["size"], mode="bilinear")[:, 0][None]
    return down, mask_w


@torch.no_grad()
def paste_back(frames, edit_w, down_src, plan, mask_w=None, device=None):
    """The working-resolution edit ``edit_w`` [1,T,3,h,w] laid over the source ``frames`` [1,T,3,H,W] -> fp32 [1,T,3,H,W] on the device:
    the source everywhere except in the plan's box (``plan["mode"]``, ``plan["blend"]``; default residual, 8).  ``mask_w`` ([1,T,h,w] or
    [1,1,h,w]; None: ones) is the replace mode's mask."""
    _check_frames(frames, "paste_back")
    T, (w, h) = frames.shape[1], plan["size"]
    for name, t in (("edit_w", edit_w), ("down_src", down_src)):
        if not torch.is_tensor(t) or tuple(t.shape) != (1, T, 3, h, w):
            raise ValueError(f"paste_back: {name} {tuple(getattr(t, 'shape', ()))} must be [1,{T},3,{h},{w}], the plan's working clip")
    mode, blend = plan.get("mode", REGION_DEFAULTS["mode"]), plan.get("blend", REGION_DEFAULTS["blend"])
    dev = _device(edit_w, device)
    out = frames[0].to(device=dev, dtype=torch.float32).clone()
    as_w = lambda t: t[0].to(device=dev, dtype=torch.float32).contiguous()   # noqa: E731
    m = None
    if mode == "replace" and mask_w is not None:
        if tuple(mask_w.shape) not in ((1, T, h, w), (1, 1, h, w)):
            raise ValueError(f"paste_back: mask_w {tuple(mask_w.shape)} must be [1,{T},{h},{w}] or [1,1,{h},{w}]")
        m = as_w(mask_w)
    ops.region_paste(out, as_w(edit_w), as_w(down_src), plan["box"], mode=mode, blend=blend, mask_w=m)
    return out[None]


def _unit_plan(frames, mask, mask_key, params, fn, dev, track=None):
    """The plan of one unit and the mask that is cropped with the frames (None: the inner edit makes its own, or there is none).
    ``track`` (None: one box for the unit): the per-frame boxes of ``region_track``; the plan then holds ``boxes`` in place of ``box``."""
    if track is not None:
        from . import region_track
        return region_track.unit_track_plan(frames, mask, mask_key, params, region_track.check_track(track), fn, dev)
    _check_frames(frames, fn)
    frame_hw, box = tuple(frames.shape[-2:]), params["box"]
    derived = isinstance(mask, str) or mask_key is not None      # the mask exists only inside the inner edit
    if isinstance(mask, str) and mask != "auto":
        raise ValueError(f"mask must be a tensor, None or the string \"auto\", not {mask!r}")
    if torch.is_tensor(mask):
        _check_mask(mask, frames.shape, fn)
    if box is None and derived:
        raise ValueError(f"{fn}: mask=\"auto\" and mask_key= produce their mask inside the working-resolution edit, so the box cannot be derived "
                         "from it: pass region=dict(box=(x0, y0, x1, y1)) or region=dict(box=\"frame\")")
    bbox = None
    if box is None and torch.is_tensor(mask):   # one launch, one read-back of 16 bytes: the union over the frames
        m = mask[0].to(device=dev, dtype=torch.float32)
        bbox = tuple(int(v) for v in ops.mask_bbox(m, threshold=float(params["threshold"]))[m.shape[0]].cpu().tolist())
    plan = region_plan(frame_hw, params["size"], bbox=bbox, box=None if box in (None, "frame") else box, pad=params["pad"])
    return dict(plan, mode=params["mode"], blend=params["blend"]), (mask if torch.is_tensor(mask) else None)


def _check_strength_map(strength_map, fn):
    """``strength_map="mask"`` passes through to the inner edit (the mask is resampled with the frames); a tensor map would have to be
    resampled to the working clip like the mask, which is not built."""
    if strength_map is not None and not isinstance(strength_map, str):
        raise ValueError(f"{fn}: a tensor strength_map is not resampled to the working clip (not built): pass strength_map=\"mask\" with a "
                         "mask, or edit the working clip with edit_video")


def _inner_mask(est, mask_w):
    """The replace mode's mask: the composite mask the inner edit used (``shaped``), else its ``mask``, else the resampled drawn one."""
    if isinstance(est, dict):
        for k in ("shaped", "mask"):
            if torch.is_tensor(est.get(k)):
                return est[k]
    return mask_w


def _unpack(res, return_latent, return_mask):
    res = res if isinstance(res, tuple) else (res,)
    return res[0], (res[1] if return_latent else None), (res[-1] if return_mask else None)


def _crop(frames, drawn, plan, dev):
    if "boxes" in plan:
        from .region_track import crop_to_working_track
        return crop_to_working_track(frames, drawn, plan, device=dev)
    return crop_to_working(frames, drawn, plan, device=dev)


def _finish(frames, plan, down, mask_w, res, return_latent, inner_mask, return_mask):
    image, latent, est = _unpack(res, return_latent, inner_mask)
    edit_w = image.to(torch.float32)
    paste = paste_back
    if "boxes" in plan:
        from .region_track import paste_back_track as paste
    full = paste(frames, edit_w, down, plan, mask_w=_inner_mask(est, mask_w) if plan["mode"] == "replace" else None, device=edit_w.device)
    if return_mask and "boxes" in plan:
        est = dict(est or {}, region=dict(boxes=plan["boxes"], travel=plan["travel"], size=plan["size"], working=edit_w, down_src=down))
    elif return_mask:
        est = dict(est or {}, region=dict(box=plan["box"], size=plan["size"], working=edit_w, down_src=down))
    out = (full,) + ((latent,) if return_latent else ()) + ((est,) if return_mask else ())
    return out if len(out) > 1 else full


@torch.no_grad()
def edit_region(model, inf_pipe, frames, text_cond, text_uncond, region=True, track=None, **edit_kwargs):
    """``edit_video`` of a region of full-resolution ``frames`` [1,T,3,H,W] (H, W need not be multiples of 8): the plan's box is resampled
    to the working size, ``edit_video`` runs ONCE on that clip with every other keyword passed through (a tensor ``mask`` resampled with
    it), and the result is pasted over the source.  Returns what ``edit_video`` returns, the image fp32 at the source's size; with
    ``return_mask=True`` the dict gains ``region = dict(box, size, working, down_src)``.  ``region``: True or a dict (``check_region``).
    A [1,T,H,W] or [1,1,H,W] tensor mask costs one ``mask_bbox`` launch and one read-back of 16 bytes; ``mask="auto"`` and ``mask_key=``
    need ``box=`` (module docstring).  Flow dicts, ``cond``, ``enc_noise`` and ``init_noises`` belong to the working clip.

    ``track``: None (one box for the unit), True or a dict (``region_track.check_track``): every frame gets its own real-valued box of one
    size that follows the per-frame mask [1,T,H,W] (one ``mask_bbox`` launch, one read-back of 16 (T + 1) bytes), or the boxes of
    ``track=dict(boxes=[...])``; ``region`` then holds ``boxes`` and ``travel`` in place of ``box``."""
    from .run_loveu_tgve import edit_video
    params = check_region(region)
    _check_strength_map(edit_kwargs.get("strength_map"), "edit_region")
    dev = model.unet.device
    plan, drawn = _unit_plan(frames, edit_kwargs.get("mask"), edit_kwargs.get("mask_key"), params, "edit_region", dev, track)
    down, mask_w = _crop(frames, drawn, plan, dev)
    inner = dict(edit_kwargs)
    if mask_w is not None:
        inner["mask"] = mask_w
    return_latent, return_mask = bool(inner.get("return_latent", False)), bool(inner.pop("return_mask", False))
    inner_mask = return_mask or plan["mode"] == "replace"
    if inner_mask:
        inner["return_mask"] = True
    res = edit_video(model, inf_pipe, down, text_cond, text_uncond, **inner)
    return _finish(frames, plan, down, mask_w, res, return_latent, inner_mask, return_mask)


@torch.no_grad()
def edit_regions(model, inf_pipe, units, return_latent=False, return_mask=False, **kwargs):
    """``edit_region`` of several units around ONE ``edit_videos`` call: each unit (a dict as for ``edit_videos``, optionally with
    ``region``: True or a dict, and ``track``: True or a dict - tracked and static units share the run) is planned and cropped alone, the working clips - which share a shape whatever the sources' sizes, as
    long as the units share ``size`` - run as one stacked chain, and each result is pasted over its own source.  ``kwargs``: the other
    keywords of ``edit_videos``.  Returns the list of what ``edit_region`` returns per unit."""
    from .run_loveu_tgve import edit_videos
    if len(units) == 0:
        return []
    dev = model.unet.device
    prepared, inner_units = [], []
    for u in units:
        _check_strength_map(u.get("strength_map"), "edit_regions")
    for u in units:
        params = check_region(u.get("region", True))
        plan, drawn = _unit_plan(u["frames"], u.get("mask"), u.get("mask_key"), params, "edit_regions", dev, u.get("track"))
        down, mask_w = _crop(u["frames"], drawn, plan, dev)
        inner = {k: v for k, v in u.items() if k not in ("region", "track")}
        inner["frames"] = down
        if mask_w is not None:
            inner["mask"] = mask_w
        prepared.append((plan, down, mask_w))
        inner_units.append(inner)
    inner_mask = return_mask or any(p["mode"] == "replace" for p, _, _ in prepared)
    more = {"return_mask": True} if inner_mask else {}
    if return_latent:
        more["return_latent"] = True
    results = edit_videos(model, inf_pipe, inner_units, **more, **kwargs)
    return [_finish(u["frames"], plan, down, mask_w, res, return_latent, inner_mask, return_mask)
            for u, (plan, down, mask_w), res in zip(units, prepared, results)]
