"""Scoring an edit in pixel space (csrc/pixel_score.hip holds the kernels, tests/pixel_score_ref.py the float64
definitions).

  warp_error     does the edit flicker?  Frame t+1 warped back onto frame t along the SOURCE video's optical flow, the squared difference
                 averaged over the pixels that stay in the frame and pass the forward-backward consistency check of the tracked mask
                 (``mask_track``: same inequality, same constants).
  fidelity       did the edit leave alone what it should?  Per-frame MSE, PSNR and SSIM between source and edit, and with a region
                 (a mask, values in [0,1]) the same inside and outside it.
  score_pixels   both for one ``edit_video`` result, next to the warp error of the source itself - the floor that flow error and
                 real appearance change put under the number.

All metrics are on [0, 1] data.  PSNR = 10 log10(1 / mse): ``inf`` for mse == 0 (a hard mask leaves the outside bit-identical), and a
region whose weight sum is 0 gives ``nan``.  SSIM: Gaussian 11-tap window, sigma 1.5, windows inside the frame only, K1 = 0.01,
K2 = 0.03, population variances, the mean over the three channels; a region weighs an SSIM value by its weight at the window centre.
The sums are fp64 and deterministic; only the divisions below happen here."""
import math

import torch

from . import ops
from .mask_track import TRACK_DEFAULTS, pair_flows

AFFINE_SIGNED = (0.5, 0.5)   # frames in [-1, 1] -> [0, 1]


def _is_num(v):
    return not isinstance(v, bool) and isinstance(v, (int, float))


def _check_frames(name, f, fn):
    if not torch.is_tensor(f) or f.dim() != 4 or f.shape[1] != 3 or f.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"{fn}: {name} must be a float16 / float32 [T,3,H,W] tensor, not {tuple(getattr(f, 'shape', ()))} {getattr(f, 'dtype', type(f).__name__)}")
    return tuple(f.shape)


def _check_region(region, T, H, W, fn):
    if region is None:
        return
    if not torch.is_tensor(region) or not region.is_floating_point() or tuple(region.shape) != (T, H, W):
        raise ValueError(f"{fn}: region must be a floating-point [T,H,W] = [{T},{H},{W}] tensor with values in [0, 1]")


def check_affine(affine, fn="pixel_score"):
    if not isinstance(affine, (tuple, list)) or len(affine) != 2 or not all(_is_num(v) and math.isfinite(v) for v in affine):
        raise ValueError(f"{fn}: affine must be (scale, shift), two finite numbers, not {affine!r}")


def check_warp_error_args(frames, fwd, bwd=None, region=None, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"], affine=(1.0, 0.0)):
    """ValueError for arguments ``warp_error`` cannot run with (nothing is launched)."""
    T, _, H, W = _check_frames("frames", frames, "warp_error")
    if T < 2:
        raise ValueError(f"warp_error: a video of {T} frame(s) has no adjacent pair")
    if H <= 1 or W <= 1:
        raise ValueError(f"warp_error: frames of {H}x{W} cannot be sampled bilinearly")
    for name, f in (("fwd", fwd), ("bwd", bwd)):
        if f is None and name == "bwd":
            continue
        if not torch.is_tensor(f) or not f.is_floating_point() or tuple(f.shape) != (T - 1, 2, H, W):
            raise ValueError(f"warp_error: {name} {tuple(getattr(f, 'shape', ()))} must be a floating-point [T-1,2,H,W] = [{T - 1},2,{H},{W}]")
    _check_region(region, T, H, W, "warp_error")
    for name, v in (("alpha", alpha), ("beta", beta)):
        if not _is_num(v) or not math.isfinite(v) or v < 0:
            raise ValueError(f"warp_error: {name} must be a finite number >= 0, not {v!r}")
    check_affine(affine, "warp_error")


def check_fidelity_args(source, edited, region=None, source_affine=(1.0, 0.0), edited_affine=(1.0, 0.0)):
    """ValueError for arguments ``fidelity`` cannot run with (nothing is launched)."""
    shape = _check_frames("source", source, "fidelity")
    if _check_frames("edited", edited, "fidelity") != shape:
        raise ValueError(f"fidelity: source {shape} and edited {tuple(edited.shape)} differ")
    T, _, H, W = shape
    if T < 1:
        raise ValueError("fidelity: no frames")
    if H < 11 or W < 11:
        raise ValueError(f"fidelity: SSIM's 11 x 11 window does not fit a frame of {H}x{W}")
    _check_region(region, T, H, W, "fidelity")
    check_affine(source_affine, "fidelity")
    check_affine(edited_affine, "fidelity")


def check_score_pixels_args(source_frames, edited_frames, flows=None, flow_estimator=None, mask=None, occlusion=True):
    """ValueError for arguments ``score_pixels`` cannot run with (nothing is launched, no flow is computed)."""
    for name, f in (("source_frames", source_frames), ("edited_frames", edited_frames)):
        if not torch.is_tensor(f) or f.dim() != 5 or f.shape[0] != 1 or f.shape[2] != 3 or f.dtype not in (torch.float16, torch.float32):
            raise ValueError(f"score_pixels: {name} must be a float16 / float32 [1,T,3,H,W] tensor in [-1, 1], not {tuple(getattr(f, 'shape', ()))}")
    if source_frames.shape != edited_frames.shape:
        raise ValueError(f"score_pixels: source {tuple(source_frames.shape)} and edit {tuple(edited_frames.shape)} differ")
    _, T, _, H, W = source_frames.shape
    if T < 1 or H < 11 or W < 11:
        raise ValueError(f"score_pixels: {T} frame(s) of {H}x{W}: at least one frame of 11 x 11 is needed")
    if not isinstance(occlusion, bool):
        raise ValueError(f"score_pixels: occlusion must be True or False, not {occlusion!r}")
    if flows is not None and flow_estimator is not None:
        raise ValueError("score_pixels: flows= and flow_estimator= are two flow sources: pass one")
    if flows is not None and T > 1:
        if not isinstance(flows, dict) or "fwd" not in flows or (occlusion and flows.get("bwd") is None):
            raise ValueError("score_pixels: flows must be dict(fwd=, bwd=) as mask_track.pair_flows returns it (bwd may be missing with occlusion=False)")
        for k in ("fwd", "bwd"):
            f = flows.get(k)
            if f is not None and (not torch.is_tensor(f) or not f.is_floating_point() or tuple(f.shape) != (T - 1, 2, H, W)):
                raise ValueError(f"score_pixels: flows[{k!r}] {tuple(getattr(f, 'shape', ()))} must be a floating-point [{T - 1},2,{H},{W}]")
    if flow_estimator is not None and not callable(flow_estimator):
        raise ValueError("score_pixels: flow_estimator must be callable: estimator(img1, img2) -> [n,2,H,W]")
    if mask is not None:
        if not torch.is_tensor(mask) or not mask.is_floating_point() or mask.dim() != 4 or mask.shape[0] != 1 \
                or mask.shape[1] not in (1, T) or tuple(mask.shape[2:]) != (H, W):
            raise ValueError(f"score_pixels: mask must be a floating-point [1,1,{H},{W}] or [1,{T},{H},{W}] tensor with values in [0, 1]")


def _dev32(t, device):
    return None if t is None else t.to(device=device, dtype=torch.float32).contiguous()


@torch.no_grad()
def warp_error(frames, fwd, bwd=None, *, region=None, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"], return_maps=False, affine=(1.0, 0.0)):
    """The flow warp error of the T - 1 adjacent pairs of ``frames`` [T,3,H,W] (values ``clamp(x * scale + shift, 0, 1)`` with
    ``affine = (scale, shift)``; ``AFFINE_SIGNED`` for frames in [-1, 1]) along ``fwd`` [T-1,2,H,W]; ``bwd`` adds the forward-backward
    consistency check (``alpha``, ``beta``: ``mask_track.TRACK_DEFAULTS``), ``region`` [T,H,W] weighs the pixels of frame t.
    -> dict(warp_error [T-1] = weighted mean of err over the valid pixels (nan where the weight sum is 0), weight [T-1], valid_count
    [T-1], valid_fraction [T-1], sums [T-1,3]) of fp64 tensors on the host (the kernel's sums, copied back; the divisions happen there),
    and with ``return_maps`` err_map / valid_map [T-1,H,W] on the device."""
    check_warp_error_args(frames, fwd, bwd, region, alpha, beta, affine)
    dev = frames.device
    r = ops.warp_error(frames, _dev32(fwd, dev), _dev32(bwd, dev), _dev32(region, dev), scale=float(affine[0]), shift=float(affine[1]),
                       alpha=float(alpha), beta=float(beta), return_maps=return_maps)
    sums = (r[0] if return_maps else r).cpu()
    out = dict(warp_error=sums[:, 0] / sums[:, 1], weight=sums[:, 1], valid_count=sums[:, 2],
               valid_fraction=sums[:, 2] / float(frames.shape[2] * frames.shape[3]), sums=sums)
    if return_maps:
        out["err_map"], out["valid_map"] = r[1], r[2]
    return out


def _psnr(mse):
    """10 log10(1 / mse): +inf for 0, nan for nan."""
    return -10.0 * torch.log10(mse)


@torch.no_grad()
def fidelity(source, edited, region=None, *, source_affine=(1.0, 0.0), edited_affine=(1.0, 0.0)):
    """Per-frame fidelity of ``edited`` to ``source`` (both [T,3,H,W]): dict(mse, psnr, ssim) of fp64 [T] host tensors over the whole frame;
    with ``region`` [T,H,W] (values in [0,1]) also ``*_inside`` (weight w) and ``*_outside`` (weight 1 - w; SSIM: the weight at the window
    centre), and ``sums`` [T,10], the kernel's own output (``ops.FIDELITY_KEYS``)."""
    check_fidelity_args(source, edited, region, source_affine, edited_affine)
    _, _, H, W = source.shape
    s = ops.frame_fidelity(source, edited, _dev32(region, source.device), x_affine=tuple(float(v) for v in source_affine),
                           y_affine=tuple(float(v) for v in edited_affine))
    s = s.cpu()
    q = dict(zip(ops.FIDELITY_KEYS, s.unbind(1)))
    mse = q["se"] / float(H * W)
    out = dict(mse=mse, psnr=_psnr(mse), ssim=q["ssim"] / float((H - 10) * (W - 10)), sums=s)
    if region is not None:
        for side in ("in", "out"):
            m = q["se_" + side] / q["w_" + side]   # 0 / 0 = nan: an empty region
            out.update({f"mse_{side}side": m, f"psnr_{side}side": _psnr(m), f"ssim_{side}side": q["ssim_" + side] / q["wc_" + side]})
    return out


@torch.no_grad()
def score_pixels(source_frames, edited_frames, *, flows=None, flow_estimator=None, mask=None, occlusion=True):
    """Score one edit: ``source_frames`` / ``edited_frames`` [1,T,3,H,W] in [-1, 1] (as ``score_edit`` takes them), ``mask`` the
    image-resolution region [1,1,H,W] or [1,T,H,W] of a localized edit.  The fidelity fields of ``fidelity`` always; with a flow source
    - ``flows=dict(fwd, bwd)`` or ``flow_estimator`` (then ``mask_track.pair_flows(source_frames, estimator)``), ALWAYS the flows of the
    source video - and T > 1 also ``warp_error`` [T-1] of the edit, ``warp_error_source`` [T-1] (the same pairs, flows and valid set on
    the source frames), ``warp_error_mean``, ``warp_error_source_mean`` and ``valid_fraction`` [T-1].  The warp error is not weighted by
    the mask.  ``occlusion=False`` drops the consistency check.  Values are fp64 tensors on the host."""
    check_score_pixels_args(source_frames, edited_frames, flows, flow_estimator, mask, occlusion)
    _, T, _, H, W = source_frames.shape
    dev = edited_frames.device
    src, edt = source_frames[0].to(dev), edited_frames[0]
    region = None if mask is None else mask[0].to(device=dev, dtype=torch.float32).expand(T, H, W).contiguous()
    out = fidelity(src, edt, region, source_affine=AFFINE_SIGNED, edited_affine=AFFINE_SIGNED)
    del out["sums"]
    if T > 1 and (flows is not None or flow_estimator is not None):
        if flows is None:
            flows = pair_flows(source_frames.to(dev), flow_estimator)
        bwd = flows.get("bwd") if occlusion else None
        we = warp_error(edt, flows["fwd"], bwd, affine=AFFINE_SIGNED)
        ws = warp_error(src, flows["fwd"], bwd, affine=AFFINE_SIGNED)
        out.update(warp_error=we["warp_error"], warp_error_source=ws["warp_error"], warp_error_mean=we["warp_error"].mean(),
                   warp_error_source_mean=ws["warp_error"].mean(), valid_fraction=we["valid_fraction"])
    return out
