"""Long-video editing driver: counterpart of insv2v_run_loveu_tgve.py.

  split_batch   insv2v_run_loveu_tgve.py:12-29  (window plan: 16-frame windows, 4-frame overlap)
  edit_video    insv2v_run_loveu_tgve.py:98, :119-165 for one (video, prompt) unit
  main          same CLI flags as :31-45; units are sharded clip-parallel over ranks (one process per GPU)

``main`` has three sources of work: ``--synthetic`` clips (random-init weights), a ``--units`` .pt file holding
{"frames": [n,T,3,H,W], "text_cond": [n,77,768], "text_uncond": [1,77,768]}, or - as the reference - the LOVEU-TGVE
dataset under ``--data-dir`` (``insv2v/video_io.py``: CSV + frames, prompts from ``--edit-prompt-file``, CLIP text tower on
the HIP kernels with the BPE vocabulary from ``--tokenizer-dir``), writing the reference's GIF / JPG result tree.

With ``--score-ckpt FILE --score-out FILE.json`` (or ``--score-synthetic`` next to ``--synthetic``) every unit is scored after its edit
with CLIP on the HIP kernels (``insv2v/clip_score.py``: the reference's ``ClipSimilarity`` numbers, text alignment, frame consistency).
``--score-pixels`` / ``--score-warp`` add the pixel-space scores to the same records, with or without a CLIP scorer
(``insv2v/pixel_score.py``: per-frame MSE / PSNR / SSIM against the source, inside and outside the unit's mask, and the flow warp error).

Masks: drawn per frame or still (``mask=``, the "mask" entry of a ``--units`` file, ``--mask-file``), estimated from the prompt
(``mask="auto"``, ``--auto-mask``), or drawn on one frame and tracked through the video with optical flow (``mask_key=``, ``--mask-key``:
``insv2v/mask_track.py``); ``--mask-image`` reads a drawn mask from a PNG or a folder of PNGs (``video_io.load_mask``).  ``mask_shape=`` /
``--mask-grow`` / ``--mask-feather`` grows, shrinks and feathers the mask of any of these sources, once per unit (``insv2v/mask_shape.py``,
DESIGN.md section 22): the composite gets the soft mask, the latent hold the hard region under it.
``strength_map=`` / ``--strength-map`` / ``--strength-from-mask`` give every pixel its own edit strength: a latent
cell is held at the source until the step its strength corresponds to and released to the model from there, inside the step kernel.

``stabilize=`` / ``--stabilize`` filters a unit's decoded frames along the SOURCE video's optical flow, once per unit and after its last
window (``insv2v/temporal_filter.py``): the switch to pull when ``--score-warp`` shows flicker.

``keyframes=`` / ``--key-stride`` denoises only every N-th frame of a unit and fills the frames in between along the SOURCE video's
optical flow (``insv2v/keyfill.py``): about N times the delivered frames per GPU second.
"""
import argparse
import os
from itertools import product

import torch

from . import ops
from .rng import stream_id, INIT
from .schedulers import strength_to_start


def split_batch(cond, frames_in_batch=16, num_ref_frames=4):
    """Split [b, T, ...] along frames: first window = frames_in_batch frames, later windows add
    (frames_in_batch - num_ref_frames) NEW frames each (the last one whatever remains).  Returns the
    new-frame chunks and, per later window, how many frames of the previous window it re-uses."""
    total = cond.shape[1]
    chunks = [cond[:, :frames_in_batch]]
    refs = []
    ptr = frames_in_batch
    while ptr < total:
        left = total - ptr
        new = left if left < frames_in_batch else frames_in_batch - num_ref_frames
        chunks.append(cond[:, ptr:ptr + new])
        refs.append(frames_in_batch - new)
        ptr += new
    return chunks, refs


def _seeded(seed, unit):
    """The seed keywords of a call - none without a seed, so that unseeded calls are exactly what they were."""
    return {} if seed is None else {"seed": seed, "unit": unit}


MASK_MODES = ("mean", "max")


AUTO_MASK_KEYS = ("n_maps", "mask_strength", "clamp_ratio", "threshold", "smooth", "dilate", "frames_in_batch", "noises")


MASK_TRACK_KEYS = ("occlusion", "alpha", "beta", "fill")


STABILIZE_KEYS = ("radius", "sigma", "strength", "occlusion", "alpha", "beta")


KEYFRAME_KEYS = ("stride", "mode", "sigma", "occlusion", "alpha", "beta")


# The per-unit keywords of an edit, listed ONCE: keywords of ``edit_video``, entries of a unit of ``edit_videos``, the arguments an
# ``_EditUnit`` is built from.  A new per-unit feature adds its keywords here (and to ``edit_video``'s signature).  The second row is
# what ``check_edit_args`` checks, in its parameters' order.
UNIT_KEYS = ("text_cfg", "video_cfg", "init_noises", "enc_noise", "cond", "flows_per_window",
             "mask", "strength", "mask_mode", "auto_mask", "mask_key", "mask_flows", "mask_track", "stabilize", "stabilize_flows", "strength_map", "mask_shape",
             "keyframes", "key_flows")
CHECKED_KEYS = UNIT_KEYS[6:]
UNIT_DEFAULTS = dict({k: None for k in UNIT_KEYS}, text_cfg=7.5, video_cfg=1.8, strength=1.0, mask_mode="max")


def check_edit_args(frames_shape, mask=None, strength=1.0, mask_mode="max", auto_mask=None, mask_key=None, mask_flows=None, mask_track=None,
                    stabilize=None, stabilize_flows=None, strength_map=None, mask_shape=None, keyframes=None, key_flows=None):
    """Host-side check of the localized / partial edit controls (nothing is launched): ``strength`` in (0, 1], ``mask_mode`` "mean" or
    "max", ``mask`` a floating-point [1,T,H,W] or [1,1,H,W] tensor for frames [1,T,3,H,W] with H and W multiples of 8 - or the string
    "auto" (the mask is estimated from the prompt, ``InferenceIP2PVideo.estimate_mask``), then optionally with ``auto_mask``, a dict of
    that method's keywords (``AUTO_MASK_KEYS``).  ``mask_key`` (a frame index: the mask, then a [1,1,H,W] tensor, is drawn on that frame
    and tracked through the video, ``insv2v/mask_track.py``) optionally with ``mask_flows``, a dict(fwd=, bwd=) of [T-1,2,H,W] flows, and
    ``mask_track``, a dict of ``propagate_mask``'s keywords (``MASK_TRACK_KEYS``).  ``stabilize`` (None, True or a dict of
    ``temporal_filter.stabilize``'s parameters, ``STABILIZE_KEYS``) optionally with ``stabilize_flows``, a dict(fwd=, bwd=) of the source
    video's [T-1,2,H,W] flows.  ``mask_shape`` (None or a dict of ``mask_shape.check_shape_args``' parameters, ``MASK_SHAPE_KEYS``) shapes
    the mask of any source, so it needs one.  ``keyframes`` (None, an int stride or a dict with keys among ``KEYFRAME_KEYS``) optionally
    with ``key_flows``, a dict(fwd=, bwd=) of the source video's [T-1,2,H,W] flows; not together with ``mask="auto"`` (an estimated mask
    exists on the key frames only).  ``strength_map`` (None, a floating-point [1,T,H,W] or [1,1,H,W] tensor in [0,1] for frames with H and
    W multiples of 8, or the string "mask": the unit's final image mask is the map, so it needs a mask, and not ``mask="auto"``, whose
    mask is hard)."""
    _check_unit(frames_shape, locals())


def _check_unit(frames_shape, u):
    """``check_edit_args`` of a unit's arguments by name (the missing ones at their defaults).  The refusals in their order: key
    frames, ``mask_shape``, ``stabilize``, the tracked mask, ``mask_mode``, ``strength_map``, ``auto_mask``, the mask itself."""
    a = {k: u.get(k, UNIT_DEFAULTS[k]) for k in CHECKED_KEYS}
    mask, auto_mask = a["mask"], a["auto_mask"]
    strength_to_start(a["strength"], 1)
    _check_keyframe_args(frames_shape, mask, a["keyframes"], a["key_flows"])
    if a["mask_shape"] is not None:
        from .mask_shape import check_mask_shape
        check_mask_shape(a["mask_shape"])
        if mask is None:
            raise ValueError("mask_shape shapes the mask of a localized edit: pass mask= (a tensor, \"auto\", or with mask_key=) with it")
    _check_stabilize_args(frames_shape, a["stabilize"], a["stabilize_flows"])
    if a["mask_key"] is None and (a["mask_flows"] is not None or a["mask_track"] is not None):
        raise ValueError("mask_flows / mask_track belong to a tracked mask: pass mask_key=, the frame the mask is drawn on, with them")
    if a["mask_key"] is not None:
        _check_track_args(frames_shape, mask, a["mask_key"], a["mask_flows"], a["mask_track"])
    if a["mask_mode"] not in MASK_MODES:
        raise ValueError(f"mask_mode {a['mask_mode']!r} is neither 'mean' nor 'max'")
    _check_strength_map(frames_shape, mask, a["strength_map"])
    if auto_mask is not None and not (isinstance(mask, str) and mask == "auto"):
        raise ValueError("auto_mask holds the parameters of an estimated mask: pass mask=\"auto\" with it")
    if isinstance(mask, str):
        if mask != "auto":
            raise ValueError(f"mask must be a tensor, None or the string \"auto\", not {mask!r}")
        b, _, _, H, W = frames_shape
        if b != 1 or H % 8 or W % 8:
            raise ValueError(f"mask=\"auto\" needs frames [1,T,3,H,W] with H and W multiples of 8 (one latent cell per 8x8 pixels), not {tuple(frames_shape)}")
        if auto_mask is not None:
            from .inference import check_automask_args
            _check_params("auto_mask (the parameters of mask=\"auto\")", auto_mask, AUTO_MASK_KEYS,
                          lambda **kw: check_automask_args(**{k: v for k, v in kw.items() if k != "noises"}))
        return
    if mask is None:
        return
    b, T, _, H, W = frames_shape
    if not torch.is_tensor(mask) or not mask.is_floating_point():
        raise ValueError("mask must be a floating-point tensor with values in [0, 1] (1 = edit, 0 = keep)")
    if mask.dim() != 4 or mask.shape[0] != 1 or b != 1 or mask.shape[1] not in (1, T) or tuple(mask.shape[2:]) != (H, W):
        raise ValueError(f"mask {tuple(mask.shape)} must be [1,{T},{H},{W}] or [1,1,{H},{W}] (image resolution) for frames {tuple(frames_shape)}")
    if H % 8 or W % 8:
        raise ValueError(f"a mask needs frame sizes that are multiples of 8 (one latent cell per 8x8 pixels), not {H}x{W}")


def _check_strength_map(frames_shape, mask, strength_map):
    """The ``strength_map`` part of ``check_edit_args``."""
    if strength_map is None:
        return
    if isinstance(strength_map, str):
        if strength_map != "mask":
            raise ValueError(f"strength_map must be a tensor, None or the string \"mask\", not {strength_map!r}")
        if mask is None:
            raise ValueError("strength_map=\"mask\" makes the unit's image mask its strength map: pass mask= (a tensor, or with mask_key=) with it")
        if isinstance(mask, str):
            raise ValueError("strength_map=\"mask\" and mask=\"auto\": an estimated mask is hard (0 or 1), it grades nothing; pass a tensor strength_map")
        return
    b, T, _, H, W = frames_shape
    if not torch.is_tensor(strength_map) or not strength_map.is_floating_point():
        raise ValueError("strength_map must be a floating-point tensor with values in [0, 1] (1 = fully re-drawn, 0 = never touched) or the string \"mask\"")
    if strength_map.dim() != 4 or strength_map.shape[0] != 1 or b != 1 or strength_map.shape[1] not in (1, T) or tuple(strength_map.shape[2:]) != (H, W):
        raise ValueError(f"strength_map {tuple(strength_map.shape)} must be [1,{T},{H},{W}] or [1,1,{H},{W}] (image resolution) for frames {tuple(frames_shape)}")
    if H % 8 or W % 8:
        raise ValueError(f"a strength_map needs frame sizes that are multiples of 8 (one latent cell per 8x8 pixels), not {H}x{W}")


def _check_params(name, params, keys, check, form=None):
    """A feature's dict of parameters: its keys among ``keys``, its values accepted by the feature's own ``check``."""
    if not isinstance(params, dict) or set(params) - set(keys):
        raise ValueError(f"{name} must be a dict with keys among {keys}, got {params!r}" if form is None else form)
    try:
        check(**params)
    except ValueError as e:
        raise ValueError(f"{name}: {e}") from None


def _check_flow_dict(name, flows, frames_shape, required, form):
    """``flows``, the argument ``name``, as a dict(fwd=, bwd=) of floating-point [T-1,2,H,W] flows for frames [1,T,3,H,W]; ``required``:
    the directions that must be there, ``form``: what the refusal says the dict holds."""
    T, H, W = frames_shape[1], frames_shape[3], frames_shape[4]
    if not isinstance(flows, dict) or not flows or set(flows) - {"fwd", "bwd"} or any(flows.get(k) is None for k in required):
        raise ValueError(f"{name} must be a dict(fwd=, bwd=) of {form}")
    for k, f in flows.items():
        if f is not None and (not torch.is_tensor(f) or not f.is_floating_point() or tuple(f.shape) != (T - 1, 2, H, W)):
            raise ValueError(f"{name}[{k!r}] {tuple(getattr(f, 'shape', ()))} must be a floating-point [{T - 1},2,{H},{W}] for frames {tuple(frames_shape)}")


def _check_track_args(frames_shape, mask, mask_key, mask_flows, mask_track):
    """The ``mask_key`` part of ``check_edit_args``."""
    from .mask_track import check_track_args
    T, H, W = frames_shape[1], frames_shape[3], frames_shape[4]
    if isinstance(mask, str) or not torch.is_tensor(mask) or mask.dim() != 4 or tuple(mask.shape[:2]) != (1, 1):
        raise ValueError(f"mask_key tracks a mask drawn on one frame: mask must be a [1,1,{H},{W}] tensor (not \"auto\", not one mask per frame)")
    if isinstance(mask_key, bool) or not isinstance(mask_key, int) or not 0 <= mask_key < T:
        raise ValueError(f"mask_key {mask_key!r} is not a frame index of a video of {T} frames")
    track = {} if mask_track is None else mask_track
    _check_params("mask_track (the parameters of a tracked mask)", track, MASK_TRACK_KEYS, check_track_args)
    if mask_flows is not None:
        _check_flow_dict("mask_flows", mask_flows, frames_shape, ("fwd", "bwd") if track.get("occlusion", True) and T > 1 else (),
                         f"[{T - 1},2,{H},{W}] flows (the occlusion check of a tracked mask needs both fwd and bwd, or mask_track=dict(occlusion=False))")


def _stabilize_params(stabilize):
    """None when the filter is off, else the dict of its parameters (``True``: the defaults)."""
    if stabilize is None or stabilize is False:
        return None
    return {} if stabilize is True else stabilize


def _check_stabilize_args(frames_shape, stabilize, stabilize_flows):
    """The ``stabilize`` part of ``check_edit_args``."""
    from .temporal_filter import check_filter_args
    params = _stabilize_params(stabilize)
    if params is None:
        if stabilize_flows is not None:
            raise ValueError("stabilize_flows belongs to a stabilized edit: pass stabilize=True (or a dict of its parameters) with it")
        return
    _check_params("stabilize (the parameters of the temporal filter)", params, STABILIZE_KEYS, check_filter_args,
                  f"stabilize must be None, True or a dict with keys among {STABILIZE_KEYS}, got {stabilize!r}")
    b, T, _, H, W = frames_shape
    if b != 1:
        raise ValueError(f"stabilize needs frames [1,T,3,H,W], not {tuple(frames_shape)}")
    if stabilize_flows is not None:
        _check_flow_dict("stabilize_flows", stabilize_flows, frames_shape, ("fwd", "bwd") if params.get("occlusion", True) else ("fwd",),
                         f"the source video's [{T - 1},2,{H},{W}] flows (bwd may be missing with occlusion=False)")


def _keyframe_params(keyframes):
    """None when every frame is denoised, else the dict of the key-frame edit's parameters (an int: its stride)."""
    if keyframes is None or keyframes is False:
        return None
    return dict(stride=keyframes) if isinstance(keyframes, int) and not isinstance(keyframes, bool) else keyframes


def _check_keyframe_args(frames_shape, mask, keyframes, key_flows):
    """The ``keyframes`` part of ``check_edit_args``."""
    from .keyfill import check_fill_args
    params = _keyframe_params(keyframes)
    if params is None:
        if key_flows is not None:
            raise ValueError("key_flows belongs to a key-frame edit: pass keyframes= (a stride, or a dict of its parameters) with it")
        return
    _check_params("keyframes (the parameters of the key-frame edit)", params, KEYFRAME_KEYS, check_fill_args,
                  f"keyframes must be None, an int stride or a dict with keys among {KEYFRAME_KEYS}, got {keyframes!r}")
    b, T, _, H, W = frames_shape
    if b != 1:
        raise ValueError(f"keyframes needs frames [1,T,3,H,W], not {tuple(frames_shape)}")
    if isinstance(mask, str):
        raise ValueError("keyframes and mask=\"auto\": an estimated mask exists on the key frames only (carrying it to the frames in between "
                         "is not built); draw the mask, or track one with mask_key=")
    if key_flows is not None:
        _check_flow_dict("key_flows", key_flows, frames_shape, ("fwd", "bwd"),
                         f"the source video's [{T - 1},2,{H},{W}] flows (the previous key is reached along bwd, the next along fwd)")


_NO_FLOW_SOURCE = {
    "keyframes": "key-frame edit (keyframes=) without a flow source: pass key_flows=, stabilize_flows=, mask_flows= or flow_estimator=, or build the pipe with flow_estimator=",
    "stabilize": "stabilized edit (stabilize=) without a flow source: pass stabilize_flows=, mask_flows= or flow_estimator=, or build the pipe with flow_estimator=",
    "mask_key": "tracked mask (mask_key=) without a flow source: pass mask_flows= or flow_estimator=, or build the pipe with flow_estimator=",
}


def _both(flows):
    """A flow dict that holds both directions, else None: only such a dict can stand in for another feature's flows."""
    return flows if flows is not None and flows.get("fwd") is not None and flows.get("bwd") is not None else None


def _source_flows(inf_pipe, frames, candidates, flow_estimator, feature, both=True, key=None):
    """The source video's adjacent-frame flows a feature of one unit follows -> (dict(fwd, bwd), whether they were computed here); (None,
    False) for a single frame, which needs no flow.  In this order: the first of ``candidates`` that is not None, ``flow_estimator``, the
    pipe's own estimator - then ONE ``mask_track.pair_flows`` of the whole unit (``both=False`` with ``key``: only the pairs the chain
    from ``key`` reads).  ``feature`` names the RuntimeError of a unit without any source."""
    if frames.shape[1] == 1:
        return None, False
    given = next((f for f in candidates if f is not None), None)
    if given is not None:
        return given, False
    est = flow_estimator if flow_estimator is not None else getattr(inf_pipe, "flow_estimator", None)
    if est is None:
        raise RuntimeError(_NO_FLOW_SOURCE[feature])
    from .mask_track import pair_flows
    return pair_flows(frames, est, both=both, key=key), True


def _start_time(inf_pipe, strength):
    """``start_time`` of an edit of this strength (full strength asks the pipe nothing: any pipe object keeps working)."""
    return 0 if strength == 1.0 else strength_to_start(strength, inf_pipe.num_ddim_steps)[1]


def _image_mask(mask, T, dev):
    """A unit's mask [1,T,H,W] or [1,1,H,W] -> one fp32 mask per frame [T,H,W] on the device."""
    return mask.to(device=dev, dtype=torch.float32).expand(1, T, *mask.shape[2:])[0].contiguous()


class _EditPlan:
    """What a localized (``mask``), partial (``strength`` < 1) or graded (``strength_map``) edit adds to the windows of one unit: the
    source latent z, the latent-resolution mask and the release map, split like ``cond``, and the level the trajectory starts from.
    ``active`` is False for a plain edit, whose calls then carry no new keyword.  ``strength_map``: a tensor, or "mask" - the unit's
    final image mask (``shaped`` with ``mask_shape``) is the map; ``release`` [1,T,h,w] and ``gate`` [T,H,W] are built ONCE
    (``ops.strength_release``), the composite then uses ``gate`` (``composite_mask``)."""

    def __init__(self, model, inf_pipe, frames, cond, mask, strength, mask_mode, frames_in_batch, num_ref_frames, z=None, mask_shape=None,
                 strength_map=None):
        dev = model.unet.device
        self.start_time = _start_time(inf_pipe, strength)
        partial = strength != 1.0   # (also a strength below 1 that rounds to every step: it starts from the noised source at timesteps[0])
        self.active = mask is not None or partial or strength_map is not None
        self.mask_img = self.masks = self.level = self.shape = self.release = self.releases = self.gate = None
        if not self.active:
            return
        if z is None:   # (a caller's ``cond`` is z / scale_factor)
            z = cond * model.scale_factor
        self.zs = split_batch(z.to(device=dev, dtype=torch.float32), frames_in_batch, num_ref_frames)[0]
        if partial:
            self.level = inf_pipe.scheduler.start_coefficients(int(inf_pipe.scheduler.timesteps[self.start_time]))
        if mask is not None:
            self.mask_img = _image_mask(mask, frames.shape[1], dev)
            if mask_shape is None:
                latent_mask = ops.mask_to_latent(self.mask_img, mask_mode)
            else:   # two masks: the soft one for the composite, the hard region under it - the whole feather - for the latent hold
                from .mask_shape import shape_mask
                self.mask_img, support = shape_mask(self.mask_img, **mask_shape)
                self.shape = dict(shaped=self.mask_img[None], support=support[None])
                latent_mask = ops.mask_to_latent(support, "max")
            self.masks = split_batch(latent_mask[None], frames_in_batch, num_ref_frames)[0]   # reduced ONCE
        if strength_map is not None:   # (with mask_shape the hold above is ``support``'s, the map ``shaped``)
            smap = self.mask_img if isinstance(strength_map, str) else _image_mask(strength_map, frames.shape[1], dev)
            release, self.gate = ops.strength_release(smap, inf_pipe.num_ddim_steps, mask_mode, mask=self.mask_img)
            self.release = release[None]
            self.releases = split_batch(self.release, frames_in_batch, num_ref_frames)[0]   # built ONCE, split and joined as the mask is

    def window(self, k, R, init):
        """(initial latent, extra keywords) of window k, whose first R frames are carried over; ``init`` = the window's initial noise."""
        if not self.active:
            return init, {}
        join = (lambda c: c[0]) if k == 0 else (lambda c: torch.cat([c[k - 1][:, -R:], c[k]], dim=1))   # exactly as cond_k
        z = join(self.zs)
        kw = {}
        latent = init
        if self.level is not None:
            latent = ops.add_noise(z, init, *self.level)
            kw["start_time"] = self.start_time
        if self.masks is not None:
            kw.update(mask=join(self.masks).contiguous(), source_latent=z, known_noise=init)
        if self.releases is not None:
            kw.update(release=join(self.releases).contiguous(), source_latent=z, known_noise=init)
        return latent, kw

    def composite_mask(self):
        """The image-resolution mask [T,H,W] of the final composite (and of ``stabilize``): the gate of a strength map, else the mask."""
        return self.mask_img if self.gate is None else self.gate

    def finish(self, image, frames):
        """Decoded frames [1,T,3,H,W] -> the result: composited against the input outside the mask, clipped to [-1,1]."""
        if self.composite_mask() is None:
            return image.clip(-1, 1)
        img = image[0].to(torch.float32).contiguous()
        orig = frames[0].to(device=img.device, dtype=torch.float32).contiguous()
        return ops.composite(img, orig, self.composite_mask(), out=img)[None]


def _stabilize(frames, image, params, flows, mask_img):
    """The unit's finished frames [1,T,3,H,W], filtered once over the whole unit - also across the hand-over of its windows."""
    from .temporal_filter import stabilize
    if flows is None:
        return image
    return stabilize(frames, image, flows=flows, mask=None if mask_img is None else mask_img[None], **params)


class _EditUnit:
    """One (video, prompt) unit, as BOTH drivers run it: ``edit_video`` drives one, ``edit_videos`` several in step, and what a unit
    does - in which order, with which arguments - is written here only.  ``args``: the unit's arguments by name (``UNIT_KEYS``; the
    missing ones take ``UNIT_DEFAULTS``).  Three phases:

      ``prepare()``   once, before the first window: the source video's flows, the tracked mask, the key-frame reduction, the VAE encode,
                      the estimated mask, the ``_EditPlan``, the window split.  Everything that can refuse refuses here, flows first -
                      a missing flow source raises before anything is sampled.
      ``window(k)``   the keywords of the pipe call of window k (``first()`` for k = 0, ``second_clip_forward`` / ``run_stacked`` after);
                      ``receive(k, out)`` takes that call's result.
      ``finish()``    after the last window: decode, composite, fill the frames between the keys, stabilize -> (image, latent, est).

    A new per-unit feature plugs in here: its keywords join ``UNIT_KEYS``, its check ``_check_unit``, and its work goes into the phase it
    belongs to - both drivers get it at once.  The unit's constructor runs nothing and touches neither model nor pipe; it only works out
    which frames are sampled (``keys``; None: all of them) and their shape."""

    def __init__(self, model, inf_pipe, frames, text_cond, text_uncond, frames_in_batch, num_ref_frames, seed, unit, flow_estimator, args,
                 number_first_window=False):
        from .keyfill import key_frames, FILL_DEFAULTS
        self.model, self.pipe, self.source, self.text = model, inf_pipe, frames, dict(text_cond=text_cond, text_uncond=text_uncond)
        self.fib, self.nref, self.seed, self.unit, self.estimator = frames_in_batch, num_ref_frames, seed, unit, flow_estimator
        self.a = dict(UNIT_DEFAULTS, **args)
        self.number_first = number_first_window   # (edit_video has always sent its first window without ``window=0``)
        self.kf, self.keys = _keyframe_params(self.a["keyframes"]), None
        if self.kf is not None:
            keys = key_frames(frames.shape[1], self.kf.get("stride", FILL_DEFAULTS["stride"]))
            self.keys = keys if len(keys) < frames.shape[1] else None   # every frame a key: edited as if ``keyframes`` were not given
        self.shape = tuple(frames.shape) if self.keys is None else (frames.shape[0], len(self.keys), *frames.shape[2:])

    def prepare(self):
        from .mask_track import propagate_mask
        a, model, pipe, source = self.a, self.model, self.pipe, self.source
        dev = self.dev = model.unet.device
        T = source.shape[1]
        # the source video's flows: at most ONE full-rate pair_flows(both=True) serves the fill, the filter and a tracked mask
        shared = None
        if self.keys is not None:
            shared, _ = _source_flows(pipe, source, [_both(a["key_flows"]), _both(a["stabilize_flows"]), _both(a["mask_flows"])], self.estimator, "keyframes")
        self.fill_flows = shared
        self.stab, self.stab_flows = _stabilize_params(a["stabilize"]), None
        if self.stab is not None:
            self.stab_flows, computed = _source_flows(pipe, source, [a["stabilize_flows"], shared, _both(a["mask_flows"])], self.estimator, "stabilize")
            if computed:
                shared = self.stab_flows
        mask, est = a["mask"], None
        if a["mask_key"] is not None:   # tracked ONCE over the full-rate video, in launches of its own; from there a user's [1,T,H,W] mask
            track = dict(a["mask_track"] or {})
            flows, _ = _source_flows(pipe, source, [a["mask_flows"], shared], self.estimator, "mask_key", both=track.get("occlusion", True), key=a["mask_key"])
            if flows is None:   # a single frame: nothing to track, no flow is needed, none is launched
                flows = {k: torch.zeros((0, 2, *source.shape[-2:]), device=dev) for k in ("fwd", "bwd")}
            fwd, bwd = (None if flows.get(k) is None else flows[k].to(device=dev, dtype=torch.float32) for k in ("fwd", "bwd"))
            est = propagate_mask(mask.to(device=dev), a["mask_key"], fwd, bwd, **track)
            mask = est["mask"]
        # the key-frame reduction: from here the unit's windows see the sub-video of its keys
        frames, cond, enc_noise = source, a["cond"], a["enc_noise"]
        self.full_mask = None
        smap = a["strength_map"]
        if self.keys is not None:
            if mask is not None:   # the full-rate mask of the composite, shaped per frame exactly as the plan shapes the keys' rows
                self.full_mask = _image_mask(mask, T, dev)
                if a["mask_shape"] is not None:
                    from .mask_shape import shape_mask
                    self.full_mask, support = shape_mask(self.full_mask, **a["mask_shape"])
                    est = dict(est or {}, shaped=self.full_mask[None], support=support[None])
                mask = mask if mask.shape[1] == 1 else mask[:, self.keys]
            if smap is not None:   # the full-rate gate serves the fill's composite; the map itself is reduced to the keys as the mask is
                full_map = self.full_mask if isinstance(smap, str) else _image_mask(smap, T, dev)
                self.full_mask = ops.strength_release(full_map, pipe.num_ddim_steps, a["mask_mode"], mask=self.full_mask)[1]
                if not isinstance(smap, str):
                    smap = smap if smap.shape[1] == 1 else smap[:, self.keys]
            frames = source[:, self.keys]
            cond, enc_noise = (None if t is None else t[:, self.keys] for t in (cond, enc_noise))
        self.frames = frames
        z = None
        if cond is None:
            z = model.encode_image_to_latent(frames, enc_noise, **_seeded(self.seed, self.unit))
            cond = z / model.scale_factor
        if isinstance(mask, str):   # "auto" (check_edit_args): estimated ONCE from the whole video, in launches of its own
            kw = dict(dict(frames_in_batch=self.fib), **(a["auto_mask"] or {}))
            est = pipe.estimate_mask(cond * model.scale_factor if z is None else z, self.text["text_cond"], self.text["text_uncond"], cond,
                                     **kw, **_seeded(self.seed, self.unit))
            mask = est["mask"]
        self.plan = _EditPlan(model, pipe, frames, cond, mask, a["strength"], a["mask_mode"], self.fib, self.nref, z=z, mask_shape=a["mask_shape"],
                              **({} if smap is None else {"strength_map": smap}))
        if self.keys is None and self.plan.shape is not None:   # return_mask gains shaped / support (a drawn mask has no dict before that)
            est = dict(est or {}, **self.plan.shape)
        if self.plan.release is not None:   # return_mask gains the release map (of the frames that are sampled) and the gate (of all frames)
            est = dict(est or {}, release=self.plan.release, gate=(self.plan.gate if self.keys is None else self.full_mask)[None])
        self.est = est
        self.conds, self.refs = split_batch(cond, self.fib, self.nref)
        self.windows = len(self.conds)
        self.wants_flow = hasattr(pipe, "obtain_flow_batched")
        if self.wants_flow and a["flows_per_window"] is None and getattr(pipe, "flow_estimator", None) is None and self.windows > 1:
            raise RuntimeError("optical-flow pipeline without a flow source: pass flows_per_window= or build the pipe with flow_estimator=")
        self.frame_chunks = split_batch(frames, self.fib, self.nref)[0] if self.wants_flow else None
        self.init = self.pred = None
        self.preds = []
        return self

    def _draw(self, k, like):
        """The initial noise of window k's NEW frames: injected, else the unit's seeded INIT stream, else the global generator."""
        if self.a["init_noises"] is not None:
            return self.a["init_noises"][k].to(device=self.dev, dtype=torch.float32)
        if self.seed is not None:
            return ops.randn(like.shape, self.seed, stream_id(INIT, self.unit, k), device=self.dev)
        return torch.randn(like.shape, device=self.dev, dtype=torch.float32)

    def window(self, k):
        a, conds = self.a, self.conds
        R = self.refs[k - 1] if k else 0
        new = self._draw(k, conds[k])
        self.init = torch.cat([self.init[:, -R:], new], dim=1) if k else new   # overlap re-uses the INITIAL noise (:139)
        start, known = self.plan.window(k, R, self.init)
        kw = dict(self.text, latent=start, img_cond=torch.cat([conds[k - 1][:, -R:], conds[k]], dim=1) if k else conds[0],
                  text_cfg=a["text_cfg"], img_cfg=a["video_cfg"], **_seeded(self.seed, self.unit), **known)
        if self.seed is not None and (k or self.number_first):
            kw["window"] = k
        if k:
            kw.update(latent_ref=self.pred[:, -R:], noise_correct_step=0.5)
            if a["flows_per_window"] is not None:
                kw["flows"] = a["flows_per_window"][k - 1]
            elif self.wants_flow:   # ref_images = the last R frames before this window, query_images = its new frames (:141-147)
                kw["ref_images"], kw["query_images"] = torch.cat(self.frame_chunks[:k], dim=1)[:, -R:], self.frame_chunks[k]
        return kw

    def receive(self, k, out):
        self.pred = out["latent"]
        self.preds.append(self.pred[:, self.refs[k - 1]:] if k else self.pred)

    def finish(self):
        latent = torch.cat(self.preds, dim=1)
        image = self.plan.finish(self.model.decode_latent_to_image(latent), self.frames)
        if self.keys is None:
            if self.stab is not None:
                image = _stabilize(self.source, image, self.stab, self.stab_flows, self.plan.composite_mask())
            return image, latent, self.est
        # the frames between the keys are filled along the source's flow; with a mask each of them is composited against the input with its
        # own mask exactly as the key frames were; the filter runs once, on the full-rate result.  The key frames stay bit for bit unless
        # it runs.  ``latent`` stays the key frames'.
        from .keyfill import keyframe_fill
        source, keys = self.source, self.keys
        fill = keyframe_fill(source, image, keys, flows=self.fill_flows, **{k: self.kf[k] for k in KEYFRAME_KEYS[1:] if k in self.kf})
        image = fill["frames"]
        if self.full_mask is not None:
            rows = torch.tensor([t for t in range(source.shape[1]) if t not in keys], dtype=torch.long, device=image.device)
            img = image[0].index_select(0, rows).to(torch.float32).contiguous()
            orig = source[0].to(device=img.device, dtype=torch.float32).index_select(0, rows).contiguous()
            img = ops.composite(img, orig, self.full_mask.index_select(0, rows).contiguous(), out=img)
            image[0].index_copy_(0, rows, img.to(image.dtype))
        if self.stab is not None:
            image = _stabilize(source, image, self.stab, self.stab_flows, self.full_mask)
        return image, latent, dict(self.est or {}, keys=list(keys), confidence=fill["confidence"])


def _result(image, latent, est, return_latent, return_mask):
    out = (image,) + ((latent,) if return_latent else ()) + ((est,) if return_mask else ())
    return out if len(out) > 1 else image


@torch.no_grad()
def edit_video(model, inf_pipe, frames, text_cond, text_uncond, text_cfg=7.5, video_cfg=1.8, frames_in_batch=16,
               num_ref_frames=4, init_noises=None, enc_noise=None, flows_per_window=None, return_latent=False, cond=None,
               seed=None, unit=0, mask=None, strength=1.0, mask_mode="max", auto_mask=None, return_mask=False,
               mask_key=None, mask_flows=None, flow_estimator=None, mask_track=None, stabilize=None, stabilize_flows=None, mask_shape=None,
               strength_map=None, keyframes=None, key_flows=None):
    """frames [1,T,3,H,W] in [-1,1] -> edited frames [1,T,3,H,W] clipped to [-1,1].

    ``seed`` (default None: every draw comes from the global torch generators, as before) makes the edit reproducible: the posterior
    noise, the initial latents of every window and the variance noise of every step come from the ENC / INIT / STEP streams of unit
    ``unit`` (insv2v/rng.py), generated by the HIP kernels - a pure function of (seed, unit, window, step, element), whatever else runs
    next to the unit and on however many GPUs.  An injected ``init_noises`` / ``enc_noise`` / ``cond`` wins over the seed.

    ``init_noises[k]`` / ``enc_noise`` optionally inject the random draws the reference takes from the
    global RNG (randn_like at :125,:139; the VAE posterior noise) so runs are reproducible.
    ``flows_per_window[k]`` (list over query frames of [R,2,H,W] flows) feeds the optical-flow variant precomputed
    flows; without it an optical-flow pipe gets the frames of the previous / current window (``ref_images`` /
    ``query_images``, insv2v_run_loveu_tgve.py:141-160) and runs its injected ``flow_estimator``.
    ``cond`` = an already encoded conditioning latent: the reference encodes a video ONCE and shares the posterior
    sample across its four prompts (:98).

    ``mask`` ([1,T,H,W] at image resolution, or [1,1,H,W] for all frames; 1 = edit, 0 = keep; soft values allowed) makes the edit
    local: it is reduced to latent resolution once (``mask_mode`` "max" - a cell is edited if any of its 8x8 pixels is - or "mean"),
    every step holds the latent outside it at the source video's, re-noised to that step's level with the window's initial noise
    (inside the step kernel), and the result is composited against the input frames, so pixels outside the mask ARE the input's.
    ``strength`` in (0, 1] makes the edit partial: only the last ``round(strength * steps)`` steps run, and at every strength below
    1.0 - also one that rounds to all steps - from the source latent noised to the first executed step's level instead of from pure noise.  With ``mask=None, strength=1.0`` the calls are exactly what they were.

    ``mask="auto"``: nobody drew a mask - it is estimated from the prompt, once per unit from the whole video and before the first
    window (``InferenceIP2PVideo.estimate_mask``), and then used exactly as a user's mask would be (it is constant
    over every 8x8 cell, so ``mask_mode`` has no effect on it).  ``auto_mask``: a dict of the estimator's keywords (``AUTO_MASK_KEYS``;
    default: its defaults, chunks of ``frames_in_batch`` frames); with ``seed`` the estimate's noise comes from the unit's MASK streams.
    ``return_mask=True`` appends the estimator's result dict (``raw``, ``soft``, ``mask_latent``, ``mask``; None without ``mask="auto"``)
    to the returned tuple.

    ``mask_key=k``: ``mask`` ([1,1,H,W]) is drawn on frame k only and follows the motion: the adjacent-frame flows
    - ``mask_flows``, a dict(fwd=, bwd=) of [T-1,2,H,W] flows, else computed by ``flow_estimator`` (default: the pipe's own) with
    ``mask_track.pair_flows`` - are chained into the flow from every frame to frame k and the mask is sampled once per frame
    (``mask_track.propagate_mask``; ``mask_track``: a dict of its keywords, ``MASK_TRACK_KEYS``).  Computed once per unit from the whole
    video, before the first window; from there it is a user's [1,T,H,W] mask.  ``return_mask=True`` then returns ``propagate_mask``'s
    dict (``mask``, ``valid``, ``flow_to_key``).  Without ``mask_key`` nothing of this runs.

    ``stabilize`` (True, or a dict of ``temporal_filter.stabilize``'s parameters, ``STABILIZE_KEYS``): the decoded frames of the WHOLE unit
    are filtered along the source video's optical flow after its last window, which also smooths the jump where one
    window hands over to the next; the result returned (and scored) is the filtered one, composited against the input under a mask like
    the edit itself.  The flows are ``stabilize_flows`` (dict(fwd=, bwd=) of [T-1,2,H,W]), else the ``mask_flows`` of a tracked mask, else
    computed by ``flow_estimator`` (default: the pipe's own) - once per unit: a tracked mask and the filter share one
    ``pair_flows(both=True)``.  Without ``stabilize`` nothing of this runs.

    ``mask_shape`` (a dict with keys among ``MASK_SHAPE_KEYS``: ``grow`` and ``feather`` in pixels, ``threshold``, ``profile``; DESIGN.md
    section 22) shapes the unit's mask - drawn, ``"auto"`` or tracked - once, before the first window: the composite (and ``stabilize``'s)
    uses ``shaped``, the mask grown by ``grow`` and feathered over ``feather`` pixels outside the grown edge; the latent hold uses
    ``support``, the hard region ``shaped > 0``, reduced with "max" - so ``mask_mode`` has no effect when ``mask_shape`` is given.  Outside
    ``support`` the pixels are the input's bit for bit.  ``return_mask=True`` then returns a dict that also holds ``shaped`` and
    ``support`` [1,T,H,W] (for a drawn mask: only those).  Without ``mask_shape`` nothing of this runs.

    ``keyframes`` (an int stride in 2 .. 8, or a dict with keys among ``KEYFRAME_KEYS``): only the key frames
    ``keyfill.key_frames(T, stride)`` - 0, stride, 2 stride, ... and always T - 1 - are denoised, and the frames in between take the edit
    from their two neighbouring keys along the SOURCE video's optical flow (``keyfill.keyframe_fill``).  The edit of the key frames is
    exactly ``edit_video(frames[:, keys], ...)`` with the same seed and unit id (``cond`` / ``enc_noise`` are indexed with the keys;
    ``init_noises`` / ``flows_per_window`` belong to that sub-video), so the key frames of the result are that call's, bit for bit.  The
    flows are ``key_flows`` (dict(fwd=, bwd=) of [T-1,2,H,W]), else ``stabilize_flows``, else ``mask_flows``, else computed by
    ``flow_estimator`` (default: the pipe's own) - ONE full-rate ``pair_flows(both=True)`` per unit, which also serves ``mask_key`` and
    ``stabilize``.  A ``mask_key`` mask is tracked over the full-rate video; with a mask every in-between frame is composited against
    the input with its own mask (``mask_shape``: shaped at full rate), so outside it every delivered frame is the input's, bit for bit;
    ``stabilize`` runs once, on the full-rate result.  ``return_latent`` returns the key frames' latent; ``return_mask`` a dict that also
    holds ``keys`` and ``confidence`` [T,H,W] (1 on the key frames).  Not with ``mask="auto"``.  Untuned starting values, as the filter's.
    Without ``keyframes`` nothing of this runs.

    ``strength_map`` (a floating-point [1,T,H,W] or [1,1,H,W] tensor in [0,1], or the string "mask") gives every
    pixel its own strength: the map is reduced per 8x8 latent cell like a mask (``mask_mode``), each cell's strength s is quantised like
    ``strength`` (``schedulers.strength_to_start``) into the step that releases it, ``release = steps - n_exec(s)``, and inside the step
    kernel the cell follows the source's re-noised latent through the steps before ``timesteps[release]`` and belongs to the model - under
    its mask value, if there is a mask - from there on; a cell of strength 0 is never released.  The result is composited with the gate
    ``G`` = 0 where the map is 0, elsewhere the unit's mask (or 1), so pixels of strength 0 ARE the input's; ``stabilize`` gets ``G`` as
    the unit's mask.  ``"mask"``: the map is the unit's final image mask - drawn or tracked, after ``mask_shape`` - so a feathered edge
    becomes a graded strength (with ``mask_shape`` the latent hold still comes from ``support``); it needs a mask, and not ``"auto"``
    (hard).  ``strength`` keeps its meaning: it decides which steps run at all, so a map value above it changes nothing more - and no
    step is skipped because no cell needs it (that would take a read-back): ``strength = max(map)`` saves those steps.  With
    ``keyframes`` the map is reduced to the keys as the mask is and the full-rate ``G`` serves the fill.  ``return_mask=True`` then
    returns a dict that also holds ``release`` [1,T,h,w] (int32; of the key frames with ``keyframes``) and ``gate`` [1,T,H,W].  Without
    ``strength_map`` nothing of this runs."""
    args = {k: v for k, v in locals().items() if k in UNIT_KEYS}
    _check_unit(frames.shape, args)
    u = _EditUnit(model, inf_pipe, frames, text_cond, text_uncond, frames_in_batch, num_ref_frames, seed, unit, flow_estimator, args).prepare()
    u.receive(0, inf_pipe(**u.window(0)))
    for k in range(1, u.windows):
        u.receive(k, inf_pipe.second_clip_forward(**u.window(k)))
    return _result(*u.finish(), return_latent, return_mask)


@torch.no_grad()
def edit_videos(model, inf_pipe, units, frames_in_batch=16, num_ref_frames=4, return_latent=False, seed=None, max_clips=None, return_mask=False,
                flow_estimator=None):
    """Several independent units at once - the throughput form of ``edit_video`` (the reference's unit loop offers them naturally: four
    prompts per video, insv2v_run_loveu_tgve.py:83,101): window k of ALL units runs as one stacked launch chain
    (``InferenceIP2PVideo.run_stacked``: B = 3 x units in every UNet launch, weights read once, every launch fills the chip), windows
    stay sequential inside a unit (latent_ref / initial-noise carry, :139-161).  ``units``: list of dicts with ``frames`` [1,T,3,H,W],
    ``text_cond``, ``text_uncond`` and optionally ``text_cfg`` (7.5), ``video_cfg`` (1.8), ``init_noises``, ``enc_noise``, ``cond`` - the
    arguments of ``edit_video`` (optical-flow pipes also ``flows_per_window``; without it the pipe's ``flow_estimator`` sees the frames
    of the previous / current window, :141-160).  All units must share T, H, W.  Returns the list of edited frames (and latents).  A
    single unit takes ``edit_video`` (one clip per launch chain, three branch streams).  The flow-warped correction is per-unit
    elementwise work behind the shared UNet launch, so optical-flow units stack like the others (round 5).
    ``seed``: as for ``edit_video``; a unit's id is ``u.get("unit", position in the list)``, so a unit that carries its id gets the same
    noise in any list, at any position.
    ``max_clips``: units per launch chain, as for ``run_stacked`` (None: its default cap, ``max_clips_in_flight``).
    A unit may carry ``mask``, ``strength`` and ``mask_mode`` as for ``edit_video``: masked and unmasked units stack together; the units
    of one call must share the number of executed steps (a stack shares ``start_time``), so strengths that round to different step
    counts raise ValueError.  A unit may also carry ``mask="auto"`` (and ``auto_mask``): its mask is estimated alone, in launches of its
    own, before the stacked windows start - so it is bit for bit the mask ``edit_video`` estimates for that unit.  ``return_mask``: as
    for ``edit_video``, per unit.  A unit may carry ``mask_key`` (and ``mask_flows``, ``mask_track``) as for ``edit_video``: its mask is
    tracked alone, before the stacked windows start, bit for bit as ``edit_video`` tracks it; ``flow_estimator`` is the flow source of
    the units without ``mask_flows`` (default: the pipe's own).  Tracked, drawn, auto and unmasked units stack together.  A unit may carry
    ``stabilize`` (and ``stabilize_flows``) as for ``edit_video``: it is filtered alone, after the stacked windows have finished, bit for
    bit as ``edit_video`` filters it; stabilized and plain units stack together.  A unit may carry ``mask_shape`` as for ``edit_video``: its
    mask is shaped alone, before the stacked windows start, bit for bit as ``edit_video`` shapes it.  A unit may carry ``keyframes`` (and
    ``key_flows``) as for ``edit_video``: the units' SUB-VIDEOS of key frames are what stack - they must share a shape, under the same
    ValueError - and each unit is filled alone, after the stacked windows, bit for bit as ``edit_video`` fills it; its latent is its key
    frames'.  A unit may carry ``strength_map`` as for ``edit_video``: its release map is built alone, before the stacked windows start;
    mapped, masked and plain units stack together (``strength`` still has to be shared)."""
    if len(units) == 0:
        return []
    for u in units:
        _check_unit(u["frames"].shape, u)
    if len({_start_time(inf_pipe, u.get("strength", 1.0)) for u in units}) > 1:
        raise ValueError("edit_videos: the units of one call must share the number of executed steps (strength); edit the others separately")
    ids = [u.get("unit", j) for j, u in enumerate(units)]
    if len(units) == 1:
        u = units[0]
        more = {"return_mask": True} if return_mask else {}   # (a plain call carries no new keyword)
        if flow_estimator is not None:
            more["flow_estimator"] = flow_estimator
        return [edit_video(model, inf_pipe, u["frames"], u["text_cond"], u["text_uncond"], frames_in_batch=frames_in_batch,
                           num_ref_frames=num_ref_frames, return_latent=return_latent, seed=seed, unit=ids[0], **more,
                           **{k: u[k] for k in UNIT_KEYS if k in u})]
    st = [_EditUnit(model, inf_pipe, u["frames"], u["text_cond"], u["text_uncond"], frames_in_batch, num_ref_frames, seed, uid, flow_estimator,
                    {k: u[k] for k in UNIT_KEYS if k in u}, number_first_window=True) for u, uid in zip(units, ids)]
    if len({s.shape for s in st}) > 1:   # (of a key-frame unit: its sub-video of key frames, which is what stacks)
        raise ValueError("edit_videos: all units must share [1,T,3,H,W]")
    cap = {} if max_clips is None else {"max_clips": max_clips}   # (a pipe without the parameter keeps working with the default)
    for s in st:   # each alone, before the first stacked window of any unit
        s.prepare()
    for k in range(st[0].windows):
        for s, r in zip(st, inf_pipe.run_stacked([s.window(k) for s in st], **cap)):
            s.receive(k, r)
    return [_result(*s.finish(), return_latent, return_mask) for s in st]   # each alone, after the stacked windows


def build_parser():
    p = argparse.ArgumentParser(description="InsV2V LOVEU-TGVE editing on MI355X")
    p.add_argument("--text-cfg", nargs="+", type=float, default=[7.5], help="Text configuration parameter")
    p.add_argument("--video-cfg", nargs="+", type=float, default=[1.8], help="Image configuration parameter")
    p.add_argument("--num-frames", nargs="+", type=int, default=[32], help="Number of frames")
    p.add_argument("--image-size", nargs="+", type=int, default=[384], help="Image size")
    p.add_argument("--prompt-source", type=str, default="edit", help="Prompt source")
    p.add_argument("--ckpt-path", type=str, help="Path to checkpoint")
    p.add_argument("--config-path", type=str, default="configs/instruct_v2v.yaml", help="Path to config file")
    p.add_argument("--data-dir", type=str, default="loveu-tgve-2023", help="Path to LOVEU dataset")
    p.add_argument("--with_optical_flow", action="store_true", help="Use motion compensation")
    # additions of this build
    p.add_argument("--edit-prompt-file", type=str, default="dataset/loveu_tgve_edit_prompt_dict.json")
    p.add_argument("--tokenizer-dir", type=str, default=None, help="directory with the CLIP vocab.json / merges.txt")
    p.add_argument("--units", type=str, default=None, help=".pt file with pre-decoded frames and text embeddings")
    p.add_argument("--synthetic", type=int, default=0, help="run on N synthetic clips with random-init weights")
    p.add_argument("--out", type=str, default="v2v_results/edited.pt")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--scheduler", type=str, default="ddpm", help="ddpm | ddim | dpmsolver++ | sde-dpmsolver++")
    p.add_argument("--solver-order", type=int, default=2, choices=(1, 2),
                   help="order of --scheduler dpmsolver++ / sde-dpmsolver++ (2 = DPM-Solver++ 2M; the other schedulers ignore it)")
    p.add_argument("--seed", type=int, default=None,
                   help="reproducible sampling: every random draw comes from the seeded noise streams of the unit (insv2v/rng.py); "
                        "units are numbered globally, so a unit's result does not depend on --gpus, stacking or unit order")
    p.add_argument("--no-stack", action="store_true",
                   help="edit one unit at a time (one clip per UNet launch chain) instead of stacking a rank's units / a video's four prompts")
    p.add_argument("--max-stack", type=int, default=None,
                   help="units per stacked launch chain (default: inference.max_clips_in_flight of the clip shape, at most 20); any stack "
                        "that fits in memory runs, a frame that no kernel can address is refused before the first launch")
    p.add_argument("--strength", type=float, default=1.0,
                   help="partial edit: in (0, 1]; only the last round(strength * steps) steps run, from the noised source latent (1.0: from pure noise)")
    p.add_argument("--mask-mode", type=str, default="max",
                   help="mean | max: how an image-resolution mask (the optional \"mask\" entry of a --units file, [n,T,H,W] or [n,1,H,W]; "
                        "--synthetic-mask) is reduced to one value per 8x8 latent cell")
    p.add_argument("--synthetic-mask", action="store_true", help="with --synthetic: edit only a centred rectangle (half the height and width) of every frame")
    p.add_argument("--auto-mask", action="store_true",
                   help="localized edit without a drawn mask: every unit's mask is estimated from its prompt (InferenceIP2PVideo.estimate_mask) "
                        "before its first window; the --auto-mask-* values are starting points, not tuned on a real checkpoint")
    p.add_argument("--auto-mask-maps", type=int, default=4, help="noised copies of the source latent the estimate averages over")
    p.add_argument("--auto-mask-strength", type=float, default=0.5, help="in (0, 1]: the noise level of those copies, as --strength")
    p.add_argument("--auto-mask-threshold", type=float, default=0.5, help="in (0, 1): a cell is edited where the normalised map exceeds it")
    p.add_argument("--auto-mask-dilate", type=int, default=1, help="latent cells the thresholded mask is grown by")
    p.add_argument("--mask-out", type=str, default=None,
                   help=".pt file for the masks this run computed: {unit id: {mask_latent, soft}} with --auto-mask, {unit id: {mask, valid}} with --mask-key; "
                        "with --mask-grow / --mask-feather each also holds the shaped mask and its support")
    p.add_argument("--mask-file", type=str, default=None,
                   help=".pt file with drawn masks: {unit id or video name: tensor [1,1,H,W] or [1,T,H,W]} (image resolution; units it does not "
                        "name are edited whole)")
    p.add_argument("--mask-image", type=str, default=None,
                   help="a drawn mask from image files: one image (a still mask for every frame) or a directory of images sorted by name (one "
                        "per frame); read as 8-bit grey, white = edit, resized like the frames; every unit gets it")
    p.add_argument("--mask-grow", type=float, default=None,
                   help="shape every unit's mask (drawn, tracked or estimated; insv2v/mask_shape.py): grow it by F pixels, negative shrinks, "
                        "[-32, 32]; the --mask-grow / --mask-feather / --mask-profile / --mask-threshold values are starting points, untuned")
    p.add_argument("--mask-feather", type=float, default=None,
                   help="feather the mask over F pixels OUTSIDE its (grown) edge, [0, 32]: the composite blends there, the latent is free there")
    p.add_argument("--mask-profile", type=str, default=None, help="linear | smooth (default): the feather's ramp")
    p.add_argument("--mask-threshold", type=float, default=None, help="a pixel is inside the mask where its value exceeds this (default 0.5)")
    p.add_argument("--strength-map", type=str, default=None,
                   help="per-pixel edit strength (DESIGN.md section 28): a .pt tensor [1,T,H,W] or [1,1,H,W] in [0,1], or an image / a directory "
                        "of images read like --mask-image (white = fully re-drawn, black = never touched); every unit gets it; a --units file "
                        "may carry its own \"strength_map\" entry [n,T,H,W] or [n,1,H,W] instead.  No step is skipped because no pixel "
                        "needs it: --strength max(map) saves those steps")
    p.add_argument("--strength-from-mask", action="store_true",
                   help="every unit's final mask (drawn or tracked, after --mask-grow / --mask-feather) is its strength map: a feathered edge "
                        "becomes a graded strength; needs a drawn mask (--mask-file, --mask-image, --synthetic-mask, the \"mask\" entry of a --units file)")
    p.add_argument("--mask-key", type=int, default=None,
                   help="the frame the masks are drawn on ([1,1,H,W] each): they follow the motion through the video (insv2v/mask_track.py); the "
                        "flows come from the estimator of --raft-ckpt (--synthetic: key-hashed weights)")
    p.add_argument("--mask-no-occlusion", action="store_true",
                   help="with --mask-key: no forward-backward consistency check (half the flow pairs; occluded pixels keep a traced mask value)")
    p.add_argument("--raft-ckpt", type=str, default=None,
                   help="torchvision raft_large checkpoint (state dict) for --with_optical_flow: the estimator runs on the HIP kernels")
    p.add_argument("--flows", type=str, default=None,
                   help=".pt file with precomputed optical flows for --with_optical_flow: flows[unit][window][query] = [R,2,H,W]")
    p.add_argument("--score-ckpt", type=str, default=None,
                   help="CLIP checkpoint (state dict, transformers CLIPModel or OpenAI clip layout) to score every edit with: CLIP text "
                        "alignment and frame consistency on the HIP kernels (insv2v/clip_score.py)")
    p.add_argument("--score-name", type=str, default="ViT-L/14", help="the CLIP model --score-ckpt holds (the reference's ViT names)")
    p.add_argument("--score-out", type=str, default=None, help="JSON file for the scores: one record per unit")
    p.add_argument("--score-synthetic", action="store_true", help="with --synthetic: score with a key-hashed CLIP (no checkpoint needed)")
    p.add_argument("--score-pixels", action="store_true",
                   help="add per-frame mse / psnr / ssim of every edit against its source to the --score-out records, and with a mask (drawn, "
                        "tracked or estimated) the same inside and outside it (insv2v/pixel_score.py); needs no CLIP scorer")
    p.add_argument("--score-warp", action="store_true",
                   help="add the flow warp error of every edit (and of its source) along the source video's optical flow to the --score-out "
                        "records; the flows come from the estimator of --raft-ckpt (--synthetic: key-hashed weights)")
    p.add_argument("--stabilize", action="store_true",
                   help="filter every edit along the SOURCE video's optical flow after its last window (insv2v/temporal_filter.py): less "
                        "flicker and a smoother hand-over between windows; the flows come from the estimator of --raft-ckpt (--synthetic: "
                        "key-hashed weights); the --stabilize-* values are starting points, not tuned on real footage")
    p.add_argument("--stabilize-radius", type=int, default=None, help="frames on either side the filter averages over, 1 .. 4 (default 2)")
    p.add_argument("--stabilize-sigma", type=float, default=None,
                   help="how much the source may differ between the two ends of a trajectory, on [0, 1] data (default 0.1)")
    p.add_argument("--stabilize-strength", type=float, default=None, help="in (0, 1]: the weight of a perfectly matching neighbour (default 1)")
    p.add_argument("--stabilize-no-occlusion", action="store_true", help="with --stabilize: no forward-backward consistency check on the trajectories")
    p.add_argument("--key-stride", type=int, default=None,
                   help="denoise only every N-th frame (and the last), 2 .. 8, and fill the frames in between along the SOURCE video's optical "
                        "flow (insv2v/keyfill.py): about N times the delivered frames per GPU second; the flows come from the estimator of "
                        "--raft-ckpt (--synthetic: key-hashed weights); the --key-* values are starting points, not tuned on real footage")
    p.add_argument("--key-mode", type=str, default=None,
                   help="residual (default): carry what the edit CHANGED on the key frames; warp: carry the edited pixels themselves")
    p.add_argument("--key-sigma", type=float, default=None,
                   help="how much the source may differ between an in-between frame and its key along a trajectory, on [0, 1] data (default 0.1)")
    p.add_argument("--key-no-occlusion", action="store_true", help="with --key-stride: no forward-backward consistency check on the trajectories")
    p.add_argument("--synthetic-tiny", action="store_true", help="with --synthetic: the reduced-width UNet / VAE (and scorer) configurations")
    p.add_argument("--region", action="store_true",
                   help="edit a region at full resolution (insv2v/region.py): the frames keep their native size, the box around the mask of "
                        "--mask-image / --mask-file (else the whole frame) is resampled to --image-size, which is then the WORKING size, "
                        "edited there and pasted back over the untouched source; scores are taken at the source's resolution; the "
                        "--region-* values are starting points, untuned")
    p.add_argument("--region-box", nargs=4, type=int, default=None, metavar=("X0", "Y0", "X1", "Y1"),
                   help="with --region: the box to edit, in source pixels, half-open (default: the box around the mask; the whole frame "
                        "without a drawn mask, also with --auto-mask / --mask-key, whose masks exist only at working resolution)")
    p.add_argument("--region-pad", type=float, default=None, help="with --region: the mask's box grows by F x its longer side (default 0.25)")
    p.add_argument("--region-mode", type=str, default=None,
                   help="residual (default): carry what the edit CHANGED up to the source's resolution; replace: blend the resampled edit in under the mask")
    p.add_argument("--region-blend", type=float, default=None, help="with --region: pixels over which the paste ramps in at the box edges (default 8)")
    p.add_argument("--region-source", nargs=2, type=int, default=None, metavar=("W", "H"),
                   help="with --synthetic and --region: the size of the synthetic source frames (default: --image-size)")
    p.add_argument("--region-track", action="store_true",
                   help="with --region: the box follows the object (insv2v/region_track.py) - every frame gets its own box of one size, moved by "
                        "fractions of a pixel along the smoothed centres of the per-frame mask of --mask-file or a --mask-image folder")
    p.add_argument("--region-track-smooth", type=float, default=None,
                   help="with --region-track: the sigma in frames of the Gaussian the box centres are smoothed with (default 2; 0: none)")
    return p


def check_args(args):
    """Fail at parse time, not after the first window has been sampled.  The optical-flow variant needs a flow source: the RAFT
    estimator runs on the HIP kernels (insv2v/raft.py) but its pretrained weights are not bundled (the reference downloads them,
    flow_utils.py:157): ``--raft-ckpt`` names torchvision's raft_large checkpoint, ``--synthetic`` runs use key-hashed weights, and
    ``--flows`` supplies precomputed flows instead."""
    if args.with_optical_flow and not (args.flows or args.raft_ckpt or args.synthetic):
        raise SystemExit("--with_optical_flow needs --raft-ckpt FILE (torchvision raft_large weights) or --flows FILE (precomputed flows)")
    if getattr(args, "max_stack", None) is not None and args.max_stack < 1:
        raise SystemExit("--max-stack needs a positive number of units")
    strength = getattr(args, "strength", 1.0)
    if not (0.0 < strength <= 1.0):
        raise SystemExit(f"--strength must be in (0, 1], not {strength}")
    if getattr(args, "mask_mode", "max") not in MASK_MODES:
        raise SystemExit(f"--mask-mode must be mean or max, not {args.mask_mode}")
    if getattr(args, "synthetic_mask", False) and not args.synthetic:
        raise SystemExit("--synthetic-mask needs --synthetic N (masks of real units come from the \"mask\" entry of a --units file)")
    if hasattr(args, "auto_mask_maps"):   # (out-of-range values are refused with or without --auto-mask)
        from .inference import check_automask_args
        try:
            check_automask_args(**auto_mask_kwargs(args))
        except ValueError as e:
            raise SystemExit(f"--auto-mask-maps / --auto-mask-strength / --auto-mask-threshold / --auto-mask-dilate: {e}")
    if getattr(args, "auto_mask", False) and getattr(args, "synthetic_mask", False):
        raise SystemExit("--auto-mask and --synthetic-mask are two masks: pass one")
    mask_key, mask_file = getattr(args, "mask_key", None), getattr(args, "mask_file", None)
    mask_image, shaping = getattr(args, "mask_image", None), bool(mask_shape_unit(args))
    if getattr(args, "mask_out", None) and not getattr(args, "auto_mask", False) and mask_key is None and not shaping:
        raise SystemExit("--mask-out holds the masks a run computes: it needs --auto-mask or --mask-key")
    if mask_file and (getattr(args, "auto_mask", False) or getattr(args, "synthetic_mask", False)):
        raise SystemExit("--mask-file next to --auto-mask / --synthetic-mask are two masks: pass one")
    if mask_image and (mask_file or getattr(args, "auto_mask", False) or getattr(args, "synthetic_mask", False)):
        raise SystemExit("--mask-image next to --mask-file / --auto-mask / --synthetic-mask are two masks: pass one")
    if mask_image and not os.path.exists(mask_image):
        raise SystemExit(f"--mask-image {mask_image} is neither a file nor a directory")
    if shaping:
        from .mask_shape import check_shape_args
        try:
            check_shape_args(**mask_shape_unit(args)["mask_shape"])
        except ValueError as e:
            raise SystemExit(f"--mask-grow / --mask-feather / --mask-profile / --mask-threshold: {e}")
        if not (mask_file or mask_image or getattr(args, "auto_mask", False) or getattr(args, "synthetic_mask", False) or args.units):
            raise SystemExit("--mask-grow / --mask-feather / --mask-profile / --mask-threshold shape a mask: they need --mask-file, --mask-image, "
                             "--auto-mask, --synthetic-mask or the \"mask\" entry of a --units file")
    smap, from_mask = getattr(args, "strength_map", None), getattr(args, "strength_from_mask", False)
    if smap and from_mask:
        raise SystemExit("--strength-map and --strength-from-mask are two strength maps: pass one")
    if smap and not os.path.exists(smap):
        raise SystemExit(f"--strength-map {smap} is neither a file nor a directory")
    if smap and getattr(args, "region", False):
        raise SystemExit("--strength-map with --region: a map is not resampled to the working clip (not built); --strength-from-mask works there")
    if from_mask and getattr(args, "auto_mask", False):
        raise SystemExit("--strength-from-mask and --auto-mask: an estimated mask is hard (0 or 1), it grades nothing; pass --strength-map")
    if from_mask and not (mask_file or mask_image or getattr(args, "synthetic_mask", False) or args.units):
        raise SystemExit("--strength-from-mask needs a mask: --mask-file FILE.pt, --mask-image PATH, the \"mask\" entry of a --units file, or --synthetic-mask")
    if mask_key is not None:
        if getattr(args, "auto_mask", False):
            raise SystemExit("--mask-key tracks a drawn mask and --auto-mask estimates one per frame: pass one")
        if mask_key < 0:
            raise SystemExit(f"--mask-key must be a frame index, not {mask_key}")
        if not (mask_file or mask_image or getattr(args, "synthetic_mask", False) or args.units):
            raise SystemExit("--mask-key needs a mask to track: --mask-file FILE.pt, --mask-image PATH, the \"mask\" entry of a --units file, or --synthetic-mask")
        if not (args.raft_ckpt or args.synthetic):
            raise SystemExit("--mask-key needs --raft-ckpt FILE (torchvision raft_large weights): the flows the mask follows come from that estimator")
    elif getattr(args, "mask_no_occlusion", False):
        raise SystemExit("--mask-no-occlusion is a parameter of --mask-key")
    if getattr(args, "stabilize", False):
        if not (args.raft_ckpt or args.synthetic):
            raise SystemExit("--stabilize needs --raft-ckpt FILE (torchvision raft_large weights): the flows the filter follows come from that estimator")
        from .temporal_filter import check_filter_args
        try:
            check_filter_args(**stabilize_unit(args)["stabilize"])
        except ValueError as e:
            raise SystemExit(f"--stabilize-radius / --stabilize-sigma / --stabilize-strength: {e}")
    elif any(getattr(args, k, None) for k in ("stabilize_radius", "stabilize_sigma", "stabilize_strength", "stabilize_no_occlusion")):
        raise SystemExit("--stabilize-radius / --stabilize-sigma / --stabilize-strength / --stabilize-no-occlusion are parameters of --stabilize")
    if getattr(args, "key_stride", None) is not None:
        if not (args.raft_ckpt or args.synthetic):
            raise SystemExit("--key-stride needs --raft-ckpt FILE (torchvision raft_large weights): the flows the frames in between are filled along come from that estimator")
        if getattr(args, "auto_mask", False):
            raise SystemExit("--key-stride and --auto-mask: an estimated mask exists on the key frames only; draw the mask, or track one with --mask-key")
        from .keyfill import check_fill_args
        try:
            check_fill_args(**keyframe_unit(args)["keyframes"])
        except ValueError as e:
            raise SystemExit(f"--key-stride / --key-mode / --key-sigma: {e}")
    elif any(getattr(args, k, None) for k in ("key_mode", "key_sigma", "key_no_occlusion")):
        raise SystemExit("--key-mode / --key-sigma / --key-no-occlusion are parameters of --key-stride")
    if args.flows and args.units is None and not args.synthetic:
        raise SystemExit("--flows is supported with --units / --synthetic (flows are indexed by unit)")
    score_synth, score_ckpt, score_out = (getattr(args, k, None) for k in ("score_synthetic", "score_ckpt", "score_out"))
    if score_synth and not args.synthetic:
        raise SystemExit("--score-synthetic needs --synthetic N (real units are scored with --score-ckpt FILE)")
    if score_synth and score_ckpt:
        raise SystemExit("--score-synthetic and --score-ckpt are two scorers: pass one")
    score_pixels, score_warp = getattr(args, "score_pixels", False), getattr(args, "score_warp", False)
    if score_warp and not (args.raft_ckpt or args.synthetic):
        raise SystemExit("--score-warp needs --raft-ckpt FILE (torchvision raft_large weights): the flows the frames are warped along come from that estimator")
    if (score_pixels or score_warp) and not score_out:
        raise SystemExit("--score-pixels / --score-warp need --score-out FILE.json for the scores")
    if score_out and not (score_ckpt or score_synth or score_pixels or score_warp):
        raise SystemExit("--score-out needs a scorer: --score-ckpt FILE (or --score-synthetic with --synthetic N)")
    if (score_ckpt or score_synth) and not score_out:
        raise SystemExit("--score-ckpt / --score-synthetic need --score-out FILE.json for the scores")
    if getattr(args, "synthetic_tiny", False) and not args.synthetic:
        raise SystemExit("--synthetic-tiny needs --synthetic N")
    if getattr(args, "region", False):
        from .region import check_region
        for size in args.image_size:
            try:
                check_region(region_unit(args, size)["region"])
            except ValueError as e:
                raise SystemExit(f"--region / --region-box / --region-pad / --region-mode / --region-blend (working size --image-size {size}): {e}")
        if getattr(args, "region_source", None) is not None and (not args.synthetic or min(args.region_source) < 1):
            raise SystemExit("--region-source W H sets the size of the --synthetic N source frames: it needs --synthetic and two positive numbers")
        if getattr(args, "region_track", False):
            from .region_track import check_track
            try:
                check_track(region_unit(args)["track"])
            except ValueError as e:
                raise SystemExit(f"--region-track / --region-track-smooth: {e}")
            if getattr(args, "region_box", None) is not None:
                raise SystemExit("--region-box fixes one box and --region-track moves it: give one of them")
            if getattr(args, "auto_mask", False) or getattr(args, "mask_key", None) is not None:
                raise SystemExit("--region-track follows a drawn per-frame mask (--mask-file, a --mask-image folder): the masks of --auto-mask and "
                                 "--mask-key exist only inside the working-resolution edit")
        elif getattr(args, "region_track_smooth", None) is not None:
            raise SystemExit("--region-track-smooth is a parameter of --region-track")
    elif getattr(args, "region_track", False) or getattr(args, "region_track_smooth", None) is not None:
        raise SystemExit("--region-track / --region-track-smooth need --region")
    elif any(getattr(args, k, None) is not None for k in ("region_box", "region_pad", "region_mode", "region_blend", "region_source")):
        raise SystemExit("--region-box / --region-pad / --region-mode / --region-blend / --region-source are parameters of --region")
    return args


def build_scorer(args, device, tokenizer=None):
    """The CLI's scorer (None without one): --score-ckpt in either layout, or key-hashed weights with --score-synthetic."""
    from .clip_score import load_scorer, synthetic_scorer
    if getattr(args, "score_synthetic", False):
        return synthetic_scorer(device=device, tiny=getattr(args, "synthetic_tiny", False))
    if getattr(args, "score_ckpt", None):
        return load_scorer(args.score_ckpt, name=args.score_name, device=device, tokenizer=tokenizer)
    return None


def score_record(scorer, unit, frames, edited, source_text, edit_text):
    """One record of --score-out: the unit id, the five per-frame lists and the two means (clip_score.ClipSimilarity.score_edit)."""
    r = scorer.score_edit(frames, edited, source_text, edit_text)
    return {"unit": int(unit), **{k: (v.tolist() if torch.is_tensor(v) else v) for k, v in r.items()}}


PIXEL_FIDELITY_KEYS = ("mse", "psnr", "ssim")   # and, for a unit with a mask, each with _inside and _outside
PIXEL_WARP_KEYS = ("warp_error", "warp_error_source", "warp_error_mean", "warp_error_source_mean", "valid_fraction")


def pixel_record(args, frames, edited, mask=None, flow_estimator=None):
    """What --score-pixels / --score-warp add to a unit's record (pixel_score.score_pixels): the fidelity fields (per-frame lists; with a
    mask also _inside / _outside) and / or the warp fields (per-pair lists and the two means).  ``inf`` (a region the edit left
    bit-identical) and ``nan`` (an empty region) are written as json's Infinity / NaN."""
    from .pixel_score import score_pixels
    pixels, warp = getattr(args, "score_pixels", False), getattr(args, "score_warp", False)
    if not (pixels or warp):
        return {}
    r = score_pixels(frames, edited, flow_estimator=flow_estimator if warp else None, mask=mask if pixels else None)
    return {k: v.tolist() for k, v in r.items() if (pixels if k not in PIXEL_WARP_KEYS else warp)}


def want_pixel_scores(args):
    return bool(getattr(args, "score_pixels", False) or getattr(args, "score_warp", False))


def unit_record(args, unit, frames, edited, scorer=None, texts=None, est=None, drawn=None, flow_estimator=None):
    """A unit's --score-out record, assembled from its parts: the CLIP scores (``scorer``, with ``texts()`` = the source and the edit
    prompt), the pixel scores (the region: the unit's image-resolution mask - shaped, tracked or estimated if the run made one, ``est``,
    else as ``drawn``) and the key-frame fields."""
    rec = {"unit": int(unit)}
    if scorer is not None:   # the edited frames are still on the device
        rec.update(score_record(scorer, unit, frames, edited, *texts()))
    if want_pixel_scores(args):
        rec.update(pixel_record(args, frames, edited, mask_region(est, drawn), flow_estimator))
    rec.update(keyframe_record(args, est))
    return rec


def _rank_path(path, rank, world):
    """This rank's output path (with several ranks each writes its own FILE.rankR.ext), its directory created."""
    if world > 1:
        root, ext = os.path.splitext(path)
        path = f"{root}.rank{rank}{ext}"
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    return path


def write_scores(path, records, rank=0, world=1):
    """The records of this rank, sorted by unit id (with several ranks each writes its own FILE.rankR.json)."""
    import json
    with open(_rank_path(path, rank, world), "w") as f:
        json.dump(sorted(records, key=lambda r: r["unit"]), f, indent=1)


def auto_mask_kwargs(args):
    """The estimator's keywords of the --auto-mask-* flags."""
    return dict(n_maps=args.auto_mask_maps, mask_strength=args.auto_mask_strength, threshold=args.auto_mask_threshold, dilate=args.auto_mask_dilate)


def auto_mask_unit(args, data=None):
    """What --auto-mask adds to every unit (nothing without it).  A --units file that carries its own ``mask`` entry is refused."""
    if not getattr(args, "auto_mask", False):
        return {}
    if data is not None and data.get("mask") is not None:
        raise SystemExit("--auto-mask estimates every unit's mask, but the --units file holds a \"mask\" entry: pass one of the two")
    return dict(mask="auto", auto_mask=auto_mask_kwargs(args))


def mask_track_unit(args):
    """What --mask-key adds to every unit that has a mask (nothing without it)."""
    if getattr(args, "mask_key", None) is None:
        return {}
    return dict(mask_key=args.mask_key, mask_track=dict(occlusion=not getattr(args, "mask_no_occlusion", False)))


def stabilize_unit(args):
    """What --stabilize adds to every unit (nothing without it)."""
    if not getattr(args, "stabilize", False):
        return {}
    from .temporal_filter import FILTER_DEFAULTS
    pick = lambda k: FILTER_DEFAULTS[k] if getattr(args, "stabilize_" + k, None) is None else getattr(args, "stabilize_" + k)   # noqa: E731
    return dict(stabilize=dict(radius=pick("radius"), sigma=pick("sigma"), strength=pick("strength"),
                               occlusion=not getattr(args, "stabilize_no_occlusion", False)))


def keyframe_unit(args):
    """What --key-stride adds to every unit (nothing without it)."""
    if getattr(args, "key_stride", None) is None:
        return {}
    from .keyfill import FILL_DEFAULTS
    pick = lambda k: FILL_DEFAULTS[k] if getattr(args, "key_" + k, None) is None else getattr(args, "key_" + k)   # noqa: E731
    return dict(keyframes=dict(stride=args.key_stride, mode=pick("mode"), sigma=pick("sigma"), occlusion=not getattr(args, "key_no_occlusion", False)))


def keyframe_record(args, est):
    """What --key-stride adds to a unit's --score-out record: the stride, the key-frame indices and the mean fill confidence per frame
    (1 on the key frames; a unit whose frames are all keys has no fill: every frame is listed as a key)."""
    if getattr(args, "key_stride", None) is None:
        return {}
    if est is None or "keys" not in est:
        return {"key_stride": args.key_stride}
    return {"key_stride": args.key_stride, "key_frames": [int(k) for k in est["keys"]],
            "key_confidence": est["confidence"].float().mean((1, 2)).tolist()}


def mask_shape_unit(args):
    """What --mask-grow / --mask-feather / --mask-profile / --mask-threshold add to every unit that has a mask (nothing without any of
    them): only the values given, the others keep ``check_shape_args``' defaults."""
    given = {k: getattr(args, "mask_" + k, None) for k in ("grow", "feather", "profile", "threshold")}
    given = {k: v for k, v in given.items() if v is not None}
    return dict(mask_shape=given) if given else {}


def load_strength_map(args, width, height):
    """The map of --strength-map at the frames' size ([1,1,H,W] or [1,T,H,W]; None without it): a .pt tensor as it is, images through
    ``video_io.load_mask``."""
    path = getattr(args, "strength_map", None)
    if not path:
        return None
    if path.lower().endswith(".pt"):
        m = torch.load(path, map_location="cpu")
        if not torch.is_tensor(m) or m.dim() != 4 or m.shape[0] != 1:
            raise SystemExit("--strength-map FILE.pt must hold a tensor [1,T,H,W] or [1,1,H,W]")
        return m
    from .video_io import load_mask
    return load_mask(path, (width, height))


def strength_map_unit(args, has_mask, smap=None):
    """What --strength-from-mask (a unit with a mask) or a strength map (``smap``: --strength-map's, or the unit's entry of a --units
    file) adds to a unit - nothing without them."""
    if getattr(args, "strength_from_mask", False):
        return dict(strength_map="mask") if has_mask else {}
    return {} if smap is None else dict(strength_map=smap)


def region_unit(args, image_size=None):
    """What --region adds to every unit (nothing without it): ``region=`` of ``region.edit_region`` with the working size --image-size
    (``image_size``: that of one combination) and only the values given; the others keep ``check_region``'s defaults.  Without
    --region-box the box comes from the unit's drawn mask; --auto-mask and --mask-key make their mask inside the working-resolution
    edit, so they take the whole frame.  --region-track adds ``track=`` (True, or the --region-track-smooth given)."""
    if not getattr(args, "region", False):
        return {}
    S = args.image_size[0] if image_size is None else image_size
    r = dict(size=(S, S))
    if getattr(args, "region_box", None) is not None:
        r["box"] = tuple(args.region_box)
    elif getattr(args, "auto_mask", False) or getattr(args, "mask_key", None) is not None:
        r["box"] = "frame"
    for k in ("pad", "mode", "blend"):
        if getattr(args, "region_" + k, None) is not None:
            r[k] = getattr(args, "region_" + k)
    if getattr(args, "region_track", False):   # the extra entry only with the switch: ``track=`` of the same drivers
        smooth = getattr(args, "region_track_smooth", None)
        return dict(region=r, track=True if smooth is None else dict(smooth=smooth))
    return dict(region=r)


def region_est(args, est):
    """The dict the scores read a unit's mask from: with --region the masks a run computed are at WORKING resolution, and the scores are
    taken at the source's, so only the drawn mask splits them."""
    if not getattr(args, "region", False) or est is None:
        return est
    return {k: v for k, v in est.items() if k not in ("shaped", "support", "mask", "release", "gate")}


def load_mask_image(args, width, height):
    """The mask of --mask-image at the frames' size ([1,1,H,W] or [1,T,H,W]; None without it); ``width=None``: at its native size."""
    if not getattr(args, "mask_image", None):
        return None
    from .video_io import load_mask
    return load_mask(args.mask_image, None if width is None else (width, height))


def mask_region(est, drawn):
    """The region --score-pixels splits a unit by: the shaped mask if the run shaped one, else the tracked / estimated one, else as drawn."""
    if est is not None and ("shaped" in est or "mask" in est):   # (a key-frame unit's dict may hold only its keys and confidence)
        return est["shaped"] if "shaped" in est else est["mask"]
    return drawn


def load_mask_file(args):
    """{unit id or video name: mask tensor} of --mask-file ({} without it)."""
    if not getattr(args, "mask_file", None):
        return {}
    masks = torch.load(args.mask_file, map_location="cpu")
    if not isinstance(masks, dict) or not all(torch.is_tensor(m) and m.dim() == 4 and m.shape[0] == 1 for m in masks.values()):
        raise SystemExit("--mask-file must hold {unit id or video name: tensor [1,1,H,W] or [1,T,H,W]}")
    return masks


def build_flow_estimator(args, device):
    """The CLI's flow estimator of --mask-key, --stabilize and --score-warp (None without any): RAFT on the HIP kernels with the weights of
    --raft-ckpt, key-hashed weights in a --synthetic run."""
    if getattr(args, "mask_key", None) is None and not getattr(args, "score_warp", False) and not getattr(args, "stabilize", False) \
            and getattr(args, "key_stride", None) is None:
        return None
    from .raft import RAFTFlow
    if args.raft_ckpt:
        return RAFTFlow(device).load_state_dict(torch.load(args.raft_ckpt, map_location="cpu"))
    from . import synth, shapes
    return RAFTFlow(device, synth.synth_raft_state_dict(shapes.raft_shapes()))


def write_masks(path, records, rank=0, world=1):
    """{unit id: {"mask_latent": [T,h,w], "soft": [T,h,w]}} (estimated, --auto-mask) or {unit id: {"mask": [T,H,W], "valid": [T,H,W]}}
    (tracked, --mask-key) of this rank's units (with several ranks each writes its own FILE.rankR.pt).  A shaped run (--mask-grow /
    --mask-feather) writes every unit's "shaped" and "support" [T,H,W] next to whatever its source returned."""
    records = {u: est for u, est in records.items() if est is not None and set(est) - {"keys", "confidence", "release", "gate"}}   # (a unit the mask file does not name has none)
    if any("shaped" in est for est in records.values()):   # --mask-grow / --mask-feather: what the source gave, and the two shaped masks
        keys = ("mask", "valid", "mask_latent", "soft", "shaped", "support")
    elif any("valid" in est for est in records.values()):
        keys = ("mask", "valid")
    else:
        keys = ("mask_latent", "soft")
    torch.save({int(u): {k: (est[k] if k == "valid" else est[k][0]).cpu() for k in keys if k in est or "shaped" not in keys}
                for u, est in sorted(records.items())}, _rank_path(path, rank, world))


def synthetic_mask(n, H, W):
    """[n,1,H,W]: 1 inside the centred rectangle of half the height and width, 0 outside (--synthetic-mask)."""
    m = torch.zeros((n, 1, H, W), dtype=torch.float32)
    m[:, :, H // 4:H - H // 4, W // 4:W - W // 4] = 1.0
    return m


def optical_flow_pipe_kwargs(args):
    """Constructor arguments of InferenceIP2PVideoOpticalFlow for the CLI's flow source (none when --flows supplies them)."""
    if not args.with_optical_flow or args.flows:
        return {}
    if args.raft_ckpt:
        return {"raft_state_dict": torch.load(args.raft_ckpt, map_location="cpu")}
    from . import synth, shapes
    return {"raft_state_dict": synth.synth_raft_state_dict(shapes.raft_shapes())}


def cli_options(args, device, data=None):
    """What the flags add to a run -> (per, more, want_masks, estimator): ``per`` = what every unit gets - ``per["all"]`` (--auto-mask,
    --stabilize, --key-stride) whatever its mask, ``per["masked"](has_mask)`` (--mask-key with a drawn mask, the shaping flags with a
    drawn or an estimated one) according to it; ``more`` = the keywords of the drivers (the flow estimator, when a feature follows the
    source's flows); ``want_masks`` = ``return_mask`` when something reads the units' masks, else nothing: a plain run carries no new
    keyword.  ``data``: the --units file, whose own "mask" entry --auto-mask refuses."""
    auto, track, shape = auto_mask_unit(args, data), mask_track_unit(args), mask_shape_unit(args)
    stab, keyf = stabilize_unit(args), keyframe_unit(args)
    estimator = build_flow_estimator(args, device)
    per = dict(all=dict(**auto, **stab, **keyf), masked=lambda has_mask: dict(**(track if has_mask else {}), **(shape if has_mask or auto else {})))
    more = {"flow_estimator": estimator} if track or stab or keyf else {}
    want_masks = {"return_mask": True} if ((auto or track or shape) and (getattr(args, "mask_out", None) or getattr(args, "score_pixels", False))) \
        or (keyf and getattr(args, "score_out", None)) else {}
    return per, more, want_masks, estimator


def run_dataset(args, model, pipe, rank=0, world=1, scorer=None):
    """The reference's main loop (insv2v_run_loveu_tgve.py:83-170): every (video, cfg, size) x 4 prompt kinds is one
    independent unit; units are dealt round-robin to ranks, each rank writes its own result files.  With ``--seed`` a unit's id is
    4 * (index of its (video, cfg, size) combination) + (index of its prompt kind): global, so it is the same on every rank and at every
    world size; the conditioning latent the four prompts share is sampled from the ENC stream of the first of them.
    ``scorer`` (build_scorer): every unit is scored after its edit, the video's original caption as text_0 and the edit prompt as text_1,
    and the records go to ``args.score_out``."""
    import json
    from .video_io import LoveuTgveVideoDataset, save_tensor_to_gif, save_tensor_to_images, output_paths
    if model.text_model is None or model.text_model.tokenizer is None:
        raise SystemExit("dataset mode needs the CLIP tokenizer: pass --tokenizer-dir DIR (vocab.json + merges.txt)")
    prompts = json.load(open(args.edit_prompt_file, "r"))
    combos = list(product(range(len(prompts)), args.text_cfg, args.video_cfg, args.num_frames, args.image_size))
    seed = getattr(args, "seed", None)
    kinds = ("style", "object", "background", "multiple")
    records = []
    drawn = load_mask_file(args)   # drawn masks are named by video here
    per, more, want_masks, estimator = cli_options(args, model.unet.device)
    masks = {}
    on_region = bool(region_unit(args))   # the frames and the mask image keep their native size; image_size is the working size
    for ci, (video_id, text_cfg, video_cfg, num_frames, image_size) in enumerate(combos):
        if ci % world != rank:
            continue
        batch = LoveuTgveVideoDataset(root_dir=args.data_dir, image_size=None if on_region else (image_size, image_size))[video_id]
        n = len(batch["frames"])
        skip = n // num_frames if n > num_frames else 1
        frames = batch["frames"][::skip].to(model.unet.device)[None]
        text_uncond = model.encode_text([""])
        if getattr(args, "mask_image", None):   # every video gets the image's mask, at this combination's frame size
            drawn = {batch["video_name"]: load_mask_image(args, *((None, None) if on_region else (image_size, image_size)))}
        # once per video, shared by the four prompts (:98); a region edit encodes its own working clip
        cond = None if on_region else model.encode_image_to_latent(frames, **_seeded(seed, 4 * ci)) / model.scale_factor
        smap = load_strength_map(args, image_size, image_size)
        todo = []
        for key in kinds:
            prompt = prompts[batch["video_name"]]["edit_" + key] if args.prompt_source == "edit" else batch[key]
            gif_path, image_dir = output_paths(args.prompt_source, image_size, video_id, video_cfg, text_cfg, num_frames,
                                               batch["video_name"], key, batch[key])
            if os.path.exists(gif_path):
                print(f"File {gif_path} exists, skip")
                continue
            todo.append((gif_path, image_dir, dict(frames=frames, text_cond=model.encode_text([prompt]), text_uncond=text_uncond,
                                                   text_cfg=text_cfg, video_cfg=video_cfg, unit=4 * ci + kinds.index(key),
                                                   **({"cond": cond} if cond is not None else {}), **region_unit(args, image_size),
                                                   strength=getattr(args, "strength", 1.0), **per["all"], **per["masked"](batch["video_name"] in drawn),
                                                   **strength_map_unit(args, batch["video_name"] in drawn, smap),
                                                   **(dict(mask=drawn[batch["video_name"]], mask_mode=getattr(args, "mask_mode", "max"))
                                                      if batch["video_name"] in drawn else {})), prompt))
        # the four prompts of a video share the conditioning latent and the window plan: one stacked launch chain per window (B = 12)
        run = edit_videos
        if on_region:
            from .region import edit_regions as run
        if getattr(args, "no_stack", False):
            edits = [run(model, pipe, [u], seed=seed, **want_masks, **more)[0] for _, _, u, _ in todo]
        else:
            edits = run(model, pipe, [u for _, _, u, _ in todo], seed=seed, max_clips=getattr(args, "max_stack", None), **want_masks, **more)
        for (gif_path, image_dir, u, prompt), edited in zip(todo, edits):
            if want_masks:
                edited, masks[u["unit"]] = edited
            records.append(unit_record(args, u["unit"], frames, edited, scorer, lambda: (batch["original"], prompt), region_est(args, masks.get(u["unit"])),
                                       u.get("mask"), estimator))
            save_tensor_to_gif(torch.cat([frames.float().cpu(), edited.float().cpu()], dim=4), gif_path, fps=5)
            save_tensor_to_images(edited.float().cpu(), image_dir)
    if scorer is not None or want_pixel_scores(args):
        write_scores(args.score_out, records, rank, world)
    if want_masks and getattr(args, "mask_out", None):
        write_masks(args.mask_out, masks, rank, world)


def _score_texts(data, i, scorer):
    """(source prompt, edit prompt) of unit i of a --units / --synthetic run: the ``source_ids`` / ``edit_ids`` [n,77] token ids of the
    file, else its ``source_text`` / ``edit_text`` strings (they need the tokenizer); synthetic runs hash their ids."""
    if "source_ids" in data and "edit_ids" in data:
        return data["source_ids"][i:i + 1], data["edit_ids"][i:i + 1]
    if "source_text" in data and "edit_text" in data:
        return data["source_text"][i], data["edit_text"][i]
    raise SystemExit("scoring --units needs source_ids / edit_ids (token ids [n,77]) or source_text / edit_text in the file")


def main(argv=None):
    import torch.distributed as dist
    from . import synth, shapes
    from .model import create_model
    from .inference import InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow
    from .clip_parallel import shard_units, gather_frames

    args = check_args(build_parser().parse_args(argv))
    tok = None
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        dist.init_process_group("nccl")
    if args.synthetic:
        ucfg, vcfg = (synth.UNET_TINY, synth.VAE_TINY) if args.synthetic_tiny else (synth.UNET_FULL, synth.VAE_FULL)
        conf = {"unet": {"params": ucfg}, "vae": {"params": vcfg}}
        model = create_model(conf, device=f"cuda:{local}")
        model.unet.load_state_dict(synth.synth_state_dict(shapes.unet_shapes(**ucfg)))
        model.vae.load_state_dict(synth.synth_state_dict(shapes.vae_shapes(**vcfg)))
    else:
        if args.tokenizer_dir:
            from transformers import CLIPTokenizer
            tok = CLIPTokenizer.from_pretrained(args.tokenizer_dir, local_files_only=True)
        model = create_model(args.config_path, device=f"cuda:{local}", tokenizer=tok)
        ckpt = torch.load(args.ckpt_path, map_location="cpu")
        model.load_state_dict(ckpt, strict=False)
    if args.synthetic:
        g = torch.Generator().manual_seed(0)
        T, S = args.num_frames[0], args.image_size[0]
        SW, SH = args.region_source or (S, S)   # (--region-source: the source's own size; --image-size is then the working size)
        data = {"frames": torch.rand((args.synthetic, T, 3, SH, SW), generator=g) * 2 - 1,
                "text_cond": torch.randn((args.synthetic, 77, ucfg["cross_attention_dim"]), generator=g),
                "text_uncond": torch.randn((1, 77, ucfg["cross_attention_dim"]), generator=g)}
        if args.synthetic_mask:
            data["mask"] = synthetic_mask(args.synthetic, SH, SW)
        if args.score_synthetic:   # no captions in a synthetic run: hashed token ids stand in for the source and the edit prompt
            vocab = (synth.CLIP_TINY if args.synthetic_tiny else synth.CLIP_FULL)["vocab_size"]
            data["source_ids"] = synth.synth_token_ids("score.source", args.synthetic, 77, vocab)
            data["edit_ids"] = synth.synth_token_ids("score.edit", args.synthetic, 77, vocab)
    elif args.units is None:
        cls = InferenceIP2PVideoOpticalFlow if args.with_optical_flow else InferenceIP2PVideo
        run_dataset(args, model, cls(unet=model.unet, num_ddim_steps=args.steps, scheduler=args.scheduler, solver_order=args.solver_order, **optical_flow_pipe_kwargs(args)), rank, world,
                    scorer=build_scorer(args, f"cuda:{local}", tok))
        if world > 1:
            dist.destroy_process_group()
        return
    else:
        data = torch.load(args.units, map_location="cpu")
    cls = InferenceIP2PVideoOpticalFlow if args.with_optical_flow else InferenceIP2PVideo
    pipe = cls(unet=model.unet, num_ddim_steps=args.steps, scheduler=args.scheduler, solver_order=args.solver_order, **optical_flow_pipe_kwargs(args))
    n = data["frames"].shape[0]
    flows = torch.load(args.flows, map_location="cpu") if args.flows else None
    item_shape = tuple(data["frames"].shape[1:])  # a rank without units still takes part in the all_gather
    drawn = load_mask_file(args)   # drawn masks are named by unit here
    image_mask = load_mask_image(args, data["frames"].shape[-1], data["frames"].shape[-2])   # every unit gets it
    if (drawn or image_mask is not None) and data.get("mask") is not None:
        raise SystemExit("--mask-file / --mask-image next to the \"mask\" entry of the --units file are two masks: pass one")
    if args.mask_key is not None and not drawn and image_mask is None and data.get("mask") is None:
        raise SystemExit("--mask-key needs a mask to track: --mask-file FILE.pt, the \"mask\" entry of a --units file, or --synthetic-mask")
    per, more, want_masks, estimator = cli_options(args, f"cuda:{local}", data)   # (refuses --auto-mask next to a "mask" entry of the file)
    est_masks = {}
    masks = data.get("mask")   # optional [n,T,H,W] / [n,1,H,W]
    smaps, smap_cli = data.get("strength_map"), load_strength_map(args, data["frames"].shape[-1], data["frames"].shape[-2])   # optional [n,T,H,W] / [n,1,H,W]
    if smaps is not None and (smap_cli is not None or args.strength_from_mask):
        raise SystemExit("--strength-map / --strength-from-mask next to the \"strength_map\" entry of the --units file are two strength maps: pass one")

    def edit(i):
        m = masks[i:i + 1] if masks is not None else drawn.get(i, image_mask)
        return dict(dict(mask=m, strength=args.strength, mask_mode=args.mask_mode), **per["all"], **per["masked"](m is not None),
                    **strength_map_unit(args, m is not None, smaps[i:i + 1] if smaps is not None else smap_cli))
    region = region_unit(args)   # with it the drivers are region.edit_region / edit_regions around the same calls
    scorer = build_scorer(args, f"cuda:{local}", tok)
    records = []
    outs = []
    for ci, (text_cfg, video_cfg) in enumerate(product(args.text_cfg, args.video_cfg)):
        mine = shard_units(n, rank, world)
        # --seed: units are numbered GLOBALLY (cfg combination ci, unit i of n -> ci * n + i) before they are dealt to the ranks, so a
        # unit keeps its noise streams on every rank, at every world size, stacked or not
        if args.no_stack and region:
            from .region import edit_region
            local_out = [edit_region(model, pipe, data["frames"][i:i + 1], data["text_cond"][i:i + 1], data["text_uncond"], text_cfg=text_cfg,
                                     video_cfg=video_cfg, flows_per_window=flows[i] if flows is not None else None,
                                     seed=args.seed, unit=ci * n + i, **region, **edit(i), **want_masks, **more) for i in mine]
        elif args.no_stack:
            local_out = [edit_video(model, pipe, data["frames"][i:i + 1], data["text_cond"][i:i + 1], data["text_uncond"],
                                    text_cfg, video_cfg, flows_per_window=flows[i] if flows is not None else None,
                                    seed=args.seed, unit=ci * n + i, **edit(i), **want_masks, **more) for i in mine]
        else:   # a rank's units as stacked launch chains (run_stacked caps the stack at what the kernels' operand window allows)
            from .inference import max_clips_in_flight
            T, S = data["frames"].shape[1], data["frames"].shape[-1]
            wh, ww = (region["region"]["size"][1], region["region"]["size"][0]) if region else (data["frames"].shape[-2], S)   # what runs through the UNet
            cap = args.max_stack or max_clips_in_flight(min(T, 16), wh // 8, ww // 8)
            run = edit_videos
            if region:
                from .region import edit_regions as run
            local_out = []
            for g in range(0, len(mine), cap):
                local_out += run(model, pipe, [dict(frames=data["frames"][i:i + 1], text_cond=data["text_cond"][i:i + 1],
                                                    text_uncond=data["text_uncond"], text_cfg=text_cfg, video_cfg=video_cfg, unit=ci * n + i, **edit(i), **region,
                                                    **({"flows_per_window": flows[i]} if flows is not None else {}))
                                               for i in mine[g:g + cap]], seed=args.seed, max_clips=args.max_stack, **want_masks, **more)
        if want_masks:
            for i, (_, est) in zip(mine, local_out):
                est_masks[ci * n + i] = est
            local_out = [img for img, _ in local_out]
        for i, edited in zip(mine, local_out if scorer is not None or want_pixel_scores(args) else []):
            records.append(unit_record(args, ci * n + i, data["frames"][i:i + 1], edited, scorer, lambda: _score_texts(data, i, scorer),
                                       region_est(args, est_masks.get(ci * n + i)), edit(i)["mask"], estimator))
        local_out = torch.cat(local_out, 0).half() if local_out else torch.zeros((0, *item_shape), device=model.unet.device).half()
        outs.append(gather_frames(local_out, n, item_shape=item_shape))
    if scorer is not None or want_pixel_scores(args):
        write_scores(args.score_out, records, rank, world)
    if want_masks and args.mask_out:
        write_masks(args.mask_out, est_masks, rank, world)
    if rank == 0:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        torch.save(torch.stack(outs, 0).cpu(), args.out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
