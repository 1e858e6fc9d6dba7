"""Stabilizing an edit along the SOURCE video's optical flow (csrc/temporal_filter.hip is the kernel,
tests/temporal_filter_ref.py the float64 definition).

The UNet denoises windows of 16 frames and the VAE decodes frame by frame: per-frame brightness wobble and a jump where one window hands
over to the next are the usual defects, and ``--score-warp`` (section 20) measures them.  This is the switch that reduces them - the
standard remedy of blind video temporal consistency (Bonneel et al. 2015; Lai et al. 2018): average the edit along the source video's
motion trajectories, each neighbour weighed by whether the trajectory is visible (the forward-backward rule of ``mask_track``) and by
whether the source itself looks the same at both of its ends.  The filter follows the source's motion, occlusions, lighting changes and
cuts, and never the edit's flicker.  A post-process on decoded frames: nothing of the denoising loop changes.

  neighbour_flows   the flows from every frame t to t + k, k in {-R..-1, 1..R}, and their validity: the adjacent-frame flows chained with
                    ``ops.mask_track_step``, one launch per distance
  temporal_filter   one launch of the filter kernel
  stabilize         both for one ``edit_video`` result

``sigma = 0.1`` is Lai et al.'s alpha = 50 (exp(-50 d2) = exp(-d2 / (2 * 0.1^2))); ``radius = 2`` and ``strength = 1`` are the other
defaults.  Starting values, NOT tuned here: there is no checkpoint and no footage to tune them on (as sections 18 and 19)."""
import math

import torch

from . import ops
from .mask_track import TRACK_DEFAULTS, pair_flows
from .pixel_score import AFFINE_SIGNED, check_affine

FILTER_DEFAULTS = dict(radius=2, sigma=0.1, strength=1.0, occlusion=True, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"])
MAX_RADIUS = 4


def _is_num(v):
    return not isinstance(v, bool) and isinstance(v, (int, float))


def check_filter_args(radius=2, sigma=0.1, strength=1.0, occlusion=True, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"]):
    """ValueError for parameters the filter cannot run with (nothing is launched)."""
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius must be an integer in 1 .. {MAX_RADIUS}, not {radius!r}")
    if not _is_num(sigma) or not math.isfinite(sigma) or sigma <= 0:
        raise ValueError(f"sigma must be a finite number > 0 (on [0, 1] data), not {sigma!r}")
    if not _is_num(strength) or not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must be in (0, 1], not {strength!r}")
    if not isinstance(occlusion, bool):
        raise ValueError(f"occlusion must be True or False, not {occlusion!r}")
    for name, v in (("alpha", alpha), ("beta", beta)):
        if not _is_num(v) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, not {v!r}")


def neighbour_offsets(radius, fwd=True, bwd=True):
    """The neighbour offsets in the filter's order: -R .. -1 (they need ``bwd``), then 1 .. R (they need ``fwd``)."""
    return tuple(range(-radius, 0)) * bool(bwd) + tuple(range(1, radius + 1)) * bool(fwd)


def filter_plan(T, radius):
    """The launches that chain the adjacent-frame flows of a video of T frames into the flows of ``neighbour_flows``: a list of steps, step
    j - 1 holding the chains of distance j, each (offset k, frame t, the frame t' whose distance-(j-1) flow it extends, index and set of b,
    index and set of c).  ``F_{t -> t+j} = fwd[t] + S(F_{t+1 -> t+j})`` for every t < T - j and the mirror with ``bwd``: up to 2 (T - j)
    chains in ONE launch, min(radius, T - 1) launches in all."""
    steps = []
    for j in range(1, min(radius, T - 1) + 1):
        step = [(j, t, t + 1, ("fwd", t), ("bwd", t)) for t in range(T - j)]
        step += [(-j, t, t - 1, ("bwd", t - 1), ("fwd", t - 1)) for t in range(j, T)]
        steps.append(step)
    return steps


def _check_flow_sets(fwd, bwd, fn):
    sets = {"fwd": fwd, "bwd": bwd}
    given = [f for f in sets.values() if f is not None]
    if not given:
        raise ValueError(f"{fn}: no flows (fwd= and bwd= are both None)")
    for name, f in sets.items():
        if f is not None and (not torch.is_tensor(f) or f.dim() != 4 or f.shape[1] != 2 or not f.is_floating_point()):
            raise ValueError(f"{fn}: {name} {tuple(getattr(f, 'shape', ()))} must be a floating-point [T-1,2,H,W]")
    if len({tuple(f.shape) for f in given}) > 1:
        raise ValueError(f"{fn}: fwd and bwd differ in shape")
    P, _, H, W = given[0].shape
    if H <= 1 or W <= 1:
        raise ValueError(f"{fn}: frames of {H}x{W} cannot be sampled bilinearly")
    return P + 1, H, W


@torch.no_grad()
def neighbour_flows(fwd, bwd=None, *, radius=2, occlusion=True, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"]):
    """The adjacent-frame flows ``fwd`` / ``bwd`` [T-1,2,H,W] (``mask_track.pair_flows``) -> dict(``flow`` [K,T,2,H,W], ``valid``
    [K,T,H,W] of 0 / 1, ``offsets``): ``flow[i, t]`` is defined on frame t and points into frame t + offsets[i], ``valid[i, t]`` says
    where that trajectory stays in the frame, passes the forward-backward check at every link (``occlusion``; ``alpha``, ``beta`` as for
    ``propagate_mask``) and lands on a valid pixel of the chain so far - bit for bit ``propagate_mask(key=t + k)``'s ``flow_to_key[t]``
    and ``valid[t]``, computed with the same step kernel (its mask output is ignored) in ``filter_plan``'s launches.  Entries whose
    neighbour lies outside the video are 0 / invalid.  ``occlusion=True`` needs both flow sets; without it a missing set drops the
    offsets of its sign.  Everything is checked before the first launch."""
    check_filter_args(radius=radius, occlusion=occlusion, alpha=alpha, beta=beta)
    T, H, W = _check_flow_sets(fwd, bwd, "neighbour_flows")
    if occlusion and (fwd is None or bwd is None):
        raise ValueError("neighbour_flows: occlusion=True checks forward against backward flow and needs both fwd= and bwd= (or pass occlusion=False)")
    dev = (fwd if fwd is not None else bwd).device
    sets = {k: (None if f is None else f.to(device=dev, dtype=torch.float32)) for k, f in (("fwd", fwd), ("bwd", bwd))}
    offsets = neighbour_offsets(radius, fwd is not None, bwd is not None)
    flow = torch.zeros((len(offsets), T, 2, H, W), device=dev, dtype=torch.float32)
    valid = torch.zeros((len(offsets), T, H, W), device=dev, dtype=torch.float32)
    index = lambda rows: torch.tensor(rows, dtype=torch.long, device=dev)   # noqa: E731
    # per sign, the flows of the previous distance [T,2,H,W] and their validity [T,H,W]: the identity for distance 0, then the slot of
    # ``flow`` / ``valid`` the last step filled (the rows of frames without that neighbour are never read)
    prev = {s: (torch.zeros((T, 2, H, W), device=dev), torch.ones((T, H, W), device=dev)) for s in (1, -1)}
    for j, step in enumerate(filter_plan(T, radius), 1):
        chains = {s: [c for c in step if c[0] == s * j and c[0] in offsets] for s in (1, -1)}   # (a missing flow set drops its sign)
        step = chains[1] + chains[-1]
        f_prev = torch.cat([prev[s][0].index_select(0, index([c[2] for c in chains[s]])) for s in (1, -1)])
        v_prev = torch.cat([prev[s][1].index_select(0, index([c[2] for c in chains[s]])) for s in (1, -1)])
        b = torch.stack([sets[name][i] for _, _, _, (name, i), _ in step])
        c = torch.stack([sets[name][i] for _, _, _, _, (name, i) in step]) if occlusion else None
        F, V, _ = ops.mask_track_step(f_prev, v_prev, b, c, torch.zeros_like(v_prev), alpha=alpha, beta=beta, fill=0.0)
        n = 0
        for s in (1, -1):
            if chains[s]:
                slot, frames, m = offsets.index(s * j), index([c[1] for c in chains[s]]), len(chains[s])
                flow[slot].index_copy_(0, frames, F[n:n + m])
                valid[slot].index_copy_(0, frames, V[n:n + m])
                prev[s], n = (flow[slot], valid[slot]), n + m
    return dict(flow=flow, valid=valid, offsets=offsets)


def _check_frames(name, f, fn):
    if not torch.is_tensor(f) or f.dim() != 4 or f.shape[1] != 3 or f.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"{fn}: {name} must be a float16 / float32 [T,3,H,W] tensor, not {tuple(getattr(f, 'shape', ()))} {getattr(f, 'dtype', type(f).__name__)}")
    return tuple(f.shape)


def check_temporal_filter_args(edited, guide, flow, valid, offsets, sigma=0.1, strength=1.0, guide_affine=(1.0, 0.0)):
    """ValueError for arguments ``temporal_filter`` cannot run with (nothing is launched)."""
    shape = _check_frames("edited", edited, "temporal_filter")
    if _check_frames("guide", guide, "temporal_filter") != shape:
        raise ValueError(f"temporal_filter: edited {shape} and guide {tuple(guide.shape)} differ")
    T, _, H, W = shape
    if T < 1 or H <= 1 or W <= 1:
        raise ValueError(f"temporal_filter: {T} frame(s) of {H}x{W} cannot be filtered")
    if not isinstance(offsets, (tuple, list)) or not 1 <= len(offsets) <= 2 * MAX_RADIUS \
            or not all(isinstance(k, int) and not isinstance(k, bool) and k != 0 and abs(k) <= MAX_RADIUS for k in offsets):
        raise ValueError(f"temporal_filter: offsets must be 1 .. {2 * MAX_RADIUS} non-zero integers within +-{MAX_RADIUS}, not {offsets!r}")
    K = len(offsets)
    for name, t, want in (("flow", flow, (K, T, 2, H, W)), ("valid", valid, (K, T, H, W))):
        if not torch.is_tensor(t) or not t.is_floating_point() or tuple(t.shape) != want:
            raise ValueError(f"temporal_filter: {name} {tuple(getattr(t, 'shape', ()))} must be a floating-point {list(want)}")
    check_filter_args(sigma=sigma, strength=strength)
    check_affine(guide_affine, "temporal_filter")


@torch.no_grad()
def temporal_filter(edited, guide, flow, valid, offsets, *, sigma=0.1, strength=1.0, guide_affine=(1.0, 0.0)):
    """``edited`` [T,3,H,W] filtered along ``flow`` [K,T,2,H,W] / ``valid`` [K,T,H,W] (``neighbour_flows``) with the photometric weight
    taken on ``guide`` [T,3,H,W], read as ``clamp(x * scale + shift, 0, 1)`` (``guide_affine``; ``AFFINE_SIGNED`` for frames in
    [-1, 1]) -> [T,3,H,W] in ``edited``'s dtype, a new tensor.  One launch."""
    check_temporal_filter_args(edited, guide, flow, valid, offsets, sigma, strength, guide_affine)
    dev = edited.device
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()   # noqa: E731
    return ops.temporal_filter(edited, guide.to(dev), f32(flow), f32(valid), tuple(offsets), sigma=float(sigma), strength=float(strength),
                               guide_affine=tuple(float(v) for v in guide_affine))


def check_stabilize_args(source_frames, edited_frames, flows=None, flow_estimator=None, mask=None, radius=2, sigma=0.1, strength=1.0,
                         occlusion=True, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"]):
    """ValueError for arguments ``stabilize`` cannot run with (nothing is launched, no flow is computed)."""
    for name, f in (("source_frames", source_frames), ("edited_frames", edited_frames)):
        if not torch.is_tensor(f) or f.dim() != 5 or f.shape[0] != 1 or f.shape[2] != 3 or f.dtype not in (torch.float16, torch.float32):
            raise ValueError(f"stabilize: {name} must be a float16 / float32 [1,T,3,H,W] tensor in [-1, 1], not {tuple(getattr(f, 'shape', ()))}")
    if source_frames.shape != edited_frames.shape:
        raise ValueError(f"stabilize: source {tuple(source_frames.shape)} and edit {tuple(edited_frames.shape)} differ")
    _, T, _, H, W = source_frames.shape
    if T < 1 or H <= 1 or W <= 1:
        raise ValueError(f"stabilize: {T} frame(s) of {H}x{W} cannot be filtered")
    try:
        check_filter_args(radius, sigma, strength, occlusion, alpha, beta)
    except ValueError as e:
        raise ValueError(f"stabilize: {e}") from None
    if flows is not None and flow_estimator is not None:
        raise ValueError("stabilize: flows= and flow_estimator= are two flow sources: pass one")
    if T > 1 and flows is None and flow_estimator is None:
        raise ValueError("stabilize: no flow source: pass flows=dict(fwd=, bwd=) or flow_estimator= (always the SOURCE video's flows)")
    if flows is not None and T > 1:
        if not isinstance(flows, dict) or set(flows) - {"fwd", "bwd"} or flows.get("fwd") is None or (occlusion and flows.get("bwd") is None):
            raise ValueError("stabilize: flows must be dict(fwd=, bwd=) as mask_track.pair_flows returns it (bwd may be missing with occlusion=False)")
        for k in ("fwd", "bwd"):
            f = flows.get(k)
            if f is not None and (not torch.is_tensor(f) or not f.is_floating_point() or tuple(f.shape) != (T - 1, 2, H, W)):
                raise ValueError(f"stabilize: flows[{k!r}] {tuple(getattr(f, 'shape', ()))} must be a floating-point [{T - 1},2,{H},{W}]")
    if flow_estimator is not None and not callable(flow_estimator):
        raise ValueError("stabilize: flow_estimator must be callable: estimator(img1, img2) -> [n,2,H,W]")
    if mask is not None:
        if not torch.is_tensor(mask) or not mask.is_floating_point() or mask.dim() != 4 or mask.shape[0] != 1 \
                or mask.shape[1] not in (1, T) or tuple(mask.shape[2:]) != (H, W):
            raise ValueError(f"stabilize: mask must be a floating-point [1,1,{H},{W}] or [1,{T},{H},{W}] tensor with values in [0, 1]")


@torch.no_grad()
def stabilize(source_frames, edited_frames, *, flows=None, flow_estimator=None, mask=None, radius=2, sigma=0.1, strength=1.0, occlusion=True,
              alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"]):
    """One ``edit_video`` result, stabilized: ``source_frames`` / ``edited_frames`` [1,T,3,H,W] in [-1, 1] -> [1,T,3,H,W] in the edit's
    dtype.  The flows are ALWAYS the source video's - ``flows=dict(fwd, bwd)`` or ``flow_estimator`` (then
    ``mask_track.pair_flows(source_frames, estimator)``) - and the photometric weight is taken on the source (``AFFINE_SIGNED``).  With
    ``mask`` ([1,1,H,W] or [1,T,H,W], the region of a localized edit) the result is composited against the source exactly as the masked
    path of ``edit_video`` composites its own: outside a hard mask the pixels stay the input's, bit for bit; without one it is clipped to
    [-1, 1] like every result of ``edit_video``.  T = 1 returns the edit and
    launches nothing.  ``radius``, ``sigma``, ``strength``: untuned starting values (module docstring)."""
    check_stabilize_args(source_frames, edited_frames, flows, flow_estimator, mask, radius, sigma, strength, occlusion, alpha, beta)
    _, T, _, H, W = source_frames.shape
    if T == 1:
        return edited_frames
    dev = edited_frames.device
    src, edt = source_frames[0].to(dev), edited_frames[0]
    if flows is None:
        flows = pair_flows(source_frames.to(dev), flow_estimator, both=True)
    on = lambda f: None if f is None else f.to(dev)   # noqa: E731
    nb = neighbour_flows(on(flows.get("fwd")), on(flows.get("bwd")), radius=radius, occlusion=occlusion, alpha=alpha, beta=beta)
    out = temporal_filter(edt, src, nb["flow"], nb["valid"], nb["offsets"], sigma=sigma, strength=strength, guide_affine=AFFINE_SIGNED)
    if mask is None:
        return out.clip_(-1, 1)[None]   # (a convex combination of values in [-1, 1]: only a rounding could leave the range)
    region = mask[0].to(device=dev, dtype=torch.float32).expand(T, H, W).contiguous()
    img = out.to(torch.float32).contiguous()
    return ops.composite(img, src.to(torch.float32).contiguous(), region, out=img).to(edt.dtype)[None]
