"""A mask drawn on ONE frame follows the motion: adjacent-frame optical flows are chained into the flow from every frame to the key
frame, and the key mask is sampled once per frame (csrc/masktrack.hip is the step kernel, tests/masktrack_ref.py
the float64 definition).

  pair_flows       the 2 (T - 1) adjacent-frame flows of a video, from any ``flow_estimator(img1, img2) -> [n,2,H,W]`` (RAFTFlow)
  propagate_mask   the chain: at most T - 1 launches of ``ops.mask_track_step``, the frames after and before the key in one launch

Flow convention: that of the estimator and of ``ops.warp_image`` - ``estimator(frame_a, frame_b)`` is defined on frame a and points into
frame b, so sampling b at ``x + flow(x)`` gives a.  ``fwd[t] = estimator(frame_t, frame_{t+1})``, ``bwd[t] = estimator(frame_{t+1}, frame_t)``.

Limits.  A pixel that cannot be traced back to the key frame - it leaves the frame, fails the forward-backward consistency check or
lands on an invalid pixel of the chain's previous frame - is invalid and takes ``fill`` (default 0: do not edit it), and it stays invalid
down the chain: an object that disappears and comes back is NOT picked up again.  One key frame per call.  ``alpha = 0.01`` and
``beta = 0.5`` are the usual forward-backward consistency constants (UnFlow, Meister et al. 2018): starting values, not tuned here."""
import math

import torch

from . import ops

TRACK_DEFAULTS = dict(occlusion=True, alpha=0.01, beta=0.5, fill=0.0)


def check_track_args(occlusion=True, alpha=0.01, beta=0.5, fill=0.0):
    """ValueError for parameters ``propagate_mask`` cannot run with (nothing is launched)."""
    if not isinstance(occlusion, bool):
        raise ValueError(f"occlusion must be True or False, not {occlusion!r}")
    for name, v in (("alpha", alpha), ("beta", beta)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, not {v!r}")
    if isinstance(fill, bool) or not isinstance(fill, (int, float)) or not 0.0 <= fill <= 1.0:
        raise ValueError(f"fill must be a mask value in [0, 1], not {fill!r}")


def needed_pairs(T, key=None):
    """(fwd indices, bwd indices) the chain from ``key`` reads without the consistency check: ``fwd[t]`` for the frames before the key,
    ``bwd[t]`` for those after it; ``key=None``: all of both."""
    if key is None:
        return list(range(T - 1)), list(range(T - 1))
    return list(range(0, key)), list(range(key, T - 1))


@torch.no_grad()
def pair_flows(frames, flow_estimator, *, both=True, key=None):
    """frames [1,T,3,H,W] -> dict(fwd, bwd), each [T-1,2,H,W] fp32: ``fwd[t] = estimator(frame_t, frame_{t+1})`` and ``bwd[t] =
    estimator(frame_{t+1}, frame_t)``.  ``both=False`` (with ``key``) computes only the pairs the chain from ``key`` needs without the
    consistency check (``needed_pairs``); the others stay zero.  The pairs go to the estimator in chunks of its ``max_pairs`` (1 if it
    advertises none), and the frames as they are: the value range ``edit_video`` hands the estimator for the noise correction."""
    if not torch.is_tensor(frames) or frames.dim() != 5 or frames.shape[0] != 1 or frames.shape[2] != 3:
        raise ValueError(f"pair_flows: frames must be [1,T,3,H,W], not {tuple(getattr(frames, 'shape', ()))}")
    if not both and key is None:
        raise ValueError("pair_flows: both=False needs key=, the frame the chain starts from")
    T, H, W = frames.shape[1], frames.shape[3], frames.shape[4]
    if key is not None and not 0 <= key < T:
        raise ValueError(f"pair_flows: key {key} is not a frame of a video of {T}")
    fi, bi = needed_pairs(T, None if both else key)
    pairs = [(t, t + 1) for t in fi] + [(t + 1, t) for t in bi]
    per = max(1, int(getattr(flow_estimator, "max_pairs", 0) or 1))
    video = frames[0]
    got = []
    for i in range(0, len(pairs), per):
        a, b = (torch.tensor(ix, dtype=torch.long, device=video.device) for ix in zip(*pairs[i:i + per]))
        got.append(flow_estimator(video.index_select(0, a), video.index_select(0, b)).to(torch.float32))
    dev = got[0].device if got else video.device
    out = {k: torch.zeros((T - 1, 2, H, W), device=dev, dtype=torch.float32) for k in ("fwd", "bwd")}
    if got:
        flows = torch.cat(got, 0)
        if tuple(flows.shape) != (len(pairs), 2, H, W):
            raise ValueError(f"pair_flows: the estimator returned {tuple(flows.shape)} for {len(pairs)} pairs of {H}x{W} frames")
        if fi:
            out["fwd"][fi] = flows[:len(fi)]
        if bi:
            out["bwd"][bi] = flows[len(fi):]
    return out


def track_plan(T, key):
    """The launches of the chain from ``key``: a list of steps, each a list of (frame t, previous frame t', index and set of b, index and
    set of c) - the frame after and the frame before the key share a step while both chains are alive.  max(key, T - 1 - key) steps."""
    steps = []
    for j in range(1, max(key, T - 1 - key) + 1):
        step = []
        if key + j <= T - 1:   # after the key: t' = t - 1, b = estimator(frame_t, frame_{t-1}) = bwd[t-1]
            step.append((key + j, key + j - 1, ("bwd", key + j - 1), ("fwd", key + j - 1)))
        if key - j >= 0:       # before the key: t' = t + 1, b = estimator(frame_t, frame_{t+1}) = fwd[t]
            step.append((key - j, key - j + 1, ("fwd", key - j), ("bwd", key - j)))
        steps.append(step)
    return steps


@torch.no_grad()
def propagate_mask(key_mask, key, fwd, bwd=None, *, occlusion=True, alpha=0.01, beta=0.5, fill=0.0):
    """The key frame's mask ``key_mask`` ([H,W] or [1,1,H,W], values in [0,1]) on frame ``key`` of a video whose adjacent-frame flows are
    ``fwd`` / ``bwd`` [T-1,2,H,W] (``pair_flows``) -> dict(``mask`` [1,T,H,W], ``valid`` [T,H,W] of 0 / 1, ``flow_to_key`` [T,2,H,W]).
    ``occlusion=True`` adds the forward-backward consistency check (``alpha``, ``beta``: untuned starting values, see the module
    docstring) and needs both flow sets; without it only the flows of ``needed_pairs(T, key)`` are read (``bwd`` may be None when the
    key is the last frame, ``fwd`` when it is the first).  Invalid pixels take ``fill`` and stay invalid down the chain.  At most T - 1
    launches; T = 1 launches nothing.  Everything is checked before the first launch."""
    check_track_args(occlusion, alpha, beta, fill)
    if not torch.is_tensor(key_mask) or not key_mask.is_floating_point():
        raise ValueError("propagate_mask: key_mask must be a floating-point tensor with values in [0, 1]")
    if key_mask.dim() == 4 and tuple(key_mask.shape[:2]) == (1, 1):
        key_mask = key_mask[0, 0]
    if key_mask.dim() != 2:
        raise ValueError(f"propagate_mask: key_mask {tuple(key_mask.shape)} must be [H,W] or [1,1,H,W]")
    H, W = key_mask.shape
    if H <= 1 or W <= 1:
        raise ValueError(f"propagate_mask: frames of {H}x{W} cannot be sampled bilinearly")
    sets = {"fwd": fwd, "bwd": bwd}
    given = [f for f in sets.values() if f is not None]
    for name, f in sets.items():
        if f is not None and (not torch.is_tensor(f) or f.dim() != 4 or tuple(f.shape[1:]) != (2, H, W) or not f.is_floating_point()):
            raise ValueError(f"propagate_mask: {name} {tuple(getattr(f, 'shape', ()))} must be a floating-point [T-1,2,{H},{W}]")
    if not given:
        raise ValueError("propagate_mask: no flows (fwd= and bwd= are both None)")
    if len({f.shape[0] for f in given}) > 1:
        raise ValueError("propagate_mask: fwd and bwd hold different numbers of frame pairs")
    T = given[0].shape[0] + 1
    if isinstance(key, bool) or not isinstance(key, int) or not 0 <= key < T:
        raise ValueError(f"propagate_mask: key {key!r} is not a frame index of a video of {T} frames")
    if occlusion and (fwd is None or bwd is None):
        raise ValueError("propagate_mask: occlusion=True checks forward against backward flow and needs both fwd= and bwd= (or pass occlusion=False)")
    plan = track_plan(T, key)
    for step in plan:
        for _, _, (bset, _), _ in step:
            if sets[bset] is None:
                raise ValueError(f"propagate_mask: the chain from key {key} of {T} frames needs {bset}=")
    dev = given[0].device
    sets = {k: (None if f is None else f.to(device=dev, dtype=torch.float32)) for k, f in sets.items()}
    M = key_mask.to(device=dev, dtype=torch.float32).contiguous()
    mask = torch.empty((1, T, H, W), device=dev, dtype=torch.float32)
    valid = torch.ones((T, H, W), device=dev, dtype=torch.float32)
    flow = torch.zeros((T, 2, H, W), device=dev, dtype=torch.float32)
    mask[0, key] = M
    Ms = {n: M.expand(n, H, W).contiguous() for n in {len(step) for step in plan}}
    for step in plan:
        n = len(step)
        f_prev = torch.stack([flow[tp] for _, tp, _, _ in step])
        v_prev = torch.stack([valid[tp] for _, tp, _, _ in step])
        b = torch.stack([sets[s][i] for _, _, (s, i), _ in step])
        c = torch.stack([sets[s][i] for _, _, _, (s, i) in step]) if occlusion else None
        F, V, m = ops.mask_track_step(f_prev, v_prev, b, c, Ms[n], alpha=alpha, beta=beta, fill=fill)
        for j, (t, _, _, _) in enumerate(step):
            flow[t], valid[t], mask[0, t] = F[j], V[j], m[j]
    return dict(mask=mask, valid=valid, flow_to_key=flow)
