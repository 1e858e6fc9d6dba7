"""Editing key frames only and filling the rest along the SOURCE video's optical flow (csrc/keyfill.hip is the
kernel, tests/keyfill_ref.py the float64 definition).

Every frame ``edit_video`` returns is a denoised frame.  The standard remedy for its cost is to denoise every N-th frame and carry the
edit to the frames in between along the source video's motion: each in-between frame takes, from its previous and its next key frame,
what the edit CHANGED there (``mode="residual"``, the default: ``E_key - A_key`` sampled along the flow and added to the frame's own
source pixels) or the edited pixels themselves (``mode="warp"``), each side weighed by its distance in time, by whether the trajectory
is visible (the forward-backward rule of ``mask_track``) and by whether the source looks the same at both of its ends (the photometric
weight of ``temporal_filter``).  A post-process on decoded frames: nothing of the denoising loop changes.

  key_frames     the key frames of a video of T frames at a stride: 0, stride, 2 stride, ... and always T - 1
  fill_plan      the launches that chain the adjacent-frame flows into the flows from every in-between frame to its two keys
  key_flows      those flows and their validity: ``ops.mask_track_step``, ONE launch per distance for all segments and both sides
  keyframe_fill  ``key_flows`` and one call of the fill kernel for one video

``residual`` is the default because it keeps the source's own change between the key and frame t - lighting, deformation, detail the
flow misses - and because a zero residual (outside a hard mask, or wherever the edit changed nothing) carries over as exact zeros: the
in-between pixel is then the source's, bit for bit.  ``stride = 4``, ``sigma = 0.1`` (the filter's) and the track defaults for
``alpha`` / ``beta`` are starting values, NOT tuned here: there is no checkpoint and no footage to tune them on (as sections 18 - 22)."""
import math

import torch

from . import ops
from .mask_track import TRACK_DEFAULTS, pair_flows
from .pixel_score import AFFINE_SIGNED

MIN_STRIDE, MAX_STRIDE = 2, 8
FILL_MODES = ("residual", "warp")
FILL_DEFAULTS = dict(stride=4, mode="residual", sigma=0.1, occlusion=True, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"])


def _is_num(v):
    return not isinstance(v, bool) and isinstance(v, (int, float))


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, int)


def check_fill_args(stride=FILL_DEFAULTS["stride"], mode="residual", sigma=0.1, occlusion=True, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"]):
    """ValueError for parameters the fill cannot run with (nothing is launched)."""
    if not _is_int(stride) or not MIN_STRIDE <= stride <= MAX_STRIDE:
        raise ValueError(f"stride must be an integer in {MIN_STRIDE} .. {MAX_STRIDE}, not {stride!r}")
    if mode not in FILL_MODES:
        raise ValueError(f"mode must be 'residual' or 'warp', not {mode!r}")
    if not _is_num(sigma) or not math.isfinite(sigma) or sigma <= 0:
        raise ValueError(f"sigma must be a finite number > 0 (on [0, 1] data), not {sigma!r}")
    if not isinstance(occlusion, bool):
        raise ValueError(f"occlusion must be True or False, not {occlusion!r}")
    for name, v in (("alpha", alpha), ("beta", beta)):
        if not _is_num(v) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, not {v!r}")


def key_frames(T, stride):
    """The key frames of a video of T frames: 0, stride, 2 stride, ... and always T - 1, so every other frame lies between two keys."""
    if not _is_int(T) or T < 1:
        raise ValueError(f"key_frames: T must be a positive integer, not {T!r}")
    if not _is_int(stride) or stride < 1:
        raise ValueError(f"key_frames: stride must be a positive integer, not {stride!r}")
    keys = list(range(0, T, stride))
    if keys[-1] != T - 1:
        keys.append(T - 1)
    return keys


def check_keys(T, keys, fn="keyfill"):
    """ValueError unless ``keys`` is a non-empty, strictly increasing list of frame indices of a video of T frames."""
    if not isinstance(keys, (list, tuple)) or not keys or not all(_is_int(k) for k in keys):
        raise ValueError(f"{fn}: keys must be a non-empty list of frame indices, not {keys!r}")
    if any(not 0 <= k < T for k in keys) or any(b <= a for a, b in zip(keys, keys[1:])):
        raise ValueError(f"{fn}: keys {list(keys)} must be strictly increasing frame indices of a video of {T} frames")
    return list(keys)


def fill_sides(T, keys):
    """Per in-between frame t in increasing order: (t, (slot_0, slot_1), (tw_0, tw_1)) - the slots in ``keys`` of the previous and the
    next key (-1: there is none) and the temporal weights ``tw_0 = (b - t) / (b - a)``, ``tw_1 = (t - a) / (b - a)``; a frame before the
    first or after the last key has one side, with weight 1."""
    keys = check_keys(T, keys, "fill_sides")
    out = []
    for t in range(T):
        if t in keys:
            continue
        nxt = next((j for j, k in enumerate(keys) if k > t), None)
        prv = (len(keys) if nxt is None else nxt) - 1
        if prv < 0:
            out.append((t, (-1, nxt), (0.0, 1.0)))
        elif nxt is None:
            out.append((t, (prv, -1), (1.0, 0.0)))
        else:
            a, b = keys[prv], keys[nxt]
            out.append((t, (prv, nxt), ((b - t) / (b - a), (t - a) / (b - a))))
    return out


def fill_plan(T, keys):
    """The launches that chain the adjacent-frame flows of a video of T frames into the flows from every in-between frame to its keys: a
    list of steps, step j - 1 holding the chains of distance j, each (side, frame t, the frame t' whose distance-(j-1) flow it extends,
    index and set of b, index and set of c).  For every key a and the frames after it up to the next key,
    ``F_{t -> a} = bwd[t-1] + S(F_{t-1 -> a})``, t = a + j (side 0); for every key b and the frames before it down to the previous key,
    ``F_{t -> b} = fwd[t] + S(F_{t+1 -> b})``, t = b - j (side 1).  ALL segments and both sides of a distance share ONE launch:
    (the longest run of in-between frames) launches in all, ``max gap - 1`` for keys that start at 0 and end at T - 1."""
    keys = check_keys(T, keys, "fill_plan")
    after = [(a, (keys[i + 1] if i + 1 < len(keys) else T) - a - 1) for i, a in enumerate(keys)]    # (key, frames that follow it)
    before = [(b, b - (keys[i - 1] if i > 0 else -1) - 1) for i, b in enumerate(keys)]              # (key, frames that precede it)
    steps = []
    for j in range(1, max(m for _, m in after + before) + 1):
        step = [(0, a + j, a + j - 1, ("bwd", a + j - 1), ("fwd", a + j - 1)) for a, m in after if j <= m]
        step += [(1, b - j, b - j + 1, ("fwd", b - j), ("bwd", b - j)) for b, m in before if j <= m]
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
def key_flows(fwd, bwd, keys, *, occlusion=True, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"]):
    """The adjacent-frame flows ``fwd`` / ``bwd`` [T-1,2,H,W] (``mask_track.pair_flows``) and the key frames ``keys`` -> dict(``flow``
    [n,2,2,H,W], ``valid`` [n,2,H,W] of 0 / 1, ``frames``, ``slots``, ``weights``): entry i is the in-between frame ``frames[i]``;
    ``flow[i, s]`` is defined on it and points into key ``keys[slots[i][s]]`` (s = 0: the previous key, s = 1: the next; slot -1: no such
    side, flow 0 and all invalid), ``valid[i, s]`` says where that trajectory stays in the frame, passes the forward-backward check at
    every link (``occlusion``; ``alpha``, ``beta`` as for ``propagate_mask``) and lands on a valid pixel of the chain so far - bit for bit
    ``propagate_mask(key=keys[slot])``'s ``flow_to_key[t]`` and ``valid[t]``, computed with the same step kernel (its mask output is
    ignored) in ``fill_plan``'s launches.  ``weights[i]`` = (tw_0, tw_1) of ``fill_sides``.  Everything is checked before the first
    launch."""
    check_fill_args(occlusion=occlusion, alpha=alpha, beta=beta)
    T, H, W = _check_flow_sets(fwd, bwd, "key_flows")
    keys = check_keys(T, keys, "key_flows")
    plan = fill_plan(T, keys)
    need = {name for step in plan for _, _, _, (name, _), _ in step} | ({"fwd", "bwd"} if occlusion and plan else set())
    for name in sorted(need):
        if {"fwd": fwd, "bwd": bwd}[name] is None:
            raise ValueError(f"key_flows: these key frames need {name}= ({'the occlusion check needs both sets; ' if occlusion else ''}side 0 chains bwd, side 1 fwd)")
    dev = (fwd if fwd is not None else bwd).device
    sets = {k: (None if f is None else f.to(device=dev, dtype=torch.float32)) for k, f in (("fwd", fwd), ("bwd", bwd))}
    index = lambda rows: torch.tensor(rows, dtype=torch.long, device=dev)   # noqa: E731
    # per side, the flow of every frame to its key of that side [T,2,H,W] and its validity [T,H,W]: the identity on the keys (distance
    # 0), then the rows each step fills
    F = [torch.zeros((T, 2, H, W), device=dev) for _ in range(2)]
    V = [torch.ones((T, H, W), device=dev) for _ in range(2)]
    for step in plan:
        chains = [[c for c in step if c[0] == s] for s in (0, 1)]
        step = chains[0] + chains[1]
        f_prev = torch.cat([F[s].index_select(0, index([c[2] for c in chains[s]])) for s in (0, 1)])
        v_prev = torch.cat([V[s].index_select(0, index([c[2] for c in chains[s]])) for s in (0, 1)])
        b = torch.stack([sets[name][i] for _, _, _, (name, i), _ in step])
        c = torch.stack([sets[name][i] for _, _, _, _, (name, i) in step]) if occlusion else None
        Fo, Vo, _ = ops.mask_track_step(f_prev, v_prev, b, c, torch.zeros_like(v_prev), alpha=alpha, beta=beta, fill=0.0)
        n = 0
        for s in (0, 1):
            if chains[s]:
                rows, m = index([c[1] for c in chains[s]]), len(chains[s])
                F[s].index_copy_(0, rows, Fo[n:n + m])
                V[s].index_copy_(0, rows, Vo[n:n + m])
                n += m
    sides = fill_sides(T, keys)
    frames = [t for t, _, _ in sides]
    rows = index(frames)
    flow = torch.stack([F[s].index_select(0, rows) for s in (0, 1)], dim=1)
    valid = torch.stack([V[s].index_select(0, rows) for s in (0, 1)], dim=1)
    for i, (_, slots, _) in enumerate(sides):   # a side that does not exist: flow 0, all invalid
        for s in (0, 1):
            if slots[s] < 0:
                flow[i, s].zero_()
                valid[i, s].zero_()
    return dict(flow=flow.contiguous(), valid=valid.contiguous(), frames=frames, slots=[s for _, s, _ in sides], weights=[w for _, _, w in sides])


def check_keyframe_fill_args(source_frames, edited_keys, keys, flows=None, flow_estimator=None, mode="residual", sigma=0.1, occlusion=True,
                             alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"]):
    """ValueError for arguments ``keyframe_fill`` cannot run with (nothing is launched, no flow is computed)."""
    for name, f in (("source_frames", source_frames), ("edited_keys", edited_keys)):
        if not torch.is_tensor(f) or f.dim() != 5 or f.shape[0] != 1 or f.shape[2] != 3 or f.dtype not in (torch.float16, torch.float32):
            raise ValueError(f"keyframe_fill: {name} must be a float16 / float32 [1,T,3,H,W] tensor in [-1, 1], not {tuple(getattr(f, 'shape', ()))}")
    _, T, _, H, W = source_frames.shape
    if T < 1 or H <= 1 or W <= 1:
        raise ValueError(f"keyframe_fill: {T} frame(s) of {H}x{W} cannot be filled")
    keys = check_keys(T, keys, "keyframe_fill")
    if tuple(edited_keys.shape) != (1, len(keys), 3, H, W):
        raise ValueError(f"keyframe_fill: edited_keys {tuple(edited_keys.shape)} must be [1,{len(keys)},3,{H},{W}]: one edited frame per key of a source {tuple(source_frames.shape)}")
    try:
        check_fill_args(mode=mode, sigma=sigma, occlusion=occlusion, alpha=alpha, beta=beta)
    except ValueError as e:
        raise ValueError(f"keyframe_fill: {e}") from None
    if flows is not None and flow_estimator is not None:
        raise ValueError("keyframe_fill: flows= and flow_estimator= are two flow sources: pass one")
    if len(keys) == T:
        return   # nothing to fill: no flow is needed
    if flows is None and flow_estimator is None:
        raise ValueError("keyframe_fill: no flow source: pass flows=dict(fwd=, bwd=) or flow_estimator= (always the SOURCE video's flows)")
    if flows is not None:
        if not isinstance(flows, dict) or set(flows) - {"fwd", "bwd"} or flows.get("fwd") is None or flows.get("bwd") is None:
            raise ValueError("keyframe_fill: flows must be dict(fwd=, bwd=) as mask_track.pair_flows returns it (side 0 chains bwd, side 1 fwd)")
        for k in ("fwd", "bwd"):
            f = flows[k]
            if not torch.is_tensor(f) or not f.is_floating_point() or tuple(f.shape) != (T - 1, 2, H, W):
                raise ValueError(f"keyframe_fill: flows[{k!r}] {tuple(getattr(f, 'shape', ()))} must be a floating-point [{T - 1},2,{H},{W}]")
    if flow_estimator is not None and not callable(flow_estimator):
        raise ValueError("keyframe_fill: flow_estimator must be callable: estimator(img1, img2) -> [n,2,H,W]")


@torch.no_grad()
def keyframe_fill(source_frames, edited_keys, keys, *, flows=None, flow_estimator=None, mode="residual", sigma=0.1, occlusion=True,
                  alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"]):
    """``source_frames`` [1,T,3,H,W] and the edited key frames ``edited_keys`` [1,Tk,3,H,W] (frame ``keys[j]`` of the source, edited), both
    in [-1, 1] -> dict(``frames`` [1,T,3,H,W] in the edit's dtype, ``confidence`` [T,H,W] fp32).  The key frames are copied into the result
    bit for bit and have confidence 1; every other frame is filled by the kernel (``mode``, ``sigma``: module docstring) and clipped to
    [-1, 1] like every result of ``edit_video``; its confidence is the sum of the weights it was blended with, 0 where no trajectory to
    either key could be followed and the keys were blended in place.  The flows are ALWAYS the source video's - ``flows=dict(fwd, bwd)`` or
    ``flow_estimator`` (then ``mask_track.pair_flows(source_frames, estimator)``) - and the photometric weight is taken on the source
    (``AFFINE_SIGNED``).  If every frame is a key the keys are returned and nothing is launched."""
    check_keyframe_fill_args(source_frames, edited_keys, keys, flows, flow_estimator, mode, sigma, occlusion, alpha, beta)
    _, T, _, H, W = source_frames.shape
    keys = list(keys)
    dev = edited_keys.device
    if len(keys) == T:
        return dict(frames=edited_keys, confidence=torch.ones((T, H, W), device=dev, dtype=torch.float32))
    src, edt = source_frames[0].to(dev), edited_keys[0]
    if flows is None:
        flows = pair_flows(source_frames.to(dev), flow_estimator, both=True)
    kf = key_flows(flows["fwd"].to(dev), flows["bwd"].to(dev), keys, occlusion=occlusion, alpha=alpha, beta=beta)
    out = torch.empty((T, 3, H, W), device=dev, dtype=edt.dtype)
    out.index_copy_(0, torch.tensor(keys, dtype=torch.long, device=dev), edt)
    _, conf = ops.keyframe_fill(src, edt, kf["flow"], kf["valid"], keys, kf["frames"], kf["slots"], kf["weights"], sigma=float(sigma), mode=mode,
                                guide_affine=AFFINE_SIGNED, out=out)
    rows = torch.tensor(kf["frames"], dtype=torch.long, device=dev)
    out.index_copy_(0, rows, out.index_select(0, rows).clip_(-1, 1))   # (a residual added to the source may leave the range)
    confidence = torch.ones((T, H, W), device=dev, dtype=torch.float32)
    confidence.index_copy_(0, rows, conf)
    return dict(frames=out[None], confidence=confidence)
