"""Region edits that follow the object, without a GPU: the float64 definition against section 26's, the planted
misreadings on the GPU file's inputs, ``track_plan`` by value, ``check_track``, the drivers with fakes, header / ctypes / wrappers, the
command line."""
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import region_ref as rr
import region_track_ref as tr
from driver_fakes import Model, RecordingPipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the definition
def test_integer_boxes_are_section_26_frame_by_frame_bit_for_bit():
    x = rr.uniform("track.cpu.int", tr.SRC_SHAPE)
    for boxes, size in (([(13, 9, 58, 38)] * 3, (24, 16)), ([(0, 0, 64, 40), (46, 29, 70, 45), (30, 20, 33, 22)], (8, 8)), ([(62, 0, 70, 8), (0, 37, 21, 45), (0, 0, 110, 75)], (24, 24))):
        for kind in ("bicubic", "bilinear"):
            got = tr.resample_track(x, [tuple(float(v) for v in b) for b in boxes], size, kind)
            for i, b in enumerate(boxes):
                assert np.array_equal(got[i], rr.resample(x[i], b, size, kind)), (boxes, kind, i)
    src, edit, down, mask = rr.paste_inputs("track.cpu.paste")
    src, edit, down, mask = (np.concatenate([a, a[:1]]) for a in (src, edit, down, mask))      # three frames
    boxes = [rr.PASTE_BOXES["two_borders"], rr.PASTE_BOXES["middle"], rr.PASTE_BOXES["half"]]
    for mode, blend, m in (("residual", 3, None), ("residual", 0, None), ("replace", 3, mask), ("replace", 0, None)):
        got = tr.paste_track(src, edit, down, [tuple(float(v) for v in b) for b in boxes], mode, blend, m)
        for i, b in enumerate(boxes):
            want = rr.paste(src[i:i + 1], edit[i:i + 1], down[i:i + 1], b, mode, blend, None if m is None else m[i:i + 1])
            assert np.array_equal(got[i:i + 1], want), (mode, blend, i)


def test_a_linear_image_is_reproduced_at_the_boxes_real_coordinates():
    """a x + b y + c0 sampled at pixel centres, up-sampled (ratios <= 1) from fractional boxes: the cubic with normalised weights
    reproduces linear functions, so every output whose taps are not clipped is the function at the output's centre in FRAME coordinates
    - which tells a half-pixel or an offset mistake from the definition."""
    H, W, a, b, c0 = 40, 60, 0.013, -0.007, 0.25
    img = (a * (np.arange(W)[None, :] + 0.5) + b * (np.arange(H)[:, None] + 0.5) + c0)[None, None]
    boxes = [(10.37109375, 8.62890625, 30.37109375, 20.62890625), (3.5, 2.25, 23.5, 14.25), (22.125, 11.0, 52.125, 35.0)]
    for (x0, y0, x1, y1), size in zip(boxes, ((40, 24), (20, 12), (48, 32))):
        w, h = size
        got = tr.resample_track(img, [(x0, y0, x1, y1)], size, "bicubic")[0, 0]
        cx, cy = x0 + (x1 - x0) / w * (np.arange(w) + 0.5), y0 + (y1 - y0) / h * (np.arange(h) + 0.5)
        want = a * cx[None, :] + b * cy[:, None] + c0
        full_x = [len(wt) == 4 for _, wt in tr.down_taps(x0, x1, w, "bicubic")]
        full_y = [len(wt) == 4 for _, wt in tr.down_taps(y0, y1, h, "bicubic")]
        inner = np.outer(full_y, full_x)
        assert inner.sum() > 0.5 * w * h and np.max(np.abs(got - want)[inner]) < 1e-12
        for wrong in ("floor_box", "no_half_pixel", "cover_scale"):
            bad = tr.resample_track(img, [(x0, y0, x1, y1)], size, "bicubic", wrong=wrong)[0, 0]
            assert np.max(np.abs(bad - want)[inner]) > 1e-4, wrong


def test_a_rolled_source_with_shifted_boxes_gives_the_same_bits():
    x = rr.uniform("track.cpu.roll", (2, 1, 50, 70))
    boxes = [(10.25, 8.5, 40.75, 30.25), (12.625, 9.75, 43.125, 31.5)]
    k = 7
    rolled = np.roll(x, (k, k), axis=(-2, -1))
    for kind, size in (("bicubic", (24, 16)), ("bilinear", (8, 8)), ("bicubic", (64, 40))):
        assert np.array_equal(tr.resample_track(x, boxes, size, kind), tr.resample_track(rolled, tr.moved(boxes[0], [(k, k)]) + tr.moved(boxes[1], [(k, k)]), size, kind))


def _all_resample_cases():
    x = rr.uniform("region_track.src", tr.SRC_SHAPE)
    for name, boxes, size, clamp in tr.RESAMPLE_CASES:
        for kind in ("bicubic", "bilinear"):
            yield name, x, boxes, size, kind, clamp


def test_the_measured_constant_of_the_bound():
    worst = max(tr.measured_k(x, boxes, size, kind) for _, x, boxes, size, kind, _ in _all_resample_cases())
    print(f"[region_track] fp32 emulation / float64 definition: worst ratio {worst:.2f} (K_MEASURED {tr.K_MEASURED})")
    assert worst <= tr.K_MEASURED and worst > 0.5 * tr.K_MEASURED


def test_the_inputs_tell_every_misreading_from_the_definition():
    seen = set()
    # the resample: every misreading on at least one case of the GPU file, by more than that case's largest bound
    cases = {name: (x, boxes, size, kind) for name, x, boxes, size, kind, _ in _all_resample_cases() if kind == "bicubic"}
    for wrong, name in (("floor_box", "subpixel_shift_ratio_1"), ("no_half_pixel", "tile_exact"), ("cover_scale", "ratio_2p67_x_eighth_y"),
                        ("frame_clip", "tile_minus_1"), ("frame0_box", "tile_plus_1"), ("plane_index", "tile_exact")):
        x, boxes, size, kind = cases[name]
        rr.need_gap(wrong, tr.resample_track(x, boxes, size, kind), tr.resample_track(x, boxes, size, kind, wrong=wrong), float(tr.resample_bound(x, boxes, size, kind).max()))
        seen.add(wrong)
    src, edit, down, mask = tr.paste_inputs("region_track.paste")
    for wrong, key in (("ramp_from_cover", "middle"), ("paste_from_cover", "middle"), ("frame0_box", "middle"), ("plane_index", "half")):
        boxes = tr.PASTE_BOXES[key]
        tol = float(tr.paste_bound(src, edit, down, boxes, "residual").max())
        rr.need_gap(wrong, tr.paste_track(src, edit, down, boxes, "residual", 3), tr.paste_track(src, edit, down, boxes, "residual", 3, wrong=wrong), tol)
        seen.add(wrong)
    # the plan: the delivered origins are multiples of 1 / 256, so any difference is at least that
    frame, size, bb = (120, 200), (48, 32), fast_motion()
    for wrong in ("smooth_unnormalised", "no_containment"):
        rr.need_gap(wrong, tr.track_plan(frame, size, bb), tr.track_plan(frame, size, bb, wrong=wrong), 0.5 / tr.TRACK_SUBPIXEL)
        seen.add(wrong)
    assert seen == set(tr.MISREADINGS)


def test_the_ramp_from_real_edges():
    r = tr.ramp_track((37, 53), (9.25, 6.5, 45.25, 30.5), 4)
    assert r.shape == (25, 37)                                       # the cover [9, 46) x [6, 31)
    assert r[12, 0] == 0.25 / 4 and r[12, 1] == 1.25 / 4 and r[12, 36] == 0.0 and r[12, 35] == 0.75 / 4    # centres 9.5, 10.5, 45.5, 44.5
    assert r[0, 18] == 0.0 and r[1, 18] == 0.25 and r[24, 18] == 0.0 and r[12, 18] == 1.0                  # centres 6.5 (on the edge), 7.5, 30.5
    hard = tr.ramp_track((37, 53), (9.25, 6.5, 45.25, 30.5), 0)
    assert hard[12, 0] == 1.0 and hard[12, 36] == 0.0 and hard[0, 18] == 1.0 and hard[24, 18] == 0.0      # half-open: 6.5 is inside, 30.5 is not
    assert np.array_equal(tr.ramp_track((37, 53), (0.0, 0.0, 53.0, 37.0), 5), np.ones((37, 53)))           # no edge that is not a border
    edge = tr.ramp_track((37, 53), (0.0, 0.0, 30.5, 20.25), 2)
    assert edge[0, 0] == 1.0 and edge[5, 30] == 0.0 and edge[5, 29] == 0.5 and edge[20, 5] == 0.0 and edge[19, 5] == 0.375
    # a pixel under a ramp of 0 keeps the source, whatever its taps give (here 0 / 0: the centre 9.5 is half a pixel left of x0 = 10)
    src, edit, down, _ = tr.paste_inputs("region_track.ramp0")
    out = tr.paste_track(src, edit, down, [(9.99609375, 6.5, 45.99609375, 30.5)] * 3, "residual", 0)
    assert not np.isnan(out).any() and np.array_equal(out[..., 9], src.astype(np.float64)[..., 9])


# ------------------------------------------------------------------------------------------------------------------ track_plan by value
def fast_motion():
    """A 20 x 16 object that jumps: the smoothed centre lags by more than the padding, so containment has to shift the box."""
    xs = [10, 12, 14, 16, 150, 152, 154, 156]
    return [(x, 40, x + 20, 56) for x in xs]


def _plan(*a, **kw):
    from insv2v.region_track import track_plan
    return track_plan(*a, **kw)


def _guarantees(plan, frame, bboxes):
    H, W = frame
    Bw, Bh = plan["boxes"][0][2] - plan["boxes"][0][0], plan["boxes"][0][3] - plan["boxes"][0][1]
    for (x0, y0, x1, y1), b in zip(plan["boxes"], bboxes):
        assert 0 <= x0 and 0 <= y0 and x1 <= W and y1 <= H
        assert x1 - x0 == Bw and y1 - y0 == Bh
        assert (x0 * 256).is_integer() and (y0 * 256).is_integer()
        if b[2] > b[0] and b[3] > b[1]:
            assert x0 <= b[0] and y0 <= b[1] and b[2] <= x1 and b[3] <= y1
    return Bw, Bh


def test_track_plan_by_value():
    frame, size = (120, 200), (48, 32)
    # a static object: every box has region_plan's size and is centred on the object (region_plan's integers put the odd pixel on one side)
    from insv2v.region import region_plan
    bb = [(90, 50, 110, 70)] * 5
    p = _plan(frame, size, bb)
    static = region_plan(frame, size, bbox=bb[0])["box"]
    assert static == (78, 45, 123, 75) and p["boxes"] == [(77.5, 45.0, 122.5, 75.0)] * 5 and p["union"] == static and p["travel"] == 0.0
    assert p["size"] == size and p["frame"] == frame and p["ratio"] == (45 / 48, 30 / 32) and p["anisotropy"] == 1.0
    # a linear motion of 3.25 pixels a frame: smoothing keeps the interior of a straight line, the size is that of one frame's box, the
    # union is much wider
    bb = [(20 + 13 * t // 4, 50, 40 + 13 * t // 4, 70) for t in range(24)]
    p = _plan(frame, size, bb, smooth=1.0)
    Bw, Bh = _guarantees(p, frame, bb)
    assert (Bw, Bh) == (45, 30) and p["union"][2] - p["union"][0] > 2 * Bw
    mid = [b[0] + Bw / 2 for b in p["boxes"]][4:20]
    raw = [(b[0] + b[2]) / 2 for b in bb][4:20]
    assert max(abs(m - r) for m, r in zip(mid, raw)) < 0.5                   # (the integer steps of the bboxes are what is smoothed away)
    steps = [b - a for a, b in zip(mid, mid[1:])]
    assert all(abs(s - 3.25) < 0.2 for s in steps) and any(not float(s).is_integer() for s in steps)
    assert abs(p["travel"] - math.hypot(p["boxes"][-1][0] - p["boxes"][0][0], p["boxes"][-1][1] - p["boxes"][0][1])) < 1e-9
    assert p["boxes"] == tr.track_plan(frame, size, bb, smooth=1.0)
    # smooth = 0 keeps the raw centres (quantised), also at the ends
    p0 = _plan(frame, size, bb, smooth=0)
    assert [b[0] for b in p0["boxes"]] == [(a[0] + a[2]) / 2 - Bw / 2 for a in bb]
    # empty frames: interpolated in the middle, held at both ends
    E = (200, 120, 0, 0)
    bb = [E, E, (40, 50, 60, 70), E, E, E, (80, 50, 100, 70), E]
    p = _plan(frame, size, bb, smooth=0)
    _guarantees(p, frame, bb)
    assert [b[0] + 22.5 for b in p["boxes"]] == [50.0, 50.0, 50.0, 60.0, 70.0, 80.0, 90.0, 90.0]
    assert p["boxes"] == tr.track_plan(frame, size, bb, smooth=0) and _plan(frame, size, bb)["boxes"] == tr.track_plan(frame, size, bb)
    with pytest.raises(ValueError, match="empty in every one"):
        _plan(frame, size, [E, E, E])
    # a fast motion: the smoothed centre lags, containment shifts the box over its own bbox
    bb = fast_motion()
    p = _plan(frame, size, bb)
    Bw, _ = _guarantees(p, frame, bb)
    loose = tr.track_plan(frame, size, bb, wrong="no_containment")
    assert any(l[0] > b[0] or l[2] < b[2] for l, b in zip(loose, bb)) and p["boxes"] == tr.track_plan(frame, size, bb)
    for got, l, b in zip(p["boxes"], loose, bb):                                               # the smallest shift: the edges then touch
        assert got[0] == (float(b[0]) if l[0] > b[0] else float(b[2] - Bw) if l[2] < b[2] else l[0])
    # a track that runs into a frame border: the boxes stop at it, the object stays inside
    bb = [(150 + 6 * t, 5, 170 + 6 * t, 25) for t in range(6)]
    p = _plan(frame, size, bb, smooth=0)
    _guarantees(p, frame, bb)
    assert p["boxes"][-1][2] == 200.0 and all(b[1] == 0.0 for b in p["boxes"]) and p["boxes"][0][2] < 200.0
    # a box that takes a whole frame dimension: tall objects in a flat frame
    bb = [(30 + 4 * t, 10, 50 + 4 * t, 110) for t in range(4)]
    p = _plan(frame, size, bb)
    assert all(b[1] == 0.0 and b[3] == 120.0 for b in p["boxes"]) and p["anisotropy"] != 1.0
    _guarantees(p, frame, bb)
    # the ratio limit, as region_plan's
    with pytest.raises(ValueError, match="differ by more than a factor of 8"):
        _plan((600, 900), (8, 8), [(100, 100, 300, 300)])
    with pytest.raises(ValueError, match="multiples of 8"):
        _plan(frame, (20, 20), [(90, 50, 110, 70)])
    with pytest.raises(ValueError, match="not inside"):
        _plan(frame, size, [(190, 50, 210, 70)])


def test_track_plan_guarantees_over_random_tracks():
    rng = random.Random(27)
    for _ in range(200):
        H, W = rng.randint(40, 300), rng.randint(40, 300)
        size = (8 * rng.randint(2, 8), 8 * rng.randint(2, 8))
        T = rng.randint(1, 20)
        bw, bh = rng.randint(2, W // 3), rng.randint(2, H // 3)
        x, y, bb = rng.uniform(0, W - bw), rng.uniform(0, H - bh), []
        for t in range(T):
            x, y = min(max(x + rng.uniform(-25, 25), 0), W - bw), min(max(y + rng.uniform(-25, 25), 0), H - bh)
            w_t, h_t = rng.randint(1, bw), rng.randint(1, bh)
            bb.append((W, H, 0, 0) if rng.random() < 0.2 else (int(x), int(y), int(x) + w_t, int(y) + h_t))
        if all(b[2] <= b[0] for b in bb):
            bb[rng.randrange(T)] = (0, 0, bw, bh)
        try:
            p = _plan((H, W), size, bb, pad=rng.choice([0.0, 0.25, 1.0]), smooth=rng.choice([0, 0.5, 2.0, 5.0]))
        except ValueError as e:
            assert "factor of 8" in str(e)
            continue
        _guarantees(p, (H, W), bb)


def test_check_track():
    from insv2v.region_track import check_track, TRACK_KEYS, TRACK_SUBPIXEL
    assert TRACK_KEYS == ("smooth", "boxes") and TRACK_SUBPIXEL == 256
    assert check_track(True) == dict(smooth=2.0, boxes=None) == check_track({})
    assert check_track(dict(smooth=0)) == dict(smooth=0, boxes=None)
    assert check_track(dict(boxes=[[1, 2, 3.5, 4]]))["boxes"] == [(1.0, 2.0, 3.5, 4.0)]
    assert check_track(dict(boxes=torch.tensor([[1.0, 2.0, 3.5, 4.0]], dtype=torch.float64)))["boxes"] == [(1.0, 2.0, 3.5, 4.0)]
    for bad in (False, None, 3, dict(sigma=1), dict(smooth=-1), dict(smooth=float("nan")), dict(smooth=True), dict(boxes=[]), dict(boxes=[(1, 2, 3)]),
                dict(boxes=[(1, 2, 3, float("inf"))]), dict(boxes=(1, 2, 3, 4))):
        with pytest.raises(ValueError, match="track"):
            check_track(bad)


# ------------------------------------------------------------------------------------------------------------------ the drivers, with fakes
class _Ops:
    """CPU stand-ins of the entries, computed by the references; every call is recorded."""

    def __init__(self):
        self.calls = []

    def mask_bbox(self, mask, *, threshold=0.5, out=None):
        self.calls.append(("mask_bbox", tuple(mask.shape)))
        return torch.from_numpy(rr.mask_bbox(mask.numpy(), threshold))

    def region_resample(self, src, box, size, *, mode="bicubic", clamp=None, out=None):
        self.calls.append(("region_resample", tuple(src.shape), tuple(box), tuple(size), mode, clamp))
        r = rr.resample(src.numpy(), box, size, mode)
        return torch.from_numpy(np.clip(r, *clamp) if clamp else r).float()

    def region_paste(self, out, edit_w, down_src, box, *, mode="residual", blend=8, mask_w=None):
        self.calls.append(("region_paste", tuple(out.shape), tuple(box), mode, blend, None if mask_w is None else tuple(mask_w.shape)))
        m = None if mask_w is None else mask_w.expand(out.shape[0], *mask_w.shape[1:]).numpy()
        out.copy_(torch.from_numpy(rr.paste(out.numpy(), edit_w.numpy(), None if down_src is None else down_src.numpy(), box, mode, blend, m)).float())
        return out

    def region_resample_track(self, src, boxes, size, *, mode="bicubic", clamp=None, out=None):
        self.calls.append(("region_resample_track", tuple(src.shape), list(boxes), tuple(size), mode, clamp))
        return torch.from_numpy(tr.resample_track(src.numpy(), list(boxes), size, mode, clamp=clamp)).float()

    def region_paste_track(self, out, edit_w, down_src, boxes, *, mode="residual", blend=8, mask_w=None):
        self.calls.append(("region_paste_track", tuple(out.shape), list(boxes), mode, blend, None if mask_w is None else tuple(mask_w.shape)))
        m = None if mask_w is None else mask_w.expand(out.shape[0], *mask_w.shape[1:]).numpy()
        out.copy_(torch.from_numpy(tr.paste_track(out.numpy(), edit_w.numpy(), None if down_src is None else down_src.numpy(), list(boxes), mode, blend, m)).float())
        return out


@pytest.fixture
def fake_ops(monkeypatch):
    from insv2v import ops
    fake = _Ops()
    for name in ("mask_bbox", "region_resample", "region_paste", "region_resample_track", "region_paste_track"):
        monkeypatch.setattr(ops, name, getattr(fake, name))
    return fake


T, H, W = 4, 75, 110
MOVING = [(20 + 9 * t, 30 + 2 * t, 40 + 9 * t, 50 + 2 * t) for t in range(T)]


def _source(name, H=H, W=W):
    return torch.from_numpy(rr.uniform(name, (1, T, 3, H, W)))


def _moving_mask(H=H, W=W):
    m = torch.zeros((1, T, H, W))
    for t, (x0, y0, x1, y1) in enumerate(MOVING):
        m[0, t, y0:y1, x0:x1] = 1.0
    return m


def _fake_edit_video(seen):
    def fake(model, pipe, frames, text_cond, text_uncond, **kw):
        seen.append(dict(kw, frames=frames, text=(text_cond, text_uncond)))
        out = (frames * 0.5,) + (("latent",) if kw.get("return_latent") else ()) + (((dict(mask=kw["mask"]) if "mask" in kw else None),) if kw.get("return_mask") else ())
        return out if len(out) > 1 else out[0]
    return fake


def test_edit_region_with_a_track_calls_edit_video_once(fake_ops, monkeypatch):
    from insv2v import region, region_track, run_loveu_tgve
    seen = []
    monkeypatch.setattr(run_loveu_tgve, "edit_video", _fake_edit_video(seen))
    frames, M = _source("track.cpu.drv"), _moving_mask()
    got = region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32), blend=3), track=True, mask=M, seed=7, stabilize=True,
                             keyframes=2, return_latent=True, return_mask=True)
    assert len(seen) == 1
    kw = seen[0]
    plan = region_track.track_plan((H, W), (48, 32), MOVING)
    assert kw["frames"].shape == (1, T, 3, 32, 48) and kw["mask"].shape == (1, T, 32, 48) and kw["text"] == ("tc", "tu")
    assert {k: kw[k] for k in ("seed", "stabilize", "keyframes", "return_latent", "return_mask")} == dict(seed=7, stabilize=True, keyframes=2, return_latent=True, return_mask=True)
    assert "track" not in kw and "region" not in kw
    assert [c[0] for c in fake_ops.calls] == ["mask_bbox", "region_resample_track", "region_resample_track", "region_paste_track"]
    assert fake_ops.calls[0][1] == (T, H, W)                                      # ONE launch on the per-frame mask
    assert fake_ops.calls[1][2:] == (plan["boxes"], (48, 32), "bicubic", (-1.0, 1.0)) and fake_ops.calls[2][2:] == (plan["boxes"], (48, 32), "bilinear", None)
    assert fake_ops.calls[3][1:] == ((T, 3, H, W), plan["boxes"], "residual", 3, None)
    image, latent, est = got
    assert latent == "latent" and image.shape == frames.shape
    assert set(est["region"]) == {"boxes", "travel", "size", "working", "down_src"} and est["region"]["boxes"] == plan["boxes"] and est["region"]["travel"] == plan["travel"] > 5
    want = tr.paste_track(frames[0].numpy(), kw["frames"][0].numpy() * 0.5, kw["frames"][0].numpy(), plan["boxes"], "residual", 3)
    assert np.allclose(image[0].numpy(), want, atol=1e-6)
    for t, b in enumerate(plan["boxes"]):                                          # every frame equals its source outside its own cover
        X0, Y0, X1, Y1 = tr.cover(b)
        outside = torch.ones((3, H, W), dtype=torch.bool)
        outside[:, Y0:Y1, X0:X1] = False
        assert torch.equal(image[0, t][outside], frames[0, t][outside]) and not torch.equal(image[0, t], frames[0, t])
    # boxes taken as given: no mask_bbox; replace mode asks the inner edit for its mask; a still mask is cropped per frame
    del seen[:], fake_ops.calls[:]
    given = [(10.5 + t, 8.25, 55.5 + t, 38.25) for t in range(T)]
    out = region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32), mode="replace"), track=dict(boxes=given), mask=torch.ones((1, 1, H, W)))
    assert torch.is_tensor(out) and [c[0] for c in fake_ops.calls] == ["region_resample_track", "region_resample_track", "region_paste_track"]
    assert seen[0]["mask"].shape == (1, T, 32, 48) and fake_ops.calls[-1][1:] == ((T, 3, H, W), given, "replace", 8, (T, 32, 48))
    # an integer box for every frame is the static edit
    B = (28, 25, 73, 55)
    a = region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32)), track=dict(boxes=[B] * T), mask=M)
    b = region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32), box=B), mask=M)
    assert torch.equal(a, b)
    # mask="auto" with explicit boxes runs: the mask is made inside the inner edit
    assert region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32)), track=dict(boxes=given), mask="auto").shape == frames.shape


def test_every_refusal_of_the_track_drivers_comes_before_any_launch(fake_ops, monkeypatch):
    from insv2v import region, run_loveu_tgve
    monkeypatch.setattr(run_loveu_tgve, "edit_video", lambda model, pipe, frames, tc, tu, **kw: frames)
    monkeypatch.setattr(run_loveu_tgve, "edit_videos", lambda model, pipe, units, **kw: [u["frames"] for u in units])
    frames, M, reg = _source("track.cpu.refuse"), _moving_mask(), dict(size=(48, 32))
    ok = [(10.0, 8.0, 55.0, 38.0)] * T
    cases = [(dict(track=True, mask=torch.ones((1, 1, H, W))), "a still mask"), (dict(track=True, mask="auto"), "nothing to follow"),
             (dict(track=True, mask=M, mask_key=1), "nothing to follow"), (dict(track=True), "follows a per-frame mask"),
             (dict(track=True, mask=M, region=dict(reg, box=(1, 2, 50, 40))), r"region\['box'\]"), (dict(track=True, mask=M, region=dict(reg, box="frame")), r"region\['box'\]"),
             (dict(track=dict(boxes=ok[:-1])), "one per frame"), (dict(track=dict(boxes=ok[:-1] + [(10.0, 8.0, 56.0, 38.0)])), "share one width"),
             (dict(track=dict(boxes=[(70.0, 8.0, 115.0, 38.0)] * T)), "not inside"), (dict(track=dict(boxes=[(10.0, 8.0, 10.0, 38.0)] * T)), "is empty"),
             (dict(track=dict(boxes=[(10.0, 8.0, 13.0, 10.0)] * T)), "factor of 8"), (dict(track=dict(smooth=-1), mask=M), "smooth must be"),
             (dict(track=dict(speed=1), mask=M), "keys among"), (dict(track=True, mask=torch.zeros((1, T, H, W))), "empty in every one"),
             (dict(track=True, mask=torch.ones((1, T, 32, 48))), "must be a floating-point")]
    for kw, msg in cases:
        del fake_ops.calls[:]
        kw = dict(dict(region=reg), **kw)
        with pytest.raises(ValueError, match=msg):
            region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", **kw)
        with pytest.raises(ValueError, match=msg):
            region.edit_regions(Model(), RecordingPipe(), [dict(frames=frames, text_cond="tc", text_uncond="tu", **kw)])
        assert [c[0] for c in fake_ops.calls if c[0] != "mask_bbox"] == [], msg       # (the empty mask is known only after mask_bbox)
    # track=None is the static path
    del fake_ops.calls[:]
    region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=reg, track=None, mask=M)
    assert [c[0] for c in fake_ops.calls] == ["mask_bbox", "region_resample", "region_resample", "region_paste"]


def test_edit_regions_runs_tracked_and_static_units_as_one_edit_videos(fake_ops, monkeypatch):
    from insv2v import region, region_track, run_loveu_tgve
    seen = []

    def fake_edit_videos(model, pipe, units, **kw):
        seen.append((units, kw))
        return [u["frames"] * 0.25 for u in units]
    monkeypatch.setattr(run_loveu_tgve, "edit_videos", fake_edit_videos)
    a, b = _source("track.cpu.a"), _source("track.cpu.b", H=61, W=97)
    units = [dict(frames=a, text_cond="a", text_uncond="u", unit=0, mask=_moving_mask(), region=dict(size=(48, 32)), track=dict(smooth=1.0)),
             dict(frames=b, text_cond="b", text_uncond="u", unit=1, region=dict(size=(48, 32), box=(5, 7, 80, 50)), text_cfg=3.0)]
    outs = region.edit_regions(Model(), RecordingPipe(), units, seed=11, max_clips=4)
    assert len(seen) == 1
    inner, kw = seen[0]
    assert kw == dict(seed=11, max_clips=4) and [tuple(u["frames"].shape) for u in inner] == [(1, T, 3, 32, 48)] * 2
    assert all("region" not in u and "track" not in u for u in inner) and inner[0]["mask"].shape == (1, T, 32, 48) and inner[1]["text_cfg"] == 3.0
    assert [c[0] for c in fake_ops.calls] == ["mask_bbox", "region_resample_track", "region_resample_track", "region_resample", "region_paste_track", "region_paste"]
    assert fake_ops.calls[1][2] == region_track.track_plan((H, W), (48, 32), MOVING, smooth=1.0)["boxes"]
    assert [tuple(o.shape) for o in outs] == [tuple(a.shape), tuple(b.shape)] and not torch.equal(outs[0], a)
    assert torch.equal(outs[1][..., :7, :], b[..., :7, :])


# ------------------------------------------------------------------------------------------------------------------ header, ctypes, wrappers
def test_header_lib_and_ops_agree_on_the_track_entries():
    from insv2v import _lib
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    c = _lib
    ctype = {"int32_t": c.c_i32, "int64_t": c.c_i64, "float": c.c_f32}
    for name, desc, static in (("resample", _lib.RegionResampleTrackDesc, _lib.RegionResampleDesc), ("paste", _lib.RegionPasteTrackDesc, _lib.RegionPasteDesc)):
        assert f"int insv2v_region_{name}_track(const insv2v_region_{name}_track_desc* d, insv2v_stream_t stream);" in header
        assert _lib.SIGNATURES[f"insv2v_region_{name}_track"] == (c.c_i32, [_lib.SIGNATURES[f"insv2v_region_{name}_track"][1][0], c.c_p])
        assert _lib.SIGNATURES[f"insv2v_region_{name}_track"][1][0]._type_ is desc
        fields = re.search(rf"typedef struct insv2v_region_{name}_track_desc \{{(.*?)\}} insv2v_region_{name}_track_desc;", header, re.S).group(1)
        declared = [n for line in fields.split("\n") for n in re.findall(r"[\s*](\w+)\s*[,;]", line.split("/*")[0])]
        assert declared == [n for n, _ in desc._fields_]
        for line in fields.split("\n"):
            line = line.split("/*")[0].strip()
            if line:
                t = c.c_p if "*" in line else ctype[line.split()[0]]
                for n in re.findall(r"[\s*](\w+)\s*[,;]", line):
                    assert dict(desc._fields_)[n] is t, (name, n)
        # the static descriptor's fields without the integer box, plus the host pointer to the boxes
        assert sorted(n for n, _ in desc._fields_) == sorted([n for n, _ in static._fields_ if n not in ("x0", "y0", "x1", "y1")] + ["boxes"])
        assert "const double* boxes;" in fields
    assert _lib.ABI_VERSION == 15 and "additions to ABI 15: no existing struct or entry changes" in header.split("insv2v_region_resample_track_desc")[0][-4500:]
    assert "int insv2v_abi_version(void) { return 15; }" in open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "elementwise.hip")).read()
    from insv2v import ops, region, region_track
    assert all(callable(getattr(ops, n)) for n in ("region_resample_track", "region_paste_track"))
    assert all(callable(getattr(region_track, n)) for n in ("check_track", "track_plan", "crop_to_working_track", "paste_back_track"))
    src = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "region.hip")).read()
    assert 'extern "C" int insv2v_region_resample_track(' in src and 'extern "C" int insv2v_region_paste_track(' in src
    assert region.REGION_KEYS == ("size", "box", "pad", "mode", "blend", "threshold")
    assert region.REGION_DEFAULTS == dict(size=(384, 384), box=None, pad=0.25, mode="residual", blend=8, threshold=0.5)
    # the wrappers refuse boxes they cannot hand to the entry before they load anything onto a GPU
    with pytest.raises(_lib.HipKernelError, match="one .* per frame"):
        ops._track_boxes([(0.0, 0.0, 1.0, 1.0)], 2, "t")
    with pytest.raises(_lib.HipKernelError, match="float64 CPU tensor"):
        ops._track_boxes(torch.zeros((2, 4)), 2, "t")
    arr = ops._track_boxes(torch.tensor([[0.5, 1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.25]], dtype=torch.float64), 2, "t")
    assert list(arr) == [0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.25]


# ------------------------------------------------------------------------------------------------------------------ the command line
def test_region_track_on_the_command_line():
    from insv2v.run_loveu_tgve import build_parser, check_args, region_unit
    base = ["--synthetic", "1", "--synthetic-tiny", "--image-size", "32"]
    parse = lambda extra: check_args(build_parser().parse_args(base + extra))   # noqa: E731
    assert region_unit(parse(["--region"])) == dict(region=dict(size=(32, 32)))                 # the existing switches: no extra entry
    assert region_unit(parse(["--region", "--region-track"])) == dict(region=dict(size=(32, 32)), track=True)
    assert region_unit(parse(["--region", "--region-track", "--region-track-smooth", "0.5", "--region-pad", "0.5"])) == dict(region=dict(size=(32, 32), pad=0.5), track=dict(smooth=0.5))
    for extra, msg in ((["--region-track"], "need --region"), (["--region-track-smooth", "1"], "need --region"),
                       (["--region", "--region-track-smooth", "1"], "parameter of --region-track"),
                       (["--region", "--region-track", "--region-track-smooth", "-1"], "smooth must be"),
                       (["--region", "--region-track", "--region-box", "1", "2", "30", "40"], "give one of them"),
                       (["--region", "--region-track", "--auto-mask"], "follows a drawn per-frame mask"),
                       (["--region", "--region-track", "--synthetic-mask", "--mask-key", "1"], "follows a drawn per-frame mask")):
        with pytest.raises(SystemExit, match=msg):
            parse(extra)
