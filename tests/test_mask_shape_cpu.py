"""CPU tests of the mask shaping: the reference (tests/mask_shape_ref.py) against an independent brute-force pair loop and against scipy,
the planner (called through the loaded library - it launches nothing) against the float64 definition, the definition's properties, planted
misreadings on the very inputs the GPU file uses, the host-side argument checks, masks from image files, and the C ABI."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import mask_shape_ref as mr
from conftest import ROOT


def _lib():
    from insv2v import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build
        build.build(verbose=False)
    return _lib, _lib.load()


def _plan(g, f):
    L, lib = _lib()
    p = L.MaskShapePlan()
    rc = lib.insv2v_mask_shape_plan(g, f, ctypes.byref(p))
    assert rc == p.rc
    return rc, {n: getattr(p, n) for n, _ in p._fields_ if n != "rc"}


# ------------------------------------------------------------------------------------------------------------------ 1. the reference
def _brute(hit, R, metric=lambda dy, dx: dy * dy + dx * dx):
    """Every pixel against every pixel of the set, one pair at a time."""
    H, W = hit.shape
    far = (R + 1) ** 2
    pts = [(y, x) for y in range(H) for x in range(W) if hit[y, x]]
    d = np.full((H, W), far, dtype=np.int64)
    for y in range(H):
        for x in range(W):
            best = min((metric(abs(y - py), abs(x - px)) for py, px in pts), default=far)
            d[y, x] = best if best <= R * R else far
    return d


def _random_mask(key, H, W):
    rng = np.random.default_rng(key)
    return mr._blobs(rng, H, W, 1 if H * W < 64 else 3).astype(np.float32)


SMALL = [(1, 1), (2, 3), (9, 13), (17, 33)]


@pytest.mark.parametrize("H,W", SMALL)
def test_reference_vs_brute_force(H, W):
    for key, R in ((1, 1), (2, 5), (3, 40)):
        m = _random_mask(key, H, W)
        if (H, W) == (1, 1):
            m[:] = 1.0 if key == 2 else 0.0
        ins, d2o, d2i = mr.distances(m[None], mr.TAU, R)
        assert np.array_equal(d2o[0], _brute(ins[0], R)) and np.array_equal(d2i[0], _brute(~ins[0], R)), (H, W, R)
        assert (d2o[0][ins[0]] == 0).all() and (d2i[0][~ins[0]] == 0).all() and (d2o[0][~ins[0]] >= 1).all() and (d2i[0][ins[0]] >= 1).all()


@pytest.mark.parametrize("H,W", SMALL[1:])
def test_reference_vs_scipy(H, W):
    """scipy's exact Euclidean transform measures the distance to the nearest ZERO and does not treat the border as one - wherever the
    array holds a zero.  Without one it returns garbage, so empty and full frames are checked against the definition below."""
    ndi = pytest.importorskip("scipy.ndimage")
    R = 5
    far = (R + 1) ** 2
    for key in range(4):
        m = _random_mask(10 + key, H, W)
        ins, d2o, d2i = mr.distances(m[None], mr.TAU, R)
        assert ins.any() and not ins.all()
        for got, zeros_at in ((d2o[0], ins[0]), (d2i[0], ~ins[0])):
            want = np.rint(ndi.distance_transform_edt(~zeros_at) ** 2).astype(np.int64)
            assert np.array_equal(got, np.where(want > R * R, far, want))


def test_empty_and_full_frames_follow_the_definition():
    for g, f in ((0.0, 0.0), (4.0, 8.0), (-3.0, 2.0), (32.0, 32.0)):
        R, far = mr.radius(g, f)
        m = np.stack([np.zeros((7, 9), np.float32), np.ones((7, 9), np.float32), np.full((7, 9), np.nan, np.float32)])
        r = mr.mask_shape(m, g, f)
        assert (r["d2_out"][0] == far).all() and (r["d2_in"][0] == 0).all() and (r["shaped"][0] == 0).all()
        assert (r["d2_in"][1] == far).all() and (r["d2_out"][1] == 0).all() and (r["shaped"][1] == 1).all()   # the border is not outside
        assert (r["d2_out"][2] == far).all() and (r["shaped"][2] == 0).all()                                   # a NaN is outside


# ------------------------------------------------------------------------------------------------------------------ 2. the planner
S2, S5 = math.sqrt(2.0), math.sqrt(5.0)
UP = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))   # noqa: E731
DN = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))  # noqa: E731
# (g, f) -> (R, FAR, out_one, out_zero, in_one, in_zero), worked out by hand from floor(g^2), ceil((g+f)^2), ceil((1-g)^2), floor((1-g-f)^2)
PINNED = {
    (0.0, 0.0): (1, 4, 0, 0, 1, 1),
    (4.0, 8.0): (12, 169, 16, 144, 0, -1),
    (2.5, 4.0): (7, 64, 6, 43, 0, -1),          # 6.25 -> 6, 42.25 -> 43
    (0.5, 0.5): (1, 4, 0, 1, 1, 0),             # in_one ceil(0.25) = 1, in_zero floor(0) = 0
    (-2.0, 3.0): (3, 16, -1, 1, 9, 0),
    (-2.0, 1.5): (3, 16, -1, 0, 9, 2),          # g + f = -0.5 < 0: every outside pixel is 0; (1.5)^2 = 2.25 -> 2
    (-32.0, 0.0): (33, 1156, -1, 0, 1089, 1089),
    (-32.0, 32.0): (33, 1156, -1, 0, 1089, 1),
    (32.0, 32.0): (64, 4225, 1024, 4096, 0, -1),
    (32.0, 0.0): (32, 1089, 1024, 1024, 0, -1),
    (0.0, 32.0): (32, 1089, 0, 1024, 1, -1),
    (20.0, 12.0): (32, 1089, 400, 1024, 0, -1),
    (3.0, 2.0): (5, 36, 9, 25, 0, -1),
}
# fp32 values just below and just above a lattice distance: sqrt 2, sqrt 5, 5 = sqrt 25
EDGE = [(DN(S2), 0.0, 1), (UP(S2), 0.0, 2), (DN(S5), 0.0, 4), (UP(S5), 0.0, 5), (DN(5.0), 0.0, 24), (5.0, 0.0, 25), (UP(5.0), 0.0, 25)]
TABLE = list(PINNED) + [(g, f) for g, f, _ in EDGE] + [(1.0, DN(S2)), (1.0, UP(S2)), (0.0, DN(S5)), (0.0, UP(S5)), (-1.5, 1.5), (-1.5, UP(1.5)),
                                                        (-1.5, DN(1.5)), (-0.25, 0.75), (1.0, 0.0), (UP(1.0), 0.0), (DN(1.0), 0.0), (31.5, 32.0),
                                                        (-31.5, 0.25), (0.3, 0.0), (7.3, 11.9)]


def test_planner_pinned_values():
    for (g, f), want in PINNED.items():
        rc, p = _plan(g, f)
        assert rc == 0 and (p["R"], p["far"], p["out_one"], p["out_zero"], p["in_one"], p["in_zero"]) == want, (g, f, p)
        assert p["row_tile"] == 256
    for g, f, out_one in EDGE:
        assert _plan(g, f)[1]["out_one"] == out_one, (g, out_one)
    assert np.float32(mr.SQRT2) ** 2 < 2 and _plan(mr.SQRT2, 0.0)[1]["out_one"] == 1    # fp32(sqrt 2) lies below sqrt 2
    assert _plan(0.0, DN(S2))[1]["out_zero"] == 2 and _plan(0.0, UP(S2))[1]["out_zero"] == 3
    assert _plan(1.0 - DN(S2), 0.0)[1]["in_one"] in (2, 3)


@pytest.mark.parametrize("g,f", TABLE)
def test_planner_vs_float64_definition(g, f):
    """R, FAR and the thresholds are those of exact rational arithmetic on the fp32 (g, f); and on a 17 x 33 mask - and on every D2 from 0
    to FAR - the decision taken on the integers equals the decision taken on s in float64, for every pixel."""
    rc, p = _plan(g, f)
    assert rc == 0
    R, far = mr.radius(g, f)
    assert (p["R"], p["far"]) == (R, far) and R <= 65
    ex = mr.thresholds_exact(g, f)
    for k, v in ex.items():   # the same numbers: as they are, or capped to the range of D2 the kernel can meet (0 .. FAR) where they lie beyond it
        assert p[k] == v or (k.endswith("zero") and k.startswith("out") and v > far and p[k] == far) or \
            (k == "in_one" and v > far and p[k] == far) or (k in ("out_one", "in_zero") and v > far and p[k] == far), (k, p[k], v)
    gg, _, hh = mr.params(g, f)
    m = mr.case_input("shrink_smooth")[:1]
    r = mr.mask_shape(m, g, f)
    one, zero = mr.decide_on_integers(r["inside"], r["d2_out"], r["d2_in"], p)
    assert np.array_equal(one, r["one"]) and np.array_equal(zero, r["zero"])
    n = np.arange(1, far + 1, dtype=np.int64)          # every D2 an outside / inside pixel can have
    for ins in (False, True):
        inside = np.full(n.shape, ins)
        s = mr.signed_distance(inside, n, n)
        one, zero = mr.decide_on_integers(inside, n, n, p)
        assert np.array_equal(one, s <= gg) and np.array_equal(zero, ~(s <= gg) & (s >= hh)), (g, f, ins)
    # R decides every pixel: FAR is exactly 1 on inside pixels and exactly 0 on outside pixels, never on the ramp
    assert far >= p["in_one"] and far >= p["out_zero"] and far > p["out_one"] and far > p["in_zero"]


def test_planner_refusals():
    nan, inf = float("nan"), float("inf")
    for g, f in ((32.5, 0.0), (-32.5, 0.0), (0.0, -0.5), (0.0, 32.5), (nan, 1.0), (1.0, nan), (inf, 0.0), (0.0, inf), (-inf, 0.0), (UP(32.0), 0.0),
                 (0.0, UP(32.0)), (DN(-32.0), 0.0)):
        assert _plan(g, f)[0] == -1, (g, f)
        with pytest.raises(ValueError):
            mr.check_limits(g, f)
    _, lib = _lib()
    assert lib.insv2v_mask_shape_plan(1.0, 1.0, None) == -1


# ------------------------------------------------------------------------------------------------------------------ 3. properties
def _disc_dilation(ins, g):
    """x is in the result iff some inside pixel lies within distance g (g >= 0), by pairs."""
    H, W = ins.shape
    out = ins.copy()
    for y, x in zip(*np.nonzero(ins)):
        for yy in range(H):
            for xx in range(W):
                if (yy - y) ** 2 + (xx - x) ** 2 <= g * g:
                    out[yy, xx] = True
    return out


def test_properties():
    m = mr.case_input("shrink_smooth")
    b = (m > mr.TAU).astype(np.float32)
    r = mr.mask_shape(b, 0.0, 0.0)
    assert np.array_equal(r["shaped"], b.astype(np.float64)) and np.array_equal(r["support"], b.astype(np.float64))   # the identity
    for g in (1.0, 1.5, mr.SQRT2, 2.0, 3.7):
        grown = mr.mask_shape(b, g, 0.0)["shaped"]
        assert set(np.unique(grown)) <= {0.0, 1.0}
        for t in range(b.shape[0]):
            assert np.array_equal(grown[t] == 1, _disc_dilation(b[t] > 0.5, g)), g
        # Shrinking against growing the complement.  grow(-g) keeps sqrt(D2_in) >= g + 1, the complement of grow(g) of the complement
        # keeps sqrt(D2_in) > g.  With the offset by one in s the two are the same set wherever no lattice distance lies strictly
        # between g and g + 1 - every integer g on a 1-D frame (asserted exactly below), every straight axis-aligned edge - and in 2-D
        # the shrink is the tighter one, by exactly the pixels with g < sqrt(D2_in) < g + 1 (diagonal neighbours of the outside).
        r = mr.mask_shape(b, -g, 0.0)
        shrunk, dual = r["shaped"], 1.0 - mr.mask_shape(1.0 - b, g, 0.0)["shaped"]
        assert (shrunk <= dual).all(), g
        between = r["inside"] & (np.sqrt(r["d2_in"]) > g) & (np.sqrt(r["d2_in"]) < g + 1)
        assert np.array_equal(shrunk != dual, between), g
    for name in ("row", "column"):   # 1-D frames: every distance is an integer
        b1 = (mr.case_input(name) > mr.TAU).astype(np.float32)
        for g in (1.0, 2.0, 3.0):
            assert np.array_equal(mr.mask_shape(b1, -g, 0.0)["shaped"], 1.0 - mr.mask_shape(1.0 - b1, g, 0.0)["shaped"]), (name, g)
            assert mr.mask_shape(b1, -1.0, 0.0)["shaped"].any()
    gs = [-3.0, -2.0, -0.5, 0.0, 0.5, 1.0, 2.5, 6.0]
    for prof in mr.PROFILES:
        prev = None
        for g in gs:   # monotone in g, pixel by pixel
            cur = mr.mask_shape(m, g, 3.0, profile=prof)
            assert prev is None or (cur["shaped"] >= prev).all(), (prof, g)
            assert np.array_equal(cur["support"] == 1, cur["shaped"] > 0) and ((cur["shaped"] >= 0) & (cur["shaped"] <= 1)).all()
            assert (cur["shaped"][cur["ramp"]] > 0).all() and (cur["shaped"][cur["ramp"]] < 1).all()
            assert (cur["shaped"][cur["s"] <= g] == 1).all()                     # the feather never takes anything from the full-edit region
            prev = cur["shaped"]
    lin, smo = (mr.mask_shape(m, 1.0, 6.0, profile=p) for p in mr.PROFILES)
    u = lin["shaped"][lin["ramp"]]
    assert np.allclose(smo["shaped"][smo["ramp"]], u * u * (3 - 2 * u), rtol=0, atol=1e-15) and np.array_equal(lin["ramp"], smo["ramp"])


# ------------------------------------------------------------------------------------------------------------------ 4. planted misreadings
def _metric_distance(hit, R, combine):
    """The separable transform of another metric: min over dx of combine(|dx|, v(x + dx)), squared; > R^2 -> FAR."""
    H, W = hit.shape
    far = (R + 1) ** 2
    v = mr._vertical(hit, R + 1)
    d = np.full((H, W), far, dtype=np.int64)
    for dx in range(-R, R + 1):
        if abs(dx) >= W:
            continue
        lo, hi = max(0, -dx), min(W, W - dx)
        d[:, lo:hi] = np.minimum(d[:, lo:hi], combine(abs(dx), v[:, lo + dx:hi + dx]) ** 2)
    return np.where(d > R * R, far, d)


def _finish(ins, d2o, d2i, g, f, profile, *, s_inside_offset=1.0, feather_inside=False, support_at_half=False):
    """The reference's second half with the misreadings as switches."""
    gg, ff, hh = mr.params(g, f)
    s = np.where(ins, s_inside_offset - np.sqrt(d2i.astype(np.float64)), np.sqrt(d2o.astype(np.float64)))
    lo, hi = (gg - ff, gg) if feather_inside else (gg, hh)
    one = s <= lo
    zero = ~one & (s >= hi)
    ramp = ~one & ~zero
    shaped = one.astype(np.float64)
    if ramp.any():
        u = (hi - s[ramp]) / ff
        shaped[ramp] = np.clip(u if profile == "linear" else u * u * (3 - 2 * u), mr.RAMP_LO, mr.RAMP_HI)
    support = (shaped >= 0.5) if support_at_half else (shaped > 0)
    return dict(shaped=shaped, support=support.astype(np.float64), d2_out=d2o, d2_in=d2i)


def _misread(kind, m, g, f, profile):
    R, far = mr.radius(g, f)
    with np.errstate(invalid="ignore"):
        ins = (m >= np.float32(mr.TAU)) if kind == "ge_threshold" else mr.inside_set(m, mr.TAU)
    if kind in ("chessboard", "city_block"):
        comb = (lambda a, v: np.maximum(a, v)) if kind == "chessboard" else (lambda a, v: a + v)
        d2o = np.stack([_metric_distance(x, R, comb) for x in ins])
        d2i = np.stack([_metric_distance(~x, R, comb) for x in ins])
    elif kind == "border_outside":
        pad = np.pad(ins, ((0, 0), (R + 1, R + 1), (R + 1, R + 1)), constant_values=False)
        d2o = np.stack([mr.squared_distance(x, R) for x in ins])
        d2i = np.stack([mr.squared_distance(~x, R) for x in pad])[:, R + 1:-(R + 1), R + 1:-(R + 1)]
    elif kind == "far_leaks":   # the search radius forgets the feather: beyond it the ramp is evaluated on FAR
        Rs = max(int(math.ceil(max(mr.params(g, f)[0], 1.0))), 1)
        d2o = np.stack([mr.squared_distance(x, Rs) for x in ins])
        d2i = np.stack([mr.squared_distance(~x, Rs) for x in ins])
        return _finish(ins, d2o, d2i, g, f, profile)
    else:
        d2o = np.stack([mr.squared_distance(x, R) for x in ins])
        d2i = np.stack([mr.squared_distance(~x, R) for x in ins])
    return _finish(ins, d2o, d2i, g, f, profile, s_inside_offset=0.0 if kind == "off_by_one" else 1.0, feather_inside=kind == "feather_inside",
                   support_at_half=kind == "support_at_half")


MISREADINGS = ["chessboard", "city_block", "border_outside", "ge_threshold", "feather_inside", "support_at_half", "off_by_one", "far_leaks"]


@pytest.fixture(scope="module")
def case_refs():
    return {c[0]: mr.case_reference(c[0]) for c in mr.CASES}


def _caught(r, bad, bound):
    if any(not np.array_equal(bad[k], r[k]) for k in ("d2_out", "d2_in", "support")):
        return True
    return bool(np.abs(bad["shaped"] - r["shaped"]).max() > 10 * bound)


def test_the_correct_reading_is_not_caught(case_refs):
    for name, T, H, W, g, f, profile in mr.CASES:
        m, r = case_refs[name]
        assert not _caught(r, _misread("none", m, g, f, profile), mr.ramp_bound(r, g, f, profile)[0]), name


@pytest.mark.parametrize("kind", MISREADINGS)
def test_planted_misreadings_are_caught_on_the_gpu_files_inputs(kind, case_refs):
    """Each misreading differs from the reference in at least one pixel of d2_out, d2_in or support, or by more than 10 bounds in shaped."""
    caught = []
    for name, T, H, W, g, f, profile in mr.CASES:
        m, r = case_refs[name]
        if _caught(r, _misread(kind, m, g, f, profile), mr.ramp_bound(r, g, f, profile)[0]):
            caught.append(name)
    print(f"[mask_shape] misreading {kind}: caught by {caught}")
    assert caught, kind
    # where each one must show: the inside half of s is read only when the edge moves inwards, the border only where a mask touches it
    assert {"off_by_one": "shrink_smooth", "border_outside": "row_tiles"}.get(kind, "special_frames") in caught, kind


def test_the_gpu_cases_cover_what_they_claim(case_refs):
    L, _ = _lib()
    tile = _plan(1.0, 1.0)[1]["row_tile"]
    m, r = case_refs["row_tiles"]
    ins = r["inside"]
    W = m.shape[2]
    for b in range(tile, W, tile):   # an inside pixel on both sides of every row-tile boundary
        assert ins[:, :, b - 1].any() and ins[:, :, b].any(), b
    assert ins[:, 0].any() and ins[:, -1].any() and ins[:, :, 0].any() and ins[:, :, -1].any()
    far = mr.radius(32.0, 32.0)[1]
    assert (r["d2_out"] == far).any() and r["ramp"].any() and r["one"].any() and r["zero"].any()
    m, r = case_refs["special_frames"]
    assert not r["inside"][0].any() and r["inside"][1].all() and np.isnan(m[2]).any() and (m[2] == mr.TAU).any()
    assert r["inside"][3].sum() == 1 and r["inside"][3, -1, -1]
    assert not r["inside"][2][np.isnan(m[2]) | (m[2] == mr.TAU)].any()
    R = mr.radius(20.0, 12.0)[0]
    assert R > 9 and R > 13
    for name in ("shrink_smooth", "feather_max_smooth", "row", "column", "special_frames"):
        assert case_refs[name][1]["ramp"].any(), name
    assert case_refs["shrink_smooth"][1]["one"].any()   # the blob survives the shrink


# ------------------------------------------------------------------------------------------------------------------ 5. argument checks
def test_check_shape_args():
    from insv2v.mask_shape import check_shape_args, check_mask_shape, MASK_SHAPE_KEYS
    assert MASK_SHAPE_KEYS == ("grow", "feather", "threshold", "profile")
    par = inspect.signature(check_shape_args).parameters
    assert {k: par[k].default for k in MASK_SHAPE_KEYS} == dict(grow=0.0, feather=0.0, threshold=0.5, profile="smooth")
    for ok in (dict(), dict(grow=32, feather=32), dict(grow=-32, feather=0), dict(grow=-32.0, feather=32.0), dict(threshold=0.0), dict(threshold=-1.5),
               dict(profile="linear"), dict(grow=1.5, feather=0.25, threshold=0.3, profile="smooth")):
        check_shape_args(**ok)
        check_mask_shape(ok)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(grow=32.5), dict(grow=-33), dict(feather=-0.1), dict(feather=33), dict(grow=nan), dict(feather=nan), dict(grow=inf),
                dict(feather=inf), dict(threshold=nan), dict(threshold=inf), dict(threshold="0.5"), dict(grow="4"), dict(grow=True),
                dict(feather=None), dict(profile="cosine"), dict(profile=1), dict(profile=None)):
        with pytest.raises(ValueError):
            check_shape_args(**bad)
        with pytest.raises(ValueError, match="mask_shape"):
            check_mask_shape(bad)
    for bad in (dict(blur=3), [("grow", 1)], "grow", 4.0, dict(grow=1, dilate=2)):
        with pytest.raises(ValueError, match="mask_shape"):
            check_mask_shape(bad)


def test_check_edit_args_and_the_drivers_refuse_before_anything_runs():
    from insv2v.run_loveu_tgve import check_edit_args, edit_video, edit_videos
    assert inspect.signature(check_edit_args).parameters["mask_shape"].default is None
    assert inspect.signature(edit_video).parameters["mask_shape"].default is None
    T, H, W = 4, 32, 48
    shape = (1, T, 3, H, W)
    frames = torch.zeros(shape)
    M = torch.ones((1, T, H, W))
    f = torch.zeros((T - 1, 2, H, W))
    check_edit_args(shape, M, mask_shape=dict(grow=2, feather=4))
    check_edit_args(shape, M[:, :1], mask_shape={})
    check_edit_args(shape, "auto", mask_shape=dict(feather=8.0, profile="linear"))
    check_edit_args(shape, M[:, :1], mask_key=1, mask_flows=dict(fwd=f, bwd=f), mask_shape=dict(grow=-1))
    cases = [dict(mask=None, mask_shape={}), dict(mask=None, mask_shape=dict(grow=1)), dict(mask=M, mask_shape=dict(blur=2)),
             dict(mask=M, mask_shape=dict(grow=40)), dict(mask=M, mask_shape=dict(feather=-1)), dict(mask=M, mask_shape=dict(profile="box")),
             dict(mask=M, mask_shape=dict(threshold=float("nan"))), dict(mask=M, mask_shape=[2, 4]), dict(mask="auto", mask_shape=dict(grow=float("inf"))),
             dict(mask=M, mask_shape=True), dict(mask=torch.ones((1, T + 1, H, W)), mask_shape={})]
    for kw in cases:
        with pytest.raises(ValueError, match="mask"):
            check_edit_args(shape, kw["mask"], mask_shape=kw["mask_shape"])
        with pytest.raises(ValueError, match="mask"):   # model and pipe are never touched
            edit_video(None, None, frames, None, None, **kw)
        with pytest.raises(ValueError, match="mask"):
            edit_videos(None, None, [dict(frames=frames), dict(frames=frames, **kw)])


def test_ops_mask_shape_refuses_on_the_host():
    from insv2v import ops, _lib
    par = inspect.signature(ops.mask_shape).parameters
    assert [par[k].default for k in ("grow", "feather", "threshold", "profile", "return_d2")] == [0.0, 0.0, 0.5, "smooth", False]
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("grow", "feather", "threshold", "profile", "return_d2"))
    with pytest.raises(_lib.HipKernelError):
        ops.mask_shape(torch.zeros((2, 8, 8)))   # a CPU tensor
    with pytest.raises(_lib.HipKernelError):
        ops.mask_shape_plan(40.0, 0.0)
    assert ops.mask_shape_plan(4.0, 8.0) == dict(R=12, far=169, out_one=16, out_zero=144, in_one=0, in_zero=-1, row_tile=256)


def test_entry_refuses_bad_arguments_before_any_launch():
    """The argument checks run on the host in front of the launch: the addresses below are never dereferenced."""
    L, lib = _lib()
    T, H, W = 2, 5, 7
    n = T * H * W * 4
    need = lib.insv2v_mask_shape_workspace_bytes(T, H, W)
    assert need >= T * H * W and need % 4 == 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 5, 5), (1 << 20, 1 << 20, 1 << 20), (1 << 30, 4, 1)):
        assert lib.insv2v_mask_shape_workspace_bytes(*bad) == -1, bad
    assert lib.insv2v_mask_shape_workspace_bytes(1, 1, 1) == 4 and lib.insv2v_mask_shape_workspace_bytes(1, 1 << 20, 1 << 11) == 1 << 31
    base = dict(m=0x100000, shaped=0x200000, support=0x300000, d2_out=0x400000, d2_in=0x500000, workspace=0x600000, workspace_bytes=need,
                T=T, H=H, W=W, threshold=0.5, grow=2.0, feather=3.0, profile=1)

    def call(**kw):
        d = L.MaskShapeDesc()
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        return lib.insv2v_mask_shape(ctypes.byref(d), None)
    assert lib.insv2v_mask_shape(None, None) == -1
    nan, inf = float("nan"), float("inf")
    for k in ("m", "shaped", "support", "workspace"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(T=0), dict(H=0), dict(W=0), dict(T=-2), dict(grow=32.5), dict(grow=-32.5), dict(feather=-1.0), dict(feather=33.0), dict(grow=nan),
               dict(feather=nan), dict(grow=inf), dict(feather=-inf), dict(threshold=nan), dict(threshold=inf), dict(threshold=-inf), dict(profile=2),
               dict(profile=-1), dict(workspace_bytes=need - 1), dict(workspace_bytes=-1), dict(workspace=0x600001), dict(workspace=0x600002)):
        assert call(**kw) == -1, kw
    outs = ("shaped", "support", "d2_out", "d2_in", "workspace")
    for i, out in enumerate(outs):
        for other in ("m",) + outs[:i]:
            assert call(**{out: base[other]}) == -1, (out, other)
            assert call(**{out: base[other] + n - 4}) == -1, (out, other)                  # the last element of the other
            if out != "workspace":
                assert call(**{out: base[other] - n + 4}) == -1, (out, other)              # the last element of this output


# ------------------------------------------------------------------------------------------------------------------ 6. masks from images
def _png(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)


def test_load_mask_file_and_directory(tmp_path):
    from insv2v.video_io import load_mask
    H, W = 16, 24
    rng = np.random.default_rng(5)
    planes = [rng.integers(0, 256, size=(H, W), dtype=np.uint8) for _ in range(3)]
    planes[0][:4] = 0
    planes[0][-4:] = 255
    _png(tmp_path / "one.png", planes[0])
    m = load_mask(str(tmp_path / "one.png"), (W, H))
    assert m.shape == (1, 1, H, W) and m.dtype == torch.float32
    assert torch.equal(m[0, 0], torch.from_numpy(planes[0]).float() / 255.0) and m.min() == 0.0 and m.max() == 1.0
    rgb = np.stack([planes[1]] * 3, axis=-1)        # a colour file is read as grey
    _png(tmp_path / "rgb.png", rgb)
    assert torch.equal(load_mask(str(tmp_path / "rgb.png"), (W, H))[0, 0], torch.from_numpy(planes[1]).float() / 255.0)
    d = tmp_path / "frames"
    d.mkdir()
    for name, p in zip(("b_002.png", "a_010.png", "b_001.png"), planes):   # sorted by name: a_010, b_001, b_002
        _png(d / name, p)
    (d / "notes.txt").write_text("not an image")
    m = load_mask(str(d), (W, H))
    assert m.shape == (1, 3, H, W)
    for got, want in zip(m[0], (planes[1], planes[2], planes[0])):
        assert torch.equal(got, torch.from_numpy(want).float() / 255.0)
    # the frames' bilinear resize: PIL's, to (W, H)
    from PIL import Image
    big = load_mask(str(tmp_path / "one.png"), (2 * W, 2 * H))
    want = np.asarray(Image.fromarray(planes[0]).convert("L").resize((2 * W, 2 * H), Image.BILINEAR), dtype=np.uint8)
    assert big.shape == (1, 1, 2 * H, 2 * W) and torch.equal(big[0, 0], torch.from_numpy(want.copy()).float() / 255.0)
    empty = tmp_path / "empty"
    empty.mkdir()
    for bad in (str(empty), str(tmp_path / "missing.png")):
        with pytest.raises(FileNotFoundError):
            load_mask(bad, (W, H))
    # a wrong frame count is refused where every mask is checked
    from insv2v.run_loveu_tgve import check_edit_args
    check_edit_args((1, 3, 3, H, W), m)
    with pytest.raises(ValueError, match="mask"):
        check_edit_args((1, 4, 3, H, W), m)


def test_cli(tmp_path):
    from insv2v.run_loveu_tgve import build_parser, check_args, mask_shape_unit, load_mask_image, mask_region
    p = build_parser()
    a = check_args(p.parse_args([]))
    assert (a.mask_grow, a.mask_feather, a.mask_profile, a.mask_threshold, a.mask_image) == (None,) * 5
    assert mask_shape_unit(a) == {} and load_mask_image(a, 8, 8) is None
    a = check_args(p.parse_args(["--synthetic", "2", "--synthetic-mask", "--mask-grow", "4", "--mask-feather", "8", "--mask-out", "m.pt"]))
    assert mask_shape_unit(a) == dict(mask_shape=dict(grow=4.0, feather=8.0))
    a = check_args(p.parse_args(["--units", "u.pt", "--mask-profile", "linear", "--mask-threshold", "0.25"]))
    assert mask_shape_unit(a) == dict(mask_shape=dict(profile="linear", threshold=0.25))
    check_args(p.parse_args(["--auto-mask", "--mask-feather", "6"]))
    _png(tmp_path / "m.png", np.full((8, 8), 255, np.uint8))
    img = str(tmp_path / "m.png")
    a = check_args(p.parse_args(["--mask-image", img, "--mask-grow", "-2"]))
    assert load_mask_image(a, 16, 8).shape == (1, 1, 8, 16)
    check_args(p.parse_args(["--mask-image", img, "--mask-key", "0", "--raft-ckpt", "raft.pt"]))   # usable with --mask-key
    for other in (["--mask-file", "m.pt"], ["--synthetic", "1", "--synthetic-mask"], ["--auto-mask"]):
        with pytest.raises(SystemExit, match="--mask-image"):
            check_args(p.parse_args(["--mask-image", img] + other))
    with pytest.raises(SystemExit, match="--mask-image"):
        check_args(p.parse_args(["--mask-image", str(tmp_path / "none.png")]))
    with pytest.raises(SystemExit, match="shape a mask"):
        check_args(p.parse_args(["--mask-grow", "2"]))
    with pytest.raises(SystemExit, match="shape a mask"):
        check_args(p.parse_args(["--synthetic", "2", "--mask-feather", "2"]))
    for bad in (["--mask-grow", "40"], ["--mask-feather", "-1"], ["--mask-profile", "box"], ["--mask-threshold", "nan"]):
        with pytest.raises(SystemExit, match="--mask-grow / --mask-feather"):
            check_args(p.parse_args(["--auto-mask"] + bad))
    with pytest.raises(SystemExit, match="--mask-out"):   # still: --mask-out needs a run that computes masks
        check_args(p.parse_args(["--mask-out", "m.pt", "--mask-file", "m.pt"]))
    check_args(p.parse_args(["--mask-out", "m.pt", "--mask-file", "m.pt", "--mask-feather", "4"]))
    est = dict(mask=torch.zeros(1), shaped=torch.ones(1))
    assert mask_region(est, None) is est["shaped"] and mask_region(dict(mask=est["mask"]), None) is est["mask"] and mask_region(None, 5) == 5


def test_write_masks_holds_the_shaped_mask(tmp_path):
    from insv2v.run_loveu_tgve import write_masks
    T, H, W = 2, 8, 16
    shaped, support = torch.rand((1, T, H, W)), torch.ones((1, T, H, W))
    recs = {3: dict(shaped=shaped, support=support), 1: dict(mask=torch.zeros((1, T, H, W)), valid=torch.ones((T, H, W)), flow_to_key=torch.zeros((T, 2, H, W)),
                                                             shaped=shaped, support=support), 2: None}
    write_masks(str(tmp_path / "m.pt"), recs)
    got = torch.load(str(tmp_path / "m.pt"))
    assert sorted(got) == [1, 3] and set(got[3]) == {"shaped", "support"} and set(got[1]) == {"mask", "valid", "shaped", "support"}
    assert torch.equal(got[3]["shaped"], shaped[0]) and got[1]["valid"].shape == (T, H, W) and got[1]["mask"].shape == (T, H, W)


# ------------------------------------------------------------------------------------------------------------------ 7. drivers on the host
from driver_fakes import Model as _Model, RecordingPipe as _RecordingPipe   # noqa: E402


def test_a_call_without_mask_shape_is_what_it_was(monkeypatch):
    """The pipe sees exactly the keywords it saw before the feature existed, and the shaping entry is never reached."""
    from insv2v import ops
    from insv2v.run_loveu_tgve import edit_video, edit_videos
    monkeypatch.setattr(ops, "mask_shape", lambda *a, **k: (_ for _ in ()).throw(AssertionError("ops.mask_shape was reached")))
    frames = torch.rand((1, 20, 3, 16, 24)) * 2 - 1
    tc = torch.zeros((1, 77, 8))
    first = ["img_cfg", "img_cond", "latent", "text_cfg", "text_cond", "text_uncond"]
    second = sorted(first + ["latent_ref", "noise_correct_step"])
    pipe = _RecordingPipe()
    out = edit_video(_Model(), pipe, frames, tc, tc)
    assert out.shape == frames.shape and pipe.calls == [("call", first), ("second", second)]
    assert edit_video(_Model(), _RecordingPipe(), frames, tc, tc, return_mask=True)[1] is None
    pipe = _RecordingPipe()
    outs = edit_videos(_Model(), pipe, [dict(frames=frames, text_cond=tc, text_uncond=tc) for _ in range(2)])
    assert len(outs) == 2 and pipe.calls == [("stacked", [first, first], []), ("stacked", [second, second], [])]


# ------------------------------------------------------------------------------------------------------------------ 8. the C ABI
def header_text():
    return open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()


def _c_struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(void|float|int64_t|int32_t)\s*(\*?)\s*(.*)", decl)
        ctype = ("ptr" if m.group(3) or "*" in m.group(4) else m.group(2))
        for var in m.group(4).split(","):
            fields.append((var.strip().lstrip("*").strip(), ctype))
    return fields


@pytest.mark.parametrize("cname,pyname", [("insv2v_mask_shape_desc", "MaskShapeDesc"), ("insv2v_mask_shape_plan_t", "MaskShapePlan")])
def test_ctypes_structs_mirror_the_header(cname, pyname):
    from insv2v import _lib
    want = _c_struct_fields(cname)
    kind = {ctypes.c_void_p: "ptr", ctypes.c_int64: "int64_t", ctypes.c_int32: "int32_t", ctypes.c_float: "float"}
    got = [(n, kind[t]) for n, t in getattr(_lib, pyname)._fields_]
    assert got == want


def test_header_lib_and_build_hold_the_new_entries():
    L, lib = _lib()
    import build
    text = header_text()
    for name in ("insv2v_mask_shape", "insv2v_mask_shape_plan", "insv2v_mask_shape_workspace_bytes"):
        assert re.search(r"^\s*(?:int|int64_t)\s+%s\s*\(" % name, text, flags=re.M), name
        assert name in L.SIGNATURES and getattr(lib, name) is not None
    assert "mask_shape.hip" in build.SOURCES
    assert lib.insv2v_abi_version() == L.ABI_VERSION == 15    # an addition to ABI 15
    assert (L.MASK_SHAPE_MAX, L.MASK_PROFILES) == (32, ("linear", "smooth"))
    assert re.search(r"#define INSV2V_MASK_SHAPE_MAX 32\b", text) and re.search(r"#define INSV2V_MASK_PROFILE_LINEAR 0\b", text) \
        and re.search(r"#define INSV2V_MASK_PROFILE_SMOOTH 1\b", text)
    src = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "mask_shape.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and "malloc" not in src.lower()   # plain loads and stores, nothing allocated
