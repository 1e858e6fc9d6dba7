"""Editing a region at full resolution, without a GPU: the float64 definition of tests/region_ref.py against ``interpolate``, the plan's
rules pinned by value, the planted misreadings, the drivers with fakes, and the agreement of header, ctypes and wrappers."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import region_ref as rr
from driver_fakes import Model, RecordingPipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the definition
# (n_in, n_out): ratios 8, 2.67, 1, 1/3 and 1/8; x takes entry i, y entry (i + 2) % 5, so every case mixes two ratios
AXES = [(64, 8), (64, 24), (24, 24), (8, 24), (3, 24)]


@pytest.mark.parametrize("kind", ["bicubic", "bilinear"])
@pytest.mark.parametrize("i", range(len(AXES)))
def test_reference_is_interpolate_on_the_crop(kind, i):
    (bw, w), (bh, h) = AXES[i], AXES[(i + 2) % len(AXES)]
    x = rr.uniform(f"region.cpu.{i}", (2, 3, 80, 90)).astype(np.float64)
    box = (11, 7, 11 + bw, 7 + bh)
    want = F.interpolate(torch.from_numpy(x)[..., box[1]:box[3], box[0]:box[2]], size=(h, w), mode=kind, antialias=True, align_corners=False).numpy()
    got = rr.resample(x, box, (w, h), kind)
    err = np.abs(got - want).max()
    print(f"[region] {kind} {bw}x{bh} -> {w}x{h}: max |reference - interpolate| = {err:.3e}")
    assert got.shape == want.shape and err <= 1e-12


@pytest.mark.parametrize("kind", ["bicubic", "bilinear"])
def test_equal_size_is_bit_for_bit(kind):
    x = rr.uniform("region.cpu.equal", (2, 3, 45, 70))
    box = (46, 29, 70, 45)
    for dtype in (np.float64, np.float32):
        got = rr.resample(x, box, (24, 16), kind, dtype=dtype)
        assert np.array_equal(got, x[..., 29:45, 46:70].astype(dtype))
    for i, (xmin, w) in enumerate(rr.axis_taps(24, 24, kind)):      # every weight is exactly 0, except the 1 on the pixel itself
        assert [float(v) for v in w] == [1.0 if xmin + j == i else 0.0 for j in range(len(w))]


def test_the_measured_constant_of_the_bound():
    """K of the GPU tests' bound K 2^-24 sum |w||x|: the worst ratio of the fp32 emulation to the float64 definition over the GPU
    tests' own inputs is what region_ref pins (6.71, recorded as 6.8); the tests use 4 x that."""
    x = rr.uniform("region.src", rr.SRC_SHAPE)
    worst = max(rr.measured_k(x, box, size, kind) for _, box, size in rr.RESAMPLE_CASES for kind in ("bicubic", "bilinear"))
    print(f"[region] measured K = {worst:.3f}, pinned {rr.K_MEASURED}, factor {rr.K_FACTOR}")
    assert 0.5 * rr.K_MEASURED < worst <= rr.K_MEASURED and rr.K_FACTOR == 4.0


def test_mask_bbox_reference():
    m = np.zeros((3, 9, 13), np.float32)
    m[0, 2:5, 3:7] = 1.0
    m[1, 8, 12] = 0.75
    m[2, 4, 4] = 0.5          # exactly at the threshold: outside
    m[2, 0, 1] = np.nan       # a NaN is outside
    b = rr.mask_bbox(m)
    assert b.tolist() == [[3, 2, 7, 5], [12, 8, 13, 9], [13, 9, 0, 0], [3, 2, 13, 9]]
    assert rr.mask_bbox(m, wrong="ge_threshold")[2].tolist() == [4, 4, 5, 5]


# ------------------------------------------------------------------------------------------------------------------ the plan
def test_region_plan_rules_by_value():
    from insv2v.region import region_plan
    # a box that must widen: 20 x 40 mask, pad 0.25 -> grow 10 -> 40 x 60, aspect 1 -> 60 x 60, centred on the mask
    p = region_plan((200, 300), (64, 64), bbox=(100, 50, 120, 90))
    assert p["box"] == (80, 40, 140, 100) and p["size"] == (64, 64) and p["frame"] == (200, 300) and p["ratio"] == (60 / 64, 60 / 64) and p["anisotropy"] == 1.0
    # too flat for 3 : 2: 60 x 10, pad 0 -> 60 x 40
    assert region_plan((200, 300), (48, 32), bbox=(100, 50, 160, 60), pad=0)["box"] == (100, 35, 160, 75)
    # an odd difference: the extra pixel goes to the far side
    assert region_plan((200, 300), (64, 64), bbox=(100, 50, 121, 90), pad=0)["box"] == (91, 50, 131, 90)
    # one that hits a frame border and shifts inside
    assert region_plan((200, 300), (64, 64), bbox=(280, 150, 300, 190))["box"] == (240, 140, 300, 200)
    assert region_plan((200, 300), (64, 64), bbox=(0, 0, 20, 40))["box"] == (0, 0, 60, 60)
    # wider than the frame in one dimension: the whole frame there, the anisotropy reported
    # (120 x 80, grow 30 -> 180 x 140 -> 180 x 180; 180 rows do not fit the 100 of the frame)
    p = region_plan((100, 300), (64, 64), bbox=(100, 10, 220, 90), pad=0.25)
    assert p["box"] == (70, 0, 250, 100) and p["ratio"] == (180 / 64, 100 / 64) and p["anisotropy"] == 1.8
    # the whole frame, an explicit box
    assert region_plan((75, 110), (48, 32))["box"] == (0, 0, 110, 75)
    assert region_plan((75, 110), (48, 32), box=(3, 5, 50, 70), bbox=(0, 0, 1, 1))["box"] == (3, 5, 50, 70)
    # 1080 x 1920, size (384, 384): a 96 x 54 mask -> grow 24 -> 144 x 102 -> 144 x 144
    p = region_plan((1080, 1920), (384, 384), bbox=(900, 500, 996, 554))
    assert p["box"] == (876, 455, 1020, 599) and p["ratio"] == (0.375, 0.375)
    p = region_plan((1080, 1920), (384, 384))
    assert p["box"] == (0, 0, 1920, 1080) and p["ratio"] == (5.0, 2.8125) and abs(p["anisotropy"] - 16 / 9) < 1e-15
    for case in [dict(frame_hw=(200, 300), size=(64, 64), bbox=(100, 50, 120, 90)), dict(frame_hw=(100, 300), size=(64, 64), bbox=(100, 10, 220, 90)),
                 dict(frame_hw=(75, 110), size=(48, 32)), dict(frame_hw=(1080, 1920), size=(384, 384), bbox=(1900, 1000, 1920, 1080), pad=0.5)]:
        assert region_plan(**case)["box"] == rr.region_plan(**case)


def test_region_plan_refusals():
    from insv2v.region import region_plan
    with pytest.raises(ValueError, match=r"the mask is empty in the 300x200 frame"):
        region_plan((200, 300), (64, 64), bbox=(300, 200, 0, 0))
    for size in ((60, 64), (64, 0), (-8, 8)):
        with pytest.raises(ValueError, match=rf"working size {size[0]}x{size[1]} must be positive multiples of 8"):
            region_plan((200, 300), size)
    with pytest.raises(ValueError, match=r"box \(5, 5, 5, 9\) is empty"):
        region_plan((200, 300), (64, 64), box=(5, 5, 5, 9))
    with pytest.raises(ValueError, match=r"box \(5, 5, 301, 9\) is not inside the 300x200 frame"):
        region_plan((200, 300), (64, 64), box=(5, 5, 301, 9))
    with pytest.raises(ValueError, match=r"box of 1920x1080 pixels and a working size of 64x64 differ by more than a factor of 8"):
        region_plan((1080, 1920), (64, 64))
    with pytest.raises(ValueError, match=r"box of 7x7 pixels and a working size of 64x64"):
        region_plan((200, 300), (64, 64), box=(0, 0, 7, 7))
    assert region_plan((200, 300), (64, 64), box=(0, 0, 8, 8))["ratio"] == (0.125, 0.125)      # the limits themselves run
    assert region_plan((512, 512), (64, 64))["ratio"] == (8.0, 8.0)


def test_check_region():
    from insv2v.region import check_region, REGION_KEYS, REGION_DEFAULTS
    assert REGION_KEYS == ("size", "box", "pad", "mode", "blend", "threshold")
    assert REGION_DEFAULTS == dict(size=(384, 384), box=None, pad=0.25, mode="residual", blend=8, threshold=0.5) and check_region(True) == REGION_DEFAULTS
    assert check_region(dict(size=[32, 48], box=[1, 2, 3, 4], mode="replace"))["box"] == (1, 2, 3, 4)
    assert check_region(dict(box="frame"))["box"] == "frame"
    for bad in (False, None, dict(sise=(8, 8)), dict(size=(8,)), dict(size=(8.0, 8)), dict(size=(12, 8)), dict(box=(1, 2, 3)), dict(box="mask"),
                dict(pad=-0.1), dict(pad=float("nan")), dict(pad=True), dict(mode="warp"), dict(blend=-1), dict(blend=float("inf")), dict(threshold="0.5")):
        with pytest.raises(ValueError):
            check_region(bad)


# ------------------------------------------------------------------------------------------------------------------ planted misreadings
def _resample_gap(name, case, kind, source=None):
    x = rr.uniform("region.src", rr.SRC_SHAPE) if source is None else source
    _, box, size = next(c for c in rr.RESAMPLE_CASES if c[0] == case)
    ref, other = rr.resample(x, box, size, kind), rr.resample(x, box, size, kind, wrong=name)
    return rr.need_gap(name, ref, other, rr.resample_bound(x, box, size, kind).max())


def test_the_inputs_tell_every_misreading_from_the_definition():
    gaps = {}
    gaps["a075"] = _resample_gap("a075", "middle_non_integer", "bicubic")
    gaps["no_antialias"] = _resample_gap("no_antialias", "top_left_ratio_8", "bicubic")
    gaps["unnormalised"] = _resample_gap("unnormalised", "whole_24x16", "bilinear")
    gaps["align_corners"] = _resample_gap("align_corners", "top_right_ratio_third", "bicubic")
    gaps["frame_clip"] = _resample_gap("frame_clip", "middle_non_integer", "bicubic")
    # the clamp on down_src: a source of +-1 blocks, up-sampled - the cubic overshoots
    n, C, H, W = rr.SRC_SHAPE
    blocks = np.where(((np.arange(H)[:, None] // 4 + np.arange(W)[None, :] // 4) % 2) == 0, 1.0, -1.0).astype(np.float32) * np.ones((n, C, 1, 1), np.float32)
    _, box, size = next(c for c in rr.RESAMPLE_CASES if c[0] == "top_right_ratio_third")
    gaps["no_down_clamp"] = rr.need_gap("no_down_clamp", rr.down_src(blocks, box, size), rr.down_src(blocks, box, size, wrong="no_down_clamp"),
                                        rr.resample_bound(blocks, box, size, "bicubic").max())
    # the paste: the ramp at a frame border, the mask in residual mode
    src, edit, down, mask = rr.paste_inputs("region.paste", zero_half=True)      # the inputs of the GPU paste tests
    box = rr.PASTE_BOXES["two_borders"]
    gaps["ramp_at_border"] = rr.need_gap("ramp_at_border", rr.paste(src, edit, down, box, "residual", 3), rr.paste(src, edit, down, box, "residual", 3, wrong="ramp_at_border"),
                                         rr.paste_bound(src, edit, down, box, "residual").max())
    gaps["mask_twice"] = rr.need_gap("mask_twice", rr.paste(src, edit, down, box, "residual", 3, mask), rr.paste(src, edit, down, box, "residual", 3, mask, wrong="mask_twice"),
                                     rr.paste_bound(src, edit, down, box, "residual").max())
    m = np.zeros((2, 9, 13), np.float32)
    m[0, 2:5, 3:7], m[1, 7, 11], m[1, 1, 1] = 1.0, 0.5, 0.75
    assert not np.array_equal(rr.mask_bbox(m), rr.mask_bbox(m, wrong="ge_threshold"))
    gaps["ge_threshold"] = 1.0
    print("[region] misreading gaps: " + ", ".join(f"{k} {v:.3e}" for k, v in gaps.items()))
    assert set(gaps) == set(rr.MISREADINGS)


def test_ramp_and_paste_reference():
    assert np.array_equal(rr.ramp((37, 53), (0, 0, 53, 37), 3), np.ones((37, 53)))            # the whole frame: no ramp
    r = rr.ramp((37, 53), (0, 0, 30, 20), 4)
    assert r[0, 0] == 1.0 and r[19, 0] == 0.125 and r[0, 29] == 0.125 and r[18, 28] == 0.375 and r[10, 10] == 1.0
    assert np.array_equal(rr.ramp((37, 53), (9, 6, 45, 31), 0), np.ones((25, 36)))
    src, edit, down, mask = rr.paste_inputs("region.paste", zero_half=True)
    box = rr.PASTE_BOXES["middle"]
    out = rr.paste(src, edit, down, box, "residual", 3)
    x0, y0, x1, y1 = box
    outside = np.ones(src.shape, bool)
    outside[..., y0:y1, x0:x1] = False
    assert np.array_equal(out[outside], src.astype(np.float64)[outside])
    cols = [bx for bx, (a, b) in enumerate(rr.footprint(rr.PASTE_SIZE[0], x1 - x0, "bicubic")) if a >= rr.PASTE_SIZE[0] // 2]
    assert len(cols) > 5 and np.array_equal(out[..., y0:y1, x0 + cols[0]:x1], src.astype(np.float64)[..., y0:y1, x0 + cols[0]:x1])
    assert not np.array_equal(out[..., y0:y1, x0:x0 + cols[0]], src.astype(np.float64)[..., y0:y1, x0:x0 + cols[0]])


# ------------------------------------------------------------------------------------------------------------------ the drivers, with fakes
class _Ops:
    """CPU stand-ins of the three entries, computed by the reference; every call is recorded."""

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


@pytest.fixture
def fake_ops(monkeypatch):
    from insv2v import ops
    fake = _Ops()
    for name in ("mask_bbox", "region_resample", "region_paste"):
        monkeypatch.setattr(ops, name, getattr(fake, name))
    return fake


def _source(name, T=3, H=75, W=110):
    return torch.from_numpy(rr.uniform(name, (1, T, 3, H, W)))


def _rect(T, H, W, box):
    m = torch.zeros((1, T, H, W))
    m[:, :, box[1]:box[3], box[0]:box[2]] = 1.0
    return m


def test_edit_region_calls_edit_video_once_with_the_working_clip(fake_ops, monkeypatch):
    from insv2v import region, run_loveu_tgve
    seen = []

    def fake_edit_video(model, pipe, frames, text_cond, text_uncond, **kw):
        seen.append(dict(kw, frames=frames, text=(text_cond, text_uncond), model=model, pipe=pipe))
        out = (frames * 0.5,) + (("latent",) if kw.get("return_latent") else ()) + (((dict(mask=kw["mask"]) if "mask" in kw else None),) if kw.get("return_mask") else ())
        return out if len(out) > 1 else out[0]
    monkeypatch.setattr(run_loveu_tgve, "edit_video", fake_edit_video)
    frames, M = _source("region.cpu.drv"), _rect(3, 75, 110, (40, 30, 60, 50))
    model, pipe = Model(), RecordingPipe()
    reg = dict(size=(48, 32), blend=3)
    flows = dict(fwd="f", bwd="b")
    got = region.edit_region(model, pipe, frames, "tc", "tu", region=reg, mask=M, seed=7, unit=3, strength=0.5, stabilize=True, stabilize_flows=flows,
                             text_cfg=5.0, return_latent=True)
    assert len(seen) == 1
    kw = seen[0]
    plan = region.region_plan((75, 110), (48, 32), bbox=(40, 30, 60, 50))
    assert plan["box"] == (28, 25, 73, 55)   # 20 x 20, grow 5 -> 30 x 30 -> 45 x 30 for 3 : 2
    assert kw["frames"].shape == (1, 3, 3, 32, 48) and kw["mask"].shape == (1, 3, 32, 48) and kw["text"] == ("tc", "tu") and kw["model"] is model and kw["pipe"] is pipe
    assert {k: kw[k] for k in ("seed", "unit", "strength", "stabilize", "text_cfg", "return_latent")} == dict(seed=7, unit=3, strength=0.5, stabilize=True, text_cfg=5.0, return_latent=True)
    assert kw["stabilize_flows"] is flows and "return_mask" not in kw and "region" not in kw
    assert [c[0] for c in fake_ops.calls] == ["mask_bbox", "region_resample", "region_resample", "region_paste"]
    assert fake_ops.calls[1][2:] == (plan["box"], (48, 32), "bicubic", (-1.0, 1.0)) and fake_ops.calls[2][2:] == (plan["box"], (48, 32), "bilinear", None)
    assert fake_ops.calls[3][1:] == ((3, 3, 75, 110), plan["box"], "residual", 3, None)
    image, latent = got
    assert latent == "latent" and image.shape == frames.shape
    down = rr.down_src(frames[0].numpy(), plan["box"], (48, 32))
    assert np.allclose(kw["frames"][0].numpy(), down, atol=1e-6)
    want = rr.paste(frames[0].numpy(), kw["frames"][0].numpy() * 0.5, kw["frames"][0].numpy(), plan["box"], "residual", 3)
    assert np.allclose(image[0].numpy(), want, atol=1e-6)
    # replace mode asks the inner edit for its mask and returns it only when the caller asked; return_mask gains ``region``
    del seen[:], fake_ops.calls[:]
    got = region.edit_region(model, pipe, frames, "tc", "tu", region=dict(reg, mode="replace", box=(10, 10, 60, 40)), mask=M)
    assert torch.is_tensor(got) and seen[0]["return_mask"] is True and fake_ops.calls[-1][1:] == ((3, 3, 75, 110), (10, 10, 60, 40), "replace", 3, (3, 32, 48))
    assert [c[0] for c in fake_ops.calls] == ["region_resample", "region_resample", "region_paste"]      # an explicit box: no mask_bbox
    got = region.edit_region(model, pipe, frames, "tc", "tu", region=reg, return_mask=True)
    assert set(got[1]) == {"region"} and set(got[1]["region"]) == {"box", "size", "working", "down_src"} and got[1]["region"]["box"] == (0, 0, 110, 75)


def test_edit_regions_makes_one_edit_videos_call_for_sources_of_different_size(fake_ops, monkeypatch):
    from insv2v import region, run_loveu_tgve
    seen = []

    def fake_edit_videos(model, pipe, units, **kw):
        seen.append((units, kw))
        return [u["frames"] * 0.25 for u in units]
    monkeypatch.setattr(run_loveu_tgve, "edit_videos", fake_edit_videos)
    a, b = _source("region.cpu.a"), _source("region.cpu.b", H=61, W=97)
    units = [dict(frames=a, text_cond="a", text_uncond="u", unit=0, mask=_rect(3, 75, 110, (40, 30, 60, 50)), region=dict(size=(48, 32))),
             dict(frames=b, text_cond="b", text_uncond="u", unit=1, region=dict(size=(48, 32), box=(5, 7, 80, 50)), text_cfg=3.0)]
    outs = region.edit_regions(Model(), RecordingPipe(), units, seed=11, max_clips=4)
    assert len(seen) == 1
    inner, kw = seen[0]
    assert kw == dict(seed=11, max_clips=4) and [tuple(u["frames"].shape) for u in inner] == [(1, 3, 3, 32, 48)] * 2
    assert all("region" not in u for u in inner) and inner[0]["mask"].shape == (1, 3, 32, 48) and "mask" not in inner[1] and inner[1]["text_cfg"] == 3.0
    assert [tuple(o.shape) for o in outs] == [tuple(a.shape), tuple(b.shape)]
    assert torch.equal(outs[1][..., :7, :], b[..., :7, :]) and not torch.equal(outs[1][..., 7:50, 5:80], b[..., 7:50, 5:80])
    assert region.edit_regions(Model(), RecordingPipe(), []) == []


def test_a_mask_made_inside_the_inner_edit_needs_a_box(fake_ops, monkeypatch):
    from insv2v import region, run_loveu_tgve
    monkeypatch.setattr(run_loveu_tgve, "edit_video", lambda model, pipe, frames, tc, tu, **kw: frames)
    frames = _source("region.cpu.auto")
    for kw in (dict(mask="auto"), dict(mask=torch.ones((1, 1, 75, 110)), mask_key=1)):
        del fake_ops.calls[:]
        with pytest.raises(ValueError, match="the box cannot be derived"):
            region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32)), **kw)
        assert fake_ops.calls == []
        for box in ((4, 4, 100, 70), "frame"):
            assert region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32), box=box), **kw).shape == frames.shape
    with pytest.raises(ValueError, match="the mask is empty"):
        region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32)), mask=torch.zeros((1, 3, 75, 110)))
    with pytest.raises(ValueError, match=r"must be a floating-point \[1,3,75,110\]"):
        region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", mask=torch.zeros((1, 3, 32, 48)))


# ------------------------------------------------------------------------------------------------------------------ header, ctypes, wrappers
def test_header_lib_and_ops_agree_on_the_three_entries():
    from insv2v import _lib
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    assert "int insv2v_region_resample(const insv2v_region_resample_desc* d, insv2v_stream_t stream);" in header
    assert "int insv2v_region_paste(const insv2v_region_paste_desc* d, insv2v_stream_t stream);" in header
    decl = re.search(r"int insv2v_mask_bbox\((.*?)\);", header, re.S).group(1)
    assert [a.strip().rsplit(" ", 1)[0].replace("const ", "") for a in decl.replace("\n", " ").split(",")] == \
        ["float*", "int64_t", "int64_t", "int32_t", "int32_t", "int32_t", "float", "int32_t*", "insv2v_stream_t"]
    c = _lib
    assert _lib.SIGNATURES["insv2v_mask_bbox"] == (c.c_i32, [c.c_p, c.c_i64, c.c_i64, c.c_i32, c.c_i32, c.c_i32, c.c_f32, c.c_p, c.c_p])
    for name, desc in (("resample", _lib.RegionResampleDesc), ("paste", _lib.RegionPasteDesc)):
        assert _lib.SIGNATURES[f"insv2v_region_{name}"][1][0]._type_ is desc
        fields = re.search(rf"typedef struct insv2v_region_{name}_desc \{{(.*?)\}} insv2v_region_{name}_desc;", header, re.S).group(1)
        declared = [n for line in fields.split("\n") for n in re.findall(r"[\s*](\w+)\s*[,;]", line.split("/*")[0])]
        assert declared == [n for n, _ in desc._fields_]
        ctype = {"int32_t": c.c_i32, "int64_t": c.c_i64, "float": c.c_f32}
        for line in fields.split("\n"):
            line = line.split("/*")[0].strip()
            if line:
                t = c.c_p if "*" in line else ctype[line.split()[0]]
                for n in re.findall(r"[\s*](\w+)\s*[,;]", line):
                    assert dict(desc._fields_)[n] is t, (name, n)
    for i, n in enumerate(("BICUBIC", "BILINEAR")):
        assert f"#define INSV2V_REGION_{n} {i}" in header
    for i, n in enumerate(("RESIDUAL", "REPLACE")):
        assert f"#define INSV2V_REGION_{n} {i}" in header
    assert _lib.REGION_FILTERS == ("bicubic", "bilinear") and _lib.REGION_MODES == ("residual", "replace")
    assert _lib.ABI_VERSION == 15 and "additions to ABI 15: no existing struct or entry changes" in header.split("INSV2V_REGION_BICUBIC")[0][-4000:]
    assert "int insv2v_abi_version(void) { return 15; }" in open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "elementwise.hip")).read()
    sys.path.insert(0, os.path.join(ROOT, "instruct-video-to-video_amd"))
    try:
        import build
    finally:
        sys.path.pop(0)
    assert "region.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "region.hip"))
    import insv2v
    from insv2v import ops, region
    assert all(callable(getattr(ops, n)) for n in ("mask_bbox", "region_resample", "region_paste"))
    assert insv2v.edit_region is region.edit_region and insv2v.edit_regions is region.edit_regions and insv2v.region_plan is region.region_plan
    src = open(os.path.join(build.CSRC, "region.hip")).read()
    assert 'extern "C" int insv2v_mask_bbox(' in src and 'extern "C" int insv2v_region_resample(' in src and 'extern "C" int insv2v_region_paste(' in src


# ------------------------------------------------------------------------------------------------------------------ the command line
def test_region_unit_and_the_refusals_of_check_args(tmp_path):
    from insv2v.run_loveu_tgve import build_parser, check_args, region_unit, region_est
    base = ["--synthetic", "1", "--synthetic-tiny", "--image-size", "32"]
    parse = lambda extra: check_args(build_parser().parse_args(base + extra))   # noqa: E731
    assert region_unit(parse([])) == {}
    assert region_unit(parse(["--region"])) == dict(region=dict(size=(32, 32)))
    a = parse(["--region", "--region-box", "3", "4", "50", "60", "--region-pad", "0.5", "--region-mode", "replace", "--region-blend", "2", "--region-source", "110", "75"])
    assert region_unit(a) == dict(region=dict(size=(32, 32), box=(3, 4, 50, 60), pad=0.5, mode="replace", blend=2.0)) and a.region_source == [110, 75]
    assert region_unit(a, 64)["region"]["size"] == (64, 64)
    # a mask made inside the working-resolution edit takes the whole frame unless a box is given
    assert region_unit(parse(["--region", "--auto-mask"]))["region"]["box"] == "frame"
    assert region_unit(parse(["--region", "--synthetic-mask", "--mask-key", "1"]))["region"]["box"] == "frame"
    assert region_unit(parse(["--region", "--auto-mask", "--region-box", "1", "2", "30", "40"]))["region"]["box"] == (1, 2, 30, 40)
    for extra, msg in ((["--region-box", "1", "2", "3", "4"], "parameters of --region"), (["--region-pad", "0.5"], "parameters of --region"),
                       (["--region-mode", "replace"], "parameters of --region"), (["--region-blend", "0"], "parameters of --region"),
                       (["--region-source", "64", "64"], "parameters of --region"), (["--region", "--region-mode", "warp"], "mode must be"),
                       (["--region", "--region-pad", "-1"], "pad must be"), (["--region", "--region-blend", "-2"], "blend must be"),
                       (["--region", "--region-source", "0", "64"], "--region-source W H")):
        with pytest.raises(SystemExit, match=msg):
            parse(extra)
    with pytest.raises(SystemExit, match="multiples of 8"):
        check_args(build_parser().parse_args(["--synthetic", "1", "--image-size", "36", "--region"]))
    with pytest.raises(SystemExit, match="--region-source W H"):
        check_args(build_parser().parse_args(["--units", "u.pt", "--region", "--region-source", "64", "64"]))
    est = dict(mask=1, shaped=2, support=3, keys=[0], confidence=4)
    assert region_est(parse([]), est) is est and region_est(parse(["--region"]), est) == dict(keys=[0], confidence=4) and region_est(parse(["--region"]), None) is None


def test_the_loaders_keep_the_native_size(tmp_path):
    from PIL import Image
    from insv2v.video_io import load_mask, LoveuTgveVideoDataset
    png = np.zeros((21, 34), np.uint8)
    png[5:9, 7:20] = 255
    Image.fromarray(png).save(tmp_path / "m.png")
    m = load_mask(str(tmp_path / "m.png"), None)
    assert m.shape == (1, 1, 21, 34) and torch.equal(m[0, 0], torch.from_numpy(png).float() / 255.0)
    assert load_mask(str(tmp_path / "m.png"), (16, 8)).shape == (1, 1, 8, 16)
    root = tmp_path / "data"
    (root / "DAVIS_480p" / "480p_videos" / "clip").mkdir(parents=True)
    rgb = (np.arange(21 * 34 * 3) % 251).astype(np.uint8).reshape(21, 34, 3)
    for t in range(2):
        Image.fromarray(rgb).save(root / "DAVIS_480p" / "480p_videos" / "clip" / f"{t:03d}.png")
    (root / "LOVEU-TGVE-2023_Dataset.csv").write_text("Video name,Original,Style,Object,Background,Multiple\nDAVIS Videos:,,,,,\nclip,a,b,c,d,e\n")
    native = LoveuTgveVideoDataset(str(root), image_size=None)["clip"]["frames"]
    assert native.shape == (2, 3, 21, 34) and torch.equal(native[0], (torch.from_numpy(rgb).permute(2, 0, 1).float() / 255.0 - 0.5) / 0.5)
    assert LoveuTgveVideoDataset(str(root), image_size=(16, 8))["clip"]["frames"].shape == (2, 3, 8, 16)
