"""Region edits that follow the object on the GPU: ``insv2v_region_resample_track`` and
``insv2v_region_paste_track`` against the float64 definition of ``region_track_ref`` and against the static entries of section 26, and the
drivers with ``track=`` on a tiny synthetic model.  ``[region_track]`` lines: python -m pytest tests/test_region_track_gpu.py -m gpu -s."""
import ctypes

import numpy as np
import pytest
import torch

import region_ref as rr
import region_track_ref as tr
from test_model_gpu import tiny_unet, report   # noqa: F401  (tiny_unet: the module-scoped fixture, instantiated for this module)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EAGER = dict(use_graph=False)
NAN = float("nan")
PAD = 5


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _view_in_nan(values):
    """A strided [n,C,H,W] view of ``values`` inside a NaN-filled parent (PAD elements around every plane's rows and columns)."""
    n, C, H, W = values.shape
    parent = torch.full((n, C, H + 2 * PAD, W + 2 * PAD), NAN, device=DEV)
    view = parent[:, :, PAD:PAD + H, PAD:PAD + W]
    view.copy_(_dev(values))
    return parent, view


def _sentinel(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 74,), NAN, device=DEV)
    outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    outside[37:37 + n] = False
    return buf, buf[37:37 + n].view(shape), outside


def _outside_covers(shape, boxes):
    out = np.ones(shape, bool)
    for i, b in enumerate(boxes):
        X0, Y0, X1, Y1 = tr.cover(b)
        out[i, :, Y0:Y1, X0:X1] = False
    return out


# ------------------------------------------------------------------------------------------------------------------ the resample
@pytest.fixture(scope="module")
def source():
    x = rr.uniform("region_track.src", tr.SRC_SHAPE)
    parent, view = _view_in_nan(x)
    return x, parent, view


def test_the_emulations_ratio():
    print(f"[region_track] K = {tr.K_FACTOR} x {tr.K_MEASURED}: the worst ratio of the fp32 numpy emulation to the float64 definition over the cases below, "
          "measured on the CPU (test_region_track_cpu.py recomputes it)")


@pytest.mark.parametrize("kind", ["bicubic", "bilinear"])
@pytest.mark.parametrize("name", [c[0] for c in tr.RESAMPLE_CASES])
def test_resample_track_vs_reference(source, name, kind):
    from insv2v import ops
    x, _, view = source
    _, boxes, size, clamp = next(c for c in tr.RESAMPLE_CASES if c[0] == name)
    n, C = x.shape[:2]
    buf, out, outside = _sentinel((n, C, size[1], size[0]))
    ops.region_resample_track(view, boxes, size, mode=kind, clamp=clamp, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[outside]).all()), "written outside the destination"
    got, ref, bound = out.cpu().numpy().astype(np.float64), tr.resample_track(x, boxes, size, kind, clamp=clamp), tr.resample_bound(x, boxes, size, kind)
    err = np.abs(got - ref)
    print(f"[region_track] resample {name} {kind}: -> {size}, max err {err.max():.3e}, worst err / bound {np.max(err / bound):.3f}")
    assert np.isfinite(got).all() and bool((err <= bound).all()), f"{name} {kind}: off by up to {np.max(err / bound):.2f} of the bound"
    if clamp is not None:
        free = tr.resample_track(x, boxes, size, kind)
        assert kind == "bilinear" or (np.abs(free).max() > clamp[1] and got.max() == clamp[1] and got.min() == clamp[0])


def test_a_nan_stays_a_nan_under_the_clamp():
    from insv2v import ops
    x = rr.uniform("region_track.nan", (1, 1, 20, 24))
    x[0, 0, 10, 12] = NAN
    out = ops.region_resample_track(_dev(x), [(2.5, 3.25, 20.5, 17.25)], (16, 8), clamp=(-1.0, 1.0)).cpu()
    assert bool(torch.isnan(out).any()) and not bool(torch.isnan(out).all()) and float(out[~torch.isnan(out)].abs().max()) <= 1.0


INT_BOXES = [(13, 9, 58, 38), (0, 0, 64, 40), (46, 29, 110, 75)]       # different sizes per frame, two at frame borders


def test_integer_boxes_are_the_static_entries_bit_for_bit(source):
    from insv2v import ops
    x, _, view = source
    boxes = [tuple(float(v) for v in b) for b in INT_BOXES]
    for kind, size, clamp in (("bicubic", (24, 16), None), ("bilinear", (24, 16), None), ("bicubic", (65, 17), (-0.5, 0.5)), ("bicubic", (8, 8), None)):
        got = ops.region_resample_track(view, boxes, size, mode=kind, clamp=clamp)
        for i, b in enumerate(INT_BOXES):
            assert torch.equal(got[i:i + 1], ops.region_resample(view[i:i + 1], b, size, mode=kind, clamp=clamp)), (kind, size, i)
    src, edit, down, mask = tr.paste_inputs("region_track.anchor")
    pboxes = [rr.PASTE_BOXES["two_borders"], rr.PASTE_BOXES["middle"], rr.PASTE_BOXES["half"]]
    for mode in ("residual", "replace"):
        for blend, m in ((3, mask), (0, None)):
            got = ops.region_paste_track(_dev(src), _dev(edit), _dev(down), [tuple(float(v) for v in b) for b in pboxes], mode=mode, blend=blend,
                                         mask_w=None if m is None else _dev(m))
            for i, b in enumerate(pboxes):
                want = ops.region_paste(_dev(src[i:i + 1]), _dev(edit[i:i + 1]), _dev(down[i:i + 1]), b, mode=mode, blend=blend, mask_w=None if m is None else _dev(m[i:i + 1]))
                assert torch.equal(got[i:i + 1], want), (mode, blend, i)
            assert not torch.equal(got, _dev(src))


def test_more_frames_than_one_launch_takes():
    """65 frames with a different box each: frames 63 and 64, either side of the launch boundary, against the definition."""
    from insv2v import ops
    x = rr.uniform("region_track.chunk", tr.CHUNK_SHAPE)
    out = ops.region_resample_track(_dev(x), tr.CHUNK_BOXES, tr.CHUNK_SIZE).cpu().numpy().astype(np.float64)
    edit = rr.uniform("region_track.chunk.edit", (65, 1, tr.CHUNK_SIZE[1], tr.CHUNK_SIZE[0]), -0.4, 0.4)
    down = np.zeros_like(edit)
    pasted = ops.region_paste_track(_dev(x * 0.5), _dev(edit), _dev(down), tr.CHUNK_BOXES, blend=2).cpu().numpy()
    for t in (0, 63, 64):
        sl, boxes = slice(t, t + 1), tr.CHUNK_BOXES[t:t + 1]
        err = np.abs(out[sl] - tr.resample_track(x[sl], boxes, tr.CHUNK_SIZE, "bicubic"))
        bound = tr.resample_bound(x[sl], boxes, tr.CHUNK_SIZE, "bicubic")
        perr = np.abs(pasted[sl] - tr.paste_track(x[sl] * 0.5, edit[sl], down[sl], boxes, "residual", 2))
        pbound = tr.paste_bound(x[sl] * 0.5, edit[sl], down[sl], boxes, "residual")
        inside = ~_outside_covers(x[sl].shape, boxes)
        print(f"[region_track] chunking frame {t}: resample err / bound {np.max(err / bound):.3f}, paste err / bound {np.max(perr[inside] / pbound[inside]):.3f}")
        assert bool((err <= bound).all()) and bool((perr[inside] <= pbound[inside]).all()) and np.array_equal(pasted[sl][~inside], (x[sl] * 0.5)[~inside])
        assert not np.array_equal(pasted[sl], x[sl] * 0.5)


# ------------------------------------------------------------------------------------------------------------------ the paste
def _paste(src, edit, down, boxes, mode, blend, mask):
    """The kernel on a strided view of the source inside a NaN parent -> (result as numpy, the parent's NaNs survived)."""
    from insv2v import ops
    parent, view = _view_in_nan(src)
    ops.region_paste_track(view, _dev(edit), _dev(down), boxes, mode=mode, blend=blend, mask_w=None if mask is None else _dev(mask))
    torch.cuda.synchronize()
    keep = torch.ones(parent.shape, dtype=torch.bool, device=DEV)
    keep[:, :, PAD:PAD + src.shape[2], PAD:PAD + src.shape[3]] = False
    return view.cpu().numpy(), bool(torch.isnan(parent[keep]).all())


@pytest.mark.parametrize("blend", [0, 3])
@pytest.mark.parametrize("mode", ["residual", "replace"])
@pytest.mark.parametrize("where", ["two_borders", "middle", "half", "quarter"])
def test_paste_track_vs_reference(where, mode, blend):
    src, edit, down, mask = tr.paste_inputs("region_track.paste", zero_half=True)
    boxes = tr.PASTE_BOXES[where]
    if where == "two_borders":
        mask = mask[:1]                       # one mask for every frame: [1,h,w]
    got, intact = _paste(src, edit, down, boxes, mode, blend, mask if mode == "replace" else None)
    assert intact
    full = np.broadcast_to(mask, (src.shape[0],) + mask.shape[1:])
    ref, bound = tr.paste_track(src, edit, down, boxes, mode, blend, full), tr.paste_bound(src, edit, down, boxes, mode, full)
    err = np.abs(got.astype(np.float64) - ref)
    outside = _outside_covers(src.shape, boxes)
    assert np.array_equal(got[outside].view(np.int32), src[outside].view(np.int32)), "a pixel outside its frame's cover changed"
    inside = ~outside
    print(f"[region_track] paste {where} {mode} blend {blend}: max err {err.max():.3e}, worst err / bound {np.max(err[inside] / bound[inside]):.3f}")
    assert np.isfinite(got).all() and bool((err[inside] <= bound[inside]).all())
    # the right half of the working clip holds no change (residual) / a zero mask (replace): the cover's pixels whose taps all lie there
    # - by the reference's footprints - are the source's
    w = tr.PASTE_SIZE[0]
    changed = 0
    for i, b in enumerate(boxes):
        X0, Y0, X1, Y1 = tr.cover(b)
        fp = tr.up_taps(b[0], b[2], w, "bicubic" if mode == "residual" else "bilinear")
        cols = [X0 + k for k, (m, wt) in enumerate(fp) if m >= w // 2]
        assert len(cols) >= 1 and cols == list(range(cols[0], X1))
        assert np.array_equal(got[i, :, Y0:Y1, cols[0]:X1].view(np.int32), src[i, :, Y0:Y1, cols[0]:X1].view(np.int32)), "a pixel whose taps see no change is not the source's"
        changed += not np.array_equal(got[i, :, Y0:Y1, X0:cols[0]], src[i, :, Y0:Y1, X0:cols[0]])
    assert changed == len(boxes)


def test_paste_of_a_constant_residual_is_the_ramp_in_closed_form():
    c, blend = 0.25, 3
    src, edit, down, _ = tr.paste_inputs("region_track.paste.const", constant=c)
    src = (src * 0.5).astype(np.float32)          # |src| + c < 1: nothing clips
    boxes = tr.PASTE_BOXES["two_borders"]         # frames 0, 1: top and left frame border; frame 2: bottom and right
    got, intact = _paste(src, edit, down, boxes, "residual", blend, None)
    assert intact
    bound = tr.paste_bound(src, edit, down, boxes, "residual")
    want = src.astype(np.float64).copy()
    for i, (x0, y0, x1, y1) in enumerate(boxes):
        X0, Y0, X1, Y1 = tr.cover(boxes[i])
        cx, cy = np.arange(X0, X1)[None, :] + 0.5, np.arange(Y0, Y1)[:, None] + 0.5
        d = np.minimum(x1 - cx, y1 - cy) if i < 2 else np.minimum(cx - x0, cy - y0)      # only the edges that are no frame borders count
        want[i, :, Y0:Y1, X0:X1] += np.clip(d / blend, 0.0, 1.0) * c
    assert bool((np.abs(got - want) <= bound).all())
    assert abs(float(got[0, 0, 0, 0]) - (float(src[0, 0, 0, 0]) + c)) <= bound[0, 0, 0, 0]                                   # a frame corner: the full change
    assert abs(float(got[0, 0, 19, 29]) - (float(src[0, 0, 19, 29]) + c * 0.75 / 3)) <= bound[0, 0, 19, 29]                   # centre 19.5 under y1 = 20.25
    assert got[0, 0, 20, 5] == src[0, 0, 20, 5] and got[0, 0, 5, 30] == src[0, 0, 5, 30] and got[0, 0, 5, 29] != src[0, 0, 5, 29]                                       # centres 20.5 (outside) and 30.5 (on x1 = 30.5: d = 0) keep the source
    assert got[2, 0, 16, 30] == src[2, 0, 16, 30] and got[2, 0, 17, 23] != src[2, 0, 17, 23]                                   # centre 16.5 above y0 = 16.75


# ------------------------------------------------------------------------------------------------------------------ both entries
def test_two_runs_agree_bitwise_also_on_a_second_stream(source):
    from insv2v import ops
    x, _, view = source
    src, edit, down, mask = tr.paste_inputs("region_track.paste")
    boxes = tr.RESAMPLE_CASES[0][1]

    def run():
        outs = [ops.region_resample_track(view, boxes, (65, 17)), ops.region_resample_track(view, boxes, (24, 16), mode="bilinear")]
        for mode in ("residual", "replace"):
            outs.append(ops.region_paste_track(_dev(src), _dev(edit), _dev(down), tr.PASTE_BOXES["middle"], mode=mode, blend=3, mask_w=_dev(mask)))
        return outs
    first, second = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert _same_bits(a, b) and _same_bits(a, c) and bool(torch.isfinite(a).all())


def test_refusals_leave_the_outputs_untouched():
    from insv2v import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n, C, H, W, h, w = 2, 3, 37, 53, 16, 24
    src = torch.rand((n, C, H, W), device=DEV)
    dst, out = torch.full((n, C, h, w), NAN, device=DEV), torch.full((n, C, H, W), NAN, device=DEV)
    edit, down, mask = (torch.rand(s, device=DEV) for s in ((n, C, h, w), (n, C, h, w), (n, h, w)))
    good = [(3.25, 2.5, 40.25, 30.5), (4.0, 2.0, 41.0, 30.0)]
    keep = []

    def arr(boxes):
        a = (ctypes.c_double * (4 * len(boxes)))(*[v for b in boxes for v in b])
        keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p)

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(dst).all()) and bool(torch.isnan(out).all())
    rbase = dict(src=src.data_ptr(), src_stride_n=C * H * W, src_stride_c=H * W, src_stride_h=W, dst=dst.data_ptr(), boxes=arr(good), n=n, C=C, H=H, W=W, h=h, w=w,
                 filter=0, clamp=0, clamp_lo=-1.0, clamp_hi=1.0)
    pbase = dict(edit=edit.data_ptr(), down=down.data_ptr(), mask=mask.data_ptr(), mask_stride_n=h * w, out=out.data_ptr(), out_stride_n=C * H * W,
                 out_stride_c=H * W, out_stride_h=W, boxes=arr(good), n=n, C=C, H=H, W=W, h=h, w=w, mode=0, blend=3.0)

    def call(fn, cls, base, **kw):
        d = cls()
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        return fn(ctypes.byref(d), stream)
    second = lambda b: dict(boxes=arr([good[0], b]))   # noqa: E731  (the bad box is the SECOND frame's: every box is checked before the first launch)
    geometry = [dict(n=0), dict(C=0), dict(H=0), dict(W=0), dict(h=0), dict(w=-8), dict(boxes=None),
                second((NAN, 2.0, 41.0, 30.0)), second((4.0, 2.0, float("inf"), 30.0)), second((4.0, float("-inf"), 41.0, 30.0)),
                second((4.0, 2.0, 4.0, 30.0)), second((4.0, 30.0, 41.0, 2.0)),                                    # empty
                second((-0.25, 2.0, 36.75, 30.0)), second((4.0, 2.0, 53.25, 30.0)), second((4.0, -1e-9, 41.0, 30.0)), second((4.0, 2.0, 41.0, 37.5)),   # outside the frame
                second((4.0, 2.0, 6.75, 30.0)), second((4.0, 2.0, 41.0, 3.875)),                                 # ratios below 1/8: 2.75 -> 24, 1.875 -> 16
                dict(w=4, **second((4.0, 2.0, 41.0, 30.0))), dict(h=3, **second((4.0, 2.0, 41.0, 30.0)))]          # ratios above 8
    for kw in geometry + [dict(src=None), dict(dst=None), dict(filter=2), dict(filter=-1), dict(clamp=2), dict(clamp=1, clamp_lo=1.0, clamp_hi=-1.0),
                          dict(src_stride_h=W - 1), dict(src_stride_n=-1), dict(dst=src.data_ptr() + 64)]:
        assert call(lib.insv2v_region_resample_track, _lib.RegionResampleTrackDesc, rbase, **kw) == -1 and untouched(), kw
    for kw in geometry + [dict(edit=None), dict(out=None), dict(down=None), dict(mode=2), dict(mode=-1), dict(blend=-1.0), dict(blend=NAN),
                          dict(out_stride_h=W - 1), dict(out_stride_c=-1), dict(mode=1, mask_stride_n=h * w - 1), dict(out=edit.data_ptr()),
                          dict(mode=1, out=mask.data_ptr())]:
        assert call(lib.insv2v_region_paste_track, _lib.RegionPasteTrackDesc, pbase, **kw) == -1 and untouched(), kw
    assert lib.insv2v_region_resample_track(None, None) == -1 and lib.insv2v_region_paste_track(None, None) == -1 and untouched()
    out.copy_(src)   # the same descriptors without a fault run
    assert call(lib.insv2v_region_resample_track, _lib.RegionResampleTrackDesc, rbase) == 0 and call(lib.insv2v_region_paste_track, _lib.RegionPasteTrackDesc, pbase) == 0
    assert call(lib.insv2v_region_paste_track, _lib.RegionPasteTrackDesc, pbase, mode=1, down=None, mask=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dst).all()) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def tiny_model(tiny_unet):
    from insv2v import synth, shapes
    from insv2v.vae import AutoencoderKL
    from insv2v.model import InstructP2PVideoModel
    vae = AutoencoderKL(**synth.VAE_TINY, device=DEV).load_state_dict(synth.synth_state_dict(shapes.vae_shapes(**synth.VAE_TINY)))
    return InstructP2PVideoModel(tiny_unet[0], vae)


@pytest.fixture(scope="module")
def pipe(tiny_unet):
    from insv2v.inference import InferenceIP2PVideo
    return InferenceIP2PVideo(tiny_unet[0], scheduler="sde-dpmsolver++", num_ddim_steps=4, **EAGER)


T, HS, WS, SIZE, SEED = 3, 75, 110, (32, 48), 29     # size = (W, H) of the working clip: 32 wide, 48 high
MOVING = [(30 + 7 * t, 20 + t, 52 + 7 * t, 52 + t) for t in range(T)]
COMMON = dict(text_cfg=7.5, video_cfg=1.5)


def _unit(name="a", H=HS, W=WS):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"region_track.ev.frames.{name}", (1, T, 3, H, W), kind="uniform"),
                text_cond=synth.synth_input(f"region_track.ev.tc.{name}", (1, 77, 64)), text_uncond=synth.synth_input("region_track.ev.tu", (1, 77, 64)))


def _moving_mask(H=HS, W=WS):
    m = torch.zeros((1, T, H, W))
    for t, (x0, y0, x1, y1) in enumerate(MOVING):
        m[0, t, y0:y1, x0:x1] = 1.0
    return m


def _outside_is_source(img, u, boxes):
    out = torch.from_numpy(_outside_covers(tuple(u["frames"].shape[1:]), boxes))[None]
    return torch.equal(img.cpu()[out], u["frames"].float()[out])


def test_integer_boxes_for_every_frame_are_the_static_edit(tiny_model, pipe):
    from insv2v.region import edit_region
    u, M, B = _unit(), _moving_mask(), (22, 10, 62, 70)
    run = lambda **kw: edit_region(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], mask=M, seed=SEED, unit=0, **COMMON, **kw)   # noqa: E731
    a, b = run(region=dict(size=SIZE, blend=3), track=dict(boxes=[B] * T)), run(region=dict(size=SIZE, blend=3, box=B))
    assert torch.equal(a, b) and not torch.equal(a.cpu(), u["frames"].float())


@pytest.mark.parametrize("mode", ["residual", "replace"])
def test_edit_region_with_a_track_is_the_three_steps_by_hand(tiny_model, pipe, mode):
    from insv2v.region import edit_region
    from insv2v.region_track import track_plan, crop_to_working_track, paste_back_track
    from insv2v.run_loveu_tgve import edit_video
    u, M = _unit(), _moving_mask()
    img, est = edit_region(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], region=dict(size=SIZE, mode=mode, blend=3), track=dict(smooth=1.0), mask=M,
                           seed=SEED, unit=0, return_mask=True, **COMMON)
    plan = dict(track_plan((HS, WS), SIZE, MOVING, smooth=1.0), mode=mode, blend=3)
    assert est["region"]["boxes"] == plan["boxes"] and est["region"]["travel"] == plan["travel"] > 3 and est["region"]["size"] == SIZE
    assert any(not float(b[0]).is_integer() for b in plan["boxes"]) and len(set(plan["boxes"])) == T
    down, mask_w = crop_to_working_track(u["frames"], M, plan, device=DEV)
    res = edit_video(tiny_model, pipe, down, u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, return_mask=True, mask=mask_w)
    edit_w, inner = res[0].to(torch.float32), res[-1]
    m = None
    if mode == "replace":     # the composite mask the inner edit used, else its mask, else the resampled drawn one (a drawn mask returns no dict)
        m = inner["shaped"] if inner and "shaped" in inner else (inner["mask"] if inner and "mask" in inner else mask_w)
    want = paste_back_track(u["frames"], edit_w, down, plan, mask_w=m, device=DEV)
    assert img.shape == u["frames"].shape and img.dtype == torch.float32 and _same_bits(img, want)
    assert _same_bits(est["region"]["working"], edit_w) and _same_bits(est["region"]["down_src"], down)
    assert _outside_is_source(img, u, plan["boxes"]) and not _outside_is_source(img, u, [(0.0, 0.0, 1.0, 1.0)] * T)
    for t, (x0, y0, x1, y1) in enumerate(MOVING):
        assert float((img[0, t].cpu() - u["frames"][0, t].float())[:, y0:y1, x0:x1].abs().max()) > 1e-2, "nothing was edited under the mask"
    assert bool(torch.isfinite(img).all()) and float(img.abs().max()) <= 1.0


def test_edit_regions_with_a_tracked_and_a_static_unit_is_one_edit_videos(tiny_model, pipe):
    from insv2v.region import edit_region, edit_regions, crop_to_working, paste_back, region_plan
    from insv2v.region_track import track_plan, crop_to_working_track, paste_back_track
    from insv2v.run_loveu_tgve import edit_videos
    ua, ub, M = _unit("a"), _unit("b", 61, 97), _moving_mask()
    ra, rb = dict(size=SIZE, blend=3), dict(size=SIZE, box=(5, 7, 80, 55))
    got = edit_regions(tiny_model, pipe, [dict(ua, unit=0, mask=M, region=ra, track=True, **COMMON), dict(ub, unit=1, region=rb, **COMMON)], seed=SEED)
    pa = dict(track_plan((HS, WS), SIZE, MOVING), mode="residual", blend=3)
    pb = dict(region_plan((61, 97), SIZE, box=(5, 7, 80, 55)), mode="residual", blend=8)
    ca, cb = crop_to_working_track(ua["frames"], M, pa, device=DEV), crop_to_working(ub["frames"], None, pb, device=DEV)
    res = edit_videos(tiny_model, pipe, [dict(ua, frames=ca[0], mask=ca[1], unit=0, **COMMON), dict(ub, frames=cb[0], unit=1, **COMMON)], seed=SEED)
    assert _same_bits(got[0], paste_back_track(ua["frames"], res[0].to(torch.float32), ca[0], pa, device=DEV))
    assert _same_bits(got[1], paste_back(ub["frames"], res[1].to(torch.float32), cb[0], pb, device=DEV))
    assert _outside_is_source(got[0], ua, pa["boxes"]) and not torch.equal(got[0].cpu(), ua["frames"].float()) and not torch.equal(got[1].cpu(), ub["frames"].float())
    alone = [edit_region(tiny_model, pipe, ua["frames"], ua["text_cond"], ua["text_uncond"], region=ra, track=True, mask=M, seed=SEED, unit=0, **COMMON),
             edit_region(tiny_model, pipe, ub["frames"], ub["text_cond"], ub["text_uncond"], region=rb, seed=SEED, unit=1, **COMMON)]
    same = []
    for k, (g, a) in enumerate(zip(got, alone)):
        d = (g.cpu() - a.cpu()).abs()
        same.append(torch.equal(g.cpu(), a.cpu()))
        print(f"[region_track] edit_regions unit {k} vs its own edit_region: equal {same[-1]}, max |diff| {float(d.max()):.3e}, differing pixels {int((d > 0).sum())} of {d.numel()}")
    assert all(same)


def test_stabilize_and_keyframes_pass_through(tiny_model, pipe):
    import pixel_score_ref as pr
    from insv2v.region import edit_region
    from insv2v.region_track import track_plan, crop_to_working_track, paste_back_track
    from insv2v.run_loveu_tgve import edit_video
    u, M = _unit(), _moving_mask()
    tc = pr.translation_video(SIZE[1], SIZE[0], [(1, 0), (0, 1)])
    flows = dict(fwd=torch.from_numpy(tc["fwd"]).float(), bwd=torch.from_numpy(tc["bwd"]).float())
    plan = dict(track_plan((HS, WS), SIZE, MOVING), mode="residual", blend=8)
    down, mask_w = crop_to_working_track(u["frames"], M, plan, device=DEV)
    for name, kw in (("stabilize", dict(stabilize=True, stabilize_flows=flows)), ("keyframes", dict(keyframes=2, key_flows=flows))):
        got = edit_region(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], region=dict(size=SIZE), track=True, mask=M, seed=SEED, unit=0, **COMMON, **kw)
        edit_w = edit_video(tiny_model, pipe, down, u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, mask=mask_w, **kw).to(torch.float32)
        assert _same_bits(got, paste_back_track(u["frames"], edit_w, down, plan, device=DEV)), name
        assert _outside_is_source(got, u, plan["boxes"]) and not torch.equal(got.cpu(), u["frames"].float()), name


def test_cli_synthetic_region_track(tmp_path, monkeypatch):
    """``--region --region-track`` with a ``--mask-file`` the test writes: every frame of the 75 x 110 source is pasted into its own box."""
    from insv2v import run_loveu_tgve, inference, ops
    from insv2v.region_track import track_plan

    class Eager(inference.InferenceIP2PVideo):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **EAGER))
    monkeypatch.setattr(inference, "InferenceIP2PVideo", Eager)
    seen, real = [], ops.region_paste_track

    def spy(out, edit_w, down_src, boxes, **kw):
        seen.append(dict(kw, boxes=list(boxes), out=tuple(out.shape), edit=tuple(edit_w.shape)))
        return real(out, edit_w, down_src, boxes, **kw)
    monkeypatch.setattr(ops, "region_paste_track", spy)
    torch.save({0: _moving_mask()}, tmp_path / "masks.pt")
    run_loveu_tgve.main(["--synthetic", "1", "--synthetic-tiny", "--num-frames", "3", "--image-size", "32", "--steps", "1", "--seed", "5", "--no-stack",
                         "--region", "--region-source", "110", "75", "--region-blend", "2", "--region-track", "--region-track-smooth", "1",
                         "--mask-file", str(tmp_path / "masks.pt"), "--out", str(tmp_path / "track.pt")])
    plan = track_plan((75, 110), (32, 32), MOVING, smooth=1.0)
    assert seen == [dict(mode="residual", blend=2, mask_w=None, boxes=plan["boxes"], out=(3, 3, 75, 110), edit=(3, 3, 32, 32))]
    out = torch.load(tmp_path / "track.pt")
    assert out.shape == (1, 1, 3, 3, 75, 110) and bool(torch.isfinite(out.float()).all())
    frames = (torch.rand((1, 3, 3, 75, 110), generator=torch.Generator().manual_seed(0)) * 2 - 1)
    outside = torch.from_numpy(_outside_covers((3, 3, 75, 110), plan["boxes"]))[None]
    assert torch.equal(out[0].float()[outside], frames.half().float()[outside]) and not torch.equal(out[0].float(), frames.half().float())
