"""Editing a region at full resolution on the GPU: the three entries of csrc/region.hip against the float64 definition of
tests/region_ref.py, their determinism and refusals, and the drivers ``edit_region`` / ``edit_regions`` with the tiny model.

The per-element bound of the resampling is ``K 2^-24 sum |w_y||w_x||x|`` plus one ulp of the result.  K is not tuned to the kernel: the
worst ratio of an fp32 numpy emulation of the definition to the float64 definition over these inputs is 6.71 (``region_ref.K_MEASURED``
= 6.8, recomputed by test_region_cpu.py), and the tests use 4 x that.  The paste's bound adds the roundings of its epilogue
(``region_ref.paste_bound``).  Bounding boxes, the pixels outside a box and the pixels whose taps see no change are exact."""
import numpy as np
import pytest
import torch

import region_ref as rr
from test_model_gpu import tiny_unet, report   # noqa: F401  (tiny_unet: the module-scoped fixture, instantiated for this module)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EAGER = dict(use_graph=False)
STACKED = dict(rms_tol=1e-2, max_tol=4e-2)
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


def _sentinel(shape, fill=NAN, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((n + 74,), fill, device=DEV, dtype=dtype)
    outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    outside[37:37 + n] = False
    return buf, buf[37:37 + n].view(shape), outside


# ------------------------------------------------------------------------------------------------------------------ mask_bbox
def _bbox_masks():
    H, W = 19, 300    # more than one workgroup of 2048 pixels per frame
    corners = np.zeros((4, H, W), np.float32)
    for t, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1))):
        corners[t, y, x] = 1.0
    per_frame = np.zeros((3, H, W), np.float32)
    per_frame[0, 2:5, 3:7], per_frame[1, 11:19, 250:300], per_frame[2, 8, 140:143] = 1.0, 0.9, 0.51
    at_threshold = np.full((2, H, W), 0.5, np.float32)
    at_threshold[1, 7, 9], at_threshold[1, 3, 200] = np.nextafter(np.float32(0.5), np.float32(1)), NAN
    return dict(empty=np.zeros((2, H, W), np.float32), corners=corners, full=np.ones((2, H, W), np.float32), per_frame=per_frame, at_threshold=at_threshold)


@pytest.mark.parametrize("name", ["empty", "corners", "full", "per_frame", "at_threshold"])
def test_mask_bbox_is_exact(name):
    from insv2v import ops
    m = _bbox_masks()[name]
    got = ops.mask_bbox(_dev(m)).cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, rr.mask_bbox(m)), (got, rr.mask_bbox(m))


def test_mask_bbox_on_a_broadcast_and_on_a_strided_view():
    from insv2v import ops
    m = _bbox_masks()["per_frame"]
    one = _dev(m[:1])[None]                                     # [1,1,H,W] serving 4 frames: frame stride 0
    got = ops.mask_bbox(one.expand(1, 4, *m.shape[1:])[0]).cpu().numpy()
    assert np.array_equal(got, rr.mask_bbox(np.repeat(m[:1], 4, 0)))
    parent = torch.full((3, m.shape[1] + 6, m.shape[2] + 11), 1.0, device=DEV)    # a sentinel that would be INSIDE if it were read
    view = parent[:, 2:2 + m.shape[1], 4:4 + m.shape[2]]
    view.copy_(_dev(m))
    buf, out, outside = _sentinel((4, 4), -7, torch.int32)
    ops.mask_bbox(view, out=out)
    assert np.array_equal(out.cpu().numpy(), rr.mask_bbox(m)) and bool((buf[outside] == -7).all())
    assert np.array_equal(ops.mask_bbox(view, threshold=0.6).cpu().numpy(), rr.mask_bbox(m, 0.6))


# ------------------------------------------------------------------------------------------------------------------ region_resample
@pytest.fixture(scope="module")
def source():
    x = rr.uniform("region.src", rr.SRC_SHAPE)
    parent, view = _view_in_nan(x)
    return x, parent, view


@pytest.mark.parametrize("kind", ["bicubic", "bilinear"])
@pytest.mark.parametrize("name", [c[0] for c in rr.RESAMPLE_CASES])
def test_resample_vs_reference(source, name, kind):
    from insv2v import ops
    x, _, view = source
    _, box, size = next(c for c in rr.RESAMPLE_CASES if c[0] == name)
    n, C = x.shape[:2]
    buf, out, outside = _sentinel((n, C, size[1], size[0]))
    ops.region_resample(view, box, size, mode=kind, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[outside]).all()), "written outside the destination"
    got, ref, bound = out.cpu().numpy().astype(np.float64), rr.resample(x, box, size, kind), rr.resample_bound(x, box, size, kind)
    err = np.abs(got - ref)
    print(f"[region] resample {name} {kind}: box {box} -> {size}, max err {err.max():.3e}, worst err / bound {np.max(err / bound):.3f}")
    assert np.isfinite(got).all() and bool((err <= bound).all()), f"{name} {kind}: off by up to {np.max(err / bound):.2f} of the bound"
    if (box[2] - box[0], box[3] - box[1]) == tuple(size):
        assert torch.equal(out, view[:, :, box[1]:box[3], box[0]:box[2]]), "an equal-size box is not copied bit for bit"


def test_resample_clamp(source):
    from insv2v import ops
    n, C, H, W = rr.SRC_SHAPE
    blocks = np.where(((np.arange(H)[:, None] // 4 + np.arange(W)[None, :] // 4) % 2) == 0, 1.0, -1.0).astype(np.float32) * np.ones((n, C, 1, 1), np.float32)
    _, box, size = next(c for c in rr.RESAMPLE_CASES if c[0] == "top_right_ratio_third")
    free = ops.region_resample(_dev(blocks), box, size)
    held = ops.region_resample(_dev(blocks), box, size, clamp=(-1.0, 1.0))
    assert float(free.abs().max()) > 1.01 and float(held.abs().max()) == 1.0 and torch.equal(held, free.clamp(-1, 1))
    err = np.abs(held.cpu().numpy() - rr.down_src(blocks, box, size))
    assert bool((err <= rr.resample_bound(blocks, box, size, "bicubic")).all())


# ------------------------------------------------------------------------------------------------------------------ region_paste
def _paste(src, edit, down, box, mode, blend, mask):
    """The kernel on a strided view of the source inside a NaN parent -> (result as numpy, the parent's NaNs survived)."""
    from insv2v import ops
    parent, view = _view_in_nan(src)
    ops.region_paste(view, _dev(edit), _dev(down), box, mode=mode, blend=blend, mask_w=None if mask is None else _dev(mask))
    torch.cuda.synchronize()
    keep = torch.ones(parent.shape, dtype=torch.bool, device=DEV)
    keep[:, :, PAD:PAD + src.shape[2], PAD:PAD + src.shape[3]] = False
    return view.cpu().numpy(), bool(torch.isnan(parent[keep]).all())


@pytest.mark.parametrize("blend", [0, 3])
@pytest.mark.parametrize("mode", ["residual", "replace"])
@pytest.mark.parametrize("where", ["two_borders", "middle"])
def test_paste_vs_reference(where, mode, blend):
    src, edit, down, mask = rr.paste_inputs("region.paste", zero_half=True)
    box = rr.PASTE_BOXES[where]
    x0, y0, x1, y1 = box
    got, intact = _paste(src, edit, down, box, mode, blend, mask if mode == "replace" else None)
    assert intact
    ref, bound = rr.paste(src, edit, down, box, mode, blend, mask), rr.paste_bound(src, edit, down, box, mode, mask)
    err = np.abs(got.astype(np.float64) - ref)
    outside = np.ones(src.shape, bool)
    outside[..., y0:y1, x0:x1] = False
    assert np.array_equal(got[outside].view(np.int32), src[outside].view(np.int32)), "a pixel outside the box changed"
    inside = ~outside
    print(f"[region] paste {where} {mode} blend {blend}: max err {err.max():.3e}, worst err / bound {np.max(err[inside] / bound[inside]):.3f}")
    assert np.isfinite(got).all() and bool((err[inside] <= bound[inside]).all())
    # the right half of the working clip holds no change (residual) / a zero mask (replace): the box pixels whose taps all lie there
    # - by the reference's footprints - are the source's
    w = rr.PASTE_SIZE[0]
    fp = rr.footprint(w, x1 - x0, "bicubic" if mode == "residual" else "bilinear")
    cols = [x0 + bx for bx, (a, b) in enumerate(fp) if a >= w // 2]
    assert len(cols) >= 5 and cols == list(range(cols[0], x1))
    assert np.array_equal(got[..., y0:y1, cols[0]:x1], src[..., y0:y1, cols[0]:x1]), "a pixel whose taps see no change is not the source's"
    assert not np.array_equal(got[..., y0:y1, x0:cols[0]], src[..., y0:y1, x0:cols[0]])


@pytest.mark.parametrize("mode", ["residual", "replace"])
@pytest.mark.parametrize("where", ["half", "quarter"])
def test_paste_into_a_box_smaller_than_the_working_clip(where, mode):
    """The paste DOWN-samples (ratios 2 and 4): the kernel's two larger stagings."""
    src, edit, down, mask = rr.paste_inputs("region.paste", zero_half=True)
    box = rr.PASTE_BOXES[where]
    x0, y0, x1, y1 = box
    got, intact = _paste(src, edit, down, box, mode, 1, mask if mode == "replace" else None)
    assert intact
    ref, bound = rr.paste(src, edit, down, box, mode, 1, mask), rr.paste_bound(src, edit, down, box, mode, mask)
    err = np.abs(got.astype(np.float64) - ref)
    outside = np.ones(src.shape, bool)
    outside[..., y0:y1, x0:x1] = False
    assert np.array_equal(got[outside].view(np.int32), src[outside].view(np.int32)), "a pixel outside the box changed"
    print(f"[region] paste {where} {mode} blend 1: max err {err.max():.3e}, worst err / bound {np.max(err[~outside] / bound[~outside]):.3f}")
    assert np.isfinite(got).all() and bool((err[~outside] <= bound[~outside]).all())
    assert not np.array_equal(got[..., y0:y1, x0:x1], src[..., y0:y1, x0:x1])


def test_paste_keeps_the_bits_of_a_negative_zero():
    src, edit, down, mask = rr.paste_inputs("region.paste", zero_half=True)
    src[..., 10:20, 30:45] = -0.0
    got, _ = _paste(src, edit, down, rr.PASTE_BOXES["middle"], "residual", 3, None)
    assert np.array_equal(got[..., 10:20, 38:45].view(np.int32), src[..., 10:20, 38:45].view(np.int32)) and np.signbit(got[..., 10:20, 38:45]).all()


def test_paste_of_a_constant_residual_is_the_ramp_in_closed_form():
    c, blend = 0.25, 3
    src, edit, down, _ = rr.paste_inputs("region.paste.const", constant=c)
    src = (src * 0.5).astype(np.float32)          # |src| + c < 1: nothing clips
    box = rr.PASTE_BOXES["two_borders"]           # touches the top and the left frame border: no ramp there
    x0, y0, x1, y1 = box
    got, intact = _paste(src, edit, down, box, "residual", blend, None)
    assert intact
    by, bx = np.arange(y1 - y0)[:, None], np.arange(x1 - x0)[None, :]
    d = np.minimum((x1 - x0) - 1 - bx, (y1 - y0) - 1 - by)            # only the right and the bottom edge count
    want = src.astype(np.float64).copy()
    want[..., y0:y1, x0:x1] += np.minimum(1.0, (d + 0.5) / blend) * c
    bound = rr.paste_bound(src, edit, down, box, "residual")
    assert bool((np.abs(got - want)[..., y0:y1, x0:x1] <= bound[..., y0:y1, x0:x1]).all())
    assert abs(float(got[0, 0, 0, 0]) - (float(src[0, 0, 0, 0]) + c)) <= bound[0, 0, 0, 0]        # a frame corner: the full change
    assert abs(float(got[0, 0, y1 - 1, x1 - 1]) - (float(src[0, 0, y1 - 1, x1 - 1]) + c / 6)) <= bound[0, 0, y1 - 1, x1 - 1]


# ------------------------------------------------------------------------------------------------------------------ all three entries
def test_two_runs_agree_bitwise_also_on_a_second_stream(source):
    from insv2v import ops
    x, _, view = source
    src, edit, down, mask = rr.paste_inputs("region.paste")
    m = _dev(_bbox_masks()["per_frame"])

    def run():
        outs = [ops.mask_bbox(m).float(), ops.region_resample(view, (0, 0, 70, 45), (65, 17)), ops.region_resample(view, (13, 9, 58, 38), (24, 16), mode="bilinear")]
        for mode in ("residual", "replace"):
            outs.append(ops.region_paste(_dev(src), _dev(edit), _dev(down), rr.PASTE_BOXES["middle"], mode=mode, blend=3, mask_w=_dev(mask)))
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
    import ctypes
    from insv2v import _lib
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    n, C, H, W, h, w = 2, 3, 37, 53, 16, 24
    src = torch.rand((n, C, H, W), device=DEV)
    dst, boxes, out = torch.full((n, C, h, w), NAN, device=DEV), torch.full((n + 1, 4), -7, device=DEV, dtype=torch.int32), torch.full((n, C, H, W), NAN, device=DEV)
    edit, down, mask = (torch.rand(s, device=DEV) for s in ((n, C, h, w), (n, C, h, w), (n, h, w)))

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(dst).all()) and bool((boxes == -7).all()) and bool(torch.isnan(out).all())

    def bbox(**kw):
        a = dict(dict(mask=src.data_ptr(), st=H * W, sh=W, T=n, H=H, W=W, thr=0.5, boxes=boxes.data_ptr()), **kw)
        return lib.insv2v_mask_bbox(a["mask"], a["st"], a["sh"], a["T"], a["H"], a["W"], a["thr"], a["boxes"], stream)
    for kw in (dict(mask=None), dict(boxes=None), dict(T=0), dict(H=0), dict(W=-1), dict(sh=W - 1), dict(st=-1), dict(thr=NAN), dict(boxes=src.data_ptr() + 16)):
        assert bbox(**kw) == -1 and untouched(), kw

    rbase = dict(src=src.data_ptr(), src_stride_n=C * H * W, src_stride_c=H * W, src_stride_h=W, dst=dst.data_ptr(), n=n, C=C, H=H, W=W, h=h, w=w,
                 x0=3, y0=2, x1=40, y1=30, filter=0, clamp=0, clamp_lo=-1.0, clamp_hi=1.0)
    pbase = dict(edit=edit.data_ptr(), down=down.data_ptr(), mask=mask.data_ptr(), mask_stride_n=h * w, out=out.data_ptr(), out_stride_n=C * H * W,
                 out_stride_c=H * W, out_stride_h=W, n=n, C=C, H=H, W=W, h=h, w=w, x0=3, y0=2, x1=40, y1=30, mode=0, blend=3.0)

    def call(fn, cls, base, **kw):
        d = cls()
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        return fn(ctypes.byref(d), stream)
    geometry = [dict(n=0), dict(C=0), dict(H=0), dict(W=0), dict(h=0), dict(w=-8), dict(x0=-1), dict(y0=-1), dict(x1=W + 1), dict(y1=H + 1), dict(x1=3), dict(y1=2),
                dict(x0=0, x1=2, w=24), dict(y0=0, y1=1), dict(x0=0, x1=W, y0=0, y1=H, w=6), dict(x0=0, x1=W, y0=0, y1=H, h=4)]   # the last four: ratios beyond 8
    for kw in geometry + [dict(src=None), dict(dst=None), dict(filter=2), dict(filter=-1), dict(clamp=2), dict(clamp=1, clamp_lo=1.0, clamp_hi=-1.0),
                          dict(src_stride_h=W - 1), dict(src_stride_n=-1), dict(dst=src.data_ptr() + 64)]:
        assert call(lib.insv2v_region_resample, _lib.RegionResampleDesc, rbase, **kw) == -1 and untouched(), kw
    for kw in geometry + [dict(edit=None), dict(out=None), dict(down=None), dict(mode=2), dict(mode=-1), dict(blend=-1.0), dict(blend=NAN),
                          dict(out_stride_h=W - 1), dict(out_stride_c=-1), dict(mode=1, mask_stride_n=h * w - 1), dict(out=edit.data_ptr()),
                          dict(mode=1, out=mask.data_ptr()),
                          dict(H=1 << 21, y0=0, y1=16 * 65535 + 16, h=(16 * 65535 + 16) // 8)]:   # more tile rows than a grid holds
        assert call(lib.insv2v_region_paste, _lib.RegionPasteDesc, pbase, **kw) == -1 and untouched(), kw
    assert lib.insv2v_region_resample(None, None) == -1 and lib.insv2v_region_paste(None, None) == -1 and untouched()
    out.copy_(src)   # the same descriptors without a fault run
    assert bbox() == 0 and call(lib.insv2v_region_resample, _lib.RegionResampleDesc, rbase) == 0 and call(lib.insv2v_region_paste, _lib.RegionPasteDesc, pbase) == 0
    assert call(lib.insv2v_region_paste, _lib.RegionPasteDesc, pbase, mode=1, down=None, mask=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dst).all()) and bool((boxes != -7).all()) and bool(torch.isfinite(out).all())


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


def _unit(name="a", H=HS, W=WS):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"region.ev.frames.{name}", (1, T, 3, H, W), kind="uniform"),
                text_cond=synth.synth_input(f"region.ev.tc.{name}", (1, 77, 64)), text_uncond=synth.synth_input("region.ev.tu", (1, 77, 64)))


def _rect(H=HS, W=WS, box=(38, 20, 60, 52)):
    m = torch.zeros((1, T, H, W))
    m[:, :, box[1]:box[3], box[0]:box[2]] = 1.0
    return m


def _by_hand(model, pipe, u, plan, drawn, **kw):
    from insv2v.region import crop_to_working, paste_back
    from insv2v.run_loveu_tgve import edit_video
    down, mask_w = crop_to_working(u["frames"], drawn, plan, device=DEV)
    res = edit_video(model, pipe, down, u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, return_mask=True, **dict(kw, **({} if mask_w is None else dict(mask=mask_w))))
    edit_w, est = res[0].to(torch.float32), res[-1]
    m = None
    if plan["mode"] == "replace":
        m = est["shaped"] if est and "shaped" in est else (est["mask"] if est and "mask" in est else mask_w)
    return paste_back(u["frames"], edit_w, down, plan, mask_w=m, device=DEV), edit_w, down


def _outside_is_source(img, u, box):
    out = torch.ones(u["frames"].shape, dtype=torch.bool)
    out[..., box[1]:box[3], box[0]:box[2]] = False
    return torch.equal(img.cpu()[out], u["frames"].float()[out])


@pytest.mark.parametrize("mode", ["residual", "replace"])
def test_edit_region_is_the_three_steps_by_hand(tiny_model, pipe, mode):
    from insv2v.region import edit_region, region_plan, check_region
    u, M = _unit(), _rect()
    reg = dict(size=SIZE, mode=mode, blend=3)
    got = edit_region(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], region=reg, mask=M, text_cfg=7.5, video_cfg=1.5, seed=SEED, unit=0, return_mask=True)
    img, est = got
    plan = dict(region_plan((HS, WS), SIZE, bbox=(38, 20, 60, 52)), mode=mode, blend=3)
    assert est["region"]["box"] == plan["box"] and est["region"]["size"] == SIZE and check_region(reg)["pad"] == 0.25
    want, edit_w, down = _by_hand(tiny_model, pipe, u, plan, M)
    assert img.shape == u["frames"].shape and img.dtype == torch.float32 and _same_bits(img, want)
    assert _same_bits(est["region"]["working"], edit_w) and _same_bits(est["region"]["down_src"], down) and edit_w.shape == (1, T, 3, SIZE[1], SIZE[0])
    box = plan["box"]
    assert (box[2] - box[0]) * (box[3] - box[1]) < HS * WS // 2 and _outside_is_source(img, u, box)
    inside = (img.cpu() - u["frames"].float())[..., 20:52, 38:60].abs().max()
    assert bool(torch.isfinite(img).all()) and float(inside) > 1e-2, "nothing was edited under the mask"
    assert float(img.abs().max()) <= 1.0


def _region_units():
    ua, ub, M = _unit("a"), _unit("b", 61, 97), _rect()
    common = dict(text_cfg=7.5, video_cfg=1.5)
    ra, rb = dict(size=SIZE, blend=3), dict(size=SIZE, box=(5, 7, 80, 55), mode="replace")
    return (ua, ub), (ra, rb), M, common


@pytest.fixture(scope="module")
def stacked_regions(tiny_model, pipe):
    """ONE ``edit_regions`` call of two units whose sources differ in size, shared by the tests below."""
    from insv2v.region import edit_regions
    (ua, ub), (ra, rb), M, common = _region_units()
    return edit_regions(tiny_model, pipe, [dict(ua, unit=0, mask=M, region=ra, **common), dict(ub, unit=1, region=rb, **common)], seed=SEED, return_mask=True)


def test_edit_regions_is_the_three_steps_by_hand_around_one_edit_videos(tiny_model, pipe, stacked_regions):
    """Bit for bit: every unit of ``edit_regions`` is ``crop_to_working`` -> ONE ``edit_videos`` call on the stacked working clips ->
    ``paste_back`` with the unit's own plan, down_src and mask; outside its box every unit is its source."""
    from insv2v.region import crop_to_working, paste_back, region_plan
    from insv2v.run_loveu_tgve import edit_videos
    (ua, ub), (ra, rb), M, common = _region_units()
    plans = [dict(region_plan((HS, WS), SIZE, bbox=(38, 20, 60, 52)), mode="residual", blend=3),
             dict(region_plan((61, 97), SIZE, box=(5, 7, 80, 55)), mode="replace", blend=8)]
    crops = [crop_to_working(ua["frames"], M, plans[0], device=DEV), crop_to_working(ub["frames"], None, plans[1], device=DEV)]
    inner = [dict(ua, frames=crops[0][0], mask=crops[0][1], unit=0, **common), dict(ub, frames=crops[1][0], unit=1, **common)]
    res = edit_videos(tiny_model, pipe, inner, seed=SEED, return_mask=True)
    for k, (u, plan, (down, mask_w), (img_w, est), (got, got_est)) in enumerate(zip((ua, ub), plans, crops, res, stacked_regions)):
        edit_w = img_w.to(torch.float32)
        want = paste_back(u["frames"], edit_w, down, plan, mask_w=mask_w if plan["mode"] == "replace" else None, device=DEV)
        assert got.shape == u["frames"].shape and _same_bits(got, want), f"unit {k}"
        assert got_est["region"]["box"] == plan["box"] and _same_bits(got_est["region"]["working"], edit_w) and _same_bits(got_est["region"]["down_src"], down)
        assert _outside_is_source(got, u, plan["box"]), f"unit {k}: a pixel outside the box changed"
        assert not torch.equal(got.cpu(), u["frames"].float()), f"unit {k}: nothing was edited"
    assert not _outside_is_source(stacked_regions[1][0], ub, (5, 7, 6, 8))      # (the helper does tell a changed box from an unchanged one)


def test_edit_regions_units_equal_their_own_edit_region(tiny_model, pipe, stacked_regions):
    """Every unit of ``edit_regions`` against its own ``edit_region``, ``torch.equal`` as the issue sets it.  The figures are printed
    before the assertion.  The only difference between the two is the inner run: ``edit_videos`` stacks the two working clips into one
    launch chain (B = 6), ``edit_region`` runs ``edit_video`` alone (B = 3)."""
    from insv2v.region import edit_region
    (ua, ub), (ra, rb), M, common = _region_units()
    alone = [edit_region(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], region=r, seed=SEED, unit=i, **common, **kw)
             for i, (u, r, kw) in enumerate(((ua, ra, dict(mask=M)), (ub, rb, {})))]
    same = []
    for k, ((got, _), a) in enumerate(zip(stacked_regions, alone)):
        d = (got.cpu() - a.cpu()).abs()
        same.append(torch.equal(got.cpu(), a.cpu()))
        print(f"[region] edit_regions unit {k} vs its own edit_region: equal {same[-1]}, max |diff| {float(d.max()):.3e}, differing pixels {int((d > 0).sum())} of {d.numel()}")
    assert all(same)


def test_inner_features_keep_working_at_working_resolution(tiny_model, pipe):
    """mask_shape=, keyframes= with injected working-resolution flows, and mask="auto" with an explicit box: each is the three steps by
    hand with the same keyword."""
    import pixel_score_ref as pr
    from insv2v import synth
    from insv2v.region import edit_region, region_plan
    u, M = _unit(), _rect()
    common = dict(text_cfg=7.5, video_cfg=1.5, seed=SEED, unit=0)
    tc = pr.translation_video(SIZE[1], SIZE[0], [(1, 0), (0, 1)])
    flows = dict(fwd=torch.from_numpy(tc["fwd"]).float(), bwd=torch.from_numpy(tc["bwd"]).float())
    noises = [[synth.synth_input(f"region.ev.auto.{d}", (1, T, 4, SIZE[1] // 8, SIZE[0] // 8)) for d in range(2)]]
    cases = [("mask_shape", dict(mask=M, mask_shape=dict(grow=1.5, feather=3.0)), dict(size=SIZE, mode="replace"), (38, 20, 60, 52)),
             ("keyframes", dict(mask=M, keyframes=2, key_flows=flows), dict(size=SIZE), (38, 20, 60, 52)),
             ("auto", dict(mask="auto", auto_mask=dict(n_maps=2, threshold=0.33, dilate=0, noises=noises)), dict(size=SIZE, box=(20, 5, 70, 70), mode="replace"), None)]
    for name, kw, reg, bbox in cases:
        got = edit_region(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], region=reg, **common, **kw)
        params = dict(dict(mode="residual", blend=8), **reg)
        plan = dict(region_plan((HS, WS), SIZE, bbox=bbox, box=params.get("box")), mode=params["mode"], blend=params["blend"])
        inner = {k: v for k, v in kw.items() if k != "mask" or isinstance(v, str)}
        want, _, _ = _by_hand(tiny_model, pipe, u, plan, kw["mask"] if torch.is_tensor(kw["mask"]) else None, **inner)
        assert _same_bits(got, want), name
        assert _outside_is_source(got, u, plan["box"]), name
        assert name == "auto" or not torch.equal(got.cpu(), u["frames"].float()), name   # (a random-init UNet's estimated mask may be empty)


def test_a_call_without_region_launches_none_of_the_entries(tiny_model, pipe, monkeypatch):
    from insv2v import ops
    from insv2v.run_loveu_tgve import edit_video
    from insv2v.region import edit_region
    from insv2v import synth
    u = dict(_unit(), frames=synth.synth_input("region.ev.plain", (1, T, 3, 32, 48), kind="uniform"))
    M = _rect(32, 48, (10, 8, 30, 24))
    calls = [{}, dict(mask=M), dict(mask=M, mask_shape=dict(grow=1.0, feather=2.0))]
    run = lambda kw: edit_video(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, **kw)   # noqa: E731
    before = [run(kw) for kw in calls]

    def refuse(*a, **k):
        raise AssertionError("a region entry was launched by a call without region")
    for name in ("mask_bbox", "region_resample", "region_paste"):
        monkeypatch.setattr(ops, name, refuse)
    for kw, b in zip(calls, before):
        assert _same_bits(run(kw), b)
    with pytest.raises(AssertionError, match="without region"):
        edit_region(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], region=dict(size=(32, 32)), seed=SEED)


def test_cli_synthetic_region(tmp_path, monkeypatch):
    """``--synthetic 1 --synthetic-tiny --region --region-source 110 75``: the 75 x 110 source comes back at its own size, edited in the
    box only; --image-size is the working size."""
    from insv2v import run_loveu_tgve, inference, ops

    class Eager(inference.InferenceIP2PVideo):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **EAGER))
    monkeypatch.setattr(inference, "InferenceIP2PVideo", Eager)
    seen, real = [], ops.region_paste

    def spy(out, edit_w, down_src, box, **kw):
        seen.append(dict(kw, box=tuple(box), out=tuple(out.shape), edit=tuple(edit_w.shape)))
        return real(out, edit_w, down_src, box, **kw)
    monkeypatch.setattr(ops, "region_paste", spy)
    common = ["--synthetic", "1", "--synthetic-tiny", "--num-frames", "3", "--image-size", "32", "--steps", "1", "--seed", "5", "--no-stack"]
    run_loveu_tgve.main(common + ["--region", "--region-source", "110", "75", "--region-box", "30", "10", "90", "70", "--region-blend", "2",
                                  "--out", str(tmp_path / "region.pt")])
    assert seen == [dict(mode="residual", blend=2, mask_w=None, box=(30, 10, 90, 70), out=(3, 3, 75, 110), edit=(3, 3, 32, 32))]
    out = torch.load(tmp_path / "region.pt")
    assert out.shape == (1, 1, 3, 3, 75, 110) and bool(torch.isfinite(out.float()).all())
    frames = (torch.rand((1, 3, 3, 75, 110), generator=torch.Generator().manual_seed(0)) * 2 - 1)
    outside = torch.ones(frames.shape, dtype=torch.bool)
    outside[..., 10:70, 30:90] = False
    assert torch.equal(out[0].float()[outside], frames.half().float()[outside]) and not torch.equal(out[0].float(), frames.half().float())
