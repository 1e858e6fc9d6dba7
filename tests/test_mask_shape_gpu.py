"""Shaping a mask on the GPU: insv2v_mask_shape against the integer / float64 definition of tests/mask_shape_ref.py, its determinism and
refusals, and the drivers' ``mask_shape=`` with each of the three mask sources.

Kernel level: the two integer maps, ``support`` and the sets {shaped == 0} and {shaped == 1} must match EXACTLY; the ramp is checked per
element against float64 within ``mask_shape_ref.ramp_bound`` - 4 x the worst departure of an fp32 restatement in the kernel's operation
order on the case's own inputs (the factor covers FMA contraction and the device's sqrtf), floored at one fp32 rounding.  No pixel is left
out of any comparison.  Drivers: bit for bit identities; a stacked unit against the same unit alone within the stacked bound of the
project's masked tests (rel-RMS 1e-2 / max 4e-2)."""
import numpy as np
import pytest
import torch

import mask_shape_ref as mr
import pixel_score_ref as pr
from test_model_gpu import tiny_unet, report   # noqa: F401  (tiny_unet: the module-scoped fixture, instantiated for this module)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EAGER = dict(use_graph=False)
STACKED = dict(rms_tol=1e-2, max_tol=4e-2)
PAD = 37
NAN = float("nan")


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _carve(shape, dtype, fill, values=None):
    """A contiguous view of ``shape`` in the middle of a 1-D buffer filled with ``fill`` -> (buffer, view, mask of the buffer outside the view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), fill, device=DEV, dtype=dtype)
    view = buf[PAD:PAD + n].view(shape)
    if values is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(DEV))
    outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    outside[PAD:PAD + n] = False
    return buf, view, outside


def _launch(m, g, f, profile, threshold=mr.TAU):
    """The kernel on an input between NaNs, its four outputs between sentinels (NaN / -1) -> the outputs as numpy, after checking that
    every sentinel survived."""
    from insv2v import ops
    _, mv, _ = _carve(m.shape, torch.float32, NAN, m)
    outs = [_carve(m.shape, torch.float32, NAN) for _ in range(2)] + [_carve(m.shape, torch.int32, -1) for _ in range(2)]
    ops.mask_shape(mv, grow=g, feather=f, threshold=threshold, profile=profile, return_d2=True, out=tuple(v for _, v, _ in outs))
    torch.cuda.synchronize()
    for i, (buf, _, outside) in enumerate(outs):
        s = buf[outside]
        assert bool(torch.isnan(s).all() if i < 2 else (s == -1).all()), f"output {i} was written outside its tensor"
    return [v.cpu().numpy() for _, v, _ in outs]


@pytest.mark.parametrize("name", [c[0] for c in mr.CASES])
def test_kernel_vs_reference(name):
    _, T, H, W, g, f, profile = next(c for c in mr.CASES if c[0] == name)
    m, r = mr.case_reference(name)
    shaped, support, d2o, d2i = _launch(m, g, f, profile)
    assert d2o.dtype == np.int32 and np.array_equal(d2o, r["d2_out"]), f"{name}: d2_out differs in {(d2o != r['d2_out']).sum()} pixels"
    assert np.array_equal(d2i, r["d2_in"]), f"{name}: d2_in differs in {(d2i != r['d2_in']).sum()} pixels"
    assert np.array_equal(support, r["support"]), f"{name}: support differs in {(support != r['support']).sum()} pixels"
    assert np.array_equal(shaped == 0, r["shaped"] == 0) and np.array_equal(shaped == 0, r["zero"]), f"{name}: the set shaped == 0 differs"
    assert np.array_equal(shaped == 1, r["shaped"] == 1) and np.array_equal(shaped == 1, r["one"]), f"{name}: the set shaped == 1 differs"
    bound, worst32 = mr.ramp_bound(r, g, f, profile)
    err = np.abs(shaped.astype(np.float64) - r["shaped"])   # every pixel: exactly 0 outside the ramp
    print(f"[mask_shape] {name} {T}x{H}x{W} g={g:g} f={f:g} {profile}: ramp pixels {int(r['ramp'].sum())}, fp32 restatement {worst32:.3e}, "
          f"bound {bound:.3e}, kernel max err {err.max():.3e} = {err.max() / bound:.3f} of the bound")
    assert np.isfinite(shaped).all() and err.max() <= bound, f"{name}: ramp off by {err.max():.3e} > {bound:.3e}"
    assert err[~r["ramp"]].max(initial=0.0) == 0.0


def test_identity_on_a_binary_mask_is_bit_for_bit():
    m = (mr.case_input("special_frames") > 0.5).astype(np.float32)   # (NaN -> 0)
    shaped, support, _, _ = _launch(m, 0.0, 0.0, "smooth")
    assert np.array_equal(shaped.view(np.int32), m.view(np.int32)) and np.array_equal(support.view(np.int32), m.view(np.int32))


def test_two_runs_agree_bitwise_also_on_a_second_stream():
    from insv2v import ops
    m = torch.from_numpy(mr.case_input("row_tiles")).to(DEV)

    def run():
        return ops.mask_shape(m, grow=32.0, feather=32.0, return_d2=True)
    first, second = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for a, b, c in zip(first, second, third):
        assert _same_bits(a, b) and _same_bits(a, c)
    assert bool(torch.isfinite(first[0]).all())


def test_refusals_leave_the_outputs_untouched():
    import ctypes
    from insv2v import _lib
    lib = _lib.load()
    T, H, W = 2, 9, 13
    n = T * H * W
    m = torch.rand((T, H, W), device=DEV)
    outs = [_carve((T, H, W), torch.float32, NAN) for _ in range(2)] + [_carve((T, H, W), torch.int32, -1) for _ in range(2)]
    need = lib.insv2v_mask_shape_workspace_bytes(T, H, W)
    assert need >= n and lib.insv2v_mask_shape_workspace_bytes(0, H, W) == -1 and lib.insv2v_mask_shape_workspace_bytes(T, H, -1) == -1
    ws = torch.full((need + 8,), 7, device=DEV, dtype=torch.uint8)
    base = dict(m=m.data_ptr(), shaped=outs[0][1].data_ptr(), support=outs[1][1].data_ptr(), d2_out=outs[2][1].data_ptr(), d2_in=outs[3][1].data_ptr(),
                workspace=ws.data_ptr(), workspace_bytes=need, T=T, H=H, W=W, threshold=0.5, grow=2.0, feather=3.0, profile=1)
    assert ws.data_ptr() % 4 == 0

    def call(**kw):
        d = _lib.MaskShapeDesc()
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        return lib.insv2v_mask_shape(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)

    def untouched():
        torch.cuda.synchronize()
        return all(bool(torch.isnan(b).all() if i < 2 else (b == -1).all()) for i, (b, _, _) in enumerate(outs)) and bool((ws == 7).all())
    inf = float("inf")
    bad = [dict(m=None), dict(shaped=None), dict(support=None), dict(workspace=None), dict(T=0), dict(H=0), dict(W=0), dict(T=-1),
           dict(grow=32.5), dict(grow=-32.5), dict(feather=-0.5), dict(feather=32.5), dict(grow=NAN),
           dict(feather=NAN), dict(grow=inf), dict(feather=inf), dict(threshold=NAN), dict(threshold=inf), dict(profile=2), dict(profile=-1),
           dict(workspace_bytes=need - 1), dict(workspace_bytes=0), dict(workspace=ws.data_ptr() + 1), dict(workspace=ws.data_ptr() + 2),
           dict(shaped=base["m"]), dict(support=base["m"] + 4 * (n - 1)), dict(d2_out=base["m"] - 4 * (n - 1)), dict(d2_in=base["m"]),
           dict(workspace=base["m"]), dict(support=base["shaped"]), dict(d2_out=base["support"] + 4), dict(d2_in=base["d2_out"]),
           dict(workspace=base["shaped"] + 4 * (n - 1)), dict(d2_in=base["shaped"])]
    assert lib.insv2v_mask_shape(None, None) == -1
    for kw in bad:
        assert call(**kw) == -1, kw
        assert untouched(), kw
    assert call() == 0 and not untouched()   # the same descriptor without a fault runs
    assert call(d2_out=None, d2_in=None) == 0


# ------------------------------------------------------------------------------------------------------------------ drivers
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


F, HP, WP, SEED = 4, 32, 48, 53
SHAPE = dict(grow=1.5, feather=5.0, profile="smooth")


def _unit(name="a"):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"mask_shape.ev.frames.{name}", (1, F, 3, HP, WP), kind="uniform"),
                text_cond=synth.synth_input(f"mask_shape.ev.tc.{name}", (1, 77, 64)), text_uncond=synth.synth_input("mask_shape.ev.tu", (1, 77, 64)))


def _drawn():
    """A binary [1,F,H,W] mask, not aligned to the 8 x 8 cells, one frame empty."""
    m = torch.zeros((1, F, HP, WP))
    m[:, :, 11:19, 13:26] = 1.0
    m[:, 1, 3:6, 40:44] = 1.0
    m[:, 3] = 0.0
    return m


def _edit(model, pipe, u, unit=0, **kw):
    from insv2v.run_loveu_tgve import edit_video
    return edit_video(model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=unit, return_latent=True, **kw)


def _check_identities(model, pipe, u, got, source_kw, what, stabilized=None):
    """(frames, latent, dict) of an edit with mask_shape: its latent is the latent of the edit with mask=support, its frames are the
    composite of that latent's decoded frames under shaped (then the temporal filter, if any), and outside support they are the input's."""
    from insv2v import ops
    img, lat, est = got
    shaped, support = est["shaped"], est["support"]
    assert shaped.shape == support.shape == (1, F, HP, WP)
    hard = _edit(model, pipe, u, mask=support.cpu(), **source_kw)
    assert _same_bits(lat, hard[1]), f"{what}: the latent is not that of the edit with mask=support"
    dec = model.decode_latent_to_image(lat)[0].to(torch.float32).contiguous()
    want = ops.composite(dec, u["frames"][0].to(device=DEV, dtype=torch.float32).contiguous(), shaped[0].contiguous())[None]
    if stabilized is not None:
        want = stabilized(want, shaped)
    assert _same_bits(img, want), f"{what}: the frames are not the composite of the decoded latent under shaped"
    out = (support[0] == 0)[:, None].expand(F, 3, HP, WP).cpu()
    assert bool(out.any()) and torch.equal(img[0].cpu()[out], u["frames"][0][out]), f"{what}: pixels outside support are not the input's"
    soft = ((shaped > 0) & (shaped < 1))
    assert bool(soft.any()), f"{what}: no feather"
    full = (shaped[0] == 1)[:, None].expand(F, 3, HP, WP).cpu()
    assert (img[0].cpu()[full] - u["frames"][0][full]).abs().max() > 1e-2, f"{what}: nothing was edited where shaped is 1"
    return hard


def test_drawn_mask(tiny_model, pipe):
    from insv2v import ops
    u, M = _unit(), _drawn()
    got = _edit(tiny_model, pipe, u, mask=M, mask_shape=SHAPE, return_mask=True)
    assert set(got[2]) == {"shaped", "support"}   # a drawn mask has no other record
    by_hand = ops.mask_shape(M[0].to(DEV).contiguous(), **SHAPE)
    assert _same_bits(got[2]["shaped"][0], by_hand[0]) and _same_bits(got[2]["support"][0], by_hand[1])
    r = mr.mask_shape(M[0].numpy(), SHAPE["grow"], SHAPE["feather"], 0.5, SHAPE["profile"])
    assert np.array_equal(got[2]["support"][0].cpu().numpy(), r["support"])
    _check_identities(tiny_model, pipe, u, got, {}, "drawn mask")
    plain = _edit(tiny_model, pipe, u, mask=M)
    assert not _same_bits(plain[0], got[0])
    # mask_mode has no effect with mask_shape; a [1,1,H,W] mask serves every frame
    assert _same_bits(_edit(tiny_model, pipe, u, mask=M, mask_shape=SHAPE, mask_mode="mean")[0], got[0])
    still = _edit(tiny_model, pipe, u, mask=M[:, :1], mask_shape=SHAPE, return_mask=True)
    assert still[2]["shaped"].shape == (1, F, HP, WP) and _same_bits(still[2]["shaped"][0, 2], still[2]["shaped"][0, 0])


def test_grow_0_feather_0_on_a_binary_mask_is_the_plain_masked_edit(tiny_model, pipe):
    u, M = _unit(), _drawn()
    plain = _edit(tiny_model, pipe, u, mask=M)
    got = _edit(tiny_model, pipe, u, mask=M, mask_shape=dict(grow=0, feather=0))
    assert _same_bits(got[0], plain[0]) and _same_bits(got[1], plain[1])


def test_auto_mask_with_injected_noises(tiny_model, pipe):
    from insv2v import synth
    from insv2v.mask_shape import shape_mask
    u = _unit()
    noises = [[synth.synth_input(f"mask_shape.ev.auto.{d}", (1, F, 4, HP // 8, WP // 8)) for d in range(2)]]
    auto = dict(n_maps=2, threshold=0.33, dilate=0, noises=noises)   # (a random-init UNet's map is nearly flat around 1/3: this cuts through it)
    src = dict(mask="auto", auto_mask=auto)
    got = _edit(tiny_model, pipe, u, mask_shape=SHAPE, return_mask=True, **src)
    est = got[2]
    assert {"raw", "soft", "mask_latent", "mask", "shaped", "support"} <= set(est) and 0 < float(est["mask"].mean()) < 1
    by_hand = shape_mask(est["mask"], **SHAPE)
    assert _same_bits(by_hand[0], est["shaped"]) and _same_bits(by_hand[1], est["support"])
    _check_identities(tiny_model, pipe, u, got, {}, "auto mask")
    given = _edit(tiny_model, pipe, u, mask=est["mask"].cpu(), mask_shape=SHAPE)   # shaping the returned mask by hand gives the same result
    assert _same_bits(given[0], got[0]) and _same_bits(given[1], got[1])


def _flows():
    tc = pr.translation_video(HP, WP, [((1, 0), (0, 1), (-1, 1), (2, 0))[t % 4] for t in range(F - 1)])
    return dict(fwd=torch.from_numpy(tc["fwd"]).float(), bwd=torch.from_numpy(tc["bwd"]).float())


def test_tracked_mask_with_injected_flows(tiny_model, pipe):
    u, M, flows = _unit(), _drawn()[:, :1], _flows()
    src = dict(mask=M, mask_key=1, mask_flows=flows)
    got = _edit(tiny_model, pipe, u, mask_shape=SHAPE, return_mask=True, **src)
    assert {"mask", "valid", "flow_to_key", "shaped", "support"} <= set(got[2])
    assert not _same_bits(got[2]["shaped"][0, 0], got[2]["shaped"][0, 2]), "the shaped mask does not follow the motion"
    _check_identities(tiny_model, pipe, u, got, {}, "tracked mask")
    given = _edit(tiny_model, pipe, u, mask=got[2]["mask"].cpu(), mask_shape=SHAPE)
    assert _same_bits(given[0], got[0]) and _same_bits(given[1], got[1])


def test_a_unit_inside_edit_videos(tiny_model, pipe):
    from insv2v.run_loveu_tgve import edit_videos
    ua, ub, M = _unit("a"), _unit("b"), _drawn()
    common = dict(text_cfg=7.5, video_cfg=1.5)
    outs = edit_videos(tiny_model, pipe, [dict(ua, unit=0, mask=M, mask_shape=SHAPE, **common), dict(ub, unit=1, **common)], seed=SEED,
                       return_latent=True, return_mask=True)
    alone = _edit(tiny_model, pipe, ua, mask=M, mask_shape=SHAPE, return_mask=True)
    img, lat, est = outs[0]
    assert outs[1][2] is None and _same_bits(est["shaped"], alone[2]["shaped"]) and _same_bits(est["support"], alone[2]["support"])
    report(lat, alone[1].cpu(), "edit_videos unit with mask_shape: latent vs edit_video", **STACKED)
    report(img, alone[0].cpu(), "edit_videos unit with mask_shape: frames vs edit_video", **STACKED)
    out = (est["support"][0] == 0)[:, None].expand(F, 3, HP, WP).cpu()
    assert torch.equal(img[0].cpu()[out], ua["frames"][0][out]) and torch.equal(img[0].cpu()[out], alone[0][0].cpu()[out])
    one = edit_videos(tiny_model, pipe, [dict(ua, unit=0, mask=M, mask_shape=SHAPE, **common)], seed=SEED, return_latent=True, return_mask=True)[0]
    assert _same_bits(one[0], alone[0]) and _same_bits(one[1], alone[1])   # a single unit takes edit_video


def test_stabilize_with_mask_shape(tiny_model, pipe):
    from insv2v.temporal_filter import stabilize
    u, M, flows = _unit(), _drawn(), _flows()
    params = dict(radius=2, sigma=0.25, strength=0.75)
    got = _edit(tiny_model, pipe, u, mask=M, mask_shape=SHAPE, return_mask=True, stabilize=params, stabilize_flows=flows)
    _check_identities(tiny_model, pipe, u, got, dict(stabilize=params, stabilize_flows=flows), "stabilize with mask_shape",
                      stabilized=lambda img, shaped: stabilize(u["frames"], img, flows=flows, mask=shaped, **params))
    unfiltered = _edit(tiny_model, pipe, u, mask=M, mask_shape=SHAPE)
    assert _same_bits(unfiltered[1], got[1]) and not _same_bits(unfiltered[0], got[0])


def test_a_call_without_mask_shape_launches_nothing_of_it(tiny_model, pipe, monkeypatch):
    """Without ``mask_shape`` the shaping entry is never reached - by the masked, the tracked, the stabilized or the plain edit - and the
    results are those of the same calls before the patch (the entry is not what produced them)."""
    from insv2v import ops
    u, M, flows = _unit(), _drawn(), _flows()
    calls = [{}, dict(mask=M), dict(mask=M[:, :1], mask_key=1, mask_flows=flows), dict(mask=M, stabilize=True, stabilize_flows=flows)]
    before = [_edit(tiny_model, pipe, u, **kw) for kw in calls]

    def refuse(*a, **k):
        raise AssertionError("ops.mask_shape was launched by a call without mask_shape")
    monkeypatch.setattr(ops, "mask_shape", refuse)
    for kw, b in zip(calls, before):
        a = _edit(tiny_model, pipe, u, **kw)
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    with pytest.raises(AssertionError, match="without mask_shape"):
        _edit(tiny_model, pipe, u, mask=M, mask_shape=SHAPE)


def test_cli_synthetic_mask_shape_and_mask_image(tmp_path, monkeypatch):
    """``--synthetic 1 --synthetic-tiny`` with a mask from a PNG and ``--mask-grow`` / ``--mask-feather`` (reduced-width models, 3 frames at
    64 x 64, one step): the unit's mask goes through ``ops.mask_shape`` once with the flags' parameters, ``--mask-out`` holds the shaped
    mask and its support, and the pixels outside the support are the input's."""
    from PIL import Image
    from insv2v import run_loveu_tgve, inference, ops
    from insv2v.video_io import load_mask

    class Eager(inference.InferenceIP2PVideo):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **EAGER))
    monkeypatch.setattr(inference, "InferenceIP2PVideo", Eager)
    seen, real = [], ops.mask_shape

    def spy(mask, **kw):
        seen.append(dict(kw, shape=tuple(mask.shape)))
        return real(mask, **kw)
    monkeypatch.setattr(ops, "mask_shape", spy)
    S = 64
    png = np.zeros((32, 32), np.uint8)       # half the frame's size: resized like the frames
    png[8:20, 10:24] = 255
    Image.fromarray(png).save(tmp_path / "mask.png")
    common = ["--synthetic", "1", "--synthetic-tiny", "--num-frames", "3", "--image-size", str(S), "--steps", "1", "--seed", "5", "--no-stack"]
    run_loveu_tgve.main(common + ["--mask-image", str(tmp_path / "mask.png"), "--out", str(tmp_path / "hard.pt")])
    assert seen == []
    run_loveu_tgve.main(common + ["--mask-image", str(tmp_path / "mask.png"), "--mask-grow", "2", "--mask-feather", "6", "--mask-profile", "linear",
                                  "--mask-out", str(tmp_path / "masks.pt"), "--out", str(tmp_path / "soft.pt")])
    assert len(seen) == 1 and seen[0] == dict(grow=2.0, feather=6.0, profile="linear", shape=(3, S, S))
    hard, soft, masks = torch.load(tmp_path / "hard.pt"), torch.load(tmp_path / "soft.pt"), torch.load(tmp_path / "masks.pt")
    assert hard.shape == soft.shape and bool(torch.isfinite(soft.float()).all()) and not torch.equal(hard, soft)
    assert sorted(masks) == [0] and set(masks[0]) == {"shaped", "support"} and masks[0]["shaped"].shape == (3, S, S)
    M = load_mask(str(tmp_path / "mask.png"), (S, S))
    r = mr.mask_shape(M[0].expand(3, S, S).numpy(), 2.0, 6.0, 0.5, "linear")
    assert np.array_equal(masks[0]["support"].numpy(), r["support"]) and 0 < r["support"].mean() < 1 and r["ramp"].any()
    frames = (torch.rand((1, 3, 3, S, S), generator=torch.Generator().manual_seed(0)) * 2 - 1).half()   # main's synthetic frames, as it stores them
    out = (masks[0]["support"] == 0)[:, None].expand(3, 3, S, S)
    assert torch.equal(soft[0, 0][out], frames[0][out])
