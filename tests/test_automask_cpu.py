"""The mask estimate on the host: the float64 restatement's own properties (tests/automask_ref.py), planted misreadings of the definition
that the GPU tests' inputs must tell apart, the condition the GPU tests' threshold band relies on, the stacking plan, the MASK stream
ids, and the interfaces the feature adds (C header, ctypes mirror, argument refusals of the entries, pipeline, drivers and CLI)."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

import automask_ref as ar
from conftest import ROOT


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_single_frame_smoothing_is_spatial_only():
    raw = ar.raw_input(1, 5, 7).double().numpy()
    got = ar.finish(raw, smooth=True)["soft"]
    soft0 = ar.finish(raw, smooth=False)["soft"]
    want = ar._binomial(ar._binomial(soft0, 1), 2)
    assert np.array_equal(got, want) and np.abs(got - soft0).max() > 1e-3
    assert np.array_equal(ar._binomial(soft0, 0), soft0)   # T = 1: the temporal filter sees its own frame three times


def test_zero_map_gives_zeros_and_no_nan():
    for smooth, dilate in itertools.product((True, False), (0, 1, 2)):
        r = ar.finish(np.zeros((3, 5, 7)), smooth=smooth, dilate=dilate)
        assert r["mu"] == 0.0
        for k in ("soft", "bin", "mask_latent", "mask"):
            assert np.isfinite(r[k]).all() and not r[k].any(), k


def test_image_mask_reduces_to_the_latent_mask_in_both_modes():
    r = ar.finish(ar.raw_input(3, 5, 7).double().numpy())
    assert r["mask"].shape == (3, 40, 56) and 0 < r["mask_latent"].sum() < r["mask_latent"].size
    assert set(np.unique(r["mask"])) == {0.0, 1.0}
    for mode in ("max", "mean"):
        assert np.array_equal(ar.mask_to_latent(r["mask"], mode), r["mask_latent"]), mode


def test_monotone_in_threshold_and_dilate_zero_is_the_identity():
    raw = ar.raw_input(3, 33, 47).double().numpy()
    prev = None
    for th in (0.2, 0.3, 0.5, 0.7, 0.9):
        r = ar.finish(raw, threshold=th, dilate=1)
        if prev is not None:
            assert (r["mask_latent"] <= prev).all() and (r["mask_latent"].sum() < prev.sum() or (th > 0.5 and prev.sum() == 0))
        prev = r["mask_latent"]
        r0 = ar.finish(raw, threshold=th, dilate=0)
        assert np.array_equal(r0["mask_latent"], r0["bin"]) and (r0["mask_latent"] <= r["mask_latent"]).all()
    # more dilation never removes a cell, and it stays inside its frame: a frame without a cell above the threshold stays empty
    one = np.zeros((3, 5, 7))
    one[1, 0, 6] = 1.0
    r = ar.finish(one, smooth=False, dilate=2, clamp_ratio=3.0)
    assert r["mask_latent"][1, :3, 4:].all() and r["mask_latent"].sum() == 9 and not r["mask_latent"][[0, 2]].any()


def test_exact_case_is_what_the_docstring_says():
    raw = ar.exact_raw()
    assert raw.sum() * 4 == raw.size
    r = ar.finish(raw, smooth=True, dilate=0, threshold=0.5625)
    assert r["mu"] == 0.25 and set(np.unique(ar.finish(raw, smooth=False)["soft"])) == {0.0, 1.0}
    assert r["soft"][0, 2, 2] == 0.5625 and r["soft"][0, 2, 3] == 0.75 and r["soft"][0, 3, 3] == 1.0
    assert np.array_equal(r["soft"] * 64, np.round(r["soft"] * 64))   # dyadic
    assert r["mask_latent"].sum() == 2 * 12                             # strict: the four corners are not above 9/16


# ------------------------------------------------------------------------------------------------------------------ planted mutations
def _finish_differs(raw, flags, mutate):
    """Would the checks of the GPU test (soft by ``close``; mask_latent outside the excluded band) tell ``mutate`` from the definition?"""
    smooth, dilate, th = flags
    ref = ar.finish(raw, smooth=smooth, dilate=dilate, threshold=th)
    mut = ar.finish(raw, smooth=smooth, dilate=dilate, threshold=th, mutate=mutate)
    if np.abs(mut["soft"] - ref["soft"]).max() > 1e-5 * np.abs(ref["soft"]).max():
        return True
    _, excluded = ar.near_threshold(ref["soft"], th, dilate)
    return bool((mut["mask_latent"] != ref["mask_latent"])[~excluded].any())


@pytest.mark.parametrize("mutate", ar.FINISH_MUTATIONS)
def test_finish_mutations_are_caught_by_the_gpu_inputs(mutate):
    if mutate == "ge":   # only an exact tie shows it: the exact case has soft == threshold at the rectangle's corners
        caught = [f for f in ar.EXACT_FLAGS if not np.array_equal(ar.finish(ar.exact_raw(), smooth=f[0], dilate=f[1], threshold=f[2], mutate="ge")["mask_latent"],
                                                                    ar.finish(ar.exact_raw(), smooth=f[0], dilate=f[1], threshold=f[2])["mask_latent"])]
        assert (True, 0, 0.5625) in caught and (True, 1, 0.5625) in caught
        return
    caught = 0
    for T, h, w in ar.FINISH_SHAPES:
        raw = ar.raw_input(T, h, w).double().numpy()
        caught += sum(_finish_differs(raw, f, mutate) for f in ar.FINISH_FLAGS)
    print(f"[automask] mutation {mutate}: told apart in {caught} of {len(ar.FINISH_SHAPES) * len(ar.FINISH_FLAGS)} GPU cases")
    assert caught >= 6, mutate


@pytest.mark.parametrize("mutate", ar.RAW_MUTATIONS)
def test_raw_mutations_are_caught_by_the_gpu_inputs(mutate):
    caught = 0
    for (F, h, w), n in ar.EPS_CASES:
        eps = ar.eps_input(F, h, w, n).double().numpy()
        ref, mut = ar.raw_map(eps), ar.raw_map(eps, mutate)
        caught += bool(np.abs(mut - ref).max() > 1e-5 * np.abs(ref).max())
    assert caught == (6 if mutate == "no_n" else len(ar.EPS_CASES)), mutate   # (1/n shows at n > 1)


def test_at_most_two_cells_lie_in_the_threshold_band_of_any_gpu_case():
    """The GPU test excludes the cells within ``dilate`` of a cell whose soft value is within 1e-5 of the threshold.  That exclusion
    cannot hide a failure only if it is tiny: at most 2 band cells per case, on the very inputs the GPU test uses.  (A key that
    violates this is changed; the cap is not.)"""
    worst = 0
    for T, h, w in ar.FINISH_SHAPES:
        raw = ar.raw_input(T, h, w).double().numpy()
        for smooth, dilate, th in ar.FINISH_FLAGS:
            r = ar.finish(raw, smooth=smooth, dilate=dilate, threshold=th)
            n, excluded = ar.near_threshold(r["soft"], th, dilate)
            worst = max(worst, n)
            assert n <= 2, (T, h, w, smooth, dilate, th, n)
            assert excluded.sum() <= 2 * (2 * dilate + 1) ** 2
            if h * w > 1:   # both classes present: the comparison is not vacuous
                assert 0 < r["bin"].sum() < r["bin"].size, (T, h, w, smooth, th)
    print(f"[automask] most band cells in a GPU case: {worst}")


# ------------------------------------------------------------------------------------------------------------------ plan and streams
def test_mask_plan_is_pinned():
    from insv2v.inference import mask_plan, stack_groups
    want = {(16, 4, 9): [(0, 0, 16, 0, 4)],
            (24, 4, 9): [(0, 0, 16, 0, 4), (1, 16, 8, 0, 4)],
            (28, 10, 9): [(0, 0, 16, 0, 5), (0, 0, 16, 5, 5), (1, 16, 12, 0, 5), (1, 16, 12, 5, 5)],
            (5, 1, 1): [(0, 0, 5, 0, 1)],
            (33, 3, 2): [(0, 0, 16, 0, 2), (0, 0, 16, 2, 1), (1, 16, 16, 0, 2), (1, 16, 16, 2, 1), (2, 32, 1, 0, 2), (2, 32, 1, 2, 1)]}
    for (T, n, cap), plan in want.items():
        assert mask_plan(T, 16, n, cap) == plan, (T, n, cap)
        assert [(a, a + f) for k, a, f, d0, m in plan if d0 == 0] == ar.chunks(T, 16)
        for k in {p[0] for p in plan}:   # every draw of every chunk exactly once, in groups of stack_groups
            mine = [p for p in plan if p[0] == k]
            assert [p[4] for p in mine] == stack_groups(n, cap) and all(p[4] <= cap for p in mine)
            assert [d for p in mine for d in range(p[3], p[3] + p[4])] == list(range(n))
    assert mask_plan(5, 2, 3, 20) == [(0, 0, 2, 0, 3), (1, 2, 2, 0, 3), (2, 4, 1, 0, 3)]
    for bad in ((0, 16, 4, 9), (16, 0, 4, 9), (16, 16, 0, 9), (16, 16, 4, 0)):
        with pytest.raises(ValueError):
            mask_plan(*bad)


def test_mask_stream_ids_are_injective_and_range_checked():
    from insv2v import rng
    from insv2v.rng import stream_id, ENC, INIT, STEP, MASK
    assert MASK == 3 and (ENC, INIT, STEP) == (0, 1, 2)
    units = (0, 1, 255, 2 ** 24 - 1)
    windows = (0, 1, 16, 4095)
    steps = (0, 1, 3, 65535)
    ids = [stream_id(k, u, w, s) for k, u, w, s in itertools.product((ENC, INIT, STEP, MASK), units, windows, steps)]
    assert len(set(ids)) == len(ids) and all(0 <= i < 2 ** 63 for i in ids)
    assert all(type(i) is int for i in ids)
    assert stream_id(MASK, 5, 2, 3) == (3 << 52) | (5 << 28) | (2 << 16) | 3 and stream_id(MASK, 0) >> 52 == 3
    for bad in ((MASK, 2 ** 24, 0, 0), (MASK, 0, 4096, 0), (MASK, 0, 0, 65536), (MASK, -1, 0, 0), (MASK, 0, -1, 0), (MASK, 0, 0, -1),
                (MASK, 1.5, 0, 0), (4, 0, 0, 0)):
        with pytest.raises(ValueError):
            stream_id(*bad)
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    for text in (header, rng.__doc__):
        assert re.search(r"MASK", text) and re.search(r"3 MASK|MASK = 3", text)
    assert "bits 52-53 kind (0 ENC, 1 INIT, 2 STEP, 3 MASK)" in header and "MASK: element index over the chunk's [F,4,h,w]" in header
    assert "window = chunk index, step = draw index" in rng.__doc__


# ------------------------------------------------------------------------------------------------------------------ interfaces
NEW = ("insv2v_build_unet_input_noised", "insv2v_eps_absdiff_accum", "insv2v_automask_finish", "insv2v_automask_workspace_bytes")


def test_header_ctypes_and_sources_carry_the_new_entries_and_abi_15():
    import build
    from insv2v import _lib, ops
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    i32, i64, f32, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert _lib.ABI_VERSION == 15
    for name in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % name, header, flags=re.M), name
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["insv2v_build_unet_input_noised"] == (i32, [p, p, p, p, p, f32, f32, f32, i64, i64, i32, i32, i32, i32, i32, i64, i32, p])
    assert _lib.SIGNATURES["insv2v_eps_absdiff_accum"] == (i32, [p, p, i32, i32, i32, i64, f32, i32, p])
    assert _lib.SIGNATURES["insv2v_automask_workspace_bytes"] == (i64, [i32, i32, i32])
    assert _lib.SIGNATURES["insv2v_automask_finish"] == (i32, [p, p, p, p, p, i64, i32, i32, i32, f32, f32, i32, i32, p])
    assert "automask.hip" in build.SOURCES
    for name in ("build_unet_input_noised", "eps_absdiff_accum", "automask_finish"):
        assert callable(getattr(ops, name))
    src = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "automask.hip")).read()
    assert "noised_f(" in src and "rng_normal_at(" in src and "atomicAdd" not in src   # the shared expressions; a fixed-order mean
    ew = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "elementwise.hip")).read()
    assert "out[i] = noised_f(ka, z[i], kb, noise[i]);" in ew   # insv2v_add_noise computes the same expression


def test_entries_refuse_bad_arguments_before_any_launch():
    """The argument checks run on the host in front of the launch: the addresses below are never dereferenced."""
    from insv2v import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build
        build.build(verbose=False)
    lib = _lib.load()
    ws = lib.insv2v_automask_workspace_bytes
    assert ws(16, 32, 48) > 0 and ws(1, 1, 1) >= 4 and ws(16, 32, 48) % 4 == 0
    for T, h, w in ((0, 5, 7), (3, 0, 7), (3, 5, 0), (-1, 5, 7)):
        assert ws(T, h, w) < 0

    def fin(raw=0x10000, soft=0x20000, ml=0x30000, mask=0x100000, wsp=0x40000, wsb=1 << 20, T=3, h=5, w=7, r=3.0, th=0.5, smooth=1, dilate=1):
        return lib.insv2v_automask_finish(raw, soft, ml, mask, wsp, wsb, T, h, w, r, th, smooth, dilate, None)
    for k in ("raw", "soft", "ml", "mask", "wsp"):
        assert fin(**{k: None}) == -1, k
    for k in ("T", "h", "w"):
        assert fin(**{k: 0}) == -1 and fin(**{k: -2}) == -1, k
    for th in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert fin(th=th) == -1, th
    for r in (0.0, -1.0, float("nan")):
        assert fin(r=r) == -1, r
    assert fin(dilate=-1) == -1 and fin(smooth=2) == -1 and fin(smooth=-1) == -1
    assert fin(wsb=0) == -1 and fin(wsb=ws(3, 5, 7) - 1) == -1 and fin(mask=0x100004) == -1
    assert fin(soft=0x10000) == -1 and fin(ml=0x20000) == -1 and fin(ml=0x10000 + 16) == -1   # raw / soft / mask_latent overlapping

    def acc(eps=0x10000, a=0x20000, F=3, h=5, w=7, bs=0, scale=0.25, accumulate=0):
        return lib.insv2v_eps_absdiff_accum(eps, a, F, h, w, bs, scale, accumulate, None)
    assert acc(eps=None) == -1 and acc(a=None) == -1 and acc(accumulate=2) == -1 and acc(bs=-4) == -1
    for k in ("F", "h", "w"):
        assert acc(**{k: 0}) == -1, k
    assert acc(eps=0x10004) == -1 and acc(bs=3 * 5 * 7 * 4 + 2) == -1 and acc(bs=3 * 5 * 7 * 4 - 4) == -1   # 16-byte loads; overlapping branches

    def bld(z=0x10000, cond=0x20000, noise=0x30000, out=0x40000, t=0x50000, seeded=0, F=3, h=5, w=7, ldo=8, rows=0, ts=0):
        return lib.insv2v_build_unet_input_noised(z, cond, noise, out, t, 500.0, 0.8, 0.6, 7, 11, seeded, F, h, w, ldo, rows, ts, None)
    assert bld(z=None) == -1 and bld(cond=None) == -1 and bld(out=None) == -1
    assert bld(seeded=1) == -1 and bld(noise=None, seeded=0) == -1 and bld(seeded=2) == -1   # both sources, none, not a flag
    for k in ("F", "h", "w"):
        assert bld(**{k: 0}) == -1, k
    assert bld(ldo=4) == -1 and bld(rows=3 * 5 * 7 - 1) == -1 and bld(ts=-1) == -1


def test_estimate_mask_refuses_bad_arguments_before_the_first_launch():
    from insv2v.inference import InferenceIP2PVideo, check_automask_args, AUTO_MASK_DEFAULTS

    class FakeUNet:
        device = torch.device("cpu")
    par = inspect.signature(InferenceIP2PVideo.estimate_mask).parameters
    assert {k: par[k].default for k in ar.DEFAULTS} == ar.DEFAULTS == AUTO_MASK_DEFAULTS
    assert par["frames_in_batch"].default == 16 and all(par[k].default is None for k in ("noises", "seed")) and par["unit"].default == 0
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(ar.DEFAULTS) + ["frames_in_batch", "noises", "seed", "unit"])
    check_automask_args(**ar.DEFAULTS)
    check_automask_args(n_maps=65535, mask_strength=1.0, clamp_ratio=0.1, threshold=0.999, smooth=False, dilate=0, frames_in_batch=1)
    p = InferenceIP2PVideo(FakeUNet(), scheduler="ddim", num_ddim_steps=10)   # a UNet without a forward: any launch attempt raises AttributeError
    z = torch.zeros((1, 5, 4, 6, 9))
    tc = torch.zeros((1, 77, 64))
    bad = [dict(n_maps=0), dict(n_maps=65536), dict(n_maps=2.0), dict(n_maps=True), dict(mask_strength=0.0), dict(mask_strength=1.01),
           dict(mask_strength=float("nan")), dict(clamp_ratio=0.0), dict(clamp_ratio=-3.0), dict(clamp_ratio=float("nan")), dict(threshold=0.0),
           dict(threshold=1.0), dict(threshold=float("nan")), dict(threshold="0.5"), dict(dilate=-1), dict(dilate=1.5), dict(smooth=1),
           dict(frames_in_batch=0), dict(noises=[[z[0]]]), dict(noises=[[z[0, :2]], [z[0, :2]], [z[0, :2]]], n_maps=1, frames_in_batch=2),
           dict(seed=3, unit=2 ** 24), dict(seed=3, unit=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            p.estimate_mask(z, tc, tc, z, **kw)
    with pytest.raises(ValueError):
        p.estimate_mask(torch.zeros((2, 5, 4, 6, 9)), tc, tc, torch.zeros((2, 5, 4, 6, 9)))
    with pytest.raises(ValueError):
        p.estimate_mask(z, tc, tc, z[:, :4])


def test_drivers_accept_auto_and_refuse_everything_else_before_anything_runs():
    from insv2v.run_loveu_tgve import check_edit_args, edit_video, edit_videos, AUTO_MASK_KEYS
    shape = (1, 10, 3, 32, 48)
    frames = torch.zeros(shape)
    check_edit_args(shape, "auto")
    check_edit_args(shape, "auto", 0.5, "mean", dict(n_maps=2, threshold=0.3, dilate=0, smooth=False, mask_strength=0.25, clamp_ratio=2.0))
    check_edit_args(shape, "auto", auto_mask={})
    assert set(ar.DEFAULTS) < set(AUTO_MASK_KEYS)
    par = inspect.signature(edit_video).parameters
    assert (par["mask"].default, par["auto_mask"].default, par["return_mask"].default) == (None, None, False)
    assert inspect.signature(edit_videos).parameters["return_mask"].default is False
    cases = [dict(mask="Auto"), dict(mask="automatic"), dict(mask=""), dict(mask=None, auto_mask={}), dict(mask=None, auto_mask=dict(n_maps=2)),
             dict(mask=torch.ones((1, 10, 32, 48)), auto_mask=dict(n_maps=2)), dict(mask="auto", auto_mask=dict(n_maps=0)),
             dict(mask="auto", auto_mask=dict(threshold=1.0)), dict(mask="auto", auto_mask=dict(maps=3)), dict(mask="auto", auto_mask=[("n_maps", 2)]),
             dict(mask="auto", auto_mask=dict(dilate=-1)), dict(mask="auto", auto_mask=dict(mask_strength=0.0)), dict(mask="auto", auto_mask=dict(seed=1))]
    for kw in cases:
        with pytest.raises(ValueError, match="mask"):
            check_edit_args(shape, kw.get("mask"), 1.0, "max", kw.get("auto_mask"))
        with pytest.raises(ValueError, match="mask"):   # model and pipe are never touched
            edit_video(None, None, frames, None, None, **kw)
        with pytest.raises(ValueError, match="mask"):
            edit_videos(None, None, [dict(frames=frames), dict(frames=frames, **kw)])
    with pytest.raises(ValueError, match="multiples of 8"):
        check_edit_args((1, 10, 3, 36, 48), "auto")
    with pytest.raises(ValueError, match="mask"):
        check_edit_args((2, 10, 3, 32, 48), "auto")
    with pytest.raises(ValueError, match="strength"):
        edit_video(None, None, frames, None, None, mask="auto", strength=0.0)


def test_cli():
    from insv2v.run_loveu_tgve import build_parser, check_args, auto_mask_unit, auto_mask_kwargs
    p = build_parser()
    a = check_args(p.parse_args([]))
    assert (a.auto_mask, a.auto_mask_maps, a.auto_mask_strength, a.auto_mask_threshold, a.auto_mask_dilate, a.mask_out) == (False, 4, 0.5, 0.5, 1, None)
    assert auto_mask_unit(a) == {} and auto_mask_unit(a, {"mask": torch.ones(1)}) == {}
    a = check_args(p.parse_args(["--auto-mask", "--auto-mask-maps", "6", "--auto-mask-strength", "0.25", "--auto-mask-threshold", "0.3",
                                 "--auto-mask-dilate", "0", "--mask-out", "masks.pt", "--synthetic", "2"]))
    assert auto_mask_kwargs(a) == dict(n_maps=6, mask_strength=0.25, threshold=0.3, dilate=0)
    assert auto_mask_unit(a, {"frames": None}) == dict(mask="auto", auto_mask=auto_mask_kwargs(a)) and a.mask_out == "masks.pt"
    with pytest.raises(SystemExit, match="--units"):   # at load time: the file brings its own masks
        auto_mask_unit(a, {"mask": torch.ones((2, 1, 8, 8))})
    with pytest.raises(SystemExit, match="--synthetic-mask"):
        check_args(p.parse_args(["--auto-mask", "--synthetic", "2", "--synthetic-mask"]))
    with pytest.raises(SystemExit, match="--auto-mask"):
        check_args(p.parse_args(["--mask-out", "masks.pt"]))
    for flag, values in (("--auto-mask-maps", ("0", "-1", "65536")), ("--auto-mask-strength", ("0", "1.01", "-0.5", "nan")),
                         ("--auto-mask-threshold", ("0", "1", "1.5", "nan")), ("--auto-mask-dilate", ("-1",))):
        for v in values:
            with pytest.raises(SystemExit, match=flag):
                check_args(p.parse_args(["--auto-mask", flag, v]))
