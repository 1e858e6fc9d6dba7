"""Filling the frames between edited key frames, without a GPU: the key-frame schedule and the chain's launch plan,
the argument checks and their refusals, the float64 definition (tests/keyfill_ref.py) against an independent pixel loop that samples with
``torch.nn.functional.grid_sample``, its closed forms, fourteen planted misreadings - each must miss the reference by at least 10 bounds on
the GPU file's own inputs - and the float32 restatement in the kernel's operation order, measured against float64 and printed
(``[keyfill]`` lines): its worst departure is what the GPU bound is calibrated on.

Measured here (float32 restatement against float64, worst element over a case's eight dtype / mode variants): 9.1e-8 (2 x 2), 9.4e-8
(5 x 7), 4.8e-6 (3 x 300), 3.8e-7 (17 x 33) and 1.4e-7 (n = 65) where the edit is fp32, 2.2e-4 .. 4.9e-4 where it is fp16 and the store's
rounding is all there is; the derived exp-argument term is at most 0.44 of an fp32 bound.  The misreadings miss by 88 bounds (nearest,
fp16) to 1.3e6 (fp32), or show as NaN."""
import os
import re

import numpy as np
import pytest
import torch

import keyfill_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [("f16", "f16"), ("f32", "f32"), ("f16", "f32"), ("f32", "f16")]   # (E, A)


# ------------------------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("stride", [2, 3, 4, 8])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 9, 17])
def test_key_frames_and_fill_plan(T, stride):
    from insv2v.keyfill import key_frames, fill_plan, fill_sides
    keys = key_frames(T, stride)
    assert keys == sorted(set(list(range(0, T, stride)) + [T - 1])) and keys[0] == 0 and keys[-1] == T - 1
    plan = fill_plan(T, keys)
    gaps = [b - a for a, b in zip(keys, keys[1:])]
    assert len(plan) == max(gaps, default=1) - 1, "one launch per distance: max gap - 1"
    seen = {0: [], 1: []}
    for j, step in enumerate(plan, 1):
        assert step, "no empty launch"
        for side, t, tp, (bs, bi), (cs, ci) in step:
            a = max(k for k in keys if k < t)
            b = min(k for k in keys if k > t)
            if side == 0:   # F_{t -> a} = bwd[t-1] + S(F_{t-1 -> a}),  t = a + j
                assert (t, tp, bs, bi, cs, ci) == (a + j, t - 1, "bwd", t - 1, "fwd", t - 1)
            else:           # F_{t -> b} = fwd[t] + S(F_{t+1 -> b}),   t = b - j
                assert (t, tp, bs, bi, cs, ci) == (b - j, t + 1, "fwd", t, "bwd", t)
            seen[side].append(t)
    between = [t for t in range(T) if t not in keys]
    assert sorted(seen[0]) == between and sorted(seen[1]) == between, "every in-between frame exactly once per side"
    frames, slots, weights = kr.sides_of(T, keys)
    assert fill_sides(T, keys) == list(zip(frames, slots, weights))
    for t, (s0, s1), (w0, w1) in fill_sides(T, keys):
        a, b = keys[s0], keys[s1]
        assert a < t < b and s1 == s0 + 1 and (w0, w1) == ((b - t) / (b - a), (t - a) / (b - a)) and abs(w0 + w1 - 1) < 1e-15


def test_irregular_keys_pinned():
    from insv2v.keyfill import fill_plan, fill_sides, key_frames
    assert key_frames(17, 4) == [0, 4, 8, 12, 16] and key_frames(9, 8) == [0, 8] and key_frames(10, 4) == [0, 4, 8, 9] and key_frames(1, 2) == [0]
    T, keys = 8, [1, 4, 6]
    assert fill_sides(T, keys) == [(0, (-1, 0), (0.0, 1.0)), (2, (0, 1), (2 / 3, 1 / 3)), (3, (0, 1), (1 / 3, 2 / 3)), (5, (1, 2), (0.5, 0.5)),
                                   (7, (2, -1), (1.0, 0.0))]
    assert fill_plan(T, keys) == [
        [(0, 2, 1, ("bwd", 1), ("fwd", 1)), (0, 5, 4, ("bwd", 4), ("fwd", 4)), (0, 7, 6, ("bwd", 6), ("fwd", 6)),
         (1, 0, 1, ("fwd", 0), ("bwd", 0)), (1, 3, 4, ("fwd", 3), ("bwd", 3)), (1, 5, 6, ("fwd", 5), ("bwd", 5))],
        [(0, 3, 2, ("bwd", 2), ("fwd", 2)), (1, 2, 3, ("fwd", 2), ("bwd", 2))]]
    assert fill_plan(3, [0, 1, 2]) == [] and fill_plan(1, [0]) == []
    for bad in ([], [2, 1], [0, 0], [0, 8], [-1, 3], [0.0, 2], "02", [True, 2]):
        with pytest.raises(ValueError):
            fill_plan(8, bad)
    for T, stride in ((0, 2), (5, 0), (5, True), (2.0, 2)):
        with pytest.raises(ValueError):
            key_frames(T, stride)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _video(T=5, H=8, W=16, dtype=torch.float32):
    return torch.zeros((1, T, 3, H, W), dtype=dtype)


def _flows(T=5, H=8, W=16):
    return dict(fwd=torch.zeros((T - 1, 2, H, W)), bwd=torch.zeros((T - 1, 2, H, W)))


def test_fill_parameter_refusals():
    from insv2v.keyfill import check_fill_args, FILL_DEFAULTS, MAX_STRIDE, FILL_MODES
    from insv2v.mask_track import TRACK_DEFAULTS
    assert MAX_STRIDE == 8 and FILL_MODES == ("residual", "warp")
    assert FILL_DEFAULTS == dict(stride=FILL_DEFAULTS["stride"], mode="residual", sigma=0.1, occlusion=True, alpha=TRACK_DEFAULTS["alpha"], beta=TRACK_DEFAULTS["beta"])
    check_fill_args(**FILL_DEFAULTS)
    for s in (2, 8):
        check_fill_args(stride=s)
    for kw in (dict(stride=1), dict(stride=9), dict(stride=2.0), dict(stride=True), dict(mode="blend"), dict(mode=0), dict(sigma=0), dict(sigma=-1.0),
               dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma="0.1"), dict(occlusion=1), dict(alpha=-0.1), dict(beta=float("inf")), dict(alpha=None)):
        with pytest.raises(ValueError):
            check_fill_args(**kw)


def test_keyframe_fill_refusals_before_any_launch():
    """Every refusal comes from ``check_keyframe_fill_args``: no GPU is there to launch on, and the estimator is never called."""
    from insv2v.keyfill import keyframe_fill, check_keyframe_fill_args, key_flows

    def never(a, b):
        raise AssertionError("the estimator ran before the arguments were checked")
    v, keys = _video(), [0, 4]
    e = v[:, keys]
    check_keyframe_fill_args(v, e, keys, flows=_flows())
    check_keyframe_fill_args(v, e.half(), keys, flow_estimator=never)
    check_keyframe_fill_args(v, v, [0, 1, 2, 3, 4])   # every frame a key: no flow source needed
    ok = dict(source_frames=v, edited_keys=e, keys=keys, flows=_flows())
    bad = [dict(edited_keys=e[0]), dict(edited_keys=v), dict(edited_keys=e.double()), dict(edited_keys=e[..., :8]), dict(source_frames=v[:, :, :2]),
           dict(source_frames=_video(H=1), edited_keys=_video(2, H=1)), dict(keys=[0, 5]), dict(keys=[4, 0]), dict(keys=[0]), dict(keys=()), dict(keys=[0, 4.0]),
           dict(flows=None), dict(flow_estimator=never), dict(flows=dict(fwd=_flows()["fwd"])), dict(flows=_flows(4)), dict(flows=dict(_flows(), both=1)),
           dict(flows=[1]), dict(flows=None, flow_estimator=3), dict(mode="blend"), dict(sigma=0.0), dict(sigma=float("nan")), dict(occlusion=None),
           dict(alpha=-1.0), dict(beta=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            check_keyframe_fill_args(**dict(ok, **kw))
        with pytest.raises(ValueError):
            keyframe_fill(**dict(ok, **kw))
    for kw in (dict(keys=[0, 9]), dict(fwd=None, bwd=None), dict(fwd=torch.zeros((4, 3, 8, 16))), dict(bwd=torch.zeros((3, 2, 8, 16))), dict(bwd=None),
               dict(bwd=None, occlusion=False), dict(fwd=None, occlusion=False), dict(alpha=-1.0), dict(occlusion=3)):
        with pytest.raises(ValueError):
            key_flows(**dict(dict(_flows(), keys=keys), **kw))


def test_check_edit_args_knows_keyframes():
    import inspect
    from insv2v.run_loveu_tgve import check_edit_args, KEYFRAME_KEYS, edit_video
    assert KEYFRAME_KEYS == ("stride", "mode", "sigma", "occlusion", "alpha", "beta")
    names = list(inspect.signature(check_edit_args).parameters)
    assert names[-2:] == ["keyframes", "key_flows"] and names[-3] == "mask_shape", "the new parameters come last, with defaults"
    assert list(inspect.signature(edit_video).parameters)[-2:] == ["keyframes", "key_flows"]
    shape = (1, 5, 3, 8, 16)
    check_edit_args(shape)
    check_edit_args(shape, keyframes=4)
    check_edit_args(shape, keyframes=dict(stride=2, mode="warp", sigma=0.2, occlusion=False, alpha=0.0, beta=1.0), key_flows=_flows())
    check_edit_args(shape, keyframes=dict(sigma=0.2))
    check_edit_args(shape, mask=torch.ones((1, 1, 8, 16)), mask_key=2, keyframes=4, stabilize=True)
    for kw in (dict(keyframes=1), dict(keyframes=9), dict(keyframes=True), dict(keyframes="4"), dict(keyframes=4.0), dict(keyframes=dict(strid=4)),
               dict(keyframes=dict(stride=4, radius=1)), dict(keyframes=dict(mode="blend")), dict(keyframes=dict(sigma=0)), dict(key_flows=_flows()),
               dict(keyframes=4, key_flows=_flows(4)), dict(keyframes=4, key_flows=dict(fwd=_flows()["fwd"])), dict(keyframes=4, key_flows=dict(_flows(), up=1)),
               dict(keyframes=4, key_flows=[]), dict(keyframes=4, mask="auto"), dict(keyframes=dict(stride=2), mask="auto", auto_mask=dict(n_maps=2))):
        with pytest.raises(ValueError):
            check_edit_args(shape, **kw)
    with pytest.raises(ValueError, match="key frames only"):
        check_edit_args(shape, keyframes=4, mask="auto")
    with pytest.raises(ValueError):
        check_edit_args((2, 5, 3, 8, 16), keyframes=4)


def test_cli_flags():
    from insv2v.run_loveu_tgve import build_parser, check_args, keyframe_unit, build_flow_estimator
    from insv2v.keyfill import FILL_DEFAULTS
    p = build_parser()
    a = p.parse_args(["--synthetic", "1"])
    assert (a.key_stride, a.key_mode, a.key_sigma, a.key_no_occlusion) == (None, None, None, False)
    assert keyframe_unit(check_args(a)) == {} and build_flow_estimator(a, "cpu") is None
    a = check_args(p.parse_args(["--synthetic", "1", "--key-stride", "4"]))
    assert keyframe_unit(a) == dict(keyframes=dict(stride=4, mode="residual", sigma=FILL_DEFAULTS["sigma"], occlusion=True))
    a = check_args(p.parse_args(["--units", "u.pt", "--raft-ckpt", "r.pt", "--key-stride", "8", "--key-mode", "warp", "--key-sigma", "0.25", "--key-no-occlusion"]))
    assert keyframe_unit(a) == dict(keyframes=dict(stride=8, mode="warp", sigma=0.25, occlusion=False))
    for argv in (["--units", "u.pt", "--key-stride", "4"], ["--synthetic", "1", "--key-stride", "1"], ["--synthetic", "1", "--key-stride", "9"],
                 ["--synthetic", "1", "--key-stride", "4", "--key-mode", "blend"], ["--synthetic", "1", "--key-stride", "4", "--key-sigma", "0"],
                 ["--synthetic", "1", "--key-mode", "warp"], ["--synthetic", "1", "--key-sigma", "0.2"], ["--synthetic", "1", "--key-no-occlusion"],
                 ["--synthetic", "1", "--key-stride", "4", "--auto-mask"]):
        with pytest.raises(SystemExit):
            check_args(p.parse_args(argv))


def test_score_record_of_a_key_frame_unit():
    """``--score-out`` gains the stride, the key frames and the mean confidence per frame; a unit's ``return_mask`` dict that holds only
    ``keys`` and ``confidence`` is no mask for ``--score-pixels`` or ``--mask-out``."""
    from insv2v.run_loveu_tgve import build_parser, keyframe_record, mask_region
    p = build_parser()
    assert keyframe_record(p.parse_args(["--synthetic", "1"]), dict(keys=[0], confidence=torch.ones((1, 2, 2)))) == {}
    a = p.parse_args(["--synthetic", "1", "--key-stride", "2"])
    conf = torch.stack([torch.ones((2, 2)), torch.tensor([[0.0, 0.5], [0.5, 1.0]]), torch.ones((2, 2))])
    assert keyframe_record(a, dict(keys=[0, 2], confidence=conf)) == {"key_stride": 2, "key_frames": [0, 2], "key_confidence": [1.0, 0.5, 1.0]}
    assert keyframe_record(a, None) == {"key_stride": 2}
    drawn = torch.ones((1, 1, 2, 2))
    assert mask_region(dict(keys=[0, 2], confidence=conf), drawn) is drawn and mask_region(None, drawn) is drawn
    est = dict(mask=torch.zeros((1, 3, 2, 2)), keys=[0, 2], confidence=conf)
    assert mask_region(est, drawn) is est["mask"] and mask_region(dict(est, shaped=drawn * 0.5), drawn) is not est["mask"]


def test_the_symbol_is_declared_bound_and_built():
    import sys
    from insv2v import _lib
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    assert "int insv2v_keyframe_fill(const insv2v_keyfill_desc* d, insv2v_stream_t stream);" in header
    assert "#define INSV2V_KEYFILL_MAX_FRAMES 64" in header and _lib.KEYFILL_MAX_FRAMES == 64 and _lib.KEYFILL_MODES == ("residual", "warp")
    assert _lib.SIGNATURES["insv2v_keyframe_fill"][1][0]._type_ is _lib.KeyfillDesc
    fields = re.search(r"typedef struct insv2v_keyfill_desc \{(.*?)\} insv2v_keyfill_desc;", header, re.S).group(1)
    declared = [n for line in fields.split("\n") for n in re.findall(r"[\s*](\w+)\s*[,;]", line.split("/*")[0])]
    assert declared == [n for n, _ in _lib.KeyfillDesc._fields_]
    assert _lib.ABI_VERSION == 15 and "an addition to ABI 15: no existing struct or entry changes" in header.split("insv2v_keyfill_desc")[0][-6000:]
    assert "int insv2v_abi_version(void) { return 15; }" in open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "elementwise.hip")).read()
    sys.path.insert(0, os.path.join(ROOT, "instruct-video-to-video_amd"))
    try:
        import build
    finally:
        sys.path.pop(0)
    assert "keyfill.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "keyfill.hip"))
    import insv2v
    from insv2v import keyfill, ops
    assert insv2v.keyframe_fill is keyfill.keyframe_fill and insv2v.key_frames is keyfill.key_frames and callable(ops.keyframe_fill)


from driver_fakes import Model as _Model, RecordingPipe as _RecordingPipe   # noqa: E402


def test_a_call_without_keyframes_is_what_it_was(monkeypatch):
    """The pipe sees exactly the keywords it saw before the feature existed, and neither the fill nor the chain is reached; with
    ``keyframes`` and no flow source the RuntimeError comes before the pipe is called at all."""
    from insv2v import ops
    from insv2v.run_loveu_tgve import edit_video, edit_videos
    for name in ("keyframe_fill", "mask_track_step"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: (_ for _ in ()).throw(AssertionError(f"ops.{_n} was reached")))
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
    pipe = _RecordingPipe()
    with pytest.raises(RuntimeError, match="key_flows="):
        edit_video(_Model(), pipe, frames, tc, tc, keyframes=4)
    with pytest.raises(RuntimeError, match="key_flows="):
        edit_videos(_Model(), pipe, [dict(frames=frames, text_cond=tc, text_uncond=tc, keyframes=4), dict(frames=frames[:, :6], text_cond=tc, text_uncond=tc)])
    assert pipe.calls == []
    pipe = _RecordingPipe()   # T = 2: every frame is a key, the unit is edited as if keyframes were not given
    assert edit_video(_Model(), pipe, frames[:, :2], tc, tc, keyframes=4).shape == (1, 2, 3, 16, 24) and pipe.calls == [("call", first)]


# ------------------------------------------------------------------------------------------------------------------ the definition
def _grid_sampler(plane, px, py):
    """S(.) from ``grid_sample``: bilinear, border padding, align_corners - in float64."""
    H, W = plane.shape
    g = torch.tensor([[[[2.0 * px / (W - 1) - 1.0, 2.0 * py / (H - 1) - 1.0]]]], dtype=torch.float64)
    img = torch.from_numpy(np.ascontiguousarray(plane, np.float64))[None, None]
    return float(torch.nn.functional.grid_sample(img, g, mode="bilinear", padding_mode="border", align_corners=True))


@pytest.mark.parametrize("mode", kr.MODES)
def test_float64_definition_against_a_pixel_loop_with_grid_sample(mode):
    """The 5 x 7 case (two-sided frames, holes, a whole invalid side, the fallback rectangle, planted NaN) and the 2 x 2 one-sided one."""
    for case in (kr.CASES[1], kr.CASES[0]):
        inp = kr.case_inputs(*case, "f32", "f32")
        ref = kr.fill_video(inp["A"], inp["E"], inp["key_frame"], inp["frames"], inp["slots"], inp["weights"], inp["G"], inp["U"], kr.CASE_SIGMA, mode, kr.SIGNED)
        out, conf = kr.fill_pixel_loop(inp["A"], inp["E"], inp["key_frame"], inp["frames"], inp["slots"], inp["weights"], inp["G"], inp["U"], kr.CASE_SIGMA,
                                       mode, kr.SIGNED, _grid_sampler)
        assert np.isfinite(out).all() and np.abs(out - ref["out"]).max() < 1e-12 and np.abs(conf - ref["conf"]).max() < 1e-12
        if case is kr.CASES[1]:
            assert (conf == 0).any() and (conf > 0).any(), "the case holds both a hole and blended pixels"


def _exact_case():
    c = kr.translation_case()
    return c["A"], c["G"], c["U"], (c["key_frame"], c["frames"], c["slots"], c["weights"])


@pytest.mark.parametrize("mode", kr.MODES)
def test_a_translating_source_blends_the_keys_residuals_exactly(mode):
    """The closed form of ``translation_case``: exact, everywhere in ``residual`` mode and outside the hole in ``warp`` mode."""
    c = kr.translation_case()
    for dtype in (np.float64, np.float32):
        r = kr.fill_video(c["A"], c["E"], c["key_frame"], c["frames"], c["slots"], c["weights"], c["G"], c["U"], 0.1, mode, kr.ONE, dtype=dtype)
        where = np.ones_like(c["conf"], bool) if mode == "residual" else c["conf"] > 0
        assert np.array_equal(r["conf"], c["conf"]) and set(np.unique(c["conf"])) == {0.0, 0.5, 1.0}
        assert np.array_equal(r["out"][0][:, where[0]], c["want"][0][:, where[0]])


@pytest.mark.parametrize("mode", kr.MODES)
def test_an_unchanged_edit_gives_the_source_exactly(mode):
    """E = A at the keys: out == A_t exactly - in ``residual`` mode whatever the flow is, in ``warp`` mode where the source is constant
    along the flow (here: everywhere a trajectory stays inside the frame, and in the hole only if the source does not move)."""
    inp = kr.case_inputs(*kr.CASES[3], "f32", "f32")
    if mode == "residual":
        E = inp["A"][inp["key_frame"]]
        for dtype in (np.float64, np.float32):
            r = kr.fill_video(inp["A"], E, inp["key_frame"], inp["frames"], inp["slots"], inp["weights"], inp["G"], inp["U"], 0.1, mode, kr.SIGNED, dtype=dtype)
            assert np.array_equal(r["out"], inp["A"][inp["frames"]].astype(dtype))
    A, G, U, (keys, frames, slots, weights) = _exact_case()
    r = kr.fill_video(A, A[keys], keys, frames, slots, weights, G, U, 0.1, mode, kr.ONE)
    some = (U[0] > 0.5).any(0)
    assert np.array_equal(r["out"][0][:, some], A[1][:, some]) and some.mean() > 0.4
    assert np.array_equal(r["conf"][0][(U[0] > 0.5).all(0)], np.ones(int((U[0] > 0.5).all(0).sum())))


@pytest.mark.parametrize("mode", kr.MODES)
def test_identical_frames_and_zero_flow_blend_the_keys_in_time(mode):
    """out_t = A + tw_0 (E_a - A) + tw_1 (E_b - A): dyadic values and weights, so exactly - with valid sides (d2 = 0, w = tw) and in a hole."""
    rng = kr._rng("keyfill.blend")
    H, W, T, keys = 4, 6, 5, [0, 4]
    frames, slots, weights = kr.sides_of(T, keys)
    a = rng.integers(-32, 33, (3, H, W)) / 64.0
    A = np.broadcast_to(a, (T, 3, H, W)).copy()
    E = A[keys] + rng.integers(-16, 17, (2, 3, H, W)) / 64.0
    G = np.zeros((3, 2, 2, H, W))
    for U in (np.ones((3, 2, H, W)), np.zeros((3, 2, H, W))):
        r = kr.fill_video(A, E, keys, frames, slots, weights, G, U, 0.1, mode, kr.SIGNED)
        for i, t in enumerate(frames):
            assert np.array_equal(r["out"][i], a + (4 - t) / 4 * (E[0] - a) + t / 4 * (E[1] - a))
        assert (r["conf"] == U[:, 0]).all()


def test_the_underflow_case_takes_the_fallback():
    c = kr.UNDERFLOW
    for dt in kr.DTYPES:
        inp = kr.underflow_inputs(dt)
        for dtype in (np.float64, np.float32):
            r = kr.fill_video(inp["A"], inp["E"], inp["key_frame"], inp["frames"], inp["slots"], inp["weights"], inp["G"], inp["U"], c["sigma"], "residual",
                              kr.SIGNED, dtype=dtype)
            assert (r["conf"] == 0).all() and (r["n_active"] == 2).all() and r["max_arg"] > 1e4
            want = inp["A"][1] + 0.5 * (inp["E"][0] - inp["A"][0]) + 0.5 * (inp["E"][1] - inp["A"][2])
            assert np.abs(r["out"][0] - want).max() < (1e-12 if dtype is np.float64 else 1e-6)


# ------------------------------------------------------------------------------------------------------------------ misreadings
@pytest.mark.parametrize("mutate", kr.MUTATIONS)
def test_a_planted_misreading_misses_by_ten_bounds(mutate):
    """On the GPU file's own inputs (NaN planted): the worst element of every misreading is at least 10 bounds away from the reference, or
    a NaN where the reference is finite (the GPU file refuses any NaN in an output), in both dtypes - so the GPU comparison would catch
    it."""
    assert len(kr.MUTATIONS) >= 10
    for case in kr.MUTATION_CASES:
        for dt in kr.DTYPES:
            inp, ref = kr.case_inputs(*case, dt, dt), kr.case_reference(*case, dt, dt, "residual")
            got = kr.fill_video(inp["A"], inp["E"], inp["key_frame"], inp["frames"], inp["slots"], inp["weights"], inp["G"], inp["U"], kr.CASE_SIGMA,
                                "residual", kr.SIGNED, mutate=mutate)["out"]
            with np.errstate(invalid="ignore"):
                dep = np.abs(got - ref["out"]) / ref["bound"]
            nans = int(np.isnan(got).sum())
            worst = float(np.nanmax(dep))
            print(f"[keyfill] {mutate} {case[0]}x{case[1]} {dt}: worst departure {worst:.1f} bounds, {nans} NaN")
            assert worst >= kr.MIN_DEPARTURE or nans > 0, (mutate, dt, worst)
            if mutate in ("mul_zero",):
                assert worst >= kr.MIN_DEPARTURE or nans > 0, "weighing an inactive side by 0 must leak what it reaches"


# ------------------------------------------------------------------------------------------------------------------ the float32 restatement
@pytest.mark.parametrize("case", kr.CASES, ids=lambda c: f"{c[0]}x{c[1]}xT{c[2]}")
def test_float32_restatement_measured(case):
    for mode in kr.MODES:
        for edt, adt in COMBOS:
            inp, ref = kr.case_inputs(*case, edt, adt), kr.case_reference(*case, edt, adt, mode)
            share = float((ref["terms"] / ref["bound"]).max())
            print(f"[keyfill] restatement {case[0]}x{case[1]} T={case[2]} keys={case[3]} E {edt} A {adt} {mode}: worst |float32 - float64| {ref['worst']:.3e} "
                  f"(conf {ref['worst_conf']:.3e}); bound {ref['bound'].min():.3e} .. {ref['bound'].max():.3e}, the exp-argument term at most {share:.3f} of "
                  f"it; largest d2/(2 sigma^2) {ref['max_arg']:.1f}; holes {int((ref['conf'] == 0).sum())}; NaN planted {inp['planted']}")
            one = kr.rounding(ref["out"], edt).max()
            # x + G is rounded to float32 before the taps are taken: up to 2^-24 max(H, W) of a pixel, in x and in y, times the steepest
            # step between two neighbouring taps of E or A (3 x 300: the largest share of that case's departure)
            step = max(float(np.nanmax(np.abs(np.diff(P, axis=ax)))) for P in (inp["A"], inp["E"]) for ax in (2, 3))
            coord = 2 * 2.0 ** -24 * max(case[0], case[1]) * step
            assert ref["worst"] <= (4 if edt == "f16" else 64) * one + ref["terms"].max() + coord, "the restatement is a float32 evaluation: a few roundings, not more"
            assert (ref["bound"] >= kr.rounding(ref["out"], edt)).all() and ref["max_arg"] < kr.MAX_ARG
            assert inp["planted"]["G"] > 0 and (case[0] < 5 or (ref["conf"] == 0).any()), "NaN in G, and from 5 x 7 up the fallback rectangle"
