"""The temporal filter that stabilizes an edit, without a GPU: the argument checks and their refusals, the launch
schedule, every closed form of the definition on the float64 reference (tests/temporal_filter_ref.py), nine planted misreadings - each
must miss the reference by at least 10 bounds on the GPU file's own inputs - and the float32 restatement in the kernel's operation order,
measured against float64 and printed (``[temporal_filter]`` lines): its worst departure is what the GPU bound is calibrated on.

Measured here (float32 restatement against float64, worst element of a case): 4.0e-8 / 1.2e-7 / 1.1e-7 / 2.1e-7 for the four fp32 cases
(2 x 2, 16 x 24, 17 x 33, 40 x 56) and 1.8e-4 / 2.4e-4 / 2.4e-4 / 2.4e-4 for the fp16 ones, where the store's rounding is all there is; the
derived exp-argument term is at most 0.34 of an fp32 bound.  The misreadings miss by 58 bounds (nearest, fp16) to 960 000 (fp32)."""
import numpy as np
import pytest
import torch

import temporal_filter_ref as tr


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_filter_parameter_refusals():
    from insv2v.temporal_filter import check_filter_args, FILTER_DEFAULTS
    from insv2v.mask_track import TRACK_DEFAULTS
    check_filter_args()
    check_filter_args(**FILTER_DEFAULTS)
    assert FILTER_DEFAULTS["alpha"] == TRACK_DEFAULTS["alpha"] and FILTER_DEFAULTS["beta"] == TRACK_DEFAULTS["beta"]
    assert (FILTER_DEFAULTS["radius"], FILTER_DEFAULTS["sigma"], FILTER_DEFAULTS["strength"]) == (2, 0.1, 1.0)
    for kw in (dict(radius=0), dict(radius=5), dict(radius=2.0), dict(radius=True), dict(sigma=0), dict(sigma=-0.1), dict(sigma=float("nan")),
               dict(sigma=float("inf")), dict(sigma="0.1"), dict(strength=0), dict(strength=1.5), dict(strength=float("nan")), dict(strength=True),
               dict(occlusion=1), dict(alpha=-1), dict(beta=float("inf")), dict(alpha=None)):
        with pytest.raises(ValueError):
            check_filter_args(**kw)
    for r in (1, 2, 3, 4):
        check_filter_args(radius=r, strength=1e-3, sigma=1e-3)


def _video(T=3, H=8, W=12, dtype=torch.float32):
    return torch.zeros((1, T, 3, H, W), dtype=dtype)


def _flows(T=3, H=8, W=12):
    return dict(fwd=torch.zeros((T - 1, 2, H, W)), bwd=torch.zeros((T - 1, 2, H, W)))


def test_stabilize_refusals_before_any_launch():
    """Every refusal comes from ``check_stabilize_args``: no GPU is there to launch on, and the estimator is never called."""
    from insv2v.temporal_filter import stabilize, check_stabilize_args

    def never(a, b):
        raise AssertionError("the estimator ran before the arguments were checked")
    v = _video()
    check_stabilize_args(v, v, flows=_flows())
    check_stabilize_args(v, v.half(), flows=_flows())
    check_stabilize_args(v, v, flow_estimator=never, mask=torch.ones((1, 1, 8, 12)))
    check_stabilize_args(v, v, flows=dict(fwd=_flows()["fwd"]), occlusion=False)
    check_stabilize_args(v[:, :1], v[:, :1])   # T = 1 needs no flow source
    bad = [dict(edited_frames=v[0]), dict(edited_frames=_video(4)), dict(edited_frames=v.double()), dict(source_frames=v[:, :, :2]),
           dict(flows=None), dict(flows=_flows(), flow_estimator=never), dict(flows=dict(fwd=_flows()["fwd"])), dict(flows=dict(bwd=_flows()["bwd"]), occlusion=False),
           dict(flows=_flows(4)), dict(flows=dict(_flows(), both=1)), dict(flows=[1]), dict(flow_estimator=3), dict(flows=_flows(), mask=torch.ones((1, 2, 8, 12))),
           dict(flows=_flows(), mask=torch.ones((8, 12))), dict(flows=_flows(), radius=0), dict(flows=_flows(), radius=5), dict(flows=_flows(), sigma=0.0),
           dict(flows=_flows(), strength=0.0), dict(flows=_flows(), strength=1.01), dict(flows=_flows(), occlusion=None), dict(flows=_flows(), alpha=-1.0),
           dict(source_frames=_video(3, 1, 12), edited_frames=_video(3, 1, 12), flows=_flows(3, 1, 12))]
    for kw in bad:
        args = dict(dict(source_frames=v, edited_frames=v), **kw)
        with pytest.raises(ValueError):
            stabilize(args.pop("source_frames"), args.pop("edited_frames"), **args)
    assert stabilize(v[:, :1], v[:, :1], flow_estimator=never) is not None   # T = 1: the edit, nothing launched, no flow computed


def test_temporal_filter_and_neighbour_flows_refusals():
    from insv2v.temporal_filter import temporal_filter, neighbour_flows, check_temporal_filter_args
    T, H, W = 3, 8, 12
    e = torch.zeros((T, 3, H, W))
    G, U = torch.zeros((2, T, 2, H, W)), torch.zeros((2, T, H, W))
    check_temporal_filter_args(e, e.half(), G, U, (-1, 1))
    for args, kw in (((e, e[:2], G, U, (-1, 1)), {}), ((e, e, G, U, (-1, 0)), {}), ((e, e, G, U, (-1, 5)), {}), ((e, e, G, U, ()), {}),
                     ((e, e, G, U, (-1, 1, 2)), {}), ((e, e, G[:, :, :1], U, (-1, 1)), {}), ((e, e, G, U[:1], (-1, 1)), {}),
                     ((e, e, G, U, (-1, 1)), dict(sigma=0)), ((e, e, G, U, (-1, 1)), dict(strength=2)), ((e, e, G, U, (-1, 1)), dict(guide_affine=(1.0,))),
                     ((e, e, G, U, (-1, 1)), dict(guide_affine=(float("nan"), 0.0))), ((e.double(), e, G, U, (-1, 1)), {}), ((e[:, :, :1], e[:, :, :1], G[..., :1, :], U[:, :, :1], (-1, 1)), {})):
        with pytest.raises(ValueError):
            temporal_filter(*args, **kw)
    f = torch.zeros((T - 1, 2, H, W))
    for args, kw in (((f,), {}), ((f, None), dict(occlusion=True)), ((None, None), dict(occlusion=False)), ((f, f[:1]), {}), ((f, f), dict(radius=0)),
                     ((f, f), dict(radius=5)), ((f, f), dict(alpha=-1)), ((f[:, :1], f[:, :1]), {}), ((f[..., :1], f[..., :1]), {})):
        with pytest.raises(ValueError):   # occlusion=True without both flow sets, and the rest: before any launch
            neighbour_flows(*args, **kw)


def test_check_edit_args_knows_stabilize():
    from insv2v.run_loveu_tgve import check_edit_args, STABILIZE_KEYS
    assert set(STABILIZE_KEYS) == {"radius", "sigma", "strength", "occlusion", "alpha", "beta"}
    shape = (1, 3, 3, 8, 16)
    check_edit_args(shape)
    check_edit_args(shape, stabilize=True)
    check_edit_args(shape, stabilize=dict(radius=1, sigma=0.2, strength=0.5, occlusion=False), stabilize_flows=dict(fwd=torch.zeros((2, 2, 8, 16))))
    check_edit_args(shape, stabilize=True, stabilize_flows=_flows(3, 8, 16))
    for kw in (dict(stabilize=dict(radious=1)), dict(stabilize=dict(radius=9)), dict(stabilize=dict(sigma=0)), dict(stabilize=dict(strength=0)),
               dict(stabilize=3), dict(stabilize="yes"), dict(stabilize_flows=_flows(3, 8, 16)), dict(stabilize=True, stabilize_flows=_flows(4, 8, 16)),
               dict(stabilize=True, stabilize_flows=dict(fwd=torch.zeros((2, 2, 8, 16)))), dict(stabilize=True, stabilize_flows=dict(fwd=torch.zeros((2, 2, 8, 16)), up=1)),
               dict(stabilize=True, stabilize_flows=[])):
        with pytest.raises(ValueError):
            check_edit_args(shape, **kw)
    with pytest.raises(ValueError):
        check_edit_args((2, 3, 3, 8, 16), stabilize=True)


def test_cli_flags():
    from insv2v.run_loveu_tgve import build_parser, check_args, stabilize_unit
    p = build_parser()
    a = check_args(p.parse_args(["--synthetic", "1", "--stabilize", "--stabilize-radius", "3", "--stabilize-sigma", "0.2", "--stabilize-strength", "0.5",
                                 "--stabilize-no-occlusion"]))
    assert stabilize_unit(a) == dict(stabilize=dict(radius=3, sigma=0.2, strength=0.5, occlusion=False))
    assert stabilize_unit(check_args(p.parse_args(["--synthetic", "1"]))) == {}
    assert stabilize_unit(check_args(p.parse_args(["--synthetic", "1", "--stabilize"]))) == dict(stabilize=dict(radius=2, sigma=0.1, strength=1.0, occlusion=True))
    for argv in (["--units", "u.pt", "--stabilize"], ["--synthetic", "1", "--stabilize", "--stabilize-radius", "5"], ["--synthetic", "1", "--stabilize-radius", "1"],
                 ["--synthetic", "1", "--stabilize", "--stabilize-sigma", "0"], ["--synthetic", "1", "--stabilize", "--stabilize-strength", "1.5"],
                 ["--synthetic", "1", "--stabilize-no-occlusion"]):
        with pytest.raises(SystemExit):
            check_args(p.parse_args(argv))
    check_args(p.parse_args(["--units", "u.pt", "--stabilize", "--raft-ckpt", "raft.pt"]))


# ------------------------------------------------------------------------------------------------------------------ the schedule
@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("R", [1, 2, 4])
def test_filter_plan_launch_counts(T, R):
    from insv2v.temporal_filter import filter_plan, neighbour_offsets
    plan = filter_plan(T, R)
    assert len(plan) == min(R, T - 1)               # one launch per distance that fits the video: R of them from T = R + 1 frames up
    for j, step in enumerate(plan, 1):
        assert len(step) == 2 * (T - j)             # both directions of every frame that has the neighbour, in ONE launch
        assert sorted(t for k, t, *_ in step if k == j) == list(range(T - j)) and sorted(t for k, t, *_ in step if k == -j) == list(range(j, T))
        for k, t, tp, b, c in step:
            assert abs(k) == j and tp == t + (1 if k > 0 else -1) and 0 <= t + k < T
            assert (b, c) == ((("fwd", t), ("bwd", t)) if k > 0 else (("bwd", t - 1), ("fwd", t - 1)))
    assert neighbour_offsets(R) == tr.offsets_of(R) and neighbour_offsets(2, bwd=False) == (1, 2) and neighbour_offsets(2, fwd=False) == (-2, -1)


# ------------------------------------------------------------------------------------------------------------------ closed forms (float64)
def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_no_valid_neighbour_and_constant_video_return_the_edit_bit_for_bit():
    (T, H, W, R), dt = tr.CASES[2], "f32"
    inp = tr.case_inputs(T, H, W, R, dt)
    E = inp["E"].copy()
    E[0, 0, 0, 0] = -0.0
    out = tr.filter_video(E, inp["A"], inp["G"], np.zeros_like(inp["U"]), inp["offsets"])["out"]
    assert _bits_equal(out, E)
    const = np.broadcast_to(np.array([0.3, -0.7, 0.11])[None, :, None, None], E.shape).copy()
    for dtype in (np.float64, np.float32):
        out = tr.filter_video(const, inp["A"], inp["G"], inp["U"], inp["offsets"], dtype=dtype)["out"]
        assert np.array_equal(out, const.astype(dtype))
    # a pixel without a valid neighbour inside a case that has them
    ref = tr.case_reference(T, H, W, R, dt)
    lone = ref["n_valid"] == 0
    assert lone.any() and (~lone).any()
    assert np.array_equal(ref["out"][np.broadcast_to(lone[:, None], E.shape)], inp["E"][np.broadcast_to(lone[:, None], E.shape)])


def test_two_frames_average_exactly():
    """T = 2, R = 1, zero flow, A_0 == A_1, dyadic E, s = 1: both frames become (E_0 + E_1) / 2; the same under an integer translation,
    wherever the neighbour is valid."""
    for shift in ((0, 0), (2, -1)):
        tv = tr.translation_video(2, 9, 13, shift, deltas=[0.0, 0.25])
        G, U, offs = tr.translation_neighbours(2, 9, 13, shift, 1)
        E = tv["E"].copy()
        E[1] += np.arange(13) / 64.0     # not a constant offset only
        for dtype in (np.float64, np.float32):
            out = tr.filter_video(E, tv["A"], G, U, offs, 0.1, 1.0, tr.ONE, dtype=dtype)["out"].astype(np.float64)
            dx, dy = shift
            ys, xs = np.mgrid[0:9, 0:13]
            for t, k in ((0, 1), (1, -1)):
                v = U[offs.index(k), t] > 0.5
                sy, sx = np.clip(ys + k * dy, 0, 8), np.clip(xs + k * dx, 0, 12)
                want = np.where(v, (E[t] + E[1 - t][:, sy, sx]) / 2, E[t])
                assert np.array_equal(out[t], want)
            assert (U.sum() == 2 * (9 - abs(dy)) * (13 - abs(dx)))


def test_flicker_closed_form_and_interior_share():
    c = tr.FLICKER
    T, H, W, shift, R, s = c["T"], c["H"], c["W"], c["shift"], c["radius"], c["strength"]
    inside = tr.interior(T, H, W, shift, R)
    assert inside.mean() >= 0.5, "the all-valid interior must be at least half the frame"
    tv = tr.translation_video(T, H, W, shift, c["deltas"])
    G, U, offs = tr.translation_neighbours(T, H, W, shift, R)
    out = tr.filter_video(tv["E"], tv["A"], G, U, offs, c["sigma"], s, tr.ONE)["out"]
    want = tr.flicker_closed_form(c["deltas"], R, s)
    got = (out - tv["A"])[:, :, inside]
    assert np.abs(got - want[:, None, None]).max() <= 2.0 ** -50
    edge = (out - tv["A"])[0, 0][~inside]
    assert (np.abs(edge - want[0]) > 1e-3).any(), "a pixel whose trajectory leaves the frame sees a smaller valid set and another delta'"
    before, after = np.diff(c["deltas"]) ** 2, np.diff(want) ** 2
    assert (after < before).all(), (before, after)
    # s < 1 and R = 1 obey the same formula
    out = tr.filter_video(tv["E"], tv["A"], *tr.translation_neighbours(T, H, W, shift, 1), 0.1, 0.5, tr.ONE)["out"]
    got = (out - tv["A"])[:, :, tr.interior(T, H, W, shift, 1)]
    assert np.abs(got - tr.flicker_closed_form(c["deltas"], 1, 0.5)[:, None, None]).max() <= 2.0 ** -50


def test_the_guard_keeps_a_pixel_whose_source_changed():
    """A rectangle whose SOURCE colour jumps by 1.0 in the next frame has d2 = 1 and weight exp(-50): the edit stays, the pixels around
    it are averaged."""
    H, W = 8, 12
    A = np.zeros((2, 3, H, W))
    A[1, :, 2:5, 3:8] = 1.0
    rng = tr._rng("temporal_filter.guard")
    E = rng.integers(-32, 33, (2, 3, H, W)) / 64.0
    G, U, offs = tr.translation_neighbours(2, H, W, (0, 0), 1)
    r = tr.reference(E, A, G, U, offs, 0.1, 1.0, tr.ONE, "f32")
    rect = np.zeros((H, W), bool)
    rect[2:5, 3:8] = True
    assert (np.abs(r["out"] - E)[:, :, rect] <= np.exp(-50.0) * 2).all() and (np.abs(r["out"] - E)[:, :, rect] <= r["bound"][:, :, rect]).all()
    assert np.array_equal(r["out"][:, :, ~rect], np.broadcast_to(((E[0] + E[1]) / 2)[:, ~rect], (2, 3, (~rect).sum())))


def test_nan_in_a_frame_nothing_valid_reaches_does_not_leak():
    for T, H, W, R in tr.CASES[1:]:
        inp = tr.case_inputs(T, H, W, R, "f32")
        assert inp["nan_A"].sum() >= 9 and inp["nan_E"].sum() >= 9, "the case plants no NaN"
        ref = tr.case_reference(T, H, W, R, "f32")
        assert np.isfinite(ref["out"]).all()
        out = tr.filter_video(tr.planted(inp["E"], inp["nan_E"]), ref["A"], inp["G"], inp["U"], inp["offsets"], tr.CASE_SIGMA, tr.CASE_STRENGTH)["out"]
        own = np.broadcast_to(inp["nan_E"][:, None], out.shape)
        assert np.isnan(out[own]).all() and np.array_equal(out[~own], ref["out"][~own]), "a NaN of the edit stays in its own pixel"
        assert (inp["U"][:, :, :, :].sum((2, 3))[[i for i, k in enumerate(inp["offsets"]) if k < 0], 0] == 0).all()   # out-of-video slabs


# ------------------------------------------------------------------------------------------------------------------ misreadings
@pytest.mark.parametrize("mutate", tr.MUTATIONS)
def test_a_planted_misreading_misses_by_ten_bounds(mutate):
    """On the GPU file's own inputs (NaN planted): the worst element of every misreading is at least 10 bounds away from the reference,
    in both dtypes - so the GPU comparison would catch it.  ``mul_zero`` shows as a NaN where the reference is finite."""
    for T, H, W, R in tr.MUTATION_CASES:
        for dt in tr.DTYPES:
            inp, ref = tr.case_inputs(T, H, W, R, dt), tr.case_reference(T, H, W, R, dt)
            got = tr.filter_video(inp["E"], ref["A"], inp["G"], inp["U"], inp["offsets"], tr.CASE_SIGMA, tr.CASE_STRENGTH, mutate=mutate)["out"]
            if mutate == "mul_zero":
                assert np.isnan(got).any(), "weighing an invalid neighbour by 0 must leak its NaN"
                continue
            with np.errstate(invalid="ignore"):
                dep = np.abs(got - ref["out"]) / ref["bound"]
            worst = float(np.nanmax(dep))     # over the elements that stay finite: a NaN the misreading picks up is not counted
            print(f"[temporal_filter] {mutate} {T}x{H}x{W} R={R} {dt}: worst departure {worst:.1f} bounds, {int(np.isnan(got).sum())} NaN")
            assert worst >= tr.MIN_DEPARTURE, (mutate, dt, worst)


# ------------------------------------------------------------------------------------------------------------------ the float32 restatement
@pytest.mark.parametrize("T,H,W,R", tr.CASES)
def test_float32_restatement_measured(T, H, W, R):
    for dt in tr.DTYPES:
        ref = tr.case_reference(T, H, W, R, dt)
        share = float((ref["terms"][:, None] / ref["bound"]).max())
        print(f"[temporal_filter] restatement {T}x{H}x{W} R={R} {dt}: worst |float32 - float64| {ref['worst']:.3e}; bound {ref['bound'].min():.3e} .. "
              f"{ref['bound'].max():.3e}, the exp-argument term at most {share:.3f} of it; valid neighbours per pixel {ref['n_valid'].mean():.2f}")
        one = tr.rounding(ref["out"], dt).max()
        assert ref["worst"] <= (4 if dt == "f16" else 64) * one, "the restatement is a float32 evaluation: a few roundings, not more"
        assert (ref["bound"] >= tr.rounding(ref["out"], dt)).all()
