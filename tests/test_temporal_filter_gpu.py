"""Stabilizing an edit along the source video's optical flow, on the GPU: insv2v_temporal_filter against the float64
definition (tests/temporal_filter_ref.py), its bit-exact cases, determinism and refusals, the closed form that shows the filter does what
it is for, the host chain of ``neighbour_flows`` against ``propagate_mask``, ``stabilize=`` behind ``edit_video`` / ``edit_videos`` on the
tiny UNet / VAE, the RAFT route and the command line.

Bound per element, always against float64 and never against the kernel (tests/temporal_filter_ref.py states it,
tests/test_temporal_filter_cpu.py prints the measurements behind it): 4 x the float32 restatement's worst departure on the case's inputs
(fp32 cases 4.0e-8 .. 2.1e-7, fp16 cases 1.8e-4 .. 2.4e-4: the store's rounding) + the derived term for the rounding of the
exponential's argument, floored at one rounding of the output dtype.  G and U are inputs, so the kernel takes no decision and no pixel
is left out of the comparison.  Every test prints what it measured on the device (``[temporal_filter]`` lines: the error as a share of
its bound); profiles/temporal_filter_pytest_gpu.txt holds a run.  The pipes of this file run without graph capture, as those of
tests/test_pixel_score_gpu.py."""
import math

import numpy as np
import pytest
import torch

import pixel_score_ref as pr
import temporal_filter_ref as tr
from test_model_gpu import tiny_unet   # noqa: F401  (the module-scoped fixture, instantiated for this module)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EAGER = dict(use_graph=False)
SENT = 777.0
TORCH = {"f16": torch.float16, "f32": torch.float32}


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _crop(arr, dt, grow=(1, 1, 5, 7), at=(1, 1, 2, 3), fill=float("nan")):
    """(whole buffer, view): [T,3,H,W] as a crop of a larger tensor filled with ``fill``: every stride differs from the dense one."""
    a = torch.from_numpy(np.ascontiguousarray(arr)).to(TORCH[dt])
    big = torch.full(tuple(s + g for s, g in zip(a.shape, grow)), fill, device=DEV, dtype=TORCH[dt])
    view = big[tuple(slice(o, o + s) for o, s in zip(at, a.shape))]
    view.copy_(a.to(DEV))
    return big, view


def _out(shape, dt, grow=(2, 1, 3, 9), at=(1, 0, 2, 4)):
    """(sentinel buffer, NaN-prefilled view inside it, the buffer's mask of sentinel elements)."""
    big, view = _crop(np.full(shape, np.nan), dt, grow, at, fill=SENT)
    outside = torch.ones(big.shape, dtype=torch.bool, device=DEV)
    outside[tuple(slice(o, o + s) for o, s in zip(at, shape))] = False
    return big, view, outside


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _run(E, A, G, U, offsets, dt, sigma, strength, affine):
    """One launch on strided views inside NaN-filled buffers, into a NaN-prefilled view of a sentinel buffer -> the output as float64."""
    from insv2v import ops
    e, a = _crop(E, dt)[1], _crop(A, dt, grow=(2, 0, 3, 9), at=(0, 0, 1, 8))[1]
    big, view, outside = _out(E.shape, dt)
    got = ops.temporal_filter(e, a, _dev32(G), _dev32(U), offsets, sigma=sigma, strength=strength, guide_affine=affine, out=view)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr() and bool((big[outside] == SENT).all()), "the kernel wrote outside its output"
    return _np(view)


# ------------------------------------------------------------------------------------------------------------------ 1. kernel vs float64
@pytest.mark.parametrize("dt", tr.DTYPES)
@pytest.mark.parametrize("T,H,W,R", tr.CASES)
def test_kernel_vs_float64(T, H, W, R, dt):
    """Smooth seeded G of a few pixels, U with holes and whole out-of-video slabs, NaN planted in A wherever only invalid neighbours can
    reach: every element within its bound, no NaN in the output, the sentinels untouched.  Then the same with NaN planted in E wherever
    no valid tap reads it: such a pixel's own output is NaN (out = E there) and nothing else changes by a bit."""
    inp, ref = tr.case_inputs(T, H, W, R, dt), tr.case_reference(T, H, W, R, dt)
    got = _run(inp["E"], ref["A"], inp["G"], inp["U"], inp["offsets"], dt, tr.CASE_SIGMA, tr.CASE_STRENGTH, tr.SIGNED)
    assert not np.isnan(got).any(), f"{int(np.isnan(got).sum())} NaN in the output"
    err = np.abs(got - ref["out"])
    share = err / ref["bound"]
    at = np.unravel_index(share.argmax(), share.shape)
    print(f"[temporal_filter] {T}x{H}x{W} R={R} {dt}: worst error {err.max():.3e}, worst share of the bound {share.max():.3f} (bound there "
          f"{ref['bound'][at]:.3e}; restatement worst {ref['worst']:.3e}); NaN planted in A: {int(inp['nan_A'].sum())} pixels")
    assert (err <= ref["bound"]).all(), (np.argwhere(err > ref["bound"])[:5].tolist(), float(share.max()))
    lone = np.broadcast_to((ref["n_valid"] == 0)[:, None], got.shape)
    assert np.array_equal(got[lone], inp["E"][lone]), "a pixel without a valid neighbour must come back as it is"
    got2 = _run(tr.planted(inp["E"], inp["nan_E"]), ref["A"], inp["G"], inp["U"], inp["offsets"], dt, tr.CASE_SIGMA, tr.CASE_STRENGTH, tr.SIGNED)
    own = np.broadcast_to(inp["nan_E"][:, None], got.shape)
    assert np.isnan(got2[own]).all() and np.array_equal(got2[~own], got[~own]), "a NaN of the edit must stay in its own pixel"


# ------------------------------------------------------------------------------------------------------------------ 2. bit-exact cases
def _case(dt="f32"):
    T, H, W, R = tr.CASES[2]
    return tr.case_inputs(T, H, W, R, dt), tr.case_reference(T, H, W, R, dt)


@pytest.mark.parametrize("dt", tr.DTYPES)
def test_no_valid_neighbour_and_constant_edit_come_back_bit_for_bit(dt):
    inp, ref = _case(dt)
    E = inp["E"].copy()
    E[0, 0, 0, :2] = (-0.0, 0.0)
    got = _run(E, ref["A"], inp["G"], np.zeros_like(inp["U"]), inp["offsets"], dt, 0.1, 1.0, tr.SIGNED)
    assert np.array_equal(got, E) and np.array_equal(np.signbit(got), np.signbit(E))
    const = tr.stored(np.broadcast_to(np.array([0.3, -0.7, 0.11])[None, :, None, None], E.shape), dt)
    got = _run(const, ref["A"], inp["G"], inp["U"], inp["offsets"], dt, 0.1, 1.0, tr.SIGNED)
    assert np.array_equal(got, const)


@pytest.mark.parametrize("shift", [(0, 0), (2, -1), (-1, 3)])
@pytest.mark.parametrize("dt", tr.DTYPES)
def test_two_frames_average_exactly_and_leave_no_warp_error(dt, shift):
    """T = 2, R = 1, A_1 = A_0 translated, dyadic E, s = 1: each frame becomes (E_t + the other frame along the flow) / 2 wherever the
    neighbour is valid - bit for bit - and the edit itself elsewhere; with E_1 = E_0 translated plus a constant the two outputs agree along
    the flow, so ``pixel_score.warp_error`` of the result is exactly 0.  G and U come from ``neighbour_flows`` and are the closed form."""
    from insv2v import temporal_filter as tf, pixel_score as ps
    H, W = 9, 13
    tv = tr.translation_video(2, H, W, shift, deltas=[0.0, 0.25])
    fwd, bwd = _dev32(tv["fwd"]), _dev32(tv["bwd"])
    nb = tf.neighbour_flows(fwd, bwd, radius=1)
    G, U, offs = tr.translation_neighbours(2, H, W, shift, 1)
    assert nb["offsets"] == offs and np.array_equal(_np(nb["flow"]), G) and np.array_equal(_np(nb["valid"]), U)
    e, a = _crop(tv["E"], dt)[1], _crop(tv["A"], dt)[1]
    out = tf.temporal_filter(e, a, nb["flow"], nb["valid"], nb["offsets"], sigma=0.1, strength=1.0)
    got = _np(out)
    ys, xs = np.mgrid[0:H, 0:W]
    for t, k in ((0, 1), (1, -1)):
        sy, sx = np.clip(ys + k * shift[1], 0, H - 1), np.clip(xs + k * shift[0], 0, W - 1)
        want = np.where(U[offs.index(k), t] > 0.5, (tv["E"][t] + tv["E"][1 - t][:, sy, sx]) / 2, tv["E"][t])
        assert np.array_equal(got[t], want)
    r = ps.warp_error(out, fwd, bwd)
    assert r["warp_error"].tolist() == [0.0] and r["valid_count"][0] == (H - abs(shift[1])) * (W - abs(shift[0]))
    assert ps.warp_error(e, fwd, bwd)["warp_error"].tolist() == [0.25 ** 2]   # what the filter removed


def test_two_runs_agree_bitwise_also_on_a_second_stream():
    from insv2v import ops
    inp, ref = _case("f16")
    e, a, G, U = _crop(inp["E"], "f16")[1], _crop(ref["A"], "f16")[1], _dev32(inp["G"]), _dev32(inp["U"])

    def run():
        return ops.temporal_filter(e, a, G, U, inp["offsets"], sigma=tr.CASE_SIGMA, strength=tr.CASE_STRENGTH, guide_affine=tr.SIGNED)
    first, second = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert _same_bits(first, second) and _same_bits(first, third) and bool(torch.isfinite(first).all())


def test_refusals_leave_the_output_untouched():
    from insv2v import ops, _lib
    inp, ref = _case("f32")
    T, _, H, W = inp["E"].shape
    offs = inp["offsets"]
    e, a, G, U = _crop(inp["E"], "f32")[1], _crop(ref["A"], "f32")[1], _dev32(inp["G"]), _dev32(inp["U"])
    big, view, outside = _out(inp["E"].shape, "f32")

    def untouched():
        torch.cuda.synchronize()
        return bool((big[outside] == SENT).all() and torch.isnan(view).all())
    ok = dict(sigma=0.1, strength=1.0, guide_affine=tr.SIGNED, out=view)
    bad = [dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=1e-30), dict(strength=0.0), dict(strength=1.5),
           dict(strength=float("nan")), dict(guide_affine=(float("inf"), 0.0)), dict(guide_affine=(0.5, float("nan")))]
    for kw in bad:
        with pytest.raises(_lib.HipKernelError):
            ops.temporal_filter(e, a, G, U, offs, **dict(ok, **kw))
        assert untouched(), kw
    for o in ((0,) + offs[1:], (5,) + offs[1:], (-5,) + offs[1:], offs[:-1] + (0,)):   # an offset of 0 or beyond +-4
        with pytest.raises(_lib.HipKernelError):
            ops.temporal_filter(e, a, G, U, o, **ok)
        assert untouched(), o
    with pytest.raises(_lib.HipKernelError):   # K = 0
        ops.temporal_filter(e, a, G[:0], U[:0], (), **ok)
    with pytest.raises(_lib.HipKernelError):   # K = 9
        ops.temporal_filter(e, a, G[:1].expand(9, -1, -1, -1, -1).contiguous(), U[:1].expand(9, -1, -1, -1).contiguous(), (1,) * 9, **ok)
    for sl in ((slice(None), slice(None), slice(0, 1)), (slice(None), slice(None), slice(None), slice(0, 1))):   # H = 1, W = 1
        e1, a1, v1 = e[sl], a[sl], view[sl]
        g1, u1 = G[(slice(None), *sl)].contiguous(), U[(slice(None), sl[0], *sl[2:])].contiguous()
        with pytest.raises(_lib.HipKernelError):
            ops.temporal_filter(e1, a1, g1, u1, offs, **dict(ok, out=v1))
        assert untouched()
    # aliasing: the output over the edit, over the guide, inside the flows, inside the validity (fp32: the dtypes agree)
    flat_g, flat_u = G.view(-1), U.view(-1)
    n = T * 3 * H * W
    for alias in (e, a, flat_g[5:5 + n].view(T, 3, H, W), flat_u[3:3 + n].view(T, 3, H, W)):
        keep = alias.clone()
        with pytest.raises(_lib.HipKernelError):
            ops.temporal_filter(e, a, G, U, offs, **dict(ok, out=alias))
        torch.cuda.synchronize()
        assert _same_bits(alias, keep) and untouched()
    # NULL pointers and T < 1, straight at the entry
    lib = _lib.load()

    def desc(**kw):
        d = _lib.TemporalFilterDesc()
        ops._frames_view(d.e, e, "e", 1.0, 0.0)
        ops._frames_view(d.a, a, "a", 0.5, 0.5)
        d.flow, d.valid, d.out = G.data_ptr(), U.data_ptr(), view.data_ptr()
        d.out_stride_t, d.out_stride_c, d.out_stride_h = view.stride(0), view.stride(1), view.stride(2)
        for i, k in enumerate(offs):
            d.offsets[i] = k
        d.K, d.T, d.H, d.W, d.sigma, d.strength = len(offs), T, H, W, 0.1, 1.0
        for k, v in kw.items():
            if k in ("e", "a"):
                getattr(d, k).p = v
            else:
                setattr(d, k, v)
        return d
    stream = torch.cuda.current_stream().cuda_stream
    for kw in (dict(e=None), dict(a=None), dict(flow=None), dict(valid=None), dict(out=None), dict(T=0), dict(K=0), dict(K=9), dict(H=1), dict(W=1),
               dict(out_stride_h=W - 1), dict(out_stride_t=-1)):
        assert lib.insv2v_temporal_filter(desc(**kw), stream) == -1, kw
        assert untouched(), kw
    assert lib.insv2v_temporal_filter(None, stream) == -1
    # and the same buffers do run
    assert lib.insv2v_temporal_filter(desc(), stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(view).all() and (big[outside] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ 3. what it is for
def test_flicker_on_a_translating_source_shrinks_to_its_closed_form():
    """E_t = A_t + delta_t on an integer-translating source: d2 = 0, every weight is exactly s, and a pixel whose whole window is valid
    carries delta'_t = delta_t + s sum (delta_{t+k} - delta_t) / (1 + s n_t).  Where both pixels of a pair lie in that interior the warp
    error MAP of the result is (delta'_{t+1} - delta'_t)^2 within the element's own bound - 2 |D| (b_t + b_{t+1}) + (b_t + b_{t+1})^2 from
    the filter's bounds b at the two pixels, D the closed-form difference, plus 2^-22 of the value for the score kernel's own roundings -
    and strictly below the unfiltered (delta_{t+1} - delta_t)^2, for every pair."""
    from insv2v import temporal_filter as tf, pixel_score as ps
    c = tr.FLICKER
    T, H, W, shift, R, s = c["T"], c["H"], c["W"], c["shift"], c["radius"], c["strength"]
    tv = tr.translation_video(T, H, W, shift, c["deltas"])
    fwd, bwd = _dev32(tv["fwd"]), _dev32(tv["bwd"])
    nb = tf.neighbour_flows(fwd, bwd, radius=R)
    G, U, offs = tr.translation_neighbours(T, H, W, shift, R)
    assert np.array_equal(_np(nb["flow"]), G) and np.array_equal(_np(nb["valid"]), U)
    inside = tr.interior(T, H, W, shift, R)
    assert inside.mean() >= 0.5
    want = tr.flicker_closed_form(c["deltas"], R, s)
    for dt in tr.DTYPES:
        ref = tr.reference(tv["E"], tv["A"], G, U, offs, c["sigma"], s, tr.ONE, dt)
        e, a = _crop(tv["E"], dt)[1], _crop(tv["A"], dt)[1]
        out = tf.temporal_filter(e, a, nb["flow"], nb["valid"], nb["offsets"], sigma=c["sigma"], strength=s)
        got = _np(out)
        assert (np.abs(got - ref["out"]) <= ref["bound"]).all()
        assert (np.abs((got - tv["A"])[:, :, inside] - want[:, None, None]) <= ref["bound"][:, :, inside]).all()
        r = ps.warp_error(out, fwd, bwd, return_maps=True)
        err, valid = _np(r["err_map"]), _np(r["valid_map"])
        b = ref["bound"].max(1)                                     # per pixel: the worst of the three channels
        ys, xs = np.mgrid[0:H, 0:W]
        sy, sx = np.clip(ys + shift[1], 0, H - 1), np.clip(xs + shift[0], 0, W - 1)
        both = inside & inside[sy, sx]
        assert both.any() and (valid[:, both] == 1).all()
        worst = 0.0
        for t in range(T - 1):
            D = want[t + 1] - want[t]
            bb = b[t] + b[t + 1][sy, sx]
            tol = 2 * abs(D) * bb + bb * bb + 2.0 ** -22 * D * D
            e_t = np.abs(err[t] - D * D)
            assert (e_t[both] <= tol[both]).all(), (t, float((e_t / tol)[both].max()))
            worst = max(worst, float((e_t / tol)[both].max()))
            assert (err[t][both] < (c["deltas"][t + 1] - c["deltas"][t]) ** 2).all()
        before = ps.warp_error(e, fwd, bwd)["warp_error"].numpy()
        assert np.array_equal(before, np.diff(c["deltas"]) ** 2)
        print(f"[temporal_filter] flicker {dt}: warp error per pair {np.array2string(before, precision=4)} -> "
              f"{np.array2string(r['warp_error'].numpy(), precision=5)} (interior closed form {np.array2string(np.diff(want) ** 2, precision=5)}); "
              f"worst share of the error-map bound {worst:.3f}")


@pytest.mark.parametrize("dt", tr.DTYPES)
def test_the_guard_keeps_a_pixel_whose_source_changed(dt):
    """A rectangle whose SOURCE colour jumps by 1.0 in the next frame gets weight exp(-50): there the output is the edit within the bound,
    while the pixels around it are averaged - exactly, the values are dyadic."""
    H, W = 8, 12
    A = np.zeros((2, 3, H, W))
    A[1, :, 2:5, 3:8] = 1.0
    E = tr._rng("temporal_filter.guard").integers(-32, 33, (2, 3, H, W)) / 64.0
    G, U, offs = tr.translation_neighbours(2, H, W, (0, 0), 1)
    ref = tr.reference(E, A, G, U, offs, 0.1, 1.0, tr.ONE, dt)
    got = _run(E, A, G, U, offs, dt, 0.1, 1.0, tr.ONE)
    rect = np.zeros((H, W), bool)
    rect[2:5, 3:8] = True
    assert (np.abs(got - E)[:, :, rect] <= ref["bound"][:, :, rect]).all()
    assert np.array_equal(got[:, :, ~rect], np.broadcast_to(((E[0] + E[1]) / 2)[:, ~rect], (2, 3, int((~rect).sum()))))
    assert (np.abs(E[0] - E[1])[:, rect] > 0.1).any()


# ------------------------------------------------------------------------------------------------------------------ 4. the host chain
@pytest.mark.parametrize("occlusion", [True, False])
def test_neighbour_flows_are_propagate_masks_chains_bit_for_bit(occlusion, monkeypatch):
    """T = 5, R = 2: ``flow[k, t]`` and ``valid[k, t]`` are ``propagate_mask(key=t + k)``'s ``flow_to_key[t]`` and ``valid[t]`` - the same
    kernel on the same operands - for every t and k; entries whose neighbour lies outside the video are all invalid; R launches."""
    from insv2v import ops, temporal_filter as tf
    from insv2v.mask_track import propagate_mask
    T, H, W, R = 5, 17, 23, 2
    inp = pr.warp_inputs(T, H, W, "f32")
    fwd, bwd = _dev32(inp["fwd"]), _dev32(inp["bwd"])
    calls = []
    real = ops.mask_track_step
    monkeypatch.setattr(ops, "mask_track_step", lambda *a, **kw: (calls.append(a[2].shape[0]), real(*a, **kw))[1])
    nb = tf.neighbour_flows(fwd, bwd, radius=R, occlusion=occlusion)
    assert calls == [2 * (T - 1), 2 * (T - 2)] and nb["offsets"] == (-2, -1, 1, 2)
    monkeypatch.setattr(ops, "mask_track_step", real)
    key_mask = torch.ones((H, W), device=DEV)
    some_invalid = False
    for key in range(T):
        chain = propagate_mask(key_mask, key, fwd, bwd, occlusion=occlusion)
        for i, k in enumerate(nb["offsets"]):
            t = key - k
            if 0 <= t < T:
                assert _same_bits(nb["flow"][i, t], chain["flow_to_key"][t]) and _same_bits(nb["valid"][i, t], chain["valid"][t]), (key, k)
                some_invalid |= bool((nb["valid"][i, t] == 0).any()) and bool((nb["valid"][i, t] == 1).any())
    assert some_invalid
    for i, k in enumerate(nb["offsets"]):
        for t in range(T):
            if not 0 <= t + k < T:
                assert not nb["valid"][i, t].any() and not nb["flow"][i, t].any()
    only = tf.neighbour_flows(fwd, None, radius=R, occlusion=False)
    if not occlusion:   # without bwd only the forward offsets can be chained
        assert only["offsets"] == (1, 2) and _same_bits(only["flow"], nb["flow"][2:]) and _same_bits(only["valid"], nb["valid"][2:])


# ------------------------------------------------------------------------------------------------------------------ 5. drivers
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
    return InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4, **EAGER)


HP, WP, SEED = 32, 48, 47
PARAMS = dict(radius=2, sigma=0.25, strength=0.75)


def _unit(T, name="a"):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"temporal_filter.ev.frames.{name}.{T}", (1, T, 3, HP, WP), kind="uniform"),
                text_cond=synth.synth_input(f"temporal_filter.ev.tc.{name}", (1, 77, 64)), text_uncond=synth.synth_input("temporal_filter.ev.tu", (1, 77, 64)))


def _translation_flows(T):
    disps = [((1, 0), (0, 1), (-1, 1), (2, 0))[t % 4] for t in range(T - 1)]
    tc = pr.translation_video(HP, WP, disps)
    return dict(fwd=torch.from_numpy(tc["fwd"]).float(), bwd=torch.from_numpy(tc["bwd"]).float())


@pytest.mark.parametrize("T", [4, 20])
def test_edit_video_stabilize_is_stabilize_of_the_plain_edit(tiny_model, pipe, T):
    """``edit_video(stabilize=, stabilize_flows=)`` is bit for bit ``stabilize(frames, edit_video(...) without it, flows=)`` - for one window
    and across the window boundary of a 20-frame unit, which the filter runs over because it runs once, on the whole unit."""
    from insv2v.run_loveu_tgve import edit_video
    from insv2v.temporal_filter import stabilize
    u, flows = _unit(T), _translation_flows(T)
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    plain = edit_video(*args, seed=SEED, unit=0)
    got = edit_video(*args, seed=SEED, unit=0, stabilize=PARAMS, stabilize_flows=flows)
    want = stabilize(u["frames"], plain, flows=flows, **PARAMS)
    assert got.shape == plain.shape and got.dtype == plain.dtype and bool(torch.isfinite(got).all())
    assert _same_bits(got, want) and not _same_bits(got, plain)
    if T > 16:
        changed = (got != plain).flatten(2).any(2)[0]
        assert bool(changed[14:18].all()), "the frames on both sides of the window boundary are filtered"


def test_edit_videos_stacks_a_stabilized_and_a_plain_unit(tiny_model, pipe):
    from insv2v.run_loveu_tgve import edit_video, edit_videos
    T = 4
    ua, ub, flows = _unit(T, "a"), dict(_unit(T, "b"), unit=1), _translation_flows(T)
    outs = edit_videos(tiny_model, pipe, [dict(ua, unit=0, text_cfg=7.5, video_cfg=1.5, stabilize=PARAMS, stabilize_flows=flows),
                                          dict(ub, text_cfg=7.5, video_cfg=1.5)], seed=SEED)
    one = edit_video(tiny_model, pipe, ua["frames"], ua["text_cond"], ua["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, stabilize=PARAMS, stabilize_flows=flows)
    other = edit_video(tiny_model, pipe, ub["frames"], ub["text_cond"], ub["text_uncond"], 7.5, 1.5, seed=SEED, unit=1)
    assert _same_bits(outs[0], one) and _same_bits(outs[1], other)


def test_a_hard_mask_still_leaves_the_outside_exactly_alone(tiny_model, pipe):
    from insv2v.run_loveu_tgve import edit_video
    from insv2v import pixel_score as ps
    T = 4
    u, flows = _unit(T), _translation_flows(T)
    mask = torch.zeros((1, 1, HP, WP))
    mask[:, :, 9:22, 14:30] = 1.0
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    masked = edit_video(*args, seed=SEED, unit=0, mask=mask)
    got = edit_video(*args, seed=SEED, unit=0, mask=mask, stabilize=PARAMS, stabilize_flows=flows)
    r = ps.score_pixels(u["frames"], got, mask=mask, flows=flows)
    assert (r["mse_outside"] == 0).all() and (r["psnr_outside"] == math.inf).all() and (r["mse_inside"] > 0).all()
    assert not _same_bits(got, masked), "the inside is filtered"
    outside = (mask[0, 0] == 0).to(got.device)
    assert torch.equal(got[0][:, :, outside], u["frames"][0].to(got.device)[:, :, outside])


def test_a_tracked_mask_and_the_filter_share_one_flow_computation(tiny_model, pipe):
    """``mask_key=`` and ``stabilize=`` together: the estimator sees exactly the 2 (T - 1) pairs of ONE ``pair_flows(both=True)``; alone,
    without a flow source, the RuntimeError names the ways to give one."""
    from insv2v.run_loveu_tgve import edit_video

    class Counting:
        max_pairs = 3

        def __init__(self):
            self.pairs = 0

        def __call__(self, a, b):
            self.pairs += a.shape[0]
            return torch.zeros((a.shape[0], 2, *a.shape[-2:]), device=DEV)
    T = 4
    u = _unit(T)
    mask = torch.zeros((1, 1, HP, WP))
    mask[:, :, 8:24, 16:32] = 1.0
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    est = Counting()
    both = edit_video(*args, seed=SEED, unit=0, mask=mask, mask_key=1, stabilize=True, flow_estimator=est)
    assert est.pairs == 2 * (T - 1) and bool(torch.isfinite(both).all())
    est = Counting()
    edit_video(*args, seed=SEED, unit=0, stabilize=dict(occlusion=False), flow_estimator=est)
    assert est.pairs == 2 * (T - 1)
    with pytest.raises(RuntimeError, match="stabilize_flows="):
        edit_video(*args, seed=SEED, unit=0, stabilize=True)


HR, WR = 128, 192   # the smallest frame tests/test_raft_gpu.py runs the estimator at


def test_stabilize_with_the_raft_estimator():
    """Flows from the key-hashed RAFT: the result is finite and has the input's shape and dtype (no quality claim about such flows), and
    it is ``pair_flows`` + ``neighbour_flows`` + ``temporal_filter`` on the SOURCE's flows."""
    from insv2v import synth, shapes, temporal_filter as tf
    from insv2v.raft import RAFTFlow
    from insv2v.mask_track import pair_flows
    from insv2v.pixel_score import AFFINE_SIGNED
    raft = RAFTFlow(DEV, synth.synth_raft_state_dict(shapes.raft_shapes()))
    T = 3
    src = synth.synth_input("temporal_filter.raft.frames", (1, T, 3, HR, WR), kind="uniform").to(DEV)
    edt = (src * 0.9 + 0.05 * synth.synth_input("temporal_filter.raft.edit", (1, T, 3, HR, WR), kind="uniform").to(DEV)).half()
    out = tf.stabilize(src, edt, flow_estimator=raft)
    assert out.shape == edt.shape and out.dtype == edt.dtype and bool(torch.isfinite(out).all())
    flows = pair_flows(src, raft)
    nb = tf.neighbour_flows(flows["fwd"], flows["bwd"])
    assert _same_bits(out[0], tf.temporal_filter(edt[0], src[0], nb["flow"], nb["valid"], nb["offsets"], guide_affine=AFFINE_SIGNED))


def test_cli_synthetic_stabilize(tmp_path, monkeypatch):
    """``--synthetic 1 --synthetic-tiny --stabilize`` (reduced-width models, a key-hashed RAFT, 3 frames at 128 x 128, one step) is a
    smoke path: the unit goes through ``stabilize`` once, with the flags' parameters and the estimator's flows, and the result is finite
    and shaped like the plain run's.  Nothing is claimed about the values: key-hashed flows on random frames pass no consistency check."""
    from insv2v import run_loveu_tgve, inference, temporal_filter as tf

    class Eager(inference.InferenceIP2PVideo):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **EAGER))
    monkeypatch.setattr(inference, "InferenceIP2PVideo", Eager)
    seen, real = [], tf.stabilize

    def spy(source, edited, **kw):
        seen.append(dict(kw, T=source.shape[1]))
        return real(source, edited, **kw)
    monkeypatch.setattr(tf, "stabilize", spy)
    common = ["--synthetic", "1", "--synthetic-tiny", "--num-frames", "3", "--image-size", "128", "--steps", "1", "--seed", "5"]
    outs = []
    for name, extra in (("plain", []), ("stab", ["--stabilize", "--stabilize-radius", "1", "--stabilize-no-occlusion"])):
        run_loveu_tgve.main(common + extra + ["--out", str(tmp_path / f"{name}.pt")])
        outs.append(torch.load(tmp_path / f"{name}.pt"))
        assert len(seen) == (1 if extra else 0)
    assert outs[0].shape == outs[1].shape and bool(torch.isfinite(outs[1].float()).all())
    kw = seen[0]
    assert (kw["radius"], kw["sigma"], kw["strength"], kw["occlusion"], kw["T"], kw["mask"]) == (1, 0.1, 1.0, False, 3, None)
    assert tuple(kw["flows"]["fwd"].shape) == (2, 2, 128, 128) and tuple(kw["flows"]["bwd"].shape) == (2, 2, 128, 128)
