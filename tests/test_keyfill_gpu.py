"""Filling the frames between edited key frames along the source video's optical flow, on the GPU:
insv2v_keyframe_fill against the float64 definition (tests/keyfill_ref.py), its bit-exact cases, determinism and refusals, the host chain
of ``key_flows`` against ``propagate_mask``, ``keyframes=`` behind ``edit_video`` / ``edit_videos`` on the tiny UNet / VAE, the RAFT route
and the command line.

Bound per element, always against float64 and never against the kernel (tests/keyfill_ref.py states it, tests/test_keyfill_cpu.py prints
the measurements behind it): 4 x the float32 restatement's worst departure on the case's inputs + the derived term for the rounding of
the exponential's argument through the normalised quotient, floored at one rounding of the output dtype.  G and U are inputs, so the
kernel takes no decision and no pixel is left out of any comparison.  Every test prints what it measured on the device (``[keyfill]``
lines: the error as a share of its bound); profiles/keyfill_pytest_gpu.txt holds a run.  The pipes of this file run without graph
capture, as those of tests/test_temporal_filter_gpu.py."""
import numpy as np
import pytest
import torch

import keyfill_ref as kr
import pixel_score_ref as pr
from test_model_gpu import tiny_unet   # noqa: F401  (the module-scoped fixture, instantiated for this module)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EAGER = dict(use_graph=False)
SENT, KEYSENT = 777.0, 555.0
TORCH = {"f16": torch.float16, "f32": torch.float32}
COMBOS = [("f16", "f16"), ("f32", "f32"), ("f16", "f32"), ("f32", "f16")]   # (E, A): all four instantiations


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


def _out(T, H, W, key_frame, dt, grow=(2, 1, 3, 9), at=(1, 0, 2, 4)):
    """(sentinel buffer, the full-rate view inside it - NaN-prefilled, its key-frame rows holding KEYSENT -, the buffer's mask of sentinel
    elements)."""
    init = np.full((T, 3, H, W), np.nan)
    init[list(key_frame)] = KEYSENT
    big, view = _crop(init, dt, grow, at, fill=SENT)
    outside = torch.ones(big.shape, dtype=torch.bool, device=DEV)
    outside[tuple(slice(o, o + s) for o, s in zip(at, init.shape))] = False
    return big, view, outside


def _dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).float().to(DEV)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _run(inp, edt, adt, sigma, mode, affine, E=None):
    """One call on strided views inside NaN-filled buffers, into the NaN-prefilled full-rate view of a sentinel buffer -> (the rows of the
    table's frames, conf) as float64; the key rows and everything around the view must come back untouched."""
    from insv2v import ops
    A, E = inp["A"], inp["E"] if E is None else E
    T, _, H, W = A.shape
    a, e = _crop(A, adt, grow=(2, 0, 3, 9), at=(0, 0, 1, 8))[1], _crop(E, edt)[1]
    big, view, outside = _out(T, H, W, inp["key_frame"], edt)
    conf = torch.full((len(inp["frames"]), H, W), float("nan"), device=DEV)
    got, c = ops.keyframe_fill(a, e, _dev32(inp["G"]), _dev32(inp["U"]), inp["key_frame"], inp["frames"], inp["slots"], inp["weights"], sigma=sigma,
                               mode=mode, guide_affine=affine, out=view, conf=conf)
    torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr() and c.data_ptr() == conf.data_ptr()
    assert bool((big[outside] == SENT).all()), "the kernel wrote outside its output"
    assert bool((view[list(inp["key_frame"])] == KEYSENT).all()), "the kernel touched a key frame's rows"
    return _np(view)[list(inp["frames"])], _np(conf)


# ------------------------------------------------------------------------------------------------------------------ 1. kernel vs float64
@pytest.mark.parametrize("mode", kr.MODES)
@pytest.mark.parametrize("edt,adt", COMBOS)
@pytest.mark.parametrize("case", kr.CASES, ids=lambda c: f"{c[0]}x{c[1]}xT{c[2]}k{len(c[3])}")
def test_kernel_vs_float64(case, edt, adt, mode):
    """Smooth seeded G of a few pixels, U with holes, a whole invalid side and a rectangle nothing valid reaches, NaN planted in G, A and
    E wherever only inactive sides can reach: every element within its bound, no NaN in an output, conf == 0 exactly in the holes, the
    key rows and the sentinels untouched."""
    inp, ref = kr.case_inputs(*case, edt, adt), kr.case_reference(*case, edt, adt, mode)
    got, conf = _run(inp, edt, adt, kr.CASE_SIGMA, mode, kr.SIGNED)
    assert not np.isnan(got).any() and not np.isnan(conf).any(), f"{int(np.isnan(got).sum())} NaN in the output, {int(np.isnan(conf).sum())} in conf"
    err, cerr = np.abs(got - ref["out"]), np.abs(conf - ref["conf"])
    share, cshare = err / ref["bound"], cerr / ref["conf_bound"]
    at = np.unravel_index(share.argmax(), share.shape)
    print(f"[keyfill] {case[0]}x{case[1]} T={case[2]} keys={case[3]} n={len(inp['frames'])} E {edt} A {adt} {mode}: worst error {err.max():.3e}, worst share "
          f"of the bound {share.max():.3f} (bound there {ref['bound'][at]:.3e}; restatement worst {ref['worst']:.3e}); conf share {cshare.max():.3f}; "
          f"holes {int((ref['conf'] == 0).sum())}; NaN planted {inp['planted']}")
    assert (err <= ref["bound"]).all(), (np.argwhere(err > ref["bound"])[:5].tolist(), float(share.max()))
    assert (cerr <= ref["conf_bound"]).all() and np.array_equal(conf == 0, ref["conf"] == 0) and (conf <= 1 + 1e-6).all()


@pytest.mark.parametrize("dt", kr.DTYPES)
def test_a_tiny_sigma_underflows_every_weight_and_takes_the_fallback(dt):
    c, inp = kr.UNDERFLOW, kr.underflow_inputs(dt)
    ref = kr.reference(inp, c["sigma"], "residual", kr.SIGNED, dt)
    assert (ref["conf"] == 0).all() and (ref["n_active"] == 2).all()
    got, conf = _run(inp, dt, dt, c["sigma"], "residual", kr.SIGNED)
    err = np.abs(got - ref["out"])
    print(f"[keyfill] underflow {dt}: every weight is 0 (d2/(2 sigma^2) up to {ref['max_arg']:.3g}); worst share of the bound {(err / ref['bound']).max():.3f}")
    assert (conf == 0).all() and (err <= ref["bound"]).all()


# ------------------------------------------------------------------------------------------------------------------ 2. bit-exact cases
@pytest.mark.parametrize("mode", kr.MODES)
@pytest.mark.parametrize("dt", kr.DTYPES)
def test_an_unchanged_edit_returns_the_source_bit_for_bit(dt, mode):
    """E == A in every tap: ``residual`` returns A_t's own bits at every pixel of the 17 x 33 case (holes, planted NaN and all), and conf
    is what the definition says; ``warp`` does on the integer translation wherever a trajectory can be followed."""
    if mode == "residual":
        inp = kr.case_inputs(*kr.CASES[3], dt, dt)
        A = inp["A"].copy()
        A[inp["frames"][0], 0, 0, :2] = (-0.0, 0.0)
        inp = dict(inp, A=A, E=A[inp["key_frame"]])
        ref = kr.reference(inp, kr.CASE_SIGMA, mode, kr.SIGNED, dt)
        got, conf = _run(inp, dt, dt, kr.CASE_SIGMA, mode, kr.SIGNED)
        want = A[inp["frames"]]
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))
        assert (np.abs(conf - ref["conf"]) <= ref["conf_bound"]).all() and np.array_equal(conf == 0, ref["conf"] == 0)
    else:
        c = kr.translation_case()
        got, conf = _run(c, dt, dt, 0.1, mode, kr.ONE, E=c["A"][c["key_frame"]])
        some = c["conf"][0] > 0
        assert np.array_equal(got[0][:, some], c["A"][1][:, some]) and np.array_equal(conf, c["conf"])


@pytest.mark.parametrize("mode", kr.MODES)
@pytest.mark.parametrize("edt,adt", COMBOS)
def test_a_translating_source_blends_the_keys_residuals_exactly(edt, adt, mode):
    """A_key = A_t translated by integers, a dyadic residual, d2 = 0: the exact temporal blend of the two keys' residuals (the closed form
    of ``translation_case``, which tests/test_keyfill_cpu.py holds the float64 definition against), conf exactly 0, 1/2 or 1."""
    c = kr.translation_case()
    ref = kr.fill_video(c["A"], c["E"], c["key_frame"], c["frames"], c["slots"], c["weights"], c["G"], c["U"], 0.1, mode, kr.ONE)
    got, conf = _run(c, edt, adt, 0.1, mode, kr.ONE)
    assert np.array_equal(got, ref["out"]) and np.array_equal(conf, c["conf"])
    if mode == "residual":
        assert np.array_equal(got, c["want"])


def test_two_runs_agree_bitwise_also_on_a_second_stream():
    from insv2v import ops
    inp = kr.case_inputs(*kr.CASES[3], "f16", "f16")
    T, _, H, W = inp["A"].shape
    a, e, G, U = _crop(inp["A"], "f16")[1], _crop(inp["E"], "f16")[1], _dev32(inp["G"]), _dev32(inp["U"])

    def run():
        out = torch.zeros((T, 3, H, W), device=DEV, dtype=torch.float16)
        return ops.keyframe_fill(a, e, G, U, inp["key_frame"], inp["frames"], inp["slots"], inp["weights"], sigma=kr.CASE_SIGMA, guide_affine=kr.SIGNED, out=out)
    first, second = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    for k in (0, 1):
        assert _same_bits(first[k], second[k]) and _same_bits(first[k], third[k]) and bool(torch.isfinite(first[k]).all())


def test_refusals_leave_the_output_untouched():
    import ctypes
    from insv2v import ops, _lib
    inp = kr.case_inputs(*kr.CASES[3], "f32", "f32")
    T, _, H, W = inp["A"].shape
    keys, frames, slots, weights = inp["key_frame"], inp["frames"], inp["slots"], inp["weights"]
    n, Tk = len(frames), len(keys)
    a, e, G, U = _crop(inp["A"], "f32", grow=(2, 0, 3, 9), at=(0, 0, 1, 8))[1], _crop(inp["E"], "f32")[1], _dev32(inp["G"]), _dev32(inp["U"])
    big, view, outside = _out(T, H, W, keys, "f32")
    conf = torch.full((n, H, W), float("nan"), device=DEV)
    rows = torch.tensor(frames, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return bool((big[outside] == SENT).all() and torch.isnan(view[rows]).all() and (view[keys] == KEYSENT).all() and torch.isnan(conf).all())
    ok = dict(key_frame=keys, frames=frames, slots=slots, weights=weights, sigma=0.1, mode="residual", guide_affine=kr.SIGNED, out=view, conf=conf)

    def call(**kw):
        k = dict(ok, **kw)
        return ops.keyframe_fill(a, e, G, U, k.pop("key_frame"), k.pop("frames"), k.pop("slots"), k.pop("weights"), **k)
    two = lambda i, v: [tuple(v) if j == i else tuple(w) for j, w in enumerate(weights)]   # noqa: E731
    bad = [dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(sigma=1e-30),
           dict(guide_affine=(float("inf"), 0.0)), dict(guide_affine=(0.5, float("nan"))),
           dict(frames=[T] + frames[1:]), dict(frames=[-1] + frames[1:]), dict(frames=[frames[1]] + frames[1:]), dict(frames=[keys[0]] + frames[1:]),
           dict(key_frame=[T] + keys[1:]), dict(key_frame=[-1] + keys[1:]), dict(key_frame=[frames[2]] + keys[1:]),
           dict(slots=[(0, Tk)] + slots[1:]), dict(slots=[(-2, 0)] + slots[1:]), dict(slots=[(-1, -1)] + slots[1:]),
           dict(weights=two(1, (-0.25, 1.25))), dict(weights=two(1, (float("nan"), 0.5))), dict(weights=two(1, (float("inf"), 0.0))),
           dict(weights=two(1, (0.5, 0.6))), dict(weights=two(1, (0.5, 0.5 - 1e-4))), dict(weights=two(0, (1.0, 0.5)))]
    for kw in bad:
        with pytest.raises(_lib.HipKernelError):
            call(**kw)
        assert untouched(), kw
    with pytest.raises(ValueError):
        call(mode="blend")
    for sl in ((slice(None), slice(None), slice(0, 1)), (slice(None), slice(None), slice(None), slice(0, 1))):   # H = 1, W = 1
        g1, u1 = G[(slice(None), slice(None), *sl[1:])].contiguous(), U[(slice(None), *sl[1:])].contiguous()
        with pytest.raises(_lib.HipKernelError):
            ops.keyframe_fill(a[sl], e[sl], g1, u1, keys, frames, slots, weights, sigma=0.1, guide_affine=kr.SIGNED, out=view[sl], conf=conf[(slice(None), *sl[2:])].contiguous())
        assert untouched()
    # aliasing: the output over the source, over the keys (as a full-rate view it cannot hold), inside the flows, inside the validity;
    # conf inside the flows, inside the output (fp32: the dtypes agree)
    flat_g = G.view(-1)
    m = T * 3 * H * W
    spare = torch.zeros((T, 3, H, W), device=DEV)
    keep = a.clone()
    with pytest.raises(_lib.HipKernelError):
        call(out=a)
    torch.cuda.synchronize()
    assert _same_bits(a, keep) and untouched()
    for name, t in (("flow", G), ("valid", U)):   # the operand sits in a pool whose first 100 elements are the output's last
        pool = torch.zeros(m + t.numel(), device=DEV)
        inside = pool[m - 100:m - 100 + t.numel()].view(t.shape).copy_(t)
        alias = pool[:m].view(T, 3, H, W)
        keep = pool.clone()
        with pytest.raises(_lib.HipKernelError):
            ops.keyframe_fill(a, e, inside if name == "flow" else G, inside if name == "valid" else U, keys, frames, slots, weights, sigma=0.1,
                              guide_affine=kr.SIGNED, out=alias, conf=conf)
        torch.cuda.synchronize()
        assert _same_bits(pool, keep) and untouched(), name
    for alias in (flat_g[7:7 + n * H * W].view(n, H, W), spare.view(-1)[:n * H * W].view(n, H, W)):
        keep = alias.clone()
        with pytest.raises(_lib.HipKernelError):
            call(out=spare, conf=alias)
        torch.cuda.synchronize()
        assert _same_bits(alias, keep) and not spare.any() and untouched()
    big_e = torch.zeros((T, 3, H, W), device=DEV)   # the keys live inside the output buffer
    with pytest.raises(_lib.HipKernelError):
        ops.keyframe_fill(a, big_e[:Tk], G, U, keys, frames, slots, weights, sigma=0.1, guide_affine=kr.SIGNED, out=big_e, conf=conf)
    assert untouched() and not big_e.any()
    # NULL pointers, sizes, strides and the mode, straight at the entry
    lib = _lib.load()
    tables = ((ctypes.c_int32 * Tk)(*keys), (ctypes.c_int32 * n)(*frames), (ctypes.c_int32 * (2 * n))(*[v for s in slots for v in s]),
              (ctypes.c_float * (2 * n))(*[v for w in weights for v in w]))

    def desc(**kw):
        d = _lib.KeyfillDesc()
        ops._frames_view(d.a, a, "a", 0.5, 0.5)
        ops._frames_view(d.e, e, "e", 1.0, 0.0)
        d.flow, d.valid, d.out, d.conf = G.data_ptr(), U.data_ptr(), view.data_ptr(), conf.data_ptr()
        d.out_stride_t, d.out_stride_c, d.out_stride_h = view.stride(0), view.stride(1), view.stride(2)
        d.key_frame, d.frame, d.slot, d.weight = tables
        d.n, d.T, d.Tk, d.H, d.W, d.mode, d.sigma = n, T, Tk, H, W, 0, 0.1
        for k, v in kw.items():
            if k in ("a", "e"):
                getattr(d, k).p = v
            elif k in ("a_stride_h", "e_stride_t"):
                setattr(getattr(d, k[0]), k[2:], v)
            else:
                setattr(d, k, v)
        return d
    stream = torch.cuda.current_stream().cuda_stream
    null_i, null_f = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_float)()
    for kw in (dict(a=None), dict(e=None), dict(flow=None), dict(valid=None), dict(out=None), dict(key_frame=null_i), dict(frame=null_i), dict(slot=null_i),
               dict(weight=null_f), dict(n=0), dict(T=0), dict(Tk=0), dict(H=1), dict(W=1), dict(mode=2), dict(mode=-1), dict(out_stride_h=W - 1),
               dict(out_stride_t=-1), dict(a_stride_h=W - 1), dict(e_stride_t=-1), dict(T=65536), dict(n=T + 1)):
        assert lib.insv2v_keyframe_fill(desc(**kw), stream) == -1, kw
        assert untouched(), kw
    assert lib.insv2v_keyframe_fill(None, stream) == -1
    # and the same buffers do run - with and without conf
    assert lib.insv2v_keyframe_fill(desc(conf=None), stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(view[rows]).all() and torch.isnan(conf).all() and (view[keys] == KEYSENT).all())
    assert lib.insv2v_keyframe_fill(desc(), stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(conf).all() and (big[outside] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ 3. the host chain
@pytest.mark.parametrize("occlusion", [True, False])
@pytest.mark.parametrize("T,stride", [(3, 2), (5, 2), (5, 4), (9, 2), (9, 4)])
def test_key_flows_are_propagate_masks_chains_bit_for_bit(T, stride, occlusion, monkeypatch):
    """``flow[i, s]`` and ``valid[i, s]`` are ``propagate_mask(key=keys[slot])``'s ``flow_to_key[t]`` and ``valid[t]`` - the same kernel on
    the same operands - for every in-between frame and both sides, in ``fill_plan``'s launches: ONE per distance."""
    from insv2v import ops, keyfill
    from insv2v.mask_track import propagate_mask
    H, W = 17, 23
    inp = pr.warp_inputs(T, H, W, "f32")
    fwd, bwd = _dev32(inp["fwd"]), _dev32(inp["bwd"])
    keys = keyfill.key_frames(T, stride)
    plan = keyfill.fill_plan(T, keys)
    calls = []
    real = ops.mask_track_step
    monkeypatch.setattr(ops, "mask_track_step", lambda *a, **kw: (calls.append(a[2].shape[0]), real(*a, **kw))[1])
    kf = keyfill.key_flows(fwd, bwd, keys, occlusion=occlusion)
    monkeypatch.setattr(ops, "mask_track_step", real)
    assert calls == [len(step) for step in plan] and len(calls) == max(b - a for a, b in zip(keys, keys[1:])) - 1
    assert kf["frames"] == [t for t in range(T) if t not in keys] and tuple(kf["flow"].shape) == (len(kf["frames"]), 2, 2, H, W)
    key_mask = torch.ones((H, W), device=DEV)
    chains = {k: propagate_mask(key_mask, k, fwd, bwd, occlusion=occlusion) for k in keys}
    some_invalid = False
    for i, t in enumerate(kf["frames"]):
        a, b = max(k for k in keys if k < t), min(k for k in keys if k > t)
        assert kf["slots"][i] == (keys.index(a), keys.index(b)) and kf["weights"][i] == ((b - t) / (b - a), (t - a) / (b - a))
        for s, k in enumerate((a, b)):
            assert _same_bits(kf["flow"][i, s], chains[k]["flow_to_key"][t]) and _same_bits(kf["valid"][i, s], chains[k]["valid"][t]), (t, s)
            some_invalid |= bool((kf["valid"][i, s] == 0).any()) and bool((kf["valid"][i, s] == 1).any())
    assert some_invalid


def test_key_flows_of_irregular_keys_have_one_sided_frames():
    from insv2v import keyfill
    from insv2v.mask_track import propagate_mask
    T, H, W, keys = 8, 17, 23, [1, 4, 6]
    inp = pr.warp_inputs(T, H, W, "f32")
    fwd, bwd = _dev32(inp["fwd"]), _dev32(inp["bwd"])
    kf = keyfill.key_flows(fwd, bwd, keys)
    assert kf["frames"] == [0, 2, 3, 5, 7] and kf["slots"][0] == (-1, 0) and kf["slots"][-1] == (2, -1) and kf["weights"][0] == (0.0, 1.0)
    assert not kf["valid"][0, 0].any() and not kf["flow"][0, 0].any() and not kf["valid"][4, 1].any()
    chain = propagate_mask(torch.ones((H, W), device=DEV), 1, fwd, bwd)
    assert _same_bits(kf["flow"][0, 1], chain["flow_to_key"][0]) and _same_bits(kf["valid"][0, 1], chain["valid"][0])


# ------------------------------------------------------------------------------------------------------------------ 4. drivers
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
    return InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=2, **EAGER)


HP, WP, TP, STRIDE, SEED = 64, 64, 9, 4, 53
KEYS = [0, 4, 8]
BETWEEN = [1, 2, 3, 5, 6, 7]
PARAMS = dict(stride=STRIDE, sigma=0.25)


def _unit(T=TP, name="a"):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"keyfill.ev.frames.{name}.{T}", (1, T, 3, HP, WP), kind="uniform"),
                text_cond=synth.synth_input(f"keyfill.ev.tc.{name}", (1, 77, 64)), text_uncond=synth.synth_input("keyfill.ev.tu", (1, 77, 64)))


def _translation_flows(T=TP):
    disps = [((1, 0), (0, 1), (-1, 1), (2, 0))[t % 4] for t in range(T - 1)]
    tc = pr.translation_video(HP, WP, disps)
    return dict(fwd=torch.from_numpy(tc["fwd"]).float(), bwd=torch.from_numpy(tc["bwd"]).float())


@pytest.fixture(scope="module")
def plain_keys(tiny_model, pipe):
    """``edit_video`` of the sub-video of key frames - computed once, shared by the driver tests."""
    from insv2v.run_loveu_tgve import edit_video
    u = _unit()
    return edit_video(tiny_model, pipe, u["frames"][:, KEYS], u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, return_latent=True)


def test_edit_video_keyframes_is_the_sub_video_edit_and_its_fill(tiny_model, pipe, plain_keys):
    """The key frames of ``edit_video(keyframes=)`` are bit for bit ``edit_video(frames[:, keys])`` with the same seed, the frames in
    between bit for bit ``keyframe_fill`` of those; the latent returned is the key frames'."""
    from insv2v.run_loveu_tgve import edit_video
    from insv2v.keyfill import keyframe_fill
    u, flows = _unit(), _translation_flows()
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    got, latent, est = edit_video(*args, seed=SEED, unit=0, keyframes=PARAMS, key_flows=flows, return_latent=True, return_mask=True)
    keys_img, keys_latent = plain_keys
    assert got.shape == u["frames"].shape and got.dtype == keys_img.dtype and bool(torch.isfinite(got).all())
    assert _same_bits(got[:, KEYS], keys_img) and _same_bits(latent, keys_latent)
    want = keyframe_fill(u["frames"], keys_img, KEYS, flows=flows, sigma=PARAMS["sigma"])
    assert _same_bits(got, want["frames"]) and est["keys"] == KEYS and _same_bits(est["confidence"], want["confidence"])
    assert bool((est["confidence"][KEYS] == 1).all()) and float(got.abs().max()) <= 1.0
    src = u["frames"].to(got.device)
    assert not torch.equal(got[:, BETWEEN].float(), src[:, BETWEEN].float()), "the frames in between carry the edit"
    stride_int = edit_video(*args, seed=SEED, unit=0, keyframes=STRIDE, key_flows=flows)
    assert _same_bits(stride_int[:, KEYS], keys_img) and stride_int.shape == got.shape


def _mask():
    mask = torch.zeros((1, 1, HP, WP))
    mask[:, :, 16:40, 24:48] = 1.0
    return mask


def test_a_hard_mask_leaves_the_outside_of_every_delivered_frame_exactly_alone(tiny_model, pipe):
    from insv2v.run_loveu_tgve import edit_video
    u, flows, mask = _unit(), _translation_flows(), _mask()
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    got = edit_video(*args, seed=SEED, unit=0, mask=mask, keyframes=PARAMS, key_flows=flows)
    sub = edit_video(tiny_model, pipe, u["frames"][:, KEYS], u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, mask=mask)
    assert _same_bits(got[:, KEYS], sub)
    outside = (mask[0, 0] == 0).to(got.device)
    src = u["frames"][0].to(device=got.device, dtype=got.dtype)
    assert torch.equal(got[0][:, :, outside], src[:, :, outside]) and not torch.equal(got[0][:, :, ~outside], src[:, :, ~outside])
    inside_between = got[0][BETWEEN][:, :, ~outside] != src[BETWEEN][:, :, ~outside]
    assert bool(inside_between.any()), "the frames in between are edited inside the mask"


def test_mask_shape_key_rows_of_the_full_rate_mask_are_the_sub_videos(tiny_model, pipe):
    """Shaping is per frame: the key rows of the full-rate ``shaped`` / ``support`` equal the sub-video's bit for bit, the key frames are
    the sub-video's edit, and outside ``support`` every delivered frame is the input's."""
    from insv2v.run_loveu_tgve import edit_video
    u, flows, mask = _unit(), _translation_flows(), _mask()
    shape = dict(grow=2.0, feather=3.0)
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    got, est = edit_video(*args, seed=SEED, unit=0, mask=mask, mask_key=4, mask_flows=flows, mask_shape=shape, keyframes=PARAMS, return_mask=True)
    sub_mask = est["mask"][:, KEYS]
    sub, sub_est = edit_video(tiny_model, pipe, u["frames"][:, KEYS], u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, mask=sub_mask,
                              mask_shape=shape, return_mask=True)
    assert tuple(est["shaped"].shape) == (1, TP, HP, WP)
    assert _same_bits(est["shaped"][:, KEYS], sub_est["shaped"]) and _same_bits(est["support"][:, KEYS], sub_est["support"])
    assert _same_bits(got[:, KEYS], sub)
    src = u["frames"][0].to(device=got.device, dtype=got.dtype)
    off = (est["support"][0] == 0)[:, None].expand(-1, 3, -1, -1)
    assert torch.equal(got[0][off], src[off]) and bool(off.any())


def test_a_tracked_mask_the_filter_and_the_fill_share_one_flow_computation(tiny_model, pipe):
    """``mask_key=``, ``stabilize=`` and ``keyframes=`` together: the estimator sees exactly the 2 (T - 1) pairs of ONE
    ``pair_flows(both=True)``; without a flow source the RuntimeError names the ways to give one."""
    from insv2v.run_loveu_tgve import edit_video

    class Counting:
        max_pairs = 3

        def __init__(self):
            self.pairs = 0

        def __call__(self, a, b):
            self.pairs += a.shape[0]
            return torch.zeros((a.shape[0], 2, *a.shape[-2:]), device=DEV)
    u, mask = _unit(), _mask()
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    est = Counting()
    both = edit_video(*args, seed=SEED, unit=0, mask=mask, mask_key=1, stabilize=True, keyframes=STRIDE, flow_estimator=est)
    assert est.pairs == 2 * (TP - 1) and bool(torch.isfinite(both).all()) and both.shape == u["frames"].shape
    with pytest.raises(RuntimeError, match="key_flows="):
        edit_video(*args, seed=SEED, unit=0, keyframes=STRIDE)


def test_edit_videos_stacks_a_plain_and_a_masked_key_frame_unit(tiny_model, pipe):
    from insv2v.run_loveu_tgve import edit_video, edit_videos
    ua, ub, flows, mask = _unit(name="a"), dict(_unit(name="b"), unit=1), _translation_flows(), _mask()
    outs = edit_videos(tiny_model, pipe, [dict(ua, unit=0, text_cfg=7.5, video_cfg=1.5, keyframes=PARAMS, key_flows=flows),
                                          dict(ub, text_cfg=7.5, video_cfg=1.5, mask=mask, keyframes=STRIDE, key_flows=flows)], seed=SEED)
    one = edit_video(tiny_model, pipe, ua["frames"], ua["text_cond"], ua["text_uncond"], 7.5, 1.5, seed=SEED, unit=0, keyframes=PARAMS, key_flows=flows)
    other = edit_video(tiny_model, pipe, ub["frames"], ub["text_cond"], ub["text_uncond"], 7.5, 1.5, seed=SEED, unit=1, mask=mask, keyframes=STRIDE, key_flows=flows)
    assert _same_bits(outs[0], one) and _same_bits(outs[1], other)
    with pytest.raises(ValueError, match="share"):   # the sub-videos are what stack: 3 key frames against 5 frames
        edit_videos(tiny_model, pipe, [dict(ua, keyframes=PARAMS, key_flows=flows), dict(_unit(5, "c"))], seed=SEED)


HR, WR = 128, 192   # the smallest frame tests/test_raft_gpu.py runs the estimator at


def test_keyframe_fill_with_the_raft_estimator():
    """Flows from the key-hashed RAFT: the result is finite, holds the keys bit for bit and has the source's shape (no quality claim about
    such flows), and it is ``pair_flows`` + ``key_flows`` + the kernel on the SOURCE's flows."""
    from insv2v import synth, shapes, keyfill
    from insv2v.raft import RAFTFlow
    from insv2v.mask_track import pair_flows
    raft = RAFTFlow(DEV, synth.synth_raft_state_dict(shapes.raft_shapes()))
    T, keys = 3, [0, 2]
    src = synth.synth_input("keyfill.raft.frames", (1, T, 3, HR, WR), kind="uniform").to(DEV)
    edt = (src[:, keys] * 0.9 + 0.05 * synth.synth_input("keyfill.raft.edit", (1, 2, 3, HR, WR), kind="uniform").to(DEV)).half()
    out = keyfill.keyframe_fill(src, edt, keys, flow_estimator=raft)
    assert out["frames"].shape == (1, T, 3, HR, WR) and out["frames"].dtype == edt.dtype and bool(torch.isfinite(out["frames"]).all())
    assert _same_bits(out["frames"][:, keys], edt) and tuple(out["confidence"].shape) == (T, HR, WR) and bool((out["confidence"][keys] == 1).all())
    again = keyfill.keyframe_fill(src, edt, keys, flows=pair_flows(src, raft))
    assert _same_bits(out["frames"], again["frames"]) and _same_bits(out["confidence"], again["confidence"])


def test_cli_synthetic_key_stride(tmp_path, monkeypatch):
    """``--synthetic 1 --synthetic-tiny --key-stride 2`` (reduced-width models, a key-hashed RAFT, 3 frames at 128 x 128, one step) is a
    smoke path: the unit goes through ``keyframe_fill`` once, with the flags' parameters and the estimator's flows, and the result is
    finite and shaped like the plain run's.  Nothing is claimed about the values."""
    from insv2v import run_loveu_tgve, inference, keyfill

    class Eager(inference.InferenceIP2PVideo):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **EAGER))
    monkeypatch.setattr(inference, "InferenceIP2PVideo", Eager)
    seen, real = [], keyfill.keyframe_fill

    def spy(source, edited, keys, **kw):
        seen.append(dict(kw, T=source.shape[1], keys=list(keys)))
        return real(source, edited, keys, **kw)
    monkeypatch.setattr(keyfill, "keyframe_fill", spy)
    common = ["--synthetic", "1", "--synthetic-tiny", "--num-frames", "3", "--image-size", "128", "--steps", "1", "--seed", "5"]
    outs = []
    for name, extra in (("plain", []), ("keys", ["--key-stride", "2", "--key-mode", "warp", "--key-no-occlusion"])):
        run_loveu_tgve.main(common + extra + ["--out", str(tmp_path / f"{name}.pt")])
        outs.append(torch.load(tmp_path / f"{name}.pt"))
        assert len(seen) == (1 if extra else 0)
    assert outs[0].shape == outs[1].shape and bool(torch.isfinite(outs[1].float()).all())
    kw = seen[0]
    assert (kw["mode"], kw["sigma"], kw["occlusion"], kw["T"], kw["keys"]) == ("warp", 0.1, False, 3, [0, 2])
    assert tuple(kw["flows"]["fwd"].shape) == (2, 2, 128, 128) and tuple(kw["flows"]["bwd"].shape) == (2, 2, 128, 128)
