"""A key-frame mask tracked with optical flow, on the GPU: insv2v_mask_track_step against the float64 restatement
(tests/masktrack_ref.py), its bit-exact cases, the chain of ``propagate_mask``, the entry's refusals, the drivers' ``mask_key=`` on the
tiny UNet / VAE, the RAFT route and the command line.

Bounds (tests/masktrack_ref.py states and measures them; tests/test_masktrack_cpu.py asserts the measurement).  V and the valid / fill
choice of the mask must be exact on every pixel whose three decision margins exceed the guard (1e-3 px to the frame border, 1e-3
relative to equality of the consistency inequality, 1e-3 px to a lattice line across which V_prev differs); at most 2 % of a case's
pixels may lie under the guard (0.26 % at worst on these inputs).  F and the mask element by element within
``K 2^-24 (|b| + max|F_prev| over the neighbours) + 2^-23 max(H,W) (spread of F_prev over the neighbours)`` (the mask: M in place of
F_prev), K = 4 x the measured constant ``K_MEASURED`` = 1: the float32 restatement stays under the coordinate term alone on these inputs
(largest remaining ratio 0.043), the constant is floored at the one rounding of the final sum, and the factor 4 is for the FMA contraction
of the three lerps, which the compiler chooses.  The pipes of this file run without graph capture, as those of
tests/test_automask_gpu.py and for the reason given there."""
import ctypes

import numpy as np
import pytest
import torch

import masktrack_ref as mr
from test_model_gpu import tiny_unet   # noqa: F401  (the module-scoped fixture, instantiated for this module)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EAGER = dict(use_graph=False)
SENT, PAD = 777.0, 67   # the value around every output, and how many floats of it on either side (no alignment beyond 4 bytes)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _framed(arr=None, shape=None, pad_value=float("nan"), fill=float("nan")):
    """(whole buffer, view): ``arr`` (or ``fill``) surrounded by PAD floats of ``pad_value`` on either side."""
    shape = tuple(arr.shape) if arr is not None else tuple(shape)
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), pad_value, device=DEV, dtype=torch.float32)
    view = buf[PAD:PAD + n].view(shape)
    view.copy_(_dev(arr)) if arr is not None else view.fill_(fill)
    return buf, view


def _pads_intact(buf):
    return bool((buf[:PAD] == SENT).all() and (buf[-PAD:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ 1. one step vs float64
@pytest.mark.parametrize("N,H,W", mr.STEP_SHAPES)
def test_step_vs_float64(N, H, W):
    """Inputs inside NaN-filled buffers (a read outside an input makes the output non-finite), outputs prefilled with NaN inside
    sentinel-filled buffers (every element must be written, nothing around it)."""
    from insv2v import ops
    inp = mr.step_inputs(N, H, W)
    ins = {k: _framed(inp[k])[1] for k in ("F_prev", "V_prev", "b", "c", "M")}
    outs = [_framed(shape=s, pad_value=SENT) for s in ((N, 2, H, W), (N, H, W), (N, H, W))]
    F, V, m = ops.mask_track_step(ins["F_prev"], ins["V_prev"], ins["b"], ins["c"], ins["M"], alpha=inp["alpha"], beta=inp["beta"],
                                  fill=inp["fill"], out=tuple(v for _, v in outs))
    torch.cuda.synchronize()
    assert all(_pads_intact(buf) for buf, _ in outs), "the kernel wrote outside an output"
    assert F.data_ptr() == outs[0][1].data_ptr()
    got = dict(F=F.cpu().numpy(), V=V.cpu().numpy(), mask=m.cpu().numpy())
    for n in range(N):
        fails, share = mr.compare_step(inp, n, {k: v[n] for k, v in got.items()})
        print(f"[masktrack] step {N}x{H}x{W} chain {n}: {share:.4f} of the pixels under the guard, valid {got['V'][n].mean():.2f}")
        assert share <= mr.MAX_EXCLUDED and not fails, (n, fails)
    # without c: the consistency check is off, the rest is the same definition
    F0, V0, m0 = ops.mask_track_step(ins["F_prev"], ins["V_prev"], ins["b"], None, ins["M"], alpha=inp["alpha"], beta=inp["beta"], fill=inp["fill"])
    assert _same_bits(F0, F) and bool((V0 >= V).all()) and (H < 8 or bool((V0 != V).any()))
    noc = dict(inp, c=np.zeros_like(inp["c"]), beta=1e30)   # the same decisions from the float64 side: an inequality that always holds
    for n in range(N):
        fails, _ = mr.compare_step(noc, n, dict(F=F0[n].cpu().numpy(), V=V0[n].cpu().numpy(), mask=m0[n].cpu().numpy()))
        assert not fails, (n, fails)


# ------------------------------------------------------------------------------------------------------------------ 2. bit-exact cases
def _propagate(tc, key, **kw):
    from insv2v.mask_track import propagate_mask
    return propagate_mask(_dev(tc["M"]), key, _dev(tc["fwd"]), _dev(tc["bwd"]), **kw)


def _equals(r, mask, valid, flow):
    return (np.array_equal(r["mask"][0].cpu().numpy(), mask) and np.array_equal(r["valid"].cpu().numpy(), valid)
            and np.array_equal(r["flow_to_key"].cpu().numpy(), flow))


def test_zero_flow_is_the_key_mask_on_every_frame():
    from insv2v.mask_track import propagate_mask
    H, W, T = 11, 19, 4
    M = _dev(mr.translation_case(H, W, 0, [])["M"])
    zero = torch.zeros((T - 1, 2, H, W), device=DEV)
    for key in range(T):
        for kw in (dict(), dict(occlusion=False), dict(fill=0.5)):
            r = propagate_mask(M[None, None], key, zero, zero, **kw)
            assert r["mask"].shape == (1, T, H, W) and all(_same_bits(r["mask"][0, t], M) for t in range(T))
            assert not r["flow_to_key"].any() and bool((r["valid"] == 1).all())


@pytest.mark.parametrize("H,W,key,disps,rect", mr.EXACT_CASES)
def test_integer_translations_bitwise(H, W, key, disps, rect):
    """b = -d, c = +d (after the key; the opposite before it): the mask is M shifted by the accumulated displacement, pixels whose source
    leaves the frame are invalid and ``fill`` - also a non-default one; a planted inconsistent rectangle in c invalidates exactly what
    samples it, then and later; ``occlusion=False`` ignores c."""
    for fill in (0.0, 0.375):
        tc = mr.translation_case(H, W, key, disps, fill, bad_rect=rect)
        assert _equals(_propagate(tc, key, fill=fill), tc["mask"], tc["valid"], tc["flow_to_key"]), (fill, "occlusion on")
        assert _equals(_propagate(tc, key, fill=fill, occlusion=False), tc["mask_noocc"], tc["valid_noocc"], tc["flow_noocc"]), (fill, "occlusion off")
        if fill:
            inv = tc["valid"] == 0
            assert inv.any() and (tc["mask"][inv] == np.float32(fill)).all()
    if rect is not None:
        assert (tc["valid"] != tc["valid_noocc"]).any()


# ------------------------------------------------------------------------------------------------------------------ 3. the chain
def _smooth_flows(T, H, W, key):
    rng = mr._rng(f"masktrack.chain.{T}.{H}.{W}.{key}")
    fwd = np.array([[mr._smooth(rng, H, W, 2.0) + 0.7, mr._smooth(rng, H, W, 2.0)] for _ in range(T - 1)]).reshape(T - 1, 2, H, W)
    bwd = -fwd + rng.uniform(-0.3, 0.3, fwd.shape)
    s = 0.5 + 0.5 * mr._smooth(rng, H, W, 1.0, cells=6)
    return _dev(np.where(s > 0.5, s, 0.0)), _dev(fwd), _dev(bwd)


@pytest.mark.parametrize("T,key", [(1, 0), (2, 0), (2, 1), (5, 0), (5, 2), (5, 4)])
def test_chain_launches_directions_and_determinism(monkeypatch, T, key):
    from insv2v import ops, mask_track
    H, W = 21, 35
    M, fwd, bwd = _smooth_flows(T, H, W, key)
    launches = []
    real = ops.mask_track_step
    monkeypatch.setattr(mask_track.ops, "mask_track_step", lambda *a, **kw: (launches.append(a[2].shape[0]), real(*a, **kw))[1])
    r = mask_track.propagate_mask(M, key, fwd, bwd)
    want = [len(s) for s in mr.track_plan(T, key)]
    assert launches == want and len(launches) == max(key, T - 1 - key) <= max(T - 1, 0)   # T = 1: nothing is launched
    assert r["mask"].shape == (1, T, H, W) and r["valid"].shape == (T, H, W) and r["flow_to_key"].shape == (T, 2, H, W)
    assert _same_bits(r["mask"][0, key], M) and not r["flow_to_key"][key].any() and bool((r["valid"][key] == 1).all())
    assert all(torch.isfinite(v).all() for v in r.values()) and float(r["mask"].min()) >= 0.0 and float(r["mask"].max()) <= 1.0
    again = mask_track.propagate_mask(M, key, fwd, bwd)
    assert all(_same_bits(r[k], again[k]) for k in r), "two runs differ"
    # the two directions of one launch are the two single-direction chains, bit for bit
    after = mask_track.propagate_mask(M, 0, fwd[key:], bwd[key:])
    before = mask_track.propagate_mask(M, key, fwd[:key], bwd[:key])
    for k, cat in (("valid", 0), ("flow_to_key", 0), ("mask", 1)):
        assert _same_bits(r[k].narrow(cat, key, T - key), after[k]) and _same_bits(r[k].narrow(cat, 0, key + 1), before[k]), k
    # the wiring of b and c against the float64 chain: V away from its decisions is not compared here (the step test does), the flow is
    ref = mr.chain(M.cpu().numpy().astype(np.float64), key, fwd.cpu().numpy().astype(np.float64), bwd.cpu().numpy().astype(np.float64))
    assert np.abs(r["flow_to_key"].cpu().numpy() - ref["flow_to_key"]).max() <= 1e-4 * max(1.0, np.abs(ref["flow_to_key"]).max())
    if T > 1:
        assert (r["valid"].cpu().numpy() == ref["valid"]).mean() > 0.99 and 0 < ref["valid"].mean() < 1


# ------------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_outputs_untouched(monkeypatch):
    from insv2v import ops, _lib, mask_track
    N, H, W = 2, 6, 10
    inp = mr.step_inputs(N, 16, 24)
    ins = {k: _dev(inp[k][..., :H, :W]) for k in ("F_prev", "V_prev", "b", "c", "M")}
    outs = [_framed(shape=s, pad_value=SENT) for s in ((N, 2, H, W), (N, H, W), (N, H, W))]
    views = tuple(v for _, v in outs)
    a = (ins["F_prev"], ins["V_prev"], ins["b"], ins["c"], ins["M"])

    def untouched():
        torch.cuda.synchronize()
        return all(_pads_intact(buf) and bool(torch.isnan(v).all()) for buf, v in outs)
    keep = {k: v.clone() for k, v in ins.items()}
    for bad in ((ins["b"], views[1], views[2]), (views[0], ins["V_prev"], views[2]), (views[0], views[1], ins["M"]), (ins["c"], views[1], views[2]),
                (ins["F_prev"], views[1], views[2]), (views[0], views[1], views[1]), (views[0], outs[0][0][PAD + 4:PAD + 4 + N * H * W].view(N, H, W), views[2])):   # aliasing
        with pytest.raises(_lib.HipKernelError):
            ops.mask_track_step(*a, out=bad)
        assert untouched()
    for kw in (dict(alpha=-0.01), dict(beta=-1.0), dict(alpha=float("nan")), dict(beta=float("inf")), dict(fill=float("nan"))):
        with pytest.raises(_lib.HipKernelError):
            ops.mask_track_step(*a, out=views, **kw)
        assert untouched()
    lib = _lib.load()
    names = ("f_prev", "v_prev", "b", "c", "m")
    for null in ("f_prev", "v_prev", "b", "m", "f_out", "v_out", "mask_out"):   # nulls
        d = _lib.MaskTrackDesc()
        for k, t in zip(names + ("f_out", "v_out", "mask_out"), a + views):
            setattr(d, k, None if k == null else t.data_ptr())
        d.N, d.H, d.W, d.alpha, d.beta, d.fill = N, H, W, 0.01, 0.5, 0.0
        assert lib.insv2v_mask_track_step(ctypes.byref(d), None) == -1, null
        assert untouched()
    row = [t[..., :1, :].contiguous() for t in a]   # H = 1
    with pytest.raises(_lib.HipKernelError):
        ops.mask_track_step(*row, out=(views[0][:, :, :1].contiguous(), views[1][:, :1].contiguous(), views[2][:, :1].contiguous()))
    for bad in ((a[0][:1], *a[1:]), (a[0], a[1].double(), *a[2:]), (a[0], a[1], a[2].cpu(), a[3], a[4]), (a[0], a[1], a[2].transpose(-1, -2), a[3], a[4])):
        with pytest.raises(_lib.HipKernelError):
            ops.mask_track_step(*bad, out=views)
    assert untouched() and all(torch.equal(ins[k], keep[k]) for k in ins)
    launches, real = [], ops.mask_track_step
    monkeypatch.setattr(mask_track.ops, "mask_track_step", lambda *a, **kw: launches.append(1))
    with pytest.raises(ValueError, match="occlusion"):   # missing bwd with the occlusion check on
        mask_track.propagate_mask(ins["M"][0], 0, ins["b"], None)
    assert launches == []
    ok = real(*a, out=views)   # and the same buffers do run
    torch.cuda.synchronize()
    assert all(torch.isfinite(t).all() for t in ok) and all(_pads_intact(buf) for buf, _ in outs)


# ------------------------------------------------------------------------------------------------------------------ 5. pipeline
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


HP, WP, SEED = 32, 48, 91


def _unit(key, T):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"masktrack.ev.frames.{key}.{T}", (1, T, 3, HP, WP), kind="uniform"),
                text_cond=synth.synth_input(f"masktrack.ev.tc.{key}", (1, 77, 64)), text_uncond=synth.synth_input("masktrack.ev.tu", (1, 77, 64)))


def _tracked_case(T, key, step=(2, 1)):
    """A rectangle drawn on frame ``key`` of a scene that moves by ``step`` pixels per frame -> (M [1,1,H,W], mask_flows, the expected
    [1,T,H,W] mask): integer translations, so the expectation is exact."""
    M = np.zeros((HP, WP), np.float32)
    M[9:22, 14:30] = 1.0
    tc = mr.translation_case(HP, WP, key, [step] * (T - 1), M=M)
    flows = dict(fwd=torch.from_numpy(tc["fwd"]), bwd=torch.from_numpy(tc["bwd"]))
    return torch.from_numpy(M)[None, None], flows, torch.from_numpy(tc["mask"])[None], tc


def _edit(model, pipe, u, unit, **kw):
    from insv2v.run_loveu_tgve import edit_video
    return edit_video(model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=unit, **kw)


def test_edit_video_tracked_is_the_edit_with_the_shifted_masks(tiny_model, pipe):
    """The test that cannot pass without the feature: a mask drawn on frame 2 of 6 and integer-translation flows give, bit for bit, the
    edit with the explicit [1,T,H,W] mask of shifted rectangles; outside it the pixels are the input's."""
    T, key = 6, 2
    u = _unit("a", T)
    M, flows, want, tc = _tracked_case(T, key)
    img, est = _edit(tiny_model, pipe, u, 0, mask=M, mask_key=key, mask_flows=flows, return_mask=True)
    assert set(est) == {"mask", "valid", "flow_to_key"} and est["mask"].shape == (1, T, HP, WP)
    assert torch.equal(est["mask"].cpu(), want) and np.array_equal(est["valid"].cpu().numpy(), tc["valid"])
    assert not torch.equal(want[0, 0], want[0, T - 1]) and all(want[0, t].sum() > 0 for t in range(T))   # the mask does move
    explicit = _edit(tiny_model, pipe, u, 0, mask=want)
    assert _same_bits(img, explicit), "mask_key= is not the edit with the tracked mask"
    still = _edit(tiny_model, pipe, u, 0, mask=M)   # the same drawn mask applied to every frame: another edit
    assert not _same_bits(img, still)
    keep = (want == 0.0)[:, :, None].expand_as(u["frames"])
    got = img.cpu()
    assert torch.equal(got[keep], u["frames"][keep]), "frames outside the tracked mask are not the input's"
    assert (got[~keep] - u["frames"][~keep]).abs().max() > 1e-2, "nothing was edited inside the mask"
    assert _edit(tiny_model, pipe, u, 0, return_mask=True)[1] is None
    # mask_track reaches propagate_mask: without the occlusion check only the needed half of the flows has to be there
    half = dict(fwd=flows["fwd"], bwd=flows["bwd"])
    img2 = _edit(tiny_model, pipe, u, 0, mask=M, mask_key=key, mask_flows=half, mask_track=dict(occlusion=False, fill=0.0))
    assert _same_bits(img2, img)   # consistent flows: the check changes nothing


def test_edit_videos_stacks_tracked_drawn_and_plain_units(tiny_model, pipe):
    from insv2v.run_loveu_tgve import edit_videos
    T, key = 6, 4
    ua, ub, uc = _unit("a", T), _unit("b", T), _unit("c", T)
    M, flows, want, _ = _tracked_case(T, key, step=(-1, 2))
    drawn = torch.zeros((1, T, HP, WP))
    drawn[:, :, 4:20, 30:44] = 1.0
    common = dict(text_cfg=7.5, video_cfg=1.5)
    units = [dict(ua, mask=M, mask_key=key, mask_flows=flows, unit=0, **common), dict(ub, mask=drawn, unit=1, **common), dict(uc, unit=2, **common)]
    outs = edit_videos(tiny_model, pipe, units, seed=SEED, return_mask=True)
    assert outs[1][1] is None and outs[2][1] is None
    alone = _edit(tiny_model, pipe, ua, 0, mask=M, mask_key=key, mask_flows=flows, return_mask=True)[1]
    assert all(_same_bits(outs[0][1][k], alone[k]) for k in ("mask", "valid", "flow_to_key")) and torch.equal(alone["mask"].cpu(), want)
    given = [dict(ua, mask=want, unit=0, **common), dict(ub, mask=drawn, unit=1, **common), dict(uc, unit=2, **common)]
    ref = edit_videos(tiny_model, pipe, given, seed=SEED)
    assert all(_same_bits(o[0], r) for o, r in zip(outs, ref)), "a tracked unit in a stack is not the unit with its tracked mask"
    keep = (want == 0.0)[:, :, None].expand_as(ua["frames"])
    assert torch.equal(outs[0][0].cpu()[keep], ua["frames"][keep])


def test_tracked_mask_crosses_the_window_boundary(tiny_model, pipe):
    """20 frames: a window of 16 and one of 4 new frames behind 12 carried over.  The mask keeps moving through both."""
    T, key = 20, 0
    u = _unit("w", T)
    M, flows, want, _ = _tracked_case(T, key, step=(1, 0))
    img, est = _edit(tiny_model, pipe, u, 3, mask=M, mask_key=key, mask_flows=flows, return_mask=True)
    assert torch.equal(est["mask"].cpu(), want)
    assert want[0, 15, 9:22, 29:45].all() and want[0, 19, 9:22, 33:48].all() and not want[0, 19, :, :33].any()   # 15 and 19 columns to the right
    assert _same_bits(img, _edit(tiny_model, pipe, u, 3, mask=want))
    keep = (want == 0.0)[:, :, None].expand_as(u["frames"])
    got = img.cpu()
    assert torch.equal(got[keep], u["frames"][keep])
    for t in (15, 16, 19):   # on both sides of the boundary something was edited where the rectangle has moved to
        inside = ~keep[0, t]
        assert (got[0, t][inside] - u["frames"][0, t][inside]).abs().max() > 1e-2, t


# ------------------------------------------------------------------------------------------------------------------ 6. the RAFT route
HR, WR = 128, 192   # the smallest frame tests/test_raft_gpu.py runs the estimator at


class _Chunks:
    """The estimator behind a smaller ``max_pairs``, recording the size of every call."""

    def __init__(self, est, max_pairs):
        self.est, self.max_pairs, self.calls = est, max_pairs, []

    def __call__(self, a, b):
        self.calls.append(a.shape[0])
        return self.est(a, b)


@pytest.fixture(scope="module")
def raft():
    from insv2v import synth, shapes
    from insv2v.raft import RAFTFlow
    return RAFTFlow(DEV, synth.synth_raft_state_dict(shapes.raft_shapes()))


def test_pair_flows_with_raft_in_chunks(raft):
    """No accuracy claim about flows from key-hashed weights: only that every pair reaches the estimator, in order, in chunks.  Chunked
    against the same chunks called directly: bit for bit.  Against pair-by-pair calls: the 2e-3 of max|flow| that
    tests/test_raft_gpu.py allows RAFTFlow between chunkings (other batch sizes take other GEMM tiles)."""
    from insv2v import synth
    from insv2v.mask_track import pair_flows
    T = 3
    frames = synth.synth_input("masktrack.raft.frames", (1, T, 3, HR, WR), kind="uniform").to(DEV)
    est = _Chunks(raft, 3)
    got = pair_flows(frames, est)
    assert est.calls == [3, 1] and got["fwd"].shape == got["bwd"].shape == (T - 1, 2, HR, WR)
    v = frames[0]
    direct = torch.cat([raft(v[[0, 1, 1]], v[[1, 2, 0]]), raft(v[[2]], v[[1]])])
    assert _same_bits(torch.cat([got["fwd"], got["bwd"]]), direct)
    one = _Chunks(raft, 1)
    single = pair_flows(frames, one)
    assert one.calls == [1] * 4
    for k in ("fwd", "bwd"):
        err, mx = float((single[k] - got[k]).abs().max()), float(got[k].abs().max())
        print(f"[masktrack] pair_flows {k}: chunks of 3 vs pair by pair, max-abs {err:.3e} of {mx:.3e}")
        assert torch.isfinite(got[k]).all() and err <= 2e-3 * mx
    half = pair_flows(frames, _Chunks(raft, 48), both=False, key=1)
    direct = raft(v[[0, 2]], v[[1, 1]])   # only what the chain from key 1 reads: fwd[0] and bwd[1]
    assert _same_bits(half["fwd"][0], direct[0]) and _same_bits(half["bwd"][1], direct[1]) and not half["fwd"][1].any() and not half["bwd"][0].any()


def test_edit_video_tracks_with_an_estimator(tiny_model, pipe, raft):
    from insv2v import synth
    T, key = 3, 1
    u = dict(frames=synth.synth_input("masktrack.raft.frames", (1, T, 3, HR, WR), kind="uniform"),
             text_cond=synth.synth_input("masktrack.ev.tc.r", (1, 77, 64)), text_uncond=synth.synth_input("masktrack.ev.tu", (1, 77, 64)))
    M = torch.zeros((1, 1, HR, WR))
    M[:, :, 40:90, 60:130] = 1.0
    img, est = _edit(tiny_model, pipe, u, 5, mask=M, mask_key=key, flow_estimator=raft, return_mask=True)
    assert img.shape == u["frames"].shape and torch.isfinite(img).all()
    assert est["mask"].shape == (1, T, HR, WR) and torch.isfinite(est["mask"]).all()
    assert float(est["mask"].min()) >= 0.0 and float(est["mask"].max()) <= 1.0 and torch.equal(est["mask"][0, key].cpu(), M[0, 0])
    assert set(est["valid"].unique().tolist()) <= {0.0, 1.0}
    from insv2v.run_loveu_tgve import edit_video
    with pytest.raises(RuntimeError, match="flow source"):
        edit_video(tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], mask=M, mask_key=key)


# ------------------------------------------------------------------------------------------------------------------ 7. command line
def test_cli_tracks_synthetic_and_file_masks(tmp_path, monkeypatch):
    """``--synthetic 2 --synthetic-mask --mask-key 1`` (the smoke path: reduced-width models, a key-hashed RAFT, 3 frames at 128 x 128, one
    step) writes both units' tracked masks; ``--mask-file`` naming only unit 1, unstacked and without the occlusion check, tracks that
    unit and edits the other whole.  The pipes run without graph capture, as everywhere in this file."""
    from insv2v import run_loveu_tgve, inference

    class Eager(inference.InferenceIP2PVideo):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **EAGER))
    monkeypatch.setattr(inference, "InferenceIP2PVideo", Eager)
    T, S, key = 3, 128, 1
    common = ["--synthetic", "2", "--synthetic-tiny", "--num-frames", str(T), "--image-size", str(S), "--steps", "1", "--seed", "5"]
    run_loveu_tgve.main(common + ["--synthetic-mask", "--mask-key", str(key), "--mask-out", str(tmp_path / "masks.pt"), "--out", str(tmp_path / "edited.pt")])
    masks = torch.load(tmp_path / "masks.pt")
    want = run_loveu_tgve.synthetic_mask(1, S, S)[0, 0]
    assert sorted(masks) == [0, 1]
    for m in masks.values():
        assert m["mask"].shape == m["valid"].shape == (T, S, S) and torch.equal(m["mask"][key], want) and bool((m["valid"][key] == 1).all())
        assert torch.isfinite(m["mask"]).all() and float(m["mask"].min()) >= 0.0 and float(m["mask"].max()) <= 1.0
    edited = torch.load(tmp_path / "edited.pt")
    assert tuple(edited.shape) == (1, 2, T, 3, S, S) and torch.isfinite(edited.float()).all()
    torch.save({1: want[None, None]}, tmp_path / "drawn.pt")
    run_loveu_tgve.main(common + ["--mask-file", str(tmp_path / "drawn.pt"), "--mask-key", "0", "--mask-no-occlusion", "--no-stack",
                                  "--mask-out", str(tmp_path / "masks2.pt"), "--out", str(tmp_path / "edited2.pt")])
    masks2 = torch.load(tmp_path / "masks2.pt")
    assert sorted(masks2) == [1] and torch.equal(masks2[1]["mask"][0], want)
    assert tuple(torch.load(tmp_path / "edited2.pt").shape) == (1, 2, T, 3, S, S)
