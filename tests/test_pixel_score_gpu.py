"""Scoring an edit in pixel space, on the GPU: insv2v_frame_fidelity and insv2v_warp_error against the float64
restatement (tests/pixel_score_ref.py), their bit-exact cases, determinism, refusals, ``score_pixels`` behind ``edit_video`` on the tiny
UNet / VAE, the RAFT route and the command line.

Bounds (tests/pixel_score_ref.py states them, tests/test_pixel_score_cpu.py prints and checks the measurements behind them).  Always
against the float64 definition, never against the kernel:
  err_map / se per element   4 x max(worst |float32 restatement - float64| of the case, 2^-22 |value|)
                             measured worst on these inputs: err 5.9e-7 (64 x 96), se 8.9e-9
  SSIM per element           4 x max(|float32 restatement - float64|, 2^-23); measured worst 2.8e-6 (45 x 145) - the moments are those of
                             x - 1/2, so the cancellation in E[x^2] - mu^2 does not dominate
  a sum                      4 x (the weighted sum of those element terms) + n 2^-53 sum |terms|: relative 1.5e-6 (se) and 8e-7 (SSIM) at most
                             here; the weight sums and the reduction of the kernel's own maps: n 2^-53 sum |terms| alone
  valid_map                  exact wherever the float64 decision margins exceed masktrack_ref's guards (1e-3 px to the border, 1e-3 relative
                             to equality of the consistency inequality); at most 2 % of a case's pixels may lie under them (0.09 % at worst here)
The factor 4 is for FMA contraction and another summation tree, which the compiler chooses.  Every test prints what it measured on the
device (``[pixel_score]`` lines: the error as a share of its bound).  Measured on the MI355X (profiles/pixel_score_pytest_gpu.txt):
err_map at most 0.25 of its bound (the restatement's own worst error: the kernel rounds as the restatement does); the squared-error sums
at most 0.019 of theirs (relative error <= 1.2e-8); the SSIM sums 0.48 of theirs at 11 x 12 and <= 0.04 from one tile up (relative error
<= 7.1e-8); X == Y: |ssim - 1| = 4.9e-10 against 4.8e-7; the reduction of the kernel's own maps within 5.7e-14; no valid decision flipped.  The pipes of this file run without graph capture, as those of
tests/test_masktrack_gpu.py."""
import json
import math

import numpy as np
import pytest
import torch

import masktrack_ref as mr
import pixel_score_ref as pr
from test_model_gpu import tiny_unet   # noqa: F401  (the module-scoped fixture, instantiated for this module)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EAGER = dict(use_graph=False)
SENT, PAD = 777.0, 67   # the value around every output, and how many elements of it on either side
TORCH = {"f16": torch.float16, "f32": torch.float32}
ONE = (1.0, 0.0)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _crop(arr, dt, grow=(1, 1, 5, 7), at=(1, 1, 2, 3)):
    """[T,3,H,W] as a crop of a larger tensor whose surroundings are NaN: every stride differs from the dense one."""
    a = torch.from_numpy(np.ascontiguousarray(arr)).to(TORCH[dt])
    big = torch.full(tuple(s + g for s, g in zip(a.shape, grow)), float("nan"), device=DEV, dtype=TORCH[dt])
    view = big[tuple(slice(o, o + s) for o, s in zip(at, a.shape))]
    view.copy_(a.to(DEV))
    return view


def _framed(arr=None, shape=None, pad_value=float("nan"), fill=float("nan"), dtype=torch.float32):
    """(whole buffer, view): ``arr`` (or ``fill``) with PAD elements of ``pad_value`` on either side."""
    shape = tuple(arr.shape) if arr is not None else tuple(shape)
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), pad_value, device=DEV, dtype=dtype)
    view = buf[PAD:PAD + n].view(shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(dtype).to(DEV)) if arr is not None else view.fill_(fill)
    return buf, view


def _pads_intact(buf):
    return bool((buf[:PAD] == SENT).all() and (buf[-PAD:] == SENT).all())


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ 1. fidelity vs float64
def test_tile_is_the_one_the_shapes_are_named_from():
    from insv2v import ops
    assert ops.frame_fidelity_tile() == pr.TILE


def _run_fidelity(X, Y, w, xdt, ydt, affine=pr.SIGNED):
    from insv2v import ops
    T, _, H, W = X.shape
    x, y = _crop(X, xdt), _crop(Y, ydt, grow=(2, 0, 3, 9), at=(0, 0, 1, 8))   # X and Y: different strides (and dtypes, by the case)
    region = None if w is None else _framed(w)[1]
    sbuf, sums = _framed(shape=(T, 10), pad_value=SENT, dtype=torch.float64)
    wbuf, ws = _framed(shape=(ops.frame_fidelity_workspace_elems(T, H, W),), pad_value=SENT, dtype=torch.float64)
    got = ops.frame_fidelity(x, y, region, x_affine=affine, y_affine=affine, out=sums, workspace=ws)
    torch.cuda.synchronize()
    assert got.data_ptr() == sums.data_ptr() and _pads_intact(sbuf) and _pads_intact(wbuf), "the kernels wrote outside an output"
    return _np(got)


@pytest.mark.parametrize("T,H,W,xdt,ydt", pr.FIDELITY_CASES)
def test_fidelity_vs_float64(T, H, W, xdt, ydt):
    """Inputs are crops of NaN-filled tensors (a read outside a frame makes a sum non-finite), sums and workspace prefilled with NaN
    inside sentinel-filled buffers; every sum within its bound of the float64 definition, with and without a region."""
    inp = pr.fidelity_inputs(T, H, W, xdt, ydt)
    for with_region in (True, False):
        ref, bound, _, _ = pr.fidelity_reference(T, H, W, xdt, ydt, with_region)
        got = _run_fidelity(inp["X"], inp["Y"], inp["w"] if with_region else None, xdt, ydt)
        assert np.isfinite(got).all(), got
        err = np.abs(got - ref)
        share = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        rel = err / np.maximum(np.abs(ref), 1e-300)
        print(f"[pixel_score] fidelity {T}x{H}x{W} {xdt}/{ydt} region={with_region}: worst share of the bound per sum "
              f"{np.array2string(share.max(0), precision=3)}; relative error se {rel[:, 0].max():.3e} ssim {rel[:, 5].max():.3e}")
        assert (err <= bound).all(), (np.argwhere(err > bound).tolist(), share.max())
        if not with_region:   # w = 1: the inside sums are the whole-frame sums, the outside sums are exactly 0
            assert np.array_equal(got[:, 1], got[:, 0]) and np.array_equal(got[:, 6], got[:, 5]) and not got[:, [2, 4, 7, 9]].any()
            assert np.array_equal(got[:, 3], np.full(T, float(H * W))) and np.array_equal(got[:, 8], np.full(T, float((H - 10) * (W - 10))))


def test_fidelity_exact_cases():
    """X == Y: every squared-error sum is exactly 0, PSNR inf, SSIM 1 within the bound (not bitwise: 2 mu^2 and mu^2 + mu^2 may contract
    differently).  X and Y differing only inside a binary region: the outside sum is exactly 0.  An all-zero region: nan inside."""
    from insv2v import pixel_score as ps
    T, H, W, xdt, ydt = 3, 29, 81, "f32", "f16"
    X = pr.stored(pr.fidelity_inputs(T, H, W, xdt, ydt)["X"], "f16")   # exact in both dtypes
    w = np.zeros((T, H, W))
    w[:, 6:19, 30:70] = 1.0
    w[1] = 0.0                                                         # frame 1: an empty region
    Y = pr.stored(X + 0.3 * w[:, None], "f16")
    got = _run_fidelity(X, X, w, xdt, ydt)
    assert not got[:, :3].any(), "X == Y must give squared-error sums of exactly 0"
    bounds = np.stack([pr.fidelity_frame(X[t], X[t], w[t])[1]["bound"] for t in range(T)])
    n = (H - 10) * (W - 10)
    print(f"[pixel_score] X == Y: |ssim - 1| {np.abs(got[:, 5] / n - 1).max():.3e} (bound {bounds[:, 5].max() / n:.3e})")
    assert (np.abs(got[:, 5] - n) <= bounds[:, 5]).all()
    x, y, region = _crop(X, xdt), _crop(Y, ydt), torch.from_numpy(w).float().to(DEV)
    r = ps.fidelity(x, x, region, source_affine=pr.SIGNED, edited_affine=pr.SIGNED)
    assert (r["mse"] == 0).all() and (r["psnr"] == math.inf).all() and (r["psnr_outside"] == math.inf).all()
    assert (r["psnr_inside"][[0, 2]] == math.inf).all() and math.isnan(r["psnr_inside"][1]) and math.isnan(r["mse_inside"][1])
    r = ps.fidelity(x, y, region, source_affine=pr.SIGNED, edited_affine=pr.SIGNED)
    assert not r["sums"][:, 2].any() and (r["mse_outside"] == 0).all() and (r["psnr_outside"] == math.inf).all()
    assert (r["mse_inside"][[0, 2]] > 1e-3).all() and torch.isfinite(r["psnr_inside"][[0, 2]]).all() and (r["mse"][[0, 2]] > 0).all()
    assert all(math.isnan(r[k][1]) for k in ("mse_inside", "psnr_inside", "ssim_inside")) and r["mse"][1] == 0
    assert torch.isfinite(r["ssim_outside"]).all() and torch.isfinite(r["mse_outside"]).all() and (r["ssim_inside"][[0, 2]] < 0.999).all()
    want = pr.fidelity_metrics(np.stack([pr.fidelity_frame(X[t], Y[t], w[t])[0] for t in range(T)]), H, W)
    for k in ("mse", "ssim", "mse_inside", "ssim_outside"):
        assert np.allclose(r[k].numpy(), want[k], rtol=1e-5, atol=0, equal_nan=True), k


# ------------------------------------------------------------------------------------------------------------------ 2. warp error vs float64
def _run_warp(A, fwd, bwd, w, dt, affine=pr.SIGNED, alpha=pr.ALPHA, beta=pr.BETA):
    from insv2v import ops
    T, _, H, W = A.shape
    a = _crop(A, dt)
    f, b, region = _framed(fwd)[1], (None if bwd is None else _framed(bwd)[1]), (None if w is None else _framed(w)[1])
    outs = [_framed(shape=(T - 1, 3), pad_value=SENT, dtype=torch.float64), _framed(shape=(T - 1, H, W), pad_value=SENT),
            _framed(shape=(T - 1, H, W), pad_value=SENT)]
    wbuf, ws = _framed(shape=(ops.warp_error_workspace_elems(T, H, W),), pad_value=SENT, dtype=torch.float64)
    sums, err, valid = ops.warp_error(a, f, b, region, scale=affine[0], shift=affine[1], alpha=alpha, beta=beta, return_maps=True,
                                      out=tuple(v for _, v in outs), workspace=ws)
    torch.cuda.synchronize()
    assert all(_pads_intact(buf) for buf, _ in outs) and _pads_intact(wbuf), "the kernels wrote outside an output"
    assert sums.data_ptr() == outs[0][1].data_ptr()
    return _np(sums), _np(err), _np(valid)


@pytest.mark.parametrize("T,H,W,dt", pr.WARP_CASES)
def test_warp_error_vs_float64(T, H, W, dt):
    """``valid_map`` exactly wherever the decision margins exceed the guards, ``err_map`` within the element bound on the pixels both sides
    call valid and 0 where the kernel says invalid; the fp64 sums (a) against a float64 sum of the kernel's OWN maps, within the summation
    bound - the reduction - and (b) against the definition's sums when the valid sets agree."""
    inp = pr.warp_inputs(T, H, W, dt)
    n = H * W
    for with_bwd in (True, False):
        for with_region in (True, False):
            R = pr.warp_reference(T, H, W, dt, with_bwd, with_region)
            ref, ex = R["ref"], R["excluded"]
            w = inp["w"] if with_region else None
            sums, err, valid = _run_warp(inp["A"], inp["fwd"], inp["bwd"] if with_bwd else None, w, dt)
            assert np.isfinite(sums).all() and np.isfinite(err).all() and np.isin(valid, (0.0, 1.0)).all()
            assert R["share"] <= mr.MAX_EXCLUDED
            wrong = (valid != ref["valid"]) & ~ex
            assert not wrong.any(), f"valid differs on {int(wrong.sum())} pixels outside the guard"
            assert not err[valid == 0].any(), "err must be 0 where invalid"
            both = (valid == 1) & ref["valid"]
            e = np.abs(err - ref["err"])
            assert (e[both] <= R["elem_bound"][both]).all(), float((e / R["elem_bound"])[both].max())
            # (a) the reduction
            wt = np.ones((T - 1, H, W)) if w is None else w[:T - 1]
            own = np.stack([(wt * valid * err).sum((1, 2)), (wt * valid).sum((1, 2)), valid.sum((1, 2))], 1)
            tol = n * 2.0 ** -53 * np.abs(own)
            assert (np.abs(sums - own) <= tol).all() and np.array_equal(sums[:, 2], own[:, 2]), (sums, own)
            # (b) the definition
            flips = int((valid != ref["valid"]).sum())
            share = float((e / R["elem_bound"])[both].max()) if both.any() else 0.0
            print(f"[pixel_score] warp {T}x{H}x{W} {dt} bwd={with_bwd} region={with_region}: {R['share']:.4f} under the guard, {flips} flipped, "
                  f"valid {valid.mean():.2f}, worst err share of the bound {share:.3f}, reduction error {np.abs(sums - own).max():.2e}")
            if flips == 0:
                bound = (wt * ref["valid"] * R["elem_bound"]).sum((1, 2)) + n * 2.0 ** -53 * np.abs(ref["sums"][:, 0])
                assert (np.abs(sums[:, 0] - ref["sums"][:, 0]) <= bound).all()
                assert (np.abs(sums[:, 1] - ref["sums"][:, 1]) <= n * 2.0 ** -53 * ref["sums"][:, 1]).all()


@pytest.mark.parametrize("H,W,disps,deltas,dt,rect", pr.EXACT_CASES)
def test_warp_error_exact_cases_bitwise(H, W, disps, deltas, dt, rect):
    """A random image translated by integers, fwd = +d, bwd = -d: warp error exactly 0 and (H - |dy|)(W - |dx|) valid pixels; plus a
    per-frame constant (a flicker): err = (delta_{t+1} - delta_t)^2 exactly at every valid pixel; a planted inconsistent rectangle in bwd
    removes exactly its pixels from the count; without bwd the rectangle is not seen."""
    from insv2v import pixel_score as ps
    tc = pr.translation_video(H, W, disps, deltas, rect)
    sums, err, valid = _run_warp(tc["A"], tc["fwd"], tc["bwd"], None, dt, affine=ONE)
    assert np.array_equal(valid, tc["valid"].astype(np.float64))
    assert np.array_equal(err, np.where(tc["valid"], tc["err"][:, None, None], 0.0))
    count = tc["valid"].sum((1, 2)).astype(np.float64)
    assert np.array_equal(sums[:, 2], count) and np.array_equal(sums[:, 1], count) and np.array_equal(sums[:, 0], tc["err"] * count)
    for t, (dx, dy) in enumerate(disps):
        inside = (H - abs(dy)) * (W - abs(dx))
        assert count[t] == inside - ((rect[2] - rect[1]) * (rect[4] - rect[3]) if rect is not None and rect[0] == t else 0)
    r = ps.warp_error(_crop(tc["A"], dt), torch.from_numpy(tc["fwd"]).float().to(DEV), torch.from_numpy(tc["bwd"]).float().to(DEV))
    assert np.array_equal(r["warp_error"].numpy(), tc["err"]) and np.array_equal(r["valid_count"].numpy(), count)
    assert np.array_equal(r["valid_fraction"].numpy(), count / (H * W))
    s0, _, v0 = _run_warp(tc["A"], tc["fwd"], None, None, dt, affine=ONE)
    assert np.array_equal(v0, tc["valid_plain"].astype(np.float64)) and np.array_equal(s0[:, 0], tc["err"] * tc["valid_plain"].sum((1, 2)))


def test_boundary_of_the_consistency_inequality_is_valid():
    """|d|^2 = alpha (|b|^2 + |cf|^2) + beta exactly (b = (2, 0), c = (-1, 0), alpha = 1/8, beta = 3/8): ``<=`` keeps the pixel."""
    H, W = 4, 8
    b, c = np.zeros((1, 2, H, W)), np.zeros((1, 2, H, W))
    b[:, 0], c[:, 0] = 2.0, -1.0
    A = np.full((2, 3, H, W), 0.5)
    sums, _, valid = _run_warp(A, b, c, None, "f32", affine=ONE, alpha=0.125, beta=0.375)
    assert np.array_equal(valid[0], np.tile(np.arange(W) + 2 <= W - 1, (H, 1)).astype(np.float64)) and sums[0, 2] == H * (W - 2)


def test_flicker_that_clip_consistency_cannot_see():
    """The same translated video with and without a per-frame brightness constant: the warp error goes from exactly 0 to exactly
    (delta_{t+1} - delta_t)^2, while the CLIP frame consistency of the two videos differs by less, relatively."""
    from insv2v import pixel_score as ps, synth
    from insv2v.clip_score import synthetic_scorer
    H, W, disps, deltas = 24, 32, [(1, 0), (2, -1), (0, 1)], [0, 16, 4, 24]
    calm, flicker = pr.translation_video(H, W, disps), pr.translation_video(H, W, disps, deltas)
    fwd, bwd = (torch.from_numpy(calm[k]).float().to(DEV) for k in ("fwd", "bwd"))
    vids = [torch.from_numpy(v["A"]).float().to(DEV) for v in (calm, flicker)]
    we = [ps.warp_error(v, fwd, bwd)["warp_error"].numpy() for v in vids]
    assert not we[0].any() and np.array_equal(we[1], flicker["err"]) and (we[1] > 0).all()
    sc = synthetic_scorer(device=DEV, tiny=True)
    ids = synth.synth_token_ids("pixel_score.flicker", 2, 77, synth.CLIP_TINY["vocab_size"])
    fc = [sc.score_edit(vids[0][None] * 2 - 1, v[None] * 2 - 1, ids[0], ids[1])["frame_consistency"] for v in vids]
    rel_clip = abs(fc[1] - fc[0]) / max(abs(fc[0]), abs(fc[1]))
    rel_warp = abs(we[1].mean() - we[0].mean()) / max(we[0].mean(), we[1].mean())
    print(f"[pixel_score] flicker: warp error {we[0].mean():.3e} -> {we[1].mean():.3e} (relative change {rel_warp:.3f}); "
          f"CLIP frame consistency {fc[0]:.5f} -> {fc[1]:.5f} (relative change {rel_clip:.2e})")
    assert math.isfinite(rel_clip) and rel_clip < rel_warp


# ------------------------------------------------------------------------------------------------------------------ 3. determinism, refusals
def test_two_calls_give_the_same_bits_also_on_a_second_stream():
    from insv2v import ops
    T, H, W, dt = pr.WARP_CASES[3]
    inp = pr.warp_inputs(T, H, W, dt)
    a, fwd, bwd, w = _crop(inp["A"], dt), _framed(inp["fwd"])[1], _framed(inp["bwd"])[1], _framed(inp["w"])[1]
    Tf, Hf, Wf, xdt, ydt = pr.FIDELITY_CASES[-1]
    fi = pr.fidelity_inputs(Tf, Hf, Wf, xdt, ydt)
    x, y, wf = _crop(fi["X"], xdt), _crop(fi["Y"], ydt), _framed(fi["w"])[1]

    def run():
        return (*ops.warp_error(a, fwd, bwd, w, scale=0.5, shift=0.5, return_maps=True), ops.frame_fidelity(x, y, wf, x_affine=pr.SIGNED, y_affine=pr.SIGNED))
    first, second = run(), run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert all(_same_bits(p, q) and _same_bits(p, r) for p, q, r in zip(first, second, third))


def test_refusals_leave_the_outputs_untouched():
    from insv2v import ops, _lib
    T, H, W, dt = 3, 17, 23, "f32"
    inp = pr.warp_inputs(4, H, W, dt)
    a, fwd, bwd, w = _crop(inp["A"][:T], dt), _framed(inp["fwd"][:T - 1])[1], _framed(inp["bwd"][:T - 1])[1], _framed(inp["w"][:T])[1]
    outs = [_framed(shape=(T - 1, 3), pad_value=SENT, dtype=torch.float64), _framed(shape=(T - 1, H, W), pad_value=SENT),
            _framed(shape=(T - 1, H, W), pad_value=SENT), _framed(shape=(T, 10), pad_value=SENT, dtype=torch.float64)]
    wbuf, ws = _framed(shape=(max(ops.warp_error_workspace_elems(T, H, W), ops.frame_fidelity_workspace_elems(T, H, W)),), pad_value=SENT, dtype=torch.float64)
    views = tuple(v for _, v in outs)

    def untouched():
        torch.cuda.synchronize()
        return all(_pads_intact(buf) and bool(torch.isnan(v).all()) for buf, v in outs) and _pads_intact(wbuf) and bool(torch.isnan(ws).all())
    warp_out = views[:3]
    bad = [dict(alpha=-0.01), dict(beta=-1.0), dict(alpha=float("nan")), dict(beta=float("inf")), dict(workspace=ws[:1]),
           dict(out=(ws[:(T - 1) * 3].view(T - 1, 3), views[1], views[2])),                            # sums inside the workspace
           dict(out=(views[0], views[1], views[1])),                                                      # the two maps are one buffer
           dict(out=(views[0], fwd.view(-1)[:(T - 1) * H * W].view(T - 1, H, W), views[2])),              # a map over an input
           dict(out=(views[0], views[1], outs[1][0][PAD + 4:PAD + 4 + (T - 1) * H * W].view(T - 1, H, W)))]           # valid_map inside err_map's buffer
    for kw in bad:
        with pytest.raises(_lib.HipKernelError):
            ops.warp_error(a, fwd, bwd, w, **dict(dict(scale=0.5, shift=0.5, return_maps=True, out=warp_out, workspace=ws), **kw))
        assert untouched(), kw
    for frames, f in ((a[:1], fwd[:0]), (a[:, :, :1], fwd[:, :, :1].contiguous()), (a[:, :, :, :1], fwd[:, :, :, :1].contiguous())):   # T < 2, H = 1, W = 1
        P, h, ww = frames.shape[0] - 1, frames.shape[2], frames.shape[3]
        with pytest.raises(_lib.HipKernelError):
            ops.warp_error(frames, f, None, None, out=(views[0][:max(P, 0)], None, None), workspace=ws)
        assert untouched()
    for args in ((a.transpose(2, 3), fwd), (a.double(), fwd), (a.cpu(), fwd), (a, fwd.half()), (a, fwd[:, :, ::2])):
        with pytest.raises(_lib.HipKernelError):
            ops.warp_error(*args, out=warp_out, workspace=ws, return_maps=True)
    # fidelity
    for x, y, kw in ((a[:, :, :10], a[:, :, :10], {}), (a[:, :, :, :10], a[:, :, :, :10], {}), (a, a[:, :, 1:], {}), (a, a, dict(workspace=ws[:T * 10 - 1])),
                     (a, a, dict(out=ws[:T * 10].view(T, 10))), (a, a, dict(region=w[:, 1:].contiguous())), (a.double(), a, {})):
        with pytest.raises(_lib.HipKernelError):
            ops.frame_fidelity(x, y, kw.pop("region", w), **dict(dict(out=views[3], workspace=ws), **kw))
        assert untouched()
    # and the same buffers do run
    ops.warp_error(a, fwd, bwd, w, scale=0.5, shift=0.5, return_maps=True, out=warp_out, workspace=ws)
    ops.frame_fidelity(a, a, w, x_affine=pr.SIGNED, y_affine=pr.SIGNED, out=views[3], workspace=ws)
    torch.cuda.synchronize()
    assert all(torch.isfinite(v).all() and _pads_intact(buf) for buf, v in outs) and _pads_intact(wbuf)


# ------------------------------------------------------------------------------------------------------------------ 4. pipeline
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


HP, WP, SEED = 32, 48, 91


def _unit(T):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"pixel_score.ev.frames.{T}", (1, T, 3, HP, WP), kind="uniform"),
                text_cond=synth.synth_input("pixel_score.ev.tc", (1, 77, 64)), text_uncond=synth.synth_input("pixel_score.ev.tu", (1, 77, 64)))


def test_a_hard_mask_leaves_the_outside_exactly_alone(tiny_model, pipe):
    """The end-to-end check of the masked path: for a binary mask the pixels outside it are the input's, so mse_outside is exactly 0 and
    psnr_outside inf, and something was edited inside; the same unit without the mask changes the outside too.  ``score_pixels`` with
    injected flows is ``fidelity`` + ``warp_error`` called separately, bit for bit."""
    from insv2v.run_loveu_tgve import edit_video
    from insv2v import pixel_score as ps
    T = 4
    u = _unit(T)
    mask = torch.zeros((1, 1, HP, WP))
    mask[:, :, 9:22, 14:30] = 1.0
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    masked = edit_video(*args, seed=SEED, unit=0, mask=mask)
    plain = edit_video(*args, seed=SEED, unit=0)
    tc = pr.translation_video(HP, WP, [(1, 0), (0, 1), (-1, 1)])
    flows = dict(fwd=torch.from_numpy(tc["fwd"]).float(), bwd=torch.from_numpy(tc["bwd"]).float())
    r = ps.score_pixels(u["frames"], masked, mask=mask, flows=flows)
    assert (r["mse_outside"] == 0).all() and (r["psnr_outside"] == math.inf).all() and (r["mse_inside"] > 0).all() and (r["mse"] > 0).all()
    assert torch.isfinite(r["psnr_inside"]).all() and torch.isfinite(r["ssim_outside"]).all() and (r["ssim_inside"] < 1).all()
    r0 = ps.score_pixels(u["frames"], plain, mask=mask, flows=flows)
    assert (r0["mse_outside"] > 0).all() and torch.isfinite(r0["psnr_outside"]).all()
    print(f"[pixel_score] tiny edit: mse inside {r['mse_inside'].mean():.4f}, outside {r['mse_outside'].mean():.1e}; unmasked outside "
          f"{r0['mse_outside'].mean():.4f}; warp error {r['warp_error_mean']:.4f} vs source {r['warp_error_source_mean']:.4f}")
    # the pieces, called separately
    dev = masked.device
    src, edt = u["frames"][0].to(dev), masked[0]
    region = mask[0].to(dev).expand(T, HP, WP).contiguous()
    fid = ps.fidelity(src, edt, region, source_affine=ps.AFFINE_SIGNED, edited_affine=ps.AFFINE_SIGNED)
    we = ps.warp_error(edt, flows["fwd"], flows["bwd"], affine=ps.AFFINE_SIGNED)
    ws = ps.warp_error(src, flows["fwd"], flows["bwd"], affine=ps.AFFINE_SIGNED)
    assert all(_same_bits(r[k], fid[k]) for k in fid if k != "sums") and set(fid) - {"sums"} <= set(r)
    assert _same_bits(r["warp_error"], we["warp_error"]) and _same_bits(r["warp_error_source"], ws["warp_error"])
    assert _same_bits(r["valid_fraction"], we["valid_fraction"]) and _same_bits(we["valid_count"], ws["valid_count"])   # one valid set
    assert _same_bits(r["warp_error_mean"], we["warp_error"].mean()) and r["warp_error"].shape == (T - 1,)
    # no flow source: no warp fields; T = 1: fidelity only; no mask: no inside / outside
    bare = ps.score_pixels(u["frames"], masked)
    assert set(bare) == {"mse", "psnr", "ssim"} and _same_bits(bare["mse"], r["mse"]) and _same_bits(bare["ssim"], r["ssim"])
    one = ps.score_pixels(u["frames"][:, :1], masked[:, :1], mask=mask, flows=None, flow_estimator=lambda a, b: 1 / 0)
    assert "warp_error" not in one and one["mse"].shape == (1,) and _same_bits(one["mse_outside"], r["mse_outside"][:1])
    noocc = ps.score_pixels(u["frames"], masked, flows=dict(fwd=flows["fwd"]), occlusion=False)
    assert (noocc["valid_fraction"] >= r["valid_fraction"]).all()


HR, WR = 128, 192   # the smallest frame tests/test_raft_gpu.py runs the estimator at


def test_score_pixels_with_the_raft_estimator():
    """Flows from the key-hashed RAFT (no accuracy claim): ``score_pixels`` reproduces ``pair_flows`` + ``warp_error``, on the SOURCE's flows."""
    from insv2v import synth, shapes, pixel_score as ps
    from insv2v.raft import RAFTFlow
    from insv2v.mask_track import pair_flows
    raft = RAFTFlow(DEV, synth.synth_raft_state_dict(shapes.raft_shapes()))
    T = 3
    src = synth.synth_input("pixel_score.raft.frames", (1, T, 3, HR, WR), kind="uniform").to(DEV)
    edt = (src * 0.9 + 0.05 * synth.synth_input("pixel_score.raft.edit", (1, T, 3, HR, WR), kind="uniform").to(DEV)).half()
    r = ps.score_pixels(src, edt, flow_estimator=raft)
    flows = pair_flows(src, raft)
    we = ps.warp_error(edt[0], flows["fwd"], flows["bwd"], affine=ps.AFFINE_SIGNED)
    ws = ps.warp_error(src[0], flows["fwd"], flows["bwd"], affine=ps.AFFINE_SIGNED)
    assert _same_bits(r["warp_error"], we["warp_error"]) and _same_bits(r["warp_error_source"], ws["warp_error"])
    assert r["warp_error"].shape == (T - 1,) and ((r["valid_fraction"] >= 0) & (r["valid_fraction"] <= 1)).all()
    assert all(math.isfinite(v) or math.isnan(v) for v in r["warp_error"].tolist()) and torch.isfinite(r["mse"]).all() and (r["mse"] > 0).all()


# ------------------------------------------------------------------------------------------------------------------ 5. command line
def test_cli_writes_pixel_scores_with_and_without_a_clip_scorer(tmp_path, monkeypatch):
    """``--synthetic 2 --synthetic-tiny --synthetic-mask --score-pixels --score-warp --score-out`` (reduced-width models, a key-hashed RAFT,
    3 frames at 128 x 128, one step): one record per unit with the documented keys; the hard synthetic mask gives mse_outside = 0 and
    psnr_outside = inf in the JSON; with ``--score-synthetic`` the same records also carry the CLIP keys."""
    from insv2v import run_loveu_tgve, inference
    from insv2v.clip_score import SCORE_KEYS

    class Eager(inference.InferenceIP2PVideo):
        def __init__(self, *a, **kw):
            super().__init__(*a, **dict(kw, **EAGER))
    monkeypatch.setattr(inference, "InferenceIP2PVideo", Eager)
    T, S = 3, 128
    common = ["--synthetic", "2", "--synthetic-tiny", "--synthetic-mask", "--num-frames", str(T), "--image-size", str(S), "--steps", "1", "--seed", "5",
              "--score-pixels", "--score-warp"]
    fid_keys = [k + s for k in run_loveu_tgve.PIXEL_FIDELITY_KEYS for s in ("", "_inside", "_outside")]
    recs = {}
    for name, extra in (("plain", []), ("clip", ["--score-synthetic"])):
        out = tmp_path / f"{name}.json"
        run_loveu_tgve.main(common + extra + ["--score-out", str(out), "--out", str(tmp_path / f"{name}.pt")])
        recs[name] = json.load(open(out))
        assert [r["unit"] for r in recs[name]] == [0, 1]
        for r in recs[name]:
            assert set(r) == {"unit", *fid_keys, *run_loveu_tgve.PIXEL_WARP_KEYS} | (set(SCORE_KEYS) | {"text_alignment", "frame_consistency"} if extra else set())
            assert all(len(r[k]) == T for k in fid_keys) and all(len(r[k]) == T - 1 for k in ("warp_error", "warp_error_source", "valid_fraction"))
            assert r["mse_outside"] == [0.0] * T and r["psnr_outside"] == [math.inf] * T
            for k in fid_keys:
                if k != "psnr_outside":
                    assert all(math.isfinite(v) for v in r[k]), (k, r[k])
            assert all(v > 0 for v in r["mse_inside"]) and all(0 <= v <= 1 for v in r["valid_fraction"])
            for k in ("warp_error", "warp_error_source"):   # nan only for a pair the key-hashed flows leave without a valid pixel
                assert all((math.isfinite(v) and v >= 0) or (math.isnan(v) and f == 0) for v, f in zip(r[k], r["valid_fraction"])), (k, r[k])
    for a, b in zip(recs["plain"], recs["clip"]):   # the same seed: the pixel scores do not depend on the CLIP scorer being there
        assert all(a[k] == b[k] or (k.startswith("warp") and str(a[k]) == str(b[k])) for k in a)
