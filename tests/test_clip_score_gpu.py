"""CLIP scoring on the GPU: the preprocess and score kernels against the float64 restatement (tests/clip_score_ref.py), the image tower
and the projected text features against the goldens (outputs of the real transformers models, tools/gen_golden_clip_score.py),
``score_edit`` end to end, and the driver's --score-out path.  Nothing here reads anything but tests/golden/."""
import ctypes
import json
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import clip_score_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL_IN, SENTINEL_OUT = 3.0e4, -777.0


def report(out, ref, what, rms_tol=1e-2, max_tol=4e-2):
    """The project's fp16 tolerance (report() of tests/test_model_gpu.py): rel-rms <= 1e-2, max-abs / max-ref <= 4e-2."""
    out, ref = out.detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    rms = ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    mx = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"[parity] {what}: rel-rms {rms:.3e}  max-abs/max-ref {mx:.3e}")
    assert math.isfinite(rms) and rms <= rms_tol and mx <= max_tol, f"{what}: rel-rms {rms:.3e} (tol {rms_tol}), max {mx:.3e} (tol {max_tol})"


# ---------------------------------------------------------------------------------------------------------------- preprocess kernel
GEOMETRIES = [(8, 8, 28), (40, 72, 28), (28, 28, 28), (15, 9, 28), (64, 96, 224)]


def _input(H, W, dtype, strided, unit_range, n=2):
    """Frames inside a sentinel-filled buffer: contiguous, or a crop of a larger tensor (every stride differs from the dense one).
    Values in [0, 1] (unit_range) or [-1, 1]; the sentinel is so large that one stray tap breaks the bound by orders of magnitude."""
    g = torch.Generator().manual_seed(7 * H + W + int(strided))
    vals = torch.rand((n, 3, H, W), generator=g)
    if not unit_range:
        vals = vals * 2 - 1
    vals = vals.to(dtype)
    if strided:
        big = torch.full((n + 1, 4, H + 5, W + 7), SENTINEL_IN, dtype=dtype, device=DEV)
        view = big[1:, 1:, 2:2 + H, 3:3 + W]
    else:
        big = torch.full((n * 3 * H * W + 128,), SENTINEL_IN, dtype=dtype, device=DEV)
        view = big[64:64 + n * 3 * H * W].view(n, 3, H, W)
    view.copy_(vals.to(DEV))
    return big, view, vals


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("H,W,S", GEOMETRIES)
def test_preprocess_matches_the_restatement(H, W, S, dtype):
    """Element by element against the float64 front end; bound 2^-11 |ref| + 1e-5 max(1, |ref|): one fp16 rounding of the stored value
    plus fp32 slack for 16 taps of O(1) terms (measured beyond the rounding: <= 2.1e-6 at every geometry, 0 at the identity; DESIGN.md
    section 16 has the 2e-5 a coordinate evaluated in fp32 costs, which is why the kernel takes its floor and fraction in integers).  Two forms per geometry and dtype: contiguous frames
    in [-1, 1] with the default ld (3 P^2 rounded up to 64), and a strided crop in [0, 1] with a wider ld; the guards around the output and
    the sentinels around the input stay untouched / unread, the pad columns are exact zeros."""
    from insv2v import ops
    P = 14
    rows_per = (S // P) ** 2
    for strided, unit_range, ld in ((False, False, None), (True, True, 3 * P * P + 113)):   # 640 (the GEMM's K), and an odd 701
        big, view, vals = _input(H, W, dtype, strided, unit_range)
        before = big.clone()
        n = view.shape[0]
        ldv = ld if ld is not None else -(-3 * P * P // 64) * 64
        guard = 2 * ldv
        buf = torch.full((guard + n * rows_per * ldv + guard,), SENTINEL_OUT, dtype=torch.float16, device=DEV)
        out = buf[guard:guard + n * rows_per * ldv].view(n * rows_per, ldv)
        scale, shift = (1.0, 0.0) if unit_range else (0.5, 0.5)
        got = ops.clip_preprocess(view, S, P, ld=ldv, in_scale=scale, in_shift=shift, out=out)
        assert got.data_ptr() == out.data_ptr()
        if ld is None:   # the default ld of the wrapper is the same buffer shape
            got2 = ops.clip_preprocess(view, S, P, in_scale=scale, in_shift=shift)
            assert got2.shape == out.shape and torch.equal(got2, out)
        torch.cuda.synchronize()
        assert torch.equal(big, before), "the input buffer was written"
        assert (buf[:guard] == SENTINEL_OUT).all() and (buf[-guard:] == SENTINEL_OUT).all(), "a guard element of the output was written"
        ref = R.patch_rows(R.front_end(vals.double(), S, scale, shift), P, ld=ldv)
        o = out.double().cpu()
        assert (o[:, 3 * P * P:] == 0).all(), "pad columns must be exact zeros"
        err = (o - ref).abs()
        bound = 2.0 ** -11 * ref.abs() + 1e-5 * ref.abs().clamp_min(1.0)
        slack = (err - 2.0 ** -11 * ref.abs()).max().item()
        print(f"[parity] clip_preprocess {H}x{W}->{S} {dtype} strided={strided}: max err {err.max().item():.3e}, beyond one fp16 rounding {slack:.3e}")
        assert torch.isfinite(o).all() and (err <= bound).all(), f"max excess {(err - bound).max().item():.3e}"


def test_preprocess_refusals():
    from insv2v import _lib, ops
    x = torch.rand((1, 3, 8, 8), device=DEV)
    ops.clip_preprocess(x, 28, 14)   # the accepted form of what follows
    for kw in (dict(size=30, patch=14), dict(size=28, patch=14, ld=3 * 14 * 14 - 4), dict(size=0, patch=14), dict(size=28, patch=0),
               dict(size=-28, patch=14), dict(size=28, patch=-14)):
        with pytest.raises(_lib.HipKernelError, match="invalid argument"):
            ops.clip_preprocess(x, kw["size"], kw["patch"], ld=kw.get("ld"))
    with pytest.raises(_lib.HipKernelError, match="invalid argument"):
        ops.clip_preprocess(x[:0], 28, 14)   # no frames
    with pytest.raises(_lib.HipKernelError):
        ops.clip_preprocess(x[:, :2], 28, 14)
    with pytest.raises(_lib.HipKernelError):
        ops.clip_preprocess(x.double(), 28, 14)
    lib = _lib.load()
    out = torch.empty((4, 640), dtype=torch.float16, device=DEV)

    def desc(**over):
        d = _lib.ClipPreprocessDesc()
        d.x, d.out, d.ld = x.data_ptr(), out.data_ptr(), 640
        d.stride_n, d.stride_c, d.stride_h, d.stride_w = x.stride()
        d.n, d.H, d.W, d.S, d.P, d.x_fp32, d.in_scale, d.in_shift = 1, 8, 8, 28, 14, 1, 1.0, 0.0
        d.mean[:], d.std[:] = R.CLIP_MEAN, R.CLIP_STD
        for k, v in over.items():
            setattr(d, k, v)
        return d
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.insv2v_clip_preprocess(ctypes.byref(desc()), stream) == 0
    for over in (dict(x=None), dict(out=None), dict(n=0), dict(H=0), dict(W=-1), dict(S=27), dict(ld=587)):
        assert lib.insv2v_clip_preprocess(ctypes.byref(desc(**over)), stream) == -1, over
    assert lib.insv2v_clip_preprocess(None, stream) == -1
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------------- score kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("D", [32, 768])
def test_scores_match_the_restatement(D, n, dtype):
    """Bound 4 D 2^-24 absolute.  With u = 2^-24: every operand is divided by its fp32 norm (the sum of D squares carries a relative error
    <= D u, its root half of that, the division u more: each normalised element is off by at most (D / 2 + 2) u relatively), and every dot
    product of two such unit vectors adds at most D u (its D products and additions, Cauchy-Schwarz on the magnitudes), so a cosine is off
    by at most D u + 2 (D / 2 + 2) u + the two final norms' (D / 2 + 1) u each = (3 D + 6) u < 4 D u for D >= 6.  The direction cosine
    subtracts two unit vectors first: an absolute error of (D / 2 + 2) u per operand becomes a relative error of that over |d|, so the
    same bound needs |d| >= 1 for both differences - asserted on the inputs (independent random features have |d| ~ 1.4).  The reference
    reads the very fp16 / fp32 values the kernel reads."""
    from insv2v import ops
    g = torch.Generator().manual_seed(100 * D + n)
    feats = [torch.randn(s, generator=g).to(dtype) for s in ((n, D), (n, D), (D,), (D,))]
    nz = lambda v: v.double() / v.double().norm(dim=-1, keepdim=True)
    assert (nz(feats[1]) - nz(feats[0])).norm(dim=-1).min() >= 1 and (nz(feats[3]) - nz(feats[2])).norm() >= 1
    # strided rows: the features sit in wider, sentinel-filled matrices
    wide = [torch.full((n, D + 24), float("nan"), dtype=dtype, device=DEV) for _ in range(2)]
    for w, f in zip(wide, feats):
        w[:, 8:8 + D] = f.to(DEV)
    dev = [wide[0][:, 8:8 + D], wide[1][:, 8:8 + D], feats[2].to(DEV), feats[3].to(DEV)]
    out = ops.clip_scores(*dev)
    again = ops.clip_scores(*dev)
    ref = R.scores(*feats)
    err = (out.double().cpu() - ref).abs().max().item()
    bound = 4 * D * 2.0 ** -24
    print(f"[parity] clip_scores D={D} n={n} {dtype}: max abs err {err:.3e} (bound {bound:.3e})")
    assert out.dtype == torch.float32 and tuple(out.shape) == (n, 5) and torch.isfinite(out).all()
    assert err <= bound
    assert out[-1, 4].item() == 0.0, "the last frame has no successor: exact 0"
    assert torch.equal(out, again), "two calls must give the same bits"
    # per-frame prompts ([n, D]) against the same reference, row by row
    if n > 1:
        txt = [torch.randn((n, D), generator=g).to(dtype) for _ in range(2)]
        assert (nz(txt[1]) - nz(txt[0])).norm(dim=-1).min() >= 1
        out = ops.clip_scores(dev[0], dev[1], txt[0].to(DEV), txt[1].to(DEV))
        assert (out.double().cpu() - R.scores(feats[0], feats[1], txt[0], txt[1])).abs().max().item() <= bound
    # img0 == img1: the direction has no length; torch's eps rule gives a finite value (0), never nan
    same = ops.clip_scores(dev[0], dev[0], dev[2], dev[3])
    ref = R.scores(feats[0], feats[0], feats[2], feats[3])
    assert torch.isfinite(same).all() and (same.double().cpu() - ref).abs().max().item() <= bound
    assert (same[:, 2] == 0).all() and ref[:, 2].abs().max() == 0


def test_scores_and_normalise_refusals():
    from insv2v import _lib, ops
    a = torch.randn((3, 32), device=DEV)
    t = torch.randn((32,), device=DEV)
    with pytest.raises(_lib.HipKernelError):
        ops.clip_scores(a, a[:2], t, t)
    with pytest.raises(_lib.HipKernelError):
        ops.clip_scores(a, a, t[:16], t[:16])
    with pytest.raises(_lib.HipKernelError):
        ops.clip_scores(a, a.half(), t, t)
    with pytest.raises(_lib.HipKernelError):
        ops.clip_scores(a.cpu(), a.cpu(), t.cpu(), t.cpu())
    lib = _lib.load()
    out = torch.empty((3, 5), device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda x: x.data_ptr()
    assert lib.insv2v_clip_scores(p(a), p(a), p(t), p(t), 1, 32, 32, 0, 3, 32, 1e-8, p(out), s) == 0
    for bad in ((None, p(a), p(t), p(t), 1, 32, 32, 0, 3, 32, 1e-8, p(out)), (p(a), p(a), p(t), None, 1, 32, 32, 0, 3, 32, 1e-8, p(out)),
                (p(a), p(a), p(t), p(t), 1, 32, 32, 0, 3, 32, 1e-8, None), (p(a), p(a), p(t), p(t), 1, 32, 32, 0, 0, 32, 1e-8, p(out)),
                (p(a), p(a), p(t), p(t), 1, 32, 32, 0, 3, 0, 1e-8, p(out)), (p(a), p(a), p(t), p(t), 1, 16, 32, 0, 3, 32, 1e-8, p(out)),
                (p(a), p(a), p(t), p(t), 1, 32, 32, 8, 3, 32, 1e-8, p(out)), (p(a), p(a), p(t), p(t), 1, 32, 32, 0, 3, 32, 0.0, p(out))):
        assert lib.insv2v_clip_scores(*bad, s) == -1, bad
    # x / |x| per row (encode_image / encode_text's last line), fp16 and fp32, strided rows
    for dtype in (torch.float32, torch.float16):
        x = torch.randn((3, 40), device=DEV).to(dtype)[:, 4:36]
        y = ops.l2_normalize(x)
        ref = x.double().cpu() / x.double().cpu().norm(dim=-1, keepdim=True)
        assert y.dtype == torch.float32 and (y.double().cpu() - ref).abs().max().item() <= 32 * 2.0 ** -24
    assert lib.insv2v_l2_normalize(None, 1, 32, p(out), 32, 3, 32, s) == -1 and lib.insv2v_l2_normalize(p(a), 1, 16, p(out), 32, 3, 32, s) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------- towers
def _configs(name):
    from insv2v import synth
    return (synth.CLIP_VISION_TINY, synth.CLIP_TINY) if name == "tiny" else (synth.CLIP_VISION_FULL, synth.CLIP_FULL)


def _state_dict(name):
    from insv2v import shapes, synth
    vis, txt = _configs(name)
    sd = synth.synth_state_dict(shapes.clip_vision_shapes(**vis))
    sd.update(synth.synth_state_dict(shapes.clip_text_shapes(**dict(txt, prefix="text_model.", with_projection=True))))
    return sd


_SCORERS = {}


def _scorer(name):
    """One scorer per configuration for the whole module (the full towers are 0.4 G parameters of key-hashed weights)."""
    if name not in _SCORERS:
        from insv2v.clip_score import ClipSimilarity
        vis, txt = _configs(name)
        _SCORERS[name] = ClipSimilarity(device=DEV, vision_config=vis, text_config=txt).load_state_dict(_state_dict(name))
    return _SCORERS[name]


def _unit(v):
    v = torch.as_tensor(v).double().cpu()
    return v / v.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("name", ["tiny", "full"])
def test_towers_match_the_goldens(name, golden):
    """CLIPVisionTransformer behind the preprocess kernel, and the projected text features, against the real transformers models' outputs;
    the project's fp16 tolerance.  Measured: rel-rms 6.1e-4 / 1.3e-3 (image, tiny / full) and 9.2e-4 / 1.2e-3 (text)."""
    g = golden(f"clip_score_{name}")
    sc = _scorer(name)
    for tag in ("src", "edit"):
        frames = torch.from_numpy(g[f"{tag}_frames"]).to(DEV)
        emb = sc.image_embeds(frames, 0.5, 0.5)
        assert emb.dtype == torch.float32
        report(emb, g[f"image_embeds_{tag}"], f"CLIP image tower {name} {tag} clip (golden = transformers.CLIPVisionModelWithProjection)")
        # fp32 frames in [0, 1] through the reference's own entry point give the same features, normalised
        feats = sc.encode_image(frames.float() * 0.5 + 0.5)
        report(feats, _unit(g[f"image_embeds_{tag}"]), f"encode_image {name} {tag}")
        assert (feats.double().norm(dim=-1) - 1).abs().max().item() <= 1e-5
    ids = torch.from_numpy(g["input_ids"]).long()
    report(sc.text_embeds(ids), g["text_embeds"], f"CLIP text tower + text_projection {name} (golden = transformers.CLIPTextModelWithProjection)")
    report(sc.encode_text_ids(ids), _unit(g["text_embeds"]), f"encode_text_ids {name}")
    # the first preprocessed frame, as the tower saw it, against the reference's own fp32 resize (one fp16 rounding + its fp32 error)
    from insv2v import ops
    vis = sc.vision.cfg
    rows = ops.clip_preprocess(torch.from_numpy(g["src_frames"][:1]).to(DEV), vis["image_size"], vis["patch_size"], in_scale=0.5, in_shift=0.5)
    ref = R.patch_rows(torch.from_numpy(g["pixels0"]).double()[None], vis["patch_size"], ld=rows.shape[1])
    assert ((rows.double().cpu() - ref).abs() <= 2.0 ** -11 * ref.abs() + 4e-5 * ref.abs().clamp_min(1.0)).all()


def test_openai_layout_gives_the_same_bits(golden):
    """The same weights in the OpenAI ``clip`` layout (fused in_proj, transposed projections): bit-identical features.  The key map does not
    depend on the widths, so the reduced-width towers carry this check."""
    from insv2v.clip_score import ClipSimilarity
    g = golden("clip_score_tiny")
    vis, txt = _configs("tiny")
    oa = ClipSimilarity(device=DEV, vision_config=vis, text_config=txt).load_state_dict(R.transformers_to_openai(_state_dict("tiny")))
    sc = _scorer("tiny")
    frames = torch.from_numpy(g["edit_frames"]).to(DEV)
    ids = torch.from_numpy(g["input_ids"]).long()
    assert torch.equal(oa.image_embeds(frames, 0.5, 0.5), sc.image_embeds(frames, 0.5, 0.5))
    assert torch.equal(oa.text_embeds(ids), sc.text_embeds(ids))


# --------------------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", ["tiny", "full"])
def test_score_edit_matches_the_golden_scores(name, golden):
    """``score_edit`` on the golden clips (a brightness ramp and its reverse, [1,4,3,40,72] in [-1, 1]) against the scores of the reference
    features.  The direction cosine divides by |f1 - f0|: its error is ~ 2 eps / gap for a feature error eps, so the test states its input
    condition and asserts it on the golden itself - every frame has |f1 - f0| >= 0.2 and |t1 - t0| >= 0.2 (reference values: image gaps
    0.755 / 0.317 / 0.317 / 0.755 tiny, 0.609 / 0.242 / 0.242 / 0.609 full; text gap 0.729 / 0.607).  eps = the largest L2 distance between a
    normalised feature of ours and the golden's, measured here; plain cosines may be off by 2 eps, the direction cosine by 4 eps / min(gap).
    The consecutive-frame cosines of the reference (0.953 / 0.950 / 0.983 tiny, 0.976 / 0.971 / 0.983 full) differ from 1 and from the
    skip-two cosines (0.822 / 0.878, 0.900 / 0.913) by more than that bound, so an off-by-one in the frame pairing cannot pass.
    Measured on an MI355X: eps 1.04e-3 tiny / 1.36e-3 full, so the bounds are 2.1e-3 / 1.3e-2 and 2.7e-3 / 2.2e-2; the
    worst errors were 2.7e-4 (cosines) / 2.4e-4 (direction) tiny and 1.2e-4 / 3.1e-4 full."""
    g = golden(f"clip_score_{name}")
    sc = _scorer(name)
    f0, f1, t = _unit(g["image_embeds_src"]), _unit(g["image_embeds_edit"]), _unit(g["text_embeds"])
    gap = torch.cat([(f1 - f0).norm(dim=-1), (t[1] - t[0]).norm()[None]])
    assert gap.min().item() >= 0.2, f"input condition: gaps {gap.tolist()}"
    src, edit = torch.from_numpy(g["src_frames"]).to(DEV)[None], torch.from_numpy(g["edit_frames"]).to(DEV)[None]
    ids = torch.from_numpy(g["input_ids"]).long()
    r = sc.score_edit(src, edit, ids[0], ids[1:2])
    ours = [_unit(sc.image_embeds(src[0], 0.5, 0.5)), _unit(sc.image_embeds(edit[0], 0.5, 0.5)), _unit(sc.text_embeds(ids))]
    eps = max((a - b).norm(dim=-1).max().item() for a, b in zip(ours, (f0, f1, t)))
    b_cos, b_dir = 2 * eps, 4 * eps / gap.min().item()
    ref = torch.from_numpy(g["scores"]).double()
    got = torch.stack([r[k].double() for k in ("sim_0", "sim_1", "sim_direction", "sim_image", "consistency")], 1)
    err = (got - ref).abs().max(0).values
    print(f"[parity] score_edit {name}: eps {eps:.3e}, min gap {gap.min().item():.3f}, bounds {b_cos:.3e} / {b_dir:.3e}, "
          f"errors sim_0 {err[0]:.3e} sim_1 {err[1]:.3e} sim_direction {err[2]:.3e} sim_image {err[3]:.3e} consistency {err[4]:.3e}")
    assert eps <= 2e-2, "the towers' parity test bounds the feature error; a larger one makes these bounds meaningless"
    assert torch.isfinite(got).all()
    for j in (0, 1, 3, 4):
        assert err[j].item() <= b_cos, (j, err[j].item(), b_cos)
    assert err[2].item() <= b_dir, (err[2].item(), b_dir)
    cons, skip2 = ref[:-1, 4], R.cosine(f1[:-2], f1[2:])
    assert (1 - cons).min().item() > b_cos and (cons[:-1] - skip2).abs().min().item() > b_cos and (cons[1:] - skip2).abs().min().item() > b_cos
    assert got[-1, 4].item() == 0.0
    assert r["text_alignment"] == pytest.approx(got[:, 1].mean().item(), abs=1e-6)
    assert r["frame_consistency"] == pytest.approx(got[:-1, 4].mean().item(), abs=1e-6)
    assert abs(r["text_alignment"] - ref[:, 1].mean().item()) <= b_cos and abs(r["frame_consistency"] - cons.mean().item()) <= b_cos
    # the reference's surface: forward() on images in [0, 1] and token ids gives the first four columns
    if name == "tiny":
        img0, img1 = src[0].float() * 0.5 + 0.5, edit[0].float() * 0.5 + 0.5
        four = sc(img0, img1, ids[0:1], ids[1:2])
        assert len(four) == 4 and all((four[j].double().cpu() - ref[:, j]).abs().max().item() <= (b_dir if j == 2 else b_cos) for j in range(4))
        one = sc.score_edit(src[:, :1], edit[:, :1], ids[0], ids[1])
        assert math.isnan(one["frame_consistency"]) and one["consistency"].tolist() == [0.0] and one["sim_1"].shape == (1,)
        with pytest.raises(ValueError):
            sc.score_edit(src, edit[:, :3], ids[0], ids[1])


# -------------------------------------------------------------------------------------------------------------------------- driver
def test_driver_scores_synthetic_units(tmp_path):
    """run_loveu_tgve.main with two synthetic units (reduced-width models, 1 step, 8 frames at 64 x 64) and a key-hashed scorer writes a
    JSON of two records of finite numbers; a clip scored against itself has sim_image >= 1 - 1e-3."""
    from insv2v import run_loveu_tgve
    from insv2v.clip_score import SCORE_KEYS
    out = tmp_path / "scores.json"
    run_loveu_tgve.main(["--synthetic", "2", "--synthetic-tiny", "--score-synthetic", "--score-out", str(out), "--num-frames", "8",
                         "--image-size", "64", "--steps", "1", "--out", str(tmp_path / "edited.pt")])
    recs = json.load(open(out))
    assert [r["unit"] for r in recs] == [0, 1]
    for r in recs:
        for k in SCORE_KEYS:
            assert len(r[k]) == 8 and all(math.isfinite(v) and -1.0001 <= v <= 1.0001 for v in r[k]), (k, r[k])
        assert r["consistency"][-1] == 0.0
        assert math.isfinite(r["text_alignment"]) and math.isfinite(r["frame_consistency"])
        assert r["text_alignment"] == pytest.approx(sum(r["sim_1"]) / 8, abs=1e-6)
        assert r["frame_consistency"] == pytest.approx(sum(r["consistency"][:-1]) / 7, abs=1e-6)
    assert recs[0]["sim_1"] != recs[1]["sim_1"]
    edited = torch.load(tmp_path / "edited.pt")
    assert tuple(edited.shape) == (1, 2, 8, 3, 64, 64)
    sc = _scorer("tiny")
    clip = edited[0, :1].to(DEV)
    ids = torch.from_numpy(__import__("numpy").load(os.path.join(HERE, "golden", "clip_score_tiny.npz"))["input_ids"]).long()
    self_score = sc.score_edit(clip, clip, ids[0], ids[1])
    assert self_score["sim_image"].min().item() >= 1 - 1e-3
    assert all(torch.isfinite(self_score[k]).all() for k in SCORE_KEYS)   # also the direction between a clip and itself (torch's eps rule)
