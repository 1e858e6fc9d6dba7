"""Masked and partial edits on the host: the schedulers' known_coefficients against float64 alphas_cumprod, the strength table, the
float64 restatement's limiting cases (tests/masked_ref.py), argument refusals, and the interfaces the feature adds (C header, ctypes
mirror and descriptor layout, ops / pipeline / driver keywords, CLI)."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import masked_ref as kr
import multistep_ref as mr
from conftest import ROOT

KINDS = ("ddim", "ddpm", "dpmsolver++", "sde-dpmsolver++")


def _sched(kind, n):
    from insv2v.schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
    if kind == "ddim":
        s = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False)
    elif kind == "ddpm":
        s = DDPMScheduler(clip_sample=False)
    else:
        s = DPMSolverMultistepScheduler(algorithm_type=kind)
    s.set_timesteps(n)
    return s


@pytest.mark.parametrize("n", [4, 10, 20, 50])
@pytest.mark.parametrize("kind", KINDS)
def test_known_coefficients_vs_float64_alphas_cumprod(kind, n):
    """(sqrt(a_prev), sqrt(1 - a_prev)) at every step of the grid, rounded once to fp32 from float64; the last step's end point is
    alphas_cumprod[0] for DDIM / DPM-Solver++ and exactly (1, 0) for DDPM.  coefficients() keeps its keys."""
    s = _sched(kind, n)
    ac = s.alphas_cumprod.double().numpy()
    ts = s.timesteps.tolist()
    assert ts == kr.timesteps(kind, n)
    for t in ts:
        prev = t - 1000 // n
        a = float(ac[prev]) if prev >= 0 else (1.0 if kind == "ddpm" else float(ac[0]))
        k_src, k_noise = s.known_coefficients(t)
        assert isinstance(k_src, float) and isinstance(k_noise, float)
        assert k_src == float(np.float32(math.sqrt(a))) and k_noise == float(np.float32(math.sqrt(1.0 - a)))
        assert (k_src, k_noise) == tuple(float(np.float32(v)) for v in kr.known_coefficients(kind, n, t))
        co = s.coefficients(t)
        assert set(co) == ({"sqrt_a", "sqrt_1ma", "coef", "c_hist"} if kind.endswith("dpmsolver++") else {"sqrt_a", "sqrt_1ma", "coef"})
    last = s.known_coefficients(ts[-1])
    if kind == "ddpm":
        assert last == (1.0, 0.0)
    else:
        assert last == (float(np.float32(math.sqrt(ac[0]))), float(np.float32(math.sqrt(1 - ac[0])))) and last[1] > 0
    # a deterministic first-order step with eps = n and x0 = z lands exactly on the known latent: the blend is consistent with DDIM
    if kind == "ddim":
        for t in ts:
            co = s.coefficients(t)
            k = s.known_coefficients(t)
            assert abs(co["coef"][0] - k[0]) <= 1e-7 and abs(co["coef"][1] - k[1]) <= 1e-7


def test_strength_table():
    from insv2v.schedulers import strength_to_start
    want = {(10, 0.05): (1, 9), (10, 0.5): (5, 5), (10, 0.99): (10, 0), (10, 1.0): (10, 0),
            (20, 0.05): (1, 19), (20, 0.5): (10, 10), (20, 0.99): (20, 0), (20, 1.0): (20, 0),
            (50, 0.05): (3, 47), (50, 0.5): (25, 25), (50, 0.99): (50, 0), (50, 1.0): (50, 0)}
    for (steps, s), w in want.items():
        assert strength_to_start(s, steps) == w == kr.strength_plan(steps, s), (steps, s)
    for steps in (1, 4, 10, 20, 50):
        for s in np.linspace(0.001, 1.0, 97):
            n_exec, st = strength_to_start(float(s), steps)
            assert 1 <= n_exec <= steps and st == steps - n_exec and (n_exec, st) == kr.strength_plan(steps, float(s))
    for bad in (0.0, -0.1, 1.0001, 2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="strength"):
            strength_to_start(bad, 10)


def test_driver_refuses_bad_strength_and_malformed_masks_before_anything_runs():
    from insv2v.run_loveu_tgve import check_edit_args, edit_video, edit_videos
    shape = (1, 10, 3, 32, 48)
    frames = torch.zeros(shape)
    ok = torch.ones((1, 10, 32, 48))
    check_edit_args(shape, ok, 0.5, "mean")
    check_edit_args(shape, torch.ones((1, 1, 32, 48)), 1.0, "max")
    check_edit_args(shape, None, 1.0, "max")
    for bad in (0.0, 1.5, -1.0, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            check_edit_args(shape, None, bad, "max")
        with pytest.raises(ValueError, match="strength"):   # model and pipe are never touched
            edit_video(None, None, frames, None, None, strength=bad)
    with pytest.raises(ValueError, match="mask_mode"):
        check_edit_args(shape, ok, 1.0, "median")
    masks = [torch.ones((1, 10, 32, 40)), torch.ones((1, 3, 32, 48)), torch.ones((10, 32, 48)), torch.ones((2, 10, 32, 48)),
             torch.ones((1, 10, 4, 6)), torch.ones((1, 10, 32, 48), dtype=torch.int64), np.ones((1, 10, 32, 48), dtype=np.float32)]
    for m in masks:
        with pytest.raises(ValueError, match="mask"):
            check_edit_args(shape, m, 1.0, "max")
        with pytest.raises(ValueError, match="mask"):
            edit_video(None, None, frames, None, None, mask=m)
        with pytest.raises(ValueError, match="mask"):
            edit_videos(None, None, [dict(frames=frames), dict(frames=frames, mask=m)])
    with pytest.raises(ValueError, match="multiples of 8"):
        check_edit_args((1, 10, 3, 36, 48), torch.ones((1, 10, 36, 48)), 1.0, "max")

    class Pipe:
        num_ddim_steps = 10
    with pytest.raises(ValueError, match="share"):   # a stack shares start_time
        edit_videos(None, Pipe(), [dict(frames=frames, strength=0.5), dict(frames=frames)])


def test_pipelines_refuse_a_malformed_known_region_before_the_first_launch():
    from insv2v.inference import InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow, check_known_region

    class FakeUNet:
        device = torch.device("cpu")
    lat = torch.zeros((1, 3, 4, 5, 7))
    m, z, n = torch.ones((1, 3, 5, 7)), torch.zeros_like(lat), torch.zeros_like(lat)
    check_known_region(lat, m, z, n)
    check_known_region(lat)
    bad = [dict(mask=m), dict(mask=m, source_latent=z), dict(mask=m, known_noise=n), dict(source_latent=z), dict(known_noise=n),
           dict(mask=m[0], source_latent=z, known_noise=n), dict(mask=torch.ones((1, 3, 4, 5, 7)), source_latent=z, known_noise=n),
           dict(mask=torch.ones((1, 3, 5, 8)), source_latent=z, known_noise=n), dict(mask=m, source_latent=z[:, :2], known_noise=n),
           dict(mask=m, source_latent=z, known_noise=n[0])]
    for cls in (InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow):
        p = cls(FakeUNet(), scheduler="ddim", num_ddim_steps=4)   # a UNet without a forward: any launch attempt would raise AttributeError
        for kw in bad:
            with pytest.raises(ValueError):
                p(lat, None, None, lat, **kw)
            with pytest.raises(ValueError):
                p.second_clip_forward(lat, None, None, lat, latent_ref=lat[:, :1], **kw)
            call = dict(latent=lat, text_cond=None, text_uncond=None, img_cond=lat, **kw)
            with pytest.raises(ValueError):
                p.run_stacked([dict(latent=lat, text_cond=None, text_uncond=None, img_cond=lat), call])
            with pytest.raises(ValueError):
                p.run_concurrent([call])
        lat2 = torch.zeros((2, 3, 4, 5, 7))
        with pytest.raises(ValueError):   # a batched call checks the whole batch's shapes
            p(lat2, None, None, lat2, mask=m, source_latent=torch.zeros_like(lat2), known_noise=torch.zeros_like(lat2))
    for fn in (InferenceIP2PVideo.__call__, InferenceIP2PVideo.second_clip_forward, InferenceIP2PVideoOpticalFlow.second_clip_forward):
        par = inspect.signature(fn).parameters
        assert all(par[k].default is None for k in ("mask", "source_latent", "known_noise"))


def _eps_model(x, t):
    return torch.tanh(x) * 0.7 + 0.1 + 1e-4 * t


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_limits(kind):
    """m == 1 everywhere: the masked trajectory IS the unmasked one (multistep_ref's RefScheduler; for DDPM this file's float64 step),
    bit for bit.  m == 0 everywhere: the final latent is k_src z + k_noise n of the LAST step, whatever the model predicted - and the x0
    predictions are still the model's own."""
    g = torch.Generator().manual_seed(3)
    n_steps = 10
    shape = (3, 4, 5, 7)
    z, noise = torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)
    var = [torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(n_steps)] if kind in ("ddpm", "sde-dpmsolver++") else None
    ones, zeros = torch.ones((3, 5, 7), dtype=torch.float64), torch.zeros((3, 5, 7), dtype=torch.float64)
    for strength in (1.0, 0.5):
        got, x0s = kr.trajectory(kind, n_steps, _eps_model, z, noise, ones, strength, var)
        # the unmasked trajectory, stepped by the underlying sampler directly
        ref = kr.inner_scheduler(kind, n_steps)
        st, x = kr.start_latent(kind, n_steps, strength, z, noise)
        assert st == (0 if strength == 1.0 else 5)
        for i, t in enumerate(ref.timesteps.tolist()[st:]):
            x, x0 = ref.step64(_eps_model(x, t), t, x, None if var is None else var[i])
            assert torch.equal(x0, x0s[i])
        assert torch.equal(got, x) and len(x0s) == n_steps - st
        if kind != "ddpm":
            assert isinstance(ref, mr.RefScheduler)
        kept, kx0 = kr.trajectory(kind, n_steps, _eps_model, z, noise, zeros, strength, var)
        k_src, k_noise = kr.known_coefficients(kind, n_steps, kr.timesteps(kind, n_steps)[-1])
        assert torch.equal(kept, k_src * z + k_noise * noise)
        assert (kx0[-1] - z).abs().max() > 1e-3      # the model's prediction, not the source
        kept2, _ = kr.trajectory(kind, n_steps, lambda x, t: -_eps_model(x, t), z, noise, zeros, strength, var)
        assert torch.equal(kept2, kept)
    if kind == "ddpm":
        assert kr.known_coefficients(kind, n_steps, 0) == (1.0, 0.0) and torch.equal(kept, z)
    # a half mask: kept where m == 0, the free trajectory's value nowhere (the kept half feeds back through the model only via x)
    half = zeros.clone()
    half[:, :, 4:] = 1.0
    mixed, _ = kr.trajectory(kind, n_steps, _eps_model, z, noise, half, 1.0, var)
    assert torch.equal(mixed[..., :4], (k_src * z + k_noise * noise)[..., :4])
    assert torch.equal(mixed[..., 4:], kr.trajectory(kind, n_steps, _eps_model, z, noise, ones, 1.0, var)[0][..., 4:])   # eps is pointwise here


def _c_struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(void|float|int64_t|int32_t)\s*(\*?)\s*(.*)", decl)
        ctype = "p" if m.group(3) else {"float": "f", "int64_t": "q", "int32_t": "i"}[m.group(2)]
        fields += [(v.strip(), ctype) for v in m.group(4).split(",")]
    return fields


def test_header_and_ctypes_agree_and_abi_is_15(tmp_path):
    from insv2v import _lib
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    for proto in (r"int insv2v_cfg_step_mask\(const insv2v_maskstep_desc\* d, insv2v_stream_t stream\);",
                  r"int insv2v_mask_to_latent\(const float\* mask, float\* out, int32_t N, int32_t H, int32_t W, int32_t mode, insv2v_stream_t stream\);",
                  r"int insv2v_composite\(const float\* edited, const float\* original, const float\* mask, float\* out, int32_t N, int32_t H, int32_t W,\s*insv2v_stream_t stream\);",
                  r"int insv2v_add_noise\(const float\* z, const float\* noise, float\* out, int64_t n, float ka, float kb, insv2v_stream_t stream\);"):
        assert re.search("^" + proto, header, flags=re.M), proto
    i32, i64, f32, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert _lib.SIGNATURES["insv2v_cfg_step_mask"] == (i32, [ctypes.POINTER(_lib.MaskStepDesc), p])
    assert _lib.SIGNATURES["insv2v_mask_to_latent"] == (i32, [p, p, i32, i32, i32, i32, p])
    assert _lib.SIGNATURES["insv2v_composite"] == (i32, [p, p, p, p, i32, i32, i32, p])
    assert _lib.SIGNATURES["insv2v_add_noise"] == (i32, [p, p, p, i64, f32, f32, p])
    # ABI 15 and the version function's text are pinned: these are additions
    assert _lib.ABI_VERSION == 15
    src = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"insv2v_abi_version\(void\) \{ return 15; \}", src)
    assert "insv2v_maskstep_desc must begin with the fields of insv2v_mstep_desc" in src   # the static_assert
    # the descriptor: insv2v_mstep_desc's fields in their order, then the known region
    kind = {p: "p", i64: "q", i32: "i", f32: "f"}
    tail = [("mask", "p"), ("src", "p"), ("known_noise", "p"), ("k_src", "f"), ("k_noise", "f")]
    py = [(n, kind[t]) for n, t in _lib.MaskStepDesc._fields_]
    assert py == [(n, kind[t]) for n, t in _lib.MStepDesc._fields_] + tail
    assert _c_struct_fields(header, "insv2v_maskstep_desc") == py
    assert _c_struct_fields(header, "insv2v_maskstep_desc")[:-5] == _c_struct_fields(header, "insv2v_mstep_desc")
    # the C compiler's layout of the three step descriptors == ctypes' (a host-only program against the header)
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc is not None, "no host C compiler to check the descriptor layout with"
    names = [n for n, _ in _lib.MaskStepDesc._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "insv2v_hip.h"', 'int main(void) {',
            '  printf("%zu %zu %zu\\n", sizeof(insv2v_step_desc), sizeof(insv2v_mstep_desc), sizeof(insv2v_maskstep_desc));']
    prog += [f'  printf("{n} %zu\\n", offsetof(insv2v_maskstep_desc, {n}));' for n in names]
    prog += [f'  printf("ms.{n} %zu\\n", offsetof(insv2v_mstep_desc, {n}));' for n, _ in _lib.MStepDesc._fields_]
    prog += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(prog))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [ctypes.sizeof(_lib.StepDesc), ctypes.sizeof(_lib.MStepDesc), ctypes.sizeof(_lib.MaskStepDesc)]
    offs = dict(line.split() for line in out[1:] if line)
    for n in names:
        assert int(offs[n]) == getattr(_lib.MaskStepDesc, n).offset, n
    for n, _ in _lib.MStepDesc._fields_:
        assert int(offs["ms." + n]) == getattr(_lib.MStepDesc, n).offset == getattr(_lib.MaskStepDesc, n).offset, n
    assert getattr(_lib.MaskStepDesc, "mask").offset == ctypes.sizeof(_lib.MStepDesc)


def test_ops_and_driver_keywords():
    from insv2v import ops, rng
    from insv2v.run_loveu_tgve import edit_video
    par = inspect.signature(ops.cfg_step).parameters
    assert [par[k].default for k in ("mask", "src", "known_noise", "k_src", "k_noise")] == [None, None, None, 0.0, 0.0]
    for name in ("mask_to_latent", "composite", "add_noise", "cfg_step_mask"):
        assert callable(getattr(ops, name))
    par = inspect.signature(edit_video).parameters
    assert (par["mask"].default, par["strength"].default, par["mask_mode"].default) == (None, 1.0, "max")
    assert (rng.ENC, rng.INIT, rng.STEP) == (0, 1, 2) and not hasattr(rng, "KNOWN")   # no new noise stream: n is the window's initial noise
    with pytest.raises(ValueError, match="mode"):
        ops.mask_to_latent(torch.zeros((1, 8, 8)), mode="median")


def test_cli():
    from insv2v.run_loveu_tgve import build_parser, check_args, synthetic_mask
    p = build_parser()
    a = check_args(p.parse_args([]))
    assert a.strength == 1.0 and a.mask_mode == "max" and a.synthetic_mask is False
    a = check_args(p.parse_args(["--strength", "0.35", "--mask-mode", "mean", "--synthetic", "2", "--synthetic-mask"]))
    assert a.strength == 0.35 and a.mask_mode == "mean" and a.synthetic_mask is True
    for bad in ("0", "0.0", "-0.5", "1.01", "nan"):
        with pytest.raises(SystemExit, match="--strength"):
            check_args(p.parse_args(["--strength", bad]))
    with pytest.raises(SystemExit, match="--mask-mode"):
        check_args(p.parse_args(["--mask-mode", "median"]))
    with pytest.raises(SystemExit, match="--synthetic-mask"):
        check_args(p.parse_args(["--synthetic-mask"]))
    m = synthetic_mask(2, 32, 48)
    assert m.shape == (2, 1, 32, 48) and m.dtype == torch.float32 and set(m.unique().tolist()) == {0.0, 1.0}
    assert m[0, 0, 8:24, 12:36].min() == 1.0 and m.sum() == 2 * 16 * 24
    assert torch.equal(m, m.flip(-1)) and torch.equal(m, m.flip(-2))   # centred


def test_mask_entries_refuse_bad_arguments_before_any_launch():
    """The argument checks run on the host in front of the launch, so they are testable without a GPU: the addresses below are never
    dereferenced."""
    from insv2v import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build
        build.build(verbose=False)
    lib = _lib.load()
    n = 3 * 4 * 5 * 7 * 4   # bytes of one [F,4,h,w] fp32 tensor

    def desc(**kw):
        d = _lib.MaskStepDesc()
        d.eps_in, d.latent, d.latent_out, d.pred_x0, d.eps_out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        d.nbranch, d.F, d.h, d.w = 3, 3, 5, 7
        d.sqrt_a, d.sqrt_1ma, d.c_x0, d.c_xt = 0.8, 0.6, 0.5, 0.5
        d.x0_hist, d.c_hist = 0x60000, 0.25
        d.mask, d.src, d.known_noise, d.k_src, d.k_noise = 0x70000, 0x80000, 0x90000, 0.9, 0.4
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)

    f = lib.insv2v_cfg_step_mask
    assert f(None, None) == -1
    assert f(desc(src=None), None) == -1 and f(desc(known_noise=None), None) == -1      # a mask without its source / noise
    assert f(desc(latent_out=None), None) == -1                                          # a mask blends latent_out: it must exist
    for k in ("F", "h", "w"):
        assert f(desc(**{k: 0}), None) == -1 and f(desc(**{k: -3}), None) == -1
    for out in (0x30000, 0x40000, 0x50000):                                              # read while the outputs are written
        for name, size in (("mask", n // 4), ("src", n), ("known_noise", n), ("x0_hist", n)):
            assert f(desc(**{name: out}), None) == -1, (name, hex(out))
            assert f(desc(**{name: out + n - 4}), None) == -1
            assert f(desc(**{name: out - size + 4}), None) == -1
    assert f(desc(x0_hist=None), None) == -1                                             # the checks shared with insv2v_cfg_step_ms / _step
    assert f(desc(noise=0xa0000, noise_on=1, c_noise=0.5), None) == -1
    assert f(desc(nbranch=2), None) == -1 and f(desc(correct=1), None) == -1
    # without a mask the call is insv2v_cfg_step_ms: its refusals, src / known_noise ignored
    assert f(desc(mask=None, x0_hist=None), None) == -1 and f(desc(mask=None, F=0), None) == -1
    assert f(desc(mask=None, x0_hist=0x30000), None) == -1
    g = lib.insv2v_mask_to_latent
    assert g(None, 0x1000, 1, 8, 8, 0, None) == -1 and g(0x1000, None, 1, 8, 8, 0, None) == -1
    for N, H, W, mode in ((0, 8, 8, 0), (1, 0, 8, 0), (1, 8, 0, 1), (1, 12, 8, 0), (1, 8, 20, 1), (1, 8, 8, 2), (1, 8, 8, -1), (-1, 8, 8, 0)):
        assert g(0x1000, 0x2000, N, H, W, mode, None) == -1, (N, H, W, mode)
    c = lib.insv2v_composite
    for args in ((None, 0x2000, 0x3000, 0x4000, 1, 8, 8), (0x1000, None, 0x3000, 0x4000, 1, 8, 8), (0x1000, 0x2000, None, 0x4000, 1, 8, 8),
                 (0x1000, 0x2000, 0x3000, None, 1, 8, 8), (0x1000, 0x2000, 0x3000, 0x4000, 0, 8, 8), (0x1000, 0x2000, 0x3000, 0x4000, 1, 0, 8),
                 (0x1000, 0x2000, 0x3000, 0x4000, 1, 8, -8)):
        assert c(*args, None) == -1, args
    a = lib.insv2v_add_noise
    assert a(None, 0x2000, 0x3000, 4, 1.0, 1.0, None) == -1 and a(0x1000, None, 0x3000, 4, 1.0, 1.0, None) == -1
    assert a(0x1000, 0x2000, None, 4, 1.0, 1.0, None) == -1 and a(0x1000, 0x2000, 0x3000, -1, 1.0, 1.0, None) == -1
    assert a(0x1000, 0x2000, 0x3000, 0, 1.0, 1.0, None) == 0   # nothing to do, nothing launched
