"""Per-pixel edit strength on the host: the release map against ``schedulers.strength_to_start``, the float64
restatement's limiting cases (tests/strength_map_ref.py), the misreadings the GPU file's inputs must tell from the definition, the
interfaces the feature adds (C header, ctypes mirror and descriptor layout, keywords, CLI) and every refusal, before anything runs."""
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
import strength_map_ref as sr
from conftest import ROOT
from driver_fakes import Model, RecordingPipe
from test_region_cpu import fake_ops, _source, _rect   # noqa: F401  (fake_ops: the fixture that stands in for the three region kernels)


# ------------------------------------------------------------------------------------------------ release_plan / strength_to_start
def _double_rule(s, steps):
    """The rule as the kernel forms it, restated: fp32 strength -> double, one multiply, one add, floor, the two clamps."""
    s = np.float32(s)
    if not s > 0:
        return 0
    return int(min(float(steps), max(1.0, math.floor(float(s) * float(steps) + 0.5))))


@pytest.mark.parametrize("steps", list(range(1, 101)) + [250, 1000])
def test_release_plan_is_strength_to_start_per_cell(steps):
    from insv2v.schedulers import strength_to_start
    exact = np.asarray([k / steps for k in range(1, steps + 1)], dtype=np.float64).astype(np.float32)   # every s = k / steps, as fp32
    rnd = np.random.default_rng(1000 + steps).random(100000, dtype=np.float32)
    rnd = rnd[rnd > 0]
    for s in (exact, rnd):
        rel = sr.release_of_cells(s, steps)
        assert rel.dtype == np.int32 and rel.min() >= 0 and rel.max() <= steps - 1
        want = np.asarray([strength_to_start(float(v), steps)[1] for v in s], dtype=np.int32)
        assert np.array_equal(rel, want), f"{steps} steps: {int((rel != want).sum())} of {s.size} strengths differ from strength_to_start"
        assert np.array_equal(steps - rel, np.asarray([_double_rule(v, steps) for v in s], dtype=np.int32))
    for k in range(1, steps + 1):   # s = k / steps executes k steps (the nearest fp32 of k / steps is within the rounding's half step)
        assert steps - int(sr.release_of_cells(np.float32(k / steps), steps)) == k
    special = sr.release_of_cells(np.asarray([0.0, -0.0, np.nan, 1.0], dtype=np.float32), steps)
    assert special.tolist() == [steps, steps, steps, 0]


def test_release_plan_reduces_cells_like_mask_to_latent_states_it():
    """The fp32 pairwise tree against the float64 mean of tests/test_masked_gpu.py's ``_np_reduce`` (6.1 * 2^-24, its derivation), the
    maximum exactly; a whole image goes through cell_values -> n_exec."""
    S, _ = sr.smap_case(2, 24, 40, 20)
    ok = np.nan_to_num(S, nan=0.25)
    cells = ok.reshape(2, 3, 8, 5, 8)
    assert np.array_equal(sr.cell_values(ok, "max"), cells.max(axis=(2, 4)))
    assert np.abs(sr.cell_values(ok, "mean").astype(np.float64) - cells.astype(np.float64).mean(axis=(2, 4))).max() <= 6.1 * 2.0 ** -24
    for mode in ("mean", "max"):
        rel = sr.release_plan(S, 20, mode)
        assert rel.shape == (2, 3, 5) and rel.dtype == np.int32 and np.array_equal(rel, sr.release_of_cells(sr.cell_values(S, mode), 20))
        assert np.isnan(sr.cell_values(S, mode)).sum() == 1 and (rel[np.isnan(sr.cell_values(S, mode))] == 20).all()   # the cell of NaNs is never released


# ------------------------------------------------------------------------------------------------ float64 limits of the trajectory
def _traj_inputs(n_steps, kind):
    g = torch.Generator().manual_seed(5)
    shape = (3, 4, 5, 7)
    z, noise = torch.randn(shape, generator=g, dtype=torch.float64), torch.randn(shape, generator=g, dtype=torch.float64)
    var = [torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(n_steps)] if kind in ("ddpm", "sde-dpmsolver++") else None
    mask = (torch.rand((3, 5, 7), generator=g, dtype=torch.float64) * 2 - 0.5).clamp(0, 1)
    return z, noise, var, mask


@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpmsolver++", "sde-dpmsolver++"])
def test_restatement_limits(kind):
    n = 10
    z, noise, var, mask = _traj_inputs(n, kind)
    zeros, full = np.zeros((3, 5, 7), dtype=np.int32), np.full((3, 5, 7), n, dtype=np.int32)
    for strength in (1.0, 0.5):
        # release == 0 everywhere: the masked trajectory, bit for bit - with a mask, and without one the unmasked one (m = 1)
        got, x0s = sr.trajectory(kind, n, sr.eps_model, z, noise, mask, zeros, strength, var)
        want, wx0 = kr.trajectory(kind, n, sr.eps_model, z, noise, mask, strength, var)
        assert torch.equal(got, want) and all(torch.equal(a, b) for a, b in zip(x0s, wx0))
        got, _ = sr.trajectory(kind, n, sr.eps_model, z, noise, None, zeros, strength, var)
        assert torch.equal(got, kr.trajectory(kind, n, sr.eps_model, z, noise, torch.ones((3, 5, 7), dtype=torch.float64), strength, var)[0])
        # release == steps everywhere: held through the last step - `known` of the last step, whatever the model and the mask say
        kept, kx0 = sr.trajectory(kind, n, sr.eps_model, z, noise, mask, full, strength, var)
        k_src, k_noise = kr.known_coefficients(kind, n, kr.timesteps(kind, n)[-1])
        assert torch.equal(kept, k_src * z + k_noise * noise) and (kx0[-1] - z).abs().max() > 1e-3
        assert torch.equal(kept, sr.trajectory(kind, n, lambda x, t: -sr.eps_model(x, t), z, noise, None, full, strength, var)[0])


@pytest.mark.parametrize("r", [1, 4, 9])
@pytest.mark.parametrize("kind", ["ddim", "ddpm", "dpmsolver++"])
def test_constant_release_is_strength(kind, r):
    """release == r everywhere, no mask, is ``strength = s`` with n_exec(s) = steps - r, from step r on.  Why: a held cell leaves step
    r - 1 as k_src z + k_noise n at the level that step's OUTPUT lives at, a_prev(t_{r-1}) - and on the 'leading' grid that is a(t_r), the
    level ``strength=`` noises the source to before its first executed step t_r (masked_ref.start_latent).  So both enter step r with
    the same latent, to the last bit here.

    DDIM and DDPM (the variance noises aligned: executed step i of the partial edit takes the noise of global step r + i) are one-step
    samplers, so from there on the trajectories are the same, within 1e-12.  DPM-Solver++ 2M is not: the released trajectory has kept
    sampling through the held steps, so at step r it owns a history (the model's x0 at the held latent of step r - 1) and takes a
    SECOND-order step where ``strength=`` starts at first order.  For it the equality within 1e-12 is with the strength trajectory whose
    sampler was handed that history; against the plain one the latent entering step r is still equal, and the rest differs by the 2M
    correction term (a figure is printed).  DESIGN.md section 28 states this."""
    n = 10
    z, noise, var, _ = _traj_inputs(n, kind)
    rel = np.full((3, 5, 7), r, dtype=np.int32)
    s = (n - r) / n
    assert kr.strength_plan(n, s) == (n - r, r)
    got, x0s, xs = sr.trajectory(kind, n, sr.eps_model, z, noise, None, rel, 1.0, var, all_latents=True)
    st, start = kr.start_latent(kind, n, s, z, noise)
    assert st == r and (xs[r - 1] - start).abs().max() <= 1e-12, "the latent entering step r is not strength's start latent"
    ts = kr.timesteps(kind, n)
    k_src, k_noise = kr.known_coefficients(kind, n, ts[r - 1])
    a_r = float(kr.mr.alphas_cumprod().double()[ts[r]])
    assert abs(k_src - math.sqrt(a_r)) <= 1e-15 and abs(k_noise - math.sqrt(1 - a_r)) <= 1e-15   # known's level after step r - 1 is a(t_r)
    want, wx0 = kr.trajectory(kind, n, sr.eps_model, z, noise, None, s, None if var is None else var[r:])
    if kind != "dpmsolver++":
        assert (got - want).abs().max() <= 1e-12
        assert all((a - b).abs().max() <= 1e-12 for a, b in zip(x0s[r:], wx0))
        return
    print(f"[strength_map] dpmsolver++ 2M, release == {r}: max |released - plain strength trajectory| = {(got - want).abs().max():.3e} (the 2M term of step {r})")
    ref = kr.inner_scheduler(kind, n)
    ref.x0_last, ref.t_last = x0s[r - 1], ts[r - 1]   # the history the released trajectory owns when step r starts
    x = start
    for i, t in enumerate(ts[r:]):
        x, x0 = ref.step64(sr.eps_model(x, t), t, x)
        assert (x0 - x0s[r + i]).abs().max() <= 1e-12 and (x - xs[r + i]).abs().max() <= 1e-12
    assert (x - got).abs().max() <= 1e-12


# ------------------------------------------------------------------------------------------------ planted misreadings
CASES = [(nb, c, h) for nb in (3, 0) for c in (0, 1, 2) for h in (True, False)]


def test_the_step_inputs_tell_every_misreading_from_the_definition():
    """On the operands the GPU file launches (``step_case``), at the steps it launches: every planted misreading of the gate moves an
    output by far more than the GPU file's bound (1e-5 of max|ref|), in every case - so a kernel that had it could not pass there."""
    rel = sr.step_release()
    assert sorted(rel.unique().tolist()) == list(sr.RELEASE_VALUES) and not torch.equal(rel[0], rel[1]) and not torch.equal(rel[1], rel[2])
    for nbranch, correct, hist in CASES:
        o = sr.step_case(nbranch, 1)
        c_hist = sr.f32(-0.37) if hist else 0.0
        seen = {m: 0.0 for m in sr.MISREADINGS}
        for step in sr.STEPS_LAUNCHED:
            kw = dict(nbranch=nbranch, correct=correct, c_hist=c_hist, noise=o["noise"], step=step)
            e, x0, out = sr.step64(o, **kw)
            # the definition itself: the masked blend under the explicit mask where(release <= step, m, 0)
            m_eff = torch.where(rel <= step, o["mask"].double(), torch.zeros(()).double())
            plain = sr.step64(dict(o, release=torch.zeros_like(rel)), **kw)
            assert torch.equal(out, kr.blend(_prev_of(o, kw), o["src"].double(), o["kn"].double(), m_eff, sr.KS, sr.KN))
            assert torch.equal(x0, plain[1]) and torch.equal(e, plain[0])   # pred_x0 / eps_out are the model's own
            for mis in sr.MISREADINGS:
                bad = sr.step64(o, misreading=mis, **kw)
                seen[mis] = max(seen[mis], max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(bad[1:], (x0, out))))
        for mis, d in seen.items():
            assert d > 1e-2, f"nbranch={nbranch} correct={correct} hist={hist}: the misreading {mis!r} moves the outputs by {d:.1e} only"
    # '<' for '<=' shows exactly at the steps that equal a release value
    o = sr.step_case(3, 1)
    for step in sr.STEPS_LAUNCHED:
        kw = dict(nbranch=3, correct=0, c_hist=0.0, noise=None, step=step)
        assert torch.equal(sr.step64(o, misreading="lt", **kw)[2], sr.step64(o, **kw)[2]) == (step not in sr.RELEASE_VALUES)


def _prev_of(o, kw):
    """The update in front of the blend: the step with a mask of ones and everything released."""
    free = dict(o, release=torch.zeros_like(o["release"]))
    return sr.step64(free, masked=False, **kw)[2]


def test_the_start_time_case_tells_the_local_index_from_the_global_one():
    """START_TIME_CASE (the GPU file's run with start_time > 0): counting the executed steps instead of the global index releases the
    middle level three steps late - far outside the trajectory bound (rel-RMS 3e-2); with start_time = 0 the two cannot be told apart."""
    c = sr.START_TIME_CASE
    n, st = c["steps"], c["start_time"]
    assert st < c["mid"] < n
    rel = sr.pipe_release(8, 16, 24, n, c["mid"])[0].numpy()
    assert sorted(np.unique(rel).tolist()) == [0, c["mid"], n]
    g = torch.Generator().manual_seed(9)
    z, noise = torch.randn((8, 4, 16, 24), generator=g, dtype=torch.float64), torch.randn((8, 4, 16, 24), generator=g, dtype=torch.float64)
    s = (n - st) / n
    for kind in ("ddim", "dpmsolver++"):
        good, _ = sr.trajectory(kind, n, sr.eps_model, z, noise, None, rel, s)
        bad, _ = sr.trajectory(kind, n, sr.eps_model, z, noise, None, rel, s, local_index=True)
        mid = torch.from_numpy(rel == c["mid"])[:, None].expand_as(good)
        print(f"[strength_map] {kind}, local index for the global one: rel-rms {sr.rel_rms(bad, good):.3e} (the cells of the middle level {sr.rel_rms(bad[mid], good[mid]):.3e})")
        assert sr.rel_rms(bad, good) > 1e-1 and torch.equal(bad[~mid], good[~mid])
        same = sr.trajectory(kind, n, sr.eps_model, z, noise, None, rel, 1.0, local_index=True)[0]
        assert torch.equal(same, sr.trajectory(kind, n, sr.eps_model, z, noise, None, rel, 1.0)[0])


@pytest.mark.parametrize("steps", [1, 3, 20])
@pytest.mark.parametrize("N,HH,WW", [(2, 24, 40), (1, 8, 8)])
def test_the_strength_images_tell_the_two_quantisation_misreadings(N, HH, WW, steps):
    """``smap_case`` (the GPU file's images): n_exec without the max(1, .) and G taken per cell each change entries of the 30-cell image, in both modes."""
    S, M = sr.smap_case(N, HH, WW, steps)
    big = N > 1
    if big:   # every kind of value is there
        flat = S.reshape(-1)
        assert np.isnan(flat).any() and (flat == 1.0).any() and (np.signbit(flat) & (flat == 0)).any() and ((flat == 0) & ~np.signbit(flat)).any()
        for k in sorted({0, steps // 2, steps - 1}):
            tie = np.float32((k + 0.5) / steps)
            for v in (np.nextafter(tie, np.float32(0), dtype=np.float32), tie, np.nextafter(tie, np.float32(2), dtype=np.float32), np.float32((k + 1) / steps)):
                assert (flat == v).sum() >= 64, (steps, k, v)
    for mode in ("mean", "max"):
        rel = sr.release_plan(S, steps, mode)
        assert rel.min() >= 0 and rel.max() <= steps
        if not big:   # (the one-cell image is there for the smallest grid; it holds one block only)
            continue
        assert (rel != sr.release_plan(S, steps, mode, clamp_one=False)).any(), "n_exec without max(1, .)"
        for mask in (None, M):
            assert (sr.gate(S, mask) != sr.gate(S, mask, from_cell=mode)).any(), "G from the cell"
    G = sr.gate(S, M)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(G[S > 0], M[S > 0]) and (G[~(S > 0)] == 0).all() and set(np.unique(sr.gate(S)).tolist()) <= {0.0, 1.0}


# ------------------------------------------------------------------------------------------------ interfaces
def _c_struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(void|float|int64_t|int32_t)\s*(\*?)\s*(.*)", decl)
        ctype = "p" if m.group(3) else {"float": "f", "int64_t": "q", "int32_t": "i"}[m.group(2)]
        fields += [(v.strip(), ctype) for v in m.group(4).split(",")]
    return fields


def test_header_ctypes_and_a_host_c_program_agree_on_the_descriptor(tmp_path):
    from insv2v import _lib
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    for proto in (r"int insv2v_cfg_step_release\(const insv2v_relstep_desc\* d, insv2v_stream_t stream\);",
                  r"int insv2v_strength_release\(const float\* smap, const float\* mask_img, int32_t\* release, float\* gate, int32_t N, int32_t H, int32_t W,\s*"
                  r"int32_t mode, int32_t steps, insv2v_stream_t stream\);"):
        assert re.search("^" + proto, header, flags=re.M), proto
    i32, i64, f32, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    assert _lib.SIGNATURES["insv2v_cfg_step_release"] == (i32, [ctypes.POINTER(_lib.RelStepDesc), p])
    assert _lib.SIGNATURES["insv2v_strength_release"] == (i32, [p, p, p, p, i32, i32, i32, i32, i32, p])
    assert _lib.ABI_VERSION == 15   # additions
    src = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"insv2v_abi_version\(void\) \{ return 15; \}", src)
    assert "insv2v_relstep_desc must begin with the fields of insv2v_maskstep_desc" in src   # the static_assert
    assert len(re.findall(r"mask_cell_value\(", src)) == 3, "the cell reduction is one device function, called by both kernels"
    kind = {p: "p", i64: "q", i32: "i", f32: "f"}
    py = [(n, kind[t]) for n, t in _lib.RelStepDesc._fields_]
    assert py == [(n, kind[t]) for n, t in _lib.MaskStepDesc._fields_] + [("release", "p"), ("step", "i")]
    assert _c_struct_fields(header, "insv2v_relstep_desc") == py
    assert _c_struct_fields(header, "insv2v_relstep_desc")[:-2] == _c_struct_fields(header, "insv2v_maskstep_desc")
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc is not None, "no host C compiler to check the descriptor layout with"
    names = [n for n, _ in _lib.RelStepDesc._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "insv2v_hip.h"', 'int main(void) {',
            '  printf("%zu %zu\\n", sizeof(insv2v_maskstep_desc), sizeof(insv2v_relstep_desc));']
    prog += [f'  printf("{n} %zu\\n", offsetof(insv2v_relstep_desc, {n}));' for n in names]
    prog += [f'  printf("mk.{n} %zu\\n", offsetof(insv2v_maskstep_desc, {n}));' for n, _ in _lib.MaskStepDesc._fields_]
    prog += ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(prog))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert [int(v) for v in out[0].split()] == [ctypes.sizeof(_lib.MaskStepDesc), ctypes.sizeof(_lib.RelStepDesc)]
    offs = dict(line.split() for line in out[1:] if line)
    for n in names:
        assert int(offs[n]) == getattr(_lib.RelStepDesc, n).offset, n
    for n, _ in _lib.MaskStepDesc._fields_:
        assert int(offs["mk." + n]) == getattr(_lib.MaskStepDesc, n).offset == getattr(_lib.RelStepDesc, n).offset, n
    assert _lib.RelStepDesc.release.offset == ctypes.sizeof(_lib.MaskStepDesc)


def test_keywords_and_their_positions():
    from insv2v import ops, inference, region
    from insv2v.run_loveu_tgve import edit_video, check_edit_args, UNIT_KEYS, CHECKED_KEYS, UNIT_DEFAULTS
    par = inspect.signature(ops.cfg_step).parameters
    assert (par["release"].default, par["step"].default) == (None, 0) and list(par)[-2:] == ["release", "step"]
    assert callable(ops.cfg_step_release) and list(inspect.signature(ops.strength_release).parameters) == ["smap", "steps", "mode", "mask"]
    assert inspect.signature(ops.strength_release).parameters["mode"].default == "max"
    names = list(inspect.signature(edit_video).parameters)
    assert names[names.index("mask_shape") + 1] == "strength_map" and inspect.signature(edit_video).parameters["strength_map"].default is None
    assert names[-2:] == ["keyframes", "key_flows"]
    # check_edit_args keeps mask_shape third from last (tests/test_keyfill_cpu.py pins it), so the new parameter stands in front of it;
    # CHECKED_KEYS is check_edit_args' order
    checked = list(inspect.signature(check_edit_args).parameters)
    assert checked[-4:] == ["strength_map", "mask_shape", "keyframes", "key_flows"] and tuple(checked[1:]) == CHECKED_KEYS == UNIT_KEYS[6:]
    assert UNIT_DEFAULTS["strength_map"] is None and inspect.signature(check_edit_args).parameters["strength_map"].default is None
    assert inference._KNOWN_KEYS == ("mask", "source_latent", "known_noise", "release")
    P, Q = inference.InferenceIP2PVideo, inference.InferenceIP2PVideoOpticalFlow
    for fn in (P.__call__, P.second_clip_forward, Q.second_clip_forward, inference.check_known_region):
        assert inspect.signature(fn).parameters["release"].default is None
    assert inspect.signature(P._finish_step).parameters["start_time"].default == 0
    assert callable(region._check_strength_map)


# ------------------------------------------------------------------------------------------------ refusals
SHAPE = (1, 10, 3, 32, 48)


def _bad_maps():
    return [torch.ones((1, 10, 32, 40)), torch.ones((1, 3, 32, 48)), torch.ones((10, 32, 48)), torch.ones((2, 10, 32, 48)), torch.ones((1, 10, 4, 6)),
            torch.ones((1, 10, 32, 48), dtype=torch.int64), torch.ones((1, 10, 32, 48), dtype=torch.bool), np.ones((1, 10, 32, 48), dtype=np.float32),
            "auto", "shaped", 0.5, True]


def test_drivers_refuse_a_bad_strength_map_before_anything_runs():
    from insv2v.run_loveu_tgve import check_edit_args, edit_video, edit_videos
    frames, mask = torch.zeros(SHAPE), torch.ones((1, 1, 32, 48))
    check_edit_args(SHAPE, strength_map=torch.ones((1, 10, 32, 48)))
    check_edit_args(SHAPE, strength_map=torch.ones((1, 1, 32, 48), dtype=torch.float16), mask=mask, mask_shape=dict(feather=4.0))
    check_edit_args(SHAPE, strength_map="mask", mask=mask)
    check_edit_args(SHAPE, strength_map="mask", mask=mask, mask_key=3, mask_shape=dict(feather=4.0), keyframes=2)
    check_edit_args(SHAPE, strength_map=torch.ones((1, 10, 32, 48)), mask="auto")   # a tensor map next to an estimated mask is allowed
    pipe = RecordingPipe()
    for m in _bad_maps():
        with pytest.raises(ValueError, match="strength_map"):
            check_edit_args(SHAPE, strength_map=m, mask=mask)
        with pytest.raises(ValueError, match="strength_map"):   # model and pipe are never touched
            edit_video(None, None, frames, None, None, strength_map=m, mask=mask)
        with pytest.raises(ValueError, match="strength_map"):
            edit_video(Model(), pipe, frames, "tc", "tu", strength_map=m, mask=mask)
        with pytest.raises(ValueError, match="strength_map"):
            edit_videos(Model(), pipe, [dict(frames=frames), dict(frames=frames, strength_map=m, mask=mask)])
    with pytest.raises(ValueError, match="needs a mask|pass mask="):
        check_edit_args(SHAPE, strength_map="mask")
    with pytest.raises(ValueError, match="needs a mask|pass mask="):
        edit_video(Model(), pipe, frames, "tc", "tu", strength_map="mask")
    with pytest.raises(ValueError, match="auto"):
        check_edit_args(SHAPE, strength_map="mask", mask="auto")
    with pytest.raises(ValueError, match="multiples of 8"):
        check_edit_args((1, 10, 3, 36, 48), strength_map=torch.ones((1, 10, 36, 48)))
    with pytest.raises(ValueError, match="multiples of 8"):
        edit_videos(Model(), pipe, [dict(frames=torch.zeros((1, 10, 3, 32, 44)), strength_map=torch.ones((1, 1, 32, 44)))])
    assert pipe.calls == []


def test_pipelines_refuse_a_malformed_release_map_before_the_first_launch():
    from insv2v.inference import InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow, check_known_region

    class FakeUNet:
        device = torch.device("cpu")
    lat = torch.zeros((1, 3, 4, 5, 7))
    m, z, n = torch.ones((1, 3, 5, 7)), torch.zeros_like(lat), torch.zeros_like(lat)
    r = torch.zeros((1, 3, 5, 7), dtype=torch.int32)
    check_known_region(lat, m, z, n, r)
    check_known_region(lat, None, z, n, r)          # a release map without a mask is a known region too
    check_known_region(lat, source_latent=z, known_noise=n, release=r)
    bad = [dict(release=r), dict(release=r, source_latent=z), dict(release=r, known_noise=n), dict(release=r, mask=m), dict(release=r, mask=m, source_latent=z),
           dict(release=r[0], source_latent=z, known_noise=n), dict(release=r.long(), source_latent=z, known_noise=n),
           dict(release=r.float(), source_latent=z, known_noise=n), dict(release=torch.zeros((1, 3, 5, 8), dtype=torch.int32), source_latent=z, known_noise=n),
           dict(release=torch.zeros((1, 3, 4, 5, 7), dtype=torch.int32), source_latent=z, known_noise=n), dict(release=r.numpy(), source_latent=z, known_noise=n),
           dict(release=r, mask=m[:, :2], source_latent=z, known_noise=n), dict(release=r, source_latent=z[:, :2], known_noise=n)]
    for cls in (InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow):
        p = cls(FakeUNet(), scheduler="ddim", num_ddim_steps=4)   # a UNet without a forward: any launch attempt would raise AttributeError
        for kw in bad:
            with pytest.raises(ValueError):
                check_known_region(lat, **kw)
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
            p(lat2, None, None, lat2, release=r, source_latent=torch.zeros_like(lat2), known_noise=torch.zeros_like(lat2))


def test_region_drivers_pass_the_string_through_and_refuse_a_tensor_map(fake_ops, monkeypatch):
    from insv2v import region, run_loveu_tgve
    frames, M = _source("strength_map.region"), _rect(3, 75, 110, (40, 30, 60, 50))
    seen = []

    def fake_edit_video(model, pipe, frames, text_cond, text_uncond, **kw):
        seen.append(kw)
        return frames * 0.5

    def fake_edit_videos(model, pipe, units, **kw):
        seen.extend(units)
        return [u["frames"] * 0.5 for u in units]
    monkeypatch.setattr(run_loveu_tgve, "edit_video", fake_edit_video)
    monkeypatch.setattr(run_loveu_tgve, "edit_videos", fake_edit_videos)
    # the string reaches the inner edit next to the resampled mask (a tracked box takes the same two drivers)
    out = region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32)), mask=M, strength_map="mask")
    assert out.shape == frames.shape and seen[-1]["strength_map"] == "mask" and seen[-1]["mask"].shape == (1, 3, 32, 48)
    region.edit_regions(Model(), RecordingPipe(), [dict(frames=frames, text_cond="tc", text_uncond="tu", region=dict(size=(48, 32)), mask=M, strength_map="mask")])
    assert seen[-1]["strength_map"] == "mask" and seen[-1]["frames"].shape == (1, 3, 3, 32, 48)
    del seen[:]
    for track in (None, dict(boxes=[(5.0, 5.0, 53.0, 37.0)] * 3)):
        for smap in (torch.ones((1, 3, 75, 110)), torch.ones((1, 1, 32, 48))):
            with pytest.raises(ValueError, match="strength_map"):
                region.edit_region(Model(), RecordingPipe(), frames, "tc", "tu", region=dict(size=(48, 32), box="frame"), track=track, strength_map=smap)
            with pytest.raises(ValueError, match="strength_map"):
                region.edit_regions(Model(), RecordingPipe(), [dict(frames=frames, text_cond="tc", text_uncond="tu", region=dict(size=(48, 32), box="frame"),
                                                                    **({} if track is None else {"track": track}), strength_map=smap)])
    assert seen == []


def test_cli(tmp_path):
    from insv2v.run_loveu_tgve import build_parser, check_args, strength_map_unit, load_strength_map
    p = build_parser()
    a = check_args(p.parse_args([]))
    assert a.strength_map is None and a.strength_from_mask is False and strength_map_unit(a, True) == {} and load_strength_map(a, 48, 32) is None
    pt = tmp_path / "map.pt"
    torch.save(torch.full((1, 1, 32, 48), 0.25), pt)
    a = check_args(p.parse_args(["--strength-map", str(pt)]))
    m = load_strength_map(a, 48, 32)
    assert m.shape == (1, 1, 32, 48) and strength_map_unit(a, False, m)["strength_map"] is m
    a = check_args(p.parse_args(["--strength-from-mask", "--synthetic", "1", "--synthetic-mask"]))
    assert strength_map_unit(a, True) == dict(strength_map="mask") and strength_map_unit(a, False) == {}
    with pytest.raises(SystemExit, match="two strength maps"):
        check_args(p.parse_args(["--strength-map", str(pt), "--strength-from-mask", "--synthetic", "1", "--synthetic-mask"]))
    with pytest.raises(SystemExit, match="--strength-from-mask needs a mask"):
        check_args(p.parse_args(["--strength-from-mask"]))
    with pytest.raises(SystemExit, match="--auto-mask"):
        check_args(p.parse_args(["--strength-from-mask", "--auto-mask", "--units", "u.pt"]))
    with pytest.raises(SystemExit, match="neither a file nor a directory"):
        check_args(p.parse_args(["--strength-map", str(tmp_path / "missing.png")]))
    with pytest.raises(SystemExit, match="--region"):
        check_args(p.parse_args(["--strength-map", str(pt), "--region"]))
    torch.save({"not": "a tensor"}, tmp_path / "bad.pt")
    with pytest.raises(SystemExit, match="must hold a tensor"):
        load_strength_map(check_args(p.parse_args(["--strength-map", str(tmp_path / "bad.pt")])), 48, 32)
    try:
        from PIL import Image
    except ImportError:
        return
    Image.fromarray((np.arange(32 * 48, dtype=np.uint32).reshape(32, 48) % 256).astype(np.uint8), mode="L").save(tmp_path / "map.png")
    m = load_strength_map(check_args(p.parse_args(["--strength-map", str(tmp_path / "map.png")])), 48, 32)
    assert m.shape == (1, 1, 32, 48) and m.dtype == torch.float32 and 0.0 <= float(m.min()) and float(m.max()) <= 1.0


def test_entries_refuse_bad_arguments_before_any_launch():
    """The argument checks run on the host in front of the launch, so they are testable without a GPU: the addresses below are never
    dereferenced."""
    from insv2v import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build
        build.build(verbose=False)
    lib = _lib.load()
    n = 3 * 4 * 5 * 7 * 4   # bytes of one [F,4,h,w] fp32 tensor

    def desc(**kw):
        d = _lib.RelStepDesc()
        d.eps_in, d.latent, d.latent_out, d.pred_x0, d.eps_out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        d.nbranch, d.F, d.h, d.w = 3, 3, 5, 7
        d.sqrt_a, d.sqrt_1ma, d.c_x0, d.c_xt = 0.8, 0.6, 0.5, 0.5
        d.x0_hist, d.c_hist = 0x60000, 0.25
        d.mask, d.src, d.known_noise, d.k_src, d.k_noise = 0x70000, 0x80000, 0x90000, 0.9, 0.4
        d.release, d.step = 0xa0000, 2
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)

    f = lib.insv2v_cfg_step_release
    assert f(None, None) == -1
    for mask in ({}, dict(mask=None)):                                                    # with and without a mask next to the release map
        assert f(desc(src=None, **mask), None) == -1 and f(desc(known_noise=None, **mask), None) == -1
        assert f(desc(latent_out=None, **mask), None) == -1
        assert f(desc(step=-1, **mask), None) == -1 and f(desc(step=-2 ** 31, **mask), None) == -1
        for k in ("F", "h", "w"):
            assert f(desc(**{k: 0}, **mask), None) == -1 and f(desc(**{k: -3}, **mask), None) == -1
    for out in (0x30000, 0x40000, 0x50000):                                               # read while the outputs are written
        for name, size in (("release", n // 4), ("mask", n // 4), ("src", n), ("known_noise", n), ("x0_hist", n)):
            assert f(desc(**{name: out}), None) == -1, (name, hex(out))
            assert f(desc(**{name: out + n - 4}), None) == -1
            assert f(desc(**{name: out - size + 4}), None) == -1
    assert f(desc(x0_hist=None), None) == -1                                              # the checks shared with the other step entries
    assert f(desc(noise=0xb0000, noise_on=1, c_noise=0.5), None) == -1
    assert f(desc(nbranch=2), None) == -1 and f(desc(correct=1), None) == -1
    # without a release map the call is insv2v_cfg_step_mask: its refusals, step ignored
    assert f(desc(release=None, src=None), None) == -1 and f(desc(release=None, mask=0x30000), None) == -1
    assert f(desc(release=None, mask=None, x0_hist=None), None) == -1 and f(desc(release=None, mask=None, F=0), None) == -1
    g = lib.insv2v_strength_release
    ok = (0x100000, 0x200000, 0x300000, 0x400000, 2, 24, 40, 1, 20)
    names = ("smap", "mask_img", "release", "gate", "N", "H", "W", "mode", "steps")
    img = 2 * 24 * 40 * 4

    def call(**kw):
        return g(*[kw.get(k, v) for k, v in zip(names, ok)], None)
    assert call(smap=None) == -1 and call(release=None) == -1
    for kw in (dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(H=-8), dict(H=12), dict(W=20), dict(H=7, W=7), dict(mode=2), dict(mode=-1),
               dict(steps=0), dict(steps=-4), dict(steps=2 ** 20 + 1), dict(steps=2 ** 31 - 1)):
        assert call(**kw) == -1, kw
    for src in (0x100000, 0x200000):                                                      # the gate is written while smap / mask_img are read
        for g_at in (src, src + img - 4, src - img + 4):
            assert call(gate=g_at) == -1, (hex(src), hex(g_at))
