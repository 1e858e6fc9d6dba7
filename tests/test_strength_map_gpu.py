"""Per-pixel edit strength on the GPU: insv2v_cfg_step_release against the masked entry under the equivalent
mask (bit for bit) and against the float64 restatement (tests/strength_map_ref.py), insv2v_strength_release against the integer
restatement (exactly), the pipelines' ``release=`` on the tiny UNet against the CPU oracle's loops stepping with the restatement, and the
drivers' ``strength_map=``.

Bounds are the project's: kernel level 1e-5 * max|ref| against float64 (``close``); trajectories ``TRAJ`` (rel-RMS 3e-2 / max 1e-1);
stacked against alone rel-RMS 1e-2 / max 4e-2.  The inputs of the kernel-level tests are ``strength_map_ref``'s, on which
tests/test_strength_map_cpu.py shows that every planted misreading is caught."""
import ctypes

import numpy as np
import pytest
import torch

import masked_ref as kr
import philox_ref
import strength_map_ref as sr
from strength_map_ref import F, H, W, COEF, SA, S1, KS, KN, TC, IC, f32
from test_model_gpu import tiny_unet, _pipe_inputs, report   # noqa: F401  (tiny_unet: the module-scoped fixture, instantiated for this module)
from test_multistep_gpu import close, _stack_calls, _alone, TRAJ
from test_masked_gpu import oracle_unet, tiny_model, _unit, _edit, _image_mask, _known, WIN, T, S, STACKED   # noqa: F401  (two fixtures among them)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ the step kernel
def _operands(nbranch, R):
    return {k: v.to(DEV) for k, v in sr.step_case(nbranch, R).items()}


def _launch(o, *, nbranch, correct, c_hist, fn=None, eps_in=None, **more):
    """One launch through ``fn`` (default ``ops.cfg_step``) -> (latent_out, pred_x0, eps_out); the outputs are prefilled with NaN."""
    from insv2v import ops
    new, pred, eo = (torch.full_like(o["lat"], float("nan")) for _ in range(3))
    kw = dict(nbranch=nbranch, text_cfg=TC, img_cfg=IC, sqrt_a=SA, sqrt_1ma=S1, coef=COEF, latent_out=new, pred_x0=pred, eps_out=eo,
              latent_ref=o["ref"] if correct else None, correct=correct, delta_q=o["dq"] if correct == 2 else None,
              src=o["src"], known_noise=o["kn"], k_src=KS, k_noise=KN)
    if c_hist != 0.0:
        kw.update(x0_hist=o["hist"], c_hist=c_hist)
    kw.update(more)
    (fn or ops.cfg_step)(o["eps_in"] if eps_in is None else eps_in, o["lat"], **kw)
    return new, pred, eo


def _equivalent(o, step, mask=True):
    m = o["mask"] if mask else torch.ones_like(o["mask"])
    return torch.where(o["release"] <= step, m, torch.zeros_like(m)).contiguous()


@pytest.mark.parametrize("hist", [True, False])
@pytest.mark.parametrize("correct", [0, 1, 2])
@pytest.mark.parametrize("nbranch", [3, 0])
def test_cfg_step_release_is_the_mask_form_under_the_equivalent_mask(nbranch, correct, hist):
    """At steps 0, 1, 2 and 4 of a release map with the values 0, 1, 2 and 5: all three outputs are bit for bit those of
    insv2v_cfg_step_mask with the explicit mask where(release <= step, m, 0) - the gate is the only new arithmetic - and within the kernel
    bound of the float64 restatement.  Without a mask next to the release map: bit for bit a mask of ones.  The held cells do not depend
    on what the model predicted."""
    from insv2v import ops
    c_hist = f32(-0.37) if hist else 0.0
    o = _operands(nbranch, 1)
    cpu = sr.step_case(nbranch, 1)
    kw = dict(nbranch=nbranch, correct=correct, c_hist=c_hist, noise=o["noise"])
    other = (o["eps_in"] * -1.7 + 0.3).contiguous()
    for step in sr.STEPS_LAUNCHED:
        tag = f"cfg_step_release nbranch={nbranch} correct={correct} hist={int(hist)} step={step}"
        got = _launch(o, release=o["release"], step=step, mask=o["mask"], **kw)
        want = _launch(o, fn=ops.cfg_step_mask, mask=_equivalent(o, step), **kw)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want)), tag + ": not the mask form under the equivalent mask"
        we, wx0, wprev = sr.step64(cpu, nbranch=nbranch, correct=correct, c_hist=c_hist, noise=cpu["noise"], step=step)
        close(got[2], we, tag + " eps")
        close(got[1], wx0, tag + " x0")
        close(got[0], wprev, tag + " latent")
        nomask = _launch(o, release=o["release"], step=step, mask=None, **kw)
        ones = _launch(o, release=o["release"], step=step, mask=torch.ones_like(o["mask"]), **kw)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(nomask, ones)), tag + ": mask=None is not a mask of ones"
        close(nomask[0], sr.step64(cpu, nbranch=nbranch, correct=correct, c_hist=c_hist, noise=cpu["noise"], step=step, masked=False)[2], tag + " latent, no mask")
        held = (o["release"] > step)[:, None].expand_as(got[0])
        moved = _launch(o, release=o["release"], step=step, mask=o["mask"], eps_in=other, **kw)
        assert held.any() and torch.equal(_bits(got[0][held]), _bits(moved[0][held])) and torch.equal(_bits(got[0][held]), _bits(want[0][held]))
        assert (got[1] - moved[1]).abs().max() > 0.1
        free = ((o["release"] <= step) & (o["mask"] > 0))[:, None].expand_as(got[0])
        assert free.any() and (got[0] - moved[0])[free].abs().max() > 0.1


def test_cfg_step_release_dispatch_without_a_release_map():
    """release=None through the new entry IS insv2v_cfg_step_mask (and, without a mask, what that dispatches to), every noise source."""
    from insv2v import ops
    o = _operands(3, 2)
    for hist in (f32(-0.37), 0.0):
        for src in (dict(noise=o["noise"]), dict(noise_seed=11, noise_stream=5), dict()):
            kw = dict(nbranch=3, correct=1, c_hist=hist, **src)
            a = _launch(o, fn=ops.cfg_step_release, release=None, step=3, mask=o["mask"], **kw)
            b = _launch(o, fn=ops.cfg_step_mask, mask=o["mask"], **kw)
            c = _launch(o, mask=o["mask"], release=None, step=0, **kw)
            assert all(torch.equal(_bits(p), _bits(q)) and torch.equal(_bits(p), _bits(r)) for p, q, r in zip(a, b, c)), (hist, sorted(src))
            a = _launch(o, fn=ops.cfg_step_release, release=None, step=3, mask=None, **kw)
            b = _launch(o, fn=ops.cfg_step_mask, mask=None, **kw)
            assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(a, b)), (hist, sorted(src))


@pytest.mark.parametrize("source", ["injected", "seeded", "none"])
def test_cfg_step_release_variance_noise_sources(source):
    from insv2v import ops
    from insv2v.rng import stream_id, STEP
    o, cpu = _operands(3, 2), sr.step_case(3, 2)
    seed, stream = 20240607, stream_id(STEP, 3, 1, 4)
    if source == "injected":
        more, noise = dict(noise=o["noise"]), cpu["noise"]
    elif source == "seeded":
        more, noise = dict(noise_seed=seed, noise_stream=stream), torch.from_numpy(philox_ref.normals(seed, stream, 0, F * 4 * H * W)).reshape(F, 4, H, W)
    else:
        more, noise = {}, None
    c_hist = f32(0.21)
    kw = dict(nbranch=3, correct=1, c_hist=c_hist)
    got = _launch(o, release=o["release"], step=1, mask=o["mask"], **kw, **more)
    we, wx0, wprev = sr.step64(cpu, noise=noise, step=1, **kw)
    close(got[2], we, f"cfg_step_release noise={source} eps")
    close(got[1], wx0, f"cfg_step_release noise={source} x0")
    close(got[0], wprev, f"cfg_step_release noise={source} latent")
    want = _launch(o, fn=ops.cfg_step_mask, mask=_equivalent(o, 1), **kw, **more)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))


def test_cfg_step_release_branch_stride_inside_sentinel_buffers():
    """Branch-major stacked eps (clip 1 of 2) and every operand carved out of a sentinel-filled buffer: inputs sit between NaNs (a read
    outside an operand poisons the result), outputs - prefilled with NaN - between a finite sentinel that must survive."""
    from insv2v import ops
    o, cpu = _operands(3, 2), sr.step_case(3, 2)
    rows1, pad = F * H * W, 37

    def carve(t, fill):
        buf = torch.full((t.numel() + 2 * pad,), fill, device=DEV, dtype=t.dtype)
        buf[pad:pad + t.numel()] = t.reshape(-1)
        return buf, buf[pad:pad + t.numel()].view(t.shape)

    nan = float("nan")
    ins = {k: carve(o[k], nan) for k in ("lat", "hist", "noise", "ref", "mask", "src", "kn")}
    ins["release"] = carve(o["release"], 0)   # (an int32 sentinel that would release every cell)
    big = torch.full((3, 2, rows1 * 4), nan, device=DEV)
    big[:, 1] = o["eps_in"].reshape(3, -1)
    eps_in, bstride = big.reshape(-1)[rows1 * 4:], 2 * rows1 * 4
    outs = []
    for _ in range(3):
        buf, view = carve(torch.full_like(o["lat"], nan), 12345.0)
        outs.append((buf, view))
    c_hist = f32(-0.37)
    ops.cfg_step(eps_in, ins["lat"][1], nbranch=3, text_cfg=TC, img_cfg=IC, sqrt_a=SA, sqrt_1ma=S1, coef=COEF, latent_out=outs[0][1],
                 pred_x0=outs[1][1], eps_out=outs[2][1], latent_ref=ins["ref"][1], correct=1, noise=ins["noise"][1], branch_stride=bstride,
                 x0_hist=ins["hist"][1], c_hist=c_hist, mask=ins["mask"][1], src=ins["src"][1], known_noise=ins["kn"][1], k_src=KS, k_noise=KN,
                 release=ins["release"][1], step=2)
    torch.cuda.synchronize()
    we, wx0, wprev = sr.step64(cpu, nbranch=3, correct=1, c_hist=c_hist, noise=cpu["noise"], step=2)
    close(outs[2][1], we, "cfg_step_release strided eps")
    close(outs[1][1], wx0, "cfg_step_release strided x0")
    close(outs[0][1], wprev, "cfg_step_release strided latent")
    for buf, view in outs:
        assert (buf[:pad] == 12345.0).all() and (buf[pad + view.numel():] == 12345.0).all(), "a write outside an output"
    for k, (buf, view) in ins.items():
        edge = torch.cat([buf[:pad], buf[pad + view.numel():]])
        assert ((edge == 0) if k == "release" else torch.isnan(edge)).all() and torch.equal(view, o[k]), f"input {k} was written"
    assert torch.isnan(big[:, 0]).all() and torch.equal(big[:, 1], o["eps_in"].reshape(3, -1))


def test_cfg_step_release_refusals():
    from insv2v import ops, _lib
    o = _operands(3, 2)
    out = torch.zeros_like(o["lat"])
    base = dict(nbranch=3, text_cfg=TC, img_cfg=IC, sqrt_a=SA, sqrt_1ma=S1, coef=COEF, k_src=KS, k_noise=KN, step=1)
    full = dict(release=o["release"], mask=o["mask"], src=o["src"], known_noise=o["kn"])
    bad = "invalid argument"
    for mask in (dict(), dict(mask=None)):   # a release map without its source / noise / latent_out, with and without a mask
        for drop in ("src", "known_noise"):
            with pytest.raises(_lib.HipKernelError, match=bad):
                ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, **dict(full, **{drop: None}, **mask), **base)
        with pytest.raises(_lib.HipKernelError, match=bad):
            ops.cfg_step(o["eps_in"], o["lat"], eps_out=out, **dict(full, **mask), **base)
        with pytest.raises(_lib.HipKernelError, match=bad):
            ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, **dict(full, **mask), **dict(base, step=-1))
    buf = torch.zeros(2 * out.numel(), device=DEV)
    outv = buf[:out.numel()].view(out.shape)
    inside4 = buf[8:8 + out.numel()].view(out.shape)
    inside_m = buf[out.numel() - 4:out.numel() - 4 + F * H * W].view(F, H, W)
    inside_r = inside_m.view(torch.int32)
    for which in ("latent_out", "pred_x0", "eps_out"):
        outs = {"latent_out": out, which: outv}
        for name, t in (("release", inside_r), ("mask", inside_m), ("src", inside4), ("known_noise", inside4)):
            with pytest.raises(_lib.HipKernelError, match=bad):
                ops.cfg_step(o["eps_in"], o["lat"], **outs, **dict(full, **{name: t}), **base)
        with pytest.raises(_lib.HipKernelError, match=bad):
            ops.cfg_step(o["eps_in"], o["lat"], **outs, x0_hist=inside4, c_hist=0.5, **full, **base)
    for wrong in (o["release"][:2], o["release"].float(), o["release"].long(), o["release"].cpu(), o["release"][:, :, :6]):
        with pytest.raises(_lib.HipKernelError):                                 # wrong shapes and dtypes never reach the kernel
            ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, **dict(full, release=wrong), **base)
    with pytest.raises(_lib.HipKernelError):
        ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, **full, **dict(base, step=1.5))
    lib = _lib.load()
    for k in ("F", "h", "w"):   # not expressible through ops (they come from the latent's shape): the entry itself
        d = _lib.RelStepDesc()
        d.eps_in, d.latent, d.latent_out = o["eps_in"].data_ptr(), o["lat"].data_ptr(), out.data_ptr()
        d.mask, d.src, d.known_noise, d.release = o["mask"].data_ptr(), o["src"].data_ptr(), o["kn"].data_ptr(), o["release"].data_ptr()
        d.nbranch, d.F, d.h, d.w, d.sqrt_a, d.sqrt_1ma = 3, F, H, W, SA, S1
        setattr(d, k, 0)
        assert lib.insv2v_cfg_step_release(ctypes.byref(d), None) == -1
    torch.cuda.synchronize()
    assert out.abs().sum() == 0 and buf.abs().sum() == 0


# ------------------------------------------------------------------------------------------------------------------ the release map
@pytest.mark.parametrize("steps", [1, 3, 20])
@pytest.mark.parametrize("N,HH,WW", [(2, 24, 40), (1, 8, 8)])
def test_strength_release(N, HH, WW, steps):
    """release: exactly the integer restatement, and exactly the restatement's quantisation of ops.mask_to_latent's cell values (the
    shared device function); gate: exactly G, inside sentinel buffers (the entry itself, its outputs carved out of larger buffers)."""
    from insv2v import ops, _lib
    S_np, M_np = sr.smap_case(N, HH, WW, steps)
    Sd, Md = torch.from_numpy(S_np).to(DEV), torch.from_numpy(M_np).to(DEV)
    lib = _lib.load()
    pad = 29
    for mode in ("mean", "max"):
        want_rel = sr.release_plan(S_np, steps, mode)
        cells = ops.mask_to_latent(Sd, mode).cpu().numpy()
        assert np.array_equal(np.nan_to_num(cells, nan=-7.0), np.nan_to_num(sr.cell_values(S_np, mode), nan=-7.0)), f"{mode}: mask_to_latent's cell values"
        for mask_np, mask_d in ((None, None), (M_np, Md)):
            rel, G = ops.strength_release(Sd, steps, mode, mask=mask_d)
            assert rel.dtype == torch.int32 and rel.shape == (N, HH // 8, WW // 8) and G.dtype == torch.float32 and G.shape == Sd.shape
            got = rel.cpu().numpy()
            bad = np.argwhere(got != want_rel)
            assert bad.size == 0, f"{mode} steps={steps}: release differs at {bad[:4].tolist()}: {got[tuple(bad[0])]} vs {want_rel[tuple(bad[0])]}"
            assert np.array_equal(got, sr.release_of_cells(cells, steps))
            want_G = sr.gate(S_np, mask_np)
            assert np.array_equal(G.cpu().numpy().view(np.int32), want_G.view(np.int32)), f"{mode} steps={steps}: gate"
            # the entry itself, both outputs inside sentinel buffers
            rbuf = torch.full((want_rel.size + 2 * pad,), -77, device=DEV, dtype=torch.int32)
            gbuf = torch.full((S_np.size + 2 * pad,), 12345.0, device=DEV, dtype=torch.float32)
            rc = lib.insv2v_strength_release(Sd.data_ptr(), None if mask_d is None else mask_d.data_ptr(), rbuf[pad:].data_ptr(), gbuf[pad:].data_ptr(),
                                             N, HH, WW, 1 if mode == "max" else 0, steps, None)
            torch.cuda.synchronize()
            assert rc == 0
            assert (rbuf[:pad] == -77).all() and (rbuf[pad + want_rel.size:] == -77).all() and (gbuf[:pad] == 12345.0).all() and (gbuf[pad + S_np.size:] == 12345.0).all()
            assert np.array_equal(rbuf[pad:pad + want_rel.size].cpu().numpy().reshape(want_rel.shape), want_rel)
            assert np.array_equal(gbuf[pad:pad + S_np.size].cpu().numpy().reshape(S_np.shape).view(np.int32), want_G.view(np.int32))
        # gate == NULL: only the release map is written
        rbuf = torch.full((want_rel.size + 2 * pad,), -77, device=DEV, dtype=torch.int32)
        assert lib.insv2v_strength_release(Sd.data_ptr(), None, rbuf[pad:].data_ptr(), None, N, HH, WW, 1 if mode == "max" else 0, steps, None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(rbuf[pad:pad + want_rel.size].cpu().numpy().reshape(want_rel.shape), want_rel) and (rbuf[:pad] == -77).all()
    lead, _ = ops.strength_release(Sd[None], steps, "max")
    assert lead.shape == (1, N, HH // 8, WW // 8)   # leading dimensions are kept
    with pytest.raises(ValueError, match="mode"):
        ops.strength_release(Sd, steps, "median")
    for kw in (dict(smap=torch.zeros((1, 12, 8), device=DEV)), dict(smap=torch.zeros((1, 8, 20), device=DEV)), dict(steps=0), dict(steps=2 ** 20 + 1)):
        with pytest.raises(_lib.HipKernelError, match="invalid argument"):
            ops.strength_release(**dict(dict(smap=Sd, steps=steps), **kw))
    for kw in (dict(smap=Sd.cpu()), dict(smap=Sd.double()), dict(mask=Md[..., :4]), dict(mask=Md.cpu())):   # not on the GPU: no fallback
        with pytest.raises(_lib.HipKernelError):
            ops.strength_release(**dict(dict(smap=Sd, steps=steps), **kw))


# ------------------------------------------------------------------------------------------------------------------ pipelines
def _held_is_known(latent, k, release, kind, n_steps, what):
    """Cells that are never released end as k_src z + k_noise n of the last step (kernel bound)."""
    k_src, k_noise = kr.known_coefficients(kind, n_steps, kr.timesteps(kind, n_steps)[-1])
    held = (release == n_steps)[:, :, None].expand_as(latent)
    assert held.any()
    want = k_src * k["source_latent"].double() + k_noise * k["known_noise"].double()
    close(latent.cpu()[held], want[held], what + ": never released cells vs k_src z + k_noise n")


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("case", ["call", "second_clip"])
@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++"])
def test_released_pipelines_vs_oracle_driven_restatement(tiny_unet, oracle_unet, kind, case, masked):
    """5 steps, a release map with the levels 0, 2 and 5: the product pipe against the CPU oracle's loop (fp32 UNet) stepping with the
    float64 restatement."""
    import oracle.pipelines as op
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    n = 5
    i = _pipe_inputs()
    k = _known(i)
    if not masked:
        k = dict(k, mask=None)
    rel = sr.pipe_release(i["F"], i["h"], i["w"], n, 2)
    p = InferenceIP2PVideo(unet, scheduler=kind, num_ddim_steps=n)
    o = op.InferenceIP2PVideo(oracle_unet, scheduler="ddim", num_ddim_steps=n)
    o.scheduler = sr.ReleasedScheduler(kind, n, k["source_latent"], k["known_noise"], k["mask"], rel)
    g = dict(text_cfg=7.5, img_cfg=1.5)
    a = (i["lat"], i["tc"], i["tu"], i["cond"])
    if case == "call":
        r, w = p(*a, **g, **k, release=rel), o(*a, **g)
    else:
        c = dict(latent_ref=i["lref"], noise_correct_step=0.5, **g)
        r, w = p.second_clip_forward(*a, **c, **k, release=rel), o.second_clip_forward(*a, **c)
    tag = f"released {kind} {case} mask={int(masked)}"
    assert len(r["all_latent"]) == len(w["all_latent"]) == len(r["all_pred"]) == n
    report(r["all_pred"][1], w["all_pred"][1], tag + ": x0 of the second step", **TRAJ)
    report(r["all_latent"][2], w["all_latent"][2], tag + ": latent after the step that releases the middle level", **TRAJ)
    report(r["latent"], w["latent"], tag + ": final latent", **TRAJ)
    _held_is_known(r["latent"], k, rel, kind, n, tag)
    if case == "call" and masked:   # release == 0 everywhere next to a mask: bit for bit the masked call without it
        zero = p(*a, **g, **k, release=torch.zeros_like(rel))
        plain = p(*a, **g, **k)
        assert torch.equal(_bits(zero["latent"]), _bits(plain["latent"])) and torch.equal(_bits(zero["all_pred"][2]), _bits(plain["all_pred"][2]))
        assert (r["latent"] - plain["latent"]).abs().max() > 0.1, "the release map changes nothing"


def test_released_flow_variant_gates_the_second_launch(tiny_unet, oracle_unet):
    """The optical-flow pipe: the gate sits where the mask blend sits, in the second launch of a corrected step."""
    import oracle.pipelines as op
    from insv2v.inference import InferenceIP2PVideoOpticalFlow
    from test_multistep_gpu import _flows
    unet, _ = tiny_unet
    n = 5
    i = _pipe_inputs()
    k = _known(i)
    rel = sr.pipe_release(i["F"], i["h"], i["w"], n, 2)
    p = InferenceIP2PVideoOpticalFlow(unet, scheduler="ddim", num_ddim_steps=n)
    o = op.InferenceIP2PVideoOpticalFlow(oracle_unet, scheduler="ddim", num_ddim_steps=n)
    o.scheduler = sr.ReleasedScheduler("ddim", n, k["source_latent"], k["known_noise"], k["mask"], rel)
    c = dict(latent_ref=i["lref"], flows=_flows(i), noise_correct_step=0.5, text_cfg=7.5, img_cfg=1.5)
    a = (i["lat"], i["tc"], i["tu"], i["cond"])
    r, w = p.second_clip_forward(*a, **c, **k, release=rel), o.second_clip_forward(*a, **c)
    report(r["latent"], w["latent"], "released ddim flow: final latent", **TRAJ)
    _held_is_known(r["latent"], k, rel, "ddim", n, "released ddim flow")


def test_released_ddpm_injected_noise_vs_oracle_driven_restatement(tiny_unet, oracle_unet):
    import oracle.pipelines as op
    from insv2v import synth
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    i = _pipe_inputs()
    k = _known(i)
    rel = sr.pipe_release(i["F"], i["h"], i["w"], 4, 2)
    noises = [synth.synth_input(f"strength_map.var.{j}", tuple(i["lat"].shape)) for j in range(3)] + [None]
    p = InferenceIP2PVideo(unet, scheduler="ddpm", num_ddim_steps=4)
    p.variance_noises = noises
    o = op.InferenceIP2PVideo(oracle_unet, scheduler="ddim", num_ddim_steps=4)
    o.scheduler = sr.ReleasedScheduler("ddpm", 4, k["source_latent"], k["known_noise"], k["mask"], rel, noises=noises)
    a = (i["lat"], i["tc"], i["tu"], i["cond"])
    r, w = p(*a, text_cfg=7.5, img_cfg=1.5, **k, release=rel), o(*a, text_cfg=7.5, img_cfg=1.5)
    report(r["all_latent"][0], w["all_latent"][0], "released ddpm: latent after the first step", **TRAJ)
    report(r["latent"], w["latent"], "released ddpm, injected noise: final latent", **TRAJ)
    held = (rel == 4)[:, :, None].expand_as(r["latent"])
    assert torch.equal(r["latent"].cpu()[held], k["source_latent"][held])   # DDPM's end point is alpha_bar = 1: (k_src, k_noise) = (1, 0)


def test_release_counts_the_global_step_with_start_time(tiny_unet, oracle_unet):
    """START_TIME_CASE: 10 steps, start_time 3, a release level at 6.  The loop's own index would release it three steps late, which
    tests/test_strength_map_cpu.py shows to be ten times the bound on these inputs."""
    import oracle.pipelines as op
    from insv2v import ops
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    c = sr.START_TIME_CASE
    n, st = c["steps"], c["start_time"]
    i = _pipe_inputs()
    k = dict(_known(i), mask=None)
    rel = sr.pipe_release(i["F"], i["h"], i["w"], n, c["mid"])
    p = InferenceIP2PVideo(unet, scheduler="ddim", num_ddim_steps=n)
    o = op.InferenceIP2PVideo(oracle_unet, scheduler="ddim", num_ddim_steps=n)
    o.scheduler = sr.ReleasedScheduler("ddim", n, k["source_latent"], k["known_noise"], None, rel)
    st64, x64 = kr.start_latent("ddim", n, (n - st) / n, k["source_latent"].double(), k["known_noise"].double())
    assert st64 == st
    start = ops.add_noise(k["source_latent"].to(DEV), k["known_noise"].to(DEV), *p.scheduler.start_coefficients(int(p.scheduler.timesteps[st])))
    g = dict(text_cfg=7.5, img_cfg=1.5)
    r = p(start, i["tc"], i["tu"], i["cond"], start_time=st, **g, **k, release=rel)
    w = o(x64.float(), i["tc"], i["tu"], i["cond"], start_time=st, **g)
    assert len(r["all_latent"]) == n - st
    # through the executed steps 3, 4, 5 the middle level is still held: bit for bit `known` of step 5 in the latent after it
    mid = (rel == c["mid"])[:, :, None].expand_as(r["latent"])
    k_src, k_noise = kr.known_coefficients("ddim", n, kr.timesteps("ddim", n)[c["mid"] - 1])
    close(r["all_latent"][c["mid"] - 1 - st].cpu()[mid], (k_src * k["source_latent"].double() + k_noise * k["known_noise"].double())[mid],
          "start_time 3: the middle level is held until global step 6")
    report(r["all_latent"][c["mid"] - st], w["all_latent"][c["mid"] - st], "start_time 3: latent after global step 6", **TRAJ)
    report(r["latent"], w["latent"], "start_time 3, release at 6: final latent", **TRAJ)
    _held_is_known(r["latent"], k, rel, "ddim", n, "start_time 3")


def test_run_stacked_and_run_concurrent_with_released_masked_and_plain_clips(tiny_unet):
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    i = _pipe_inputs()
    a, b = _stack_calls(i)
    ka, kb = dict(_known(i, "a"), mask=None), _known(i, "b")
    kb["known_noise"] = b["latent"]
    rel = sr.pipe_release(i["F"], i["h"], i["w"], 4, 2)
    calls = [dict(a, **{k: v for k, v in ka.items() if v is not None}, release=rel), dict(b, **kb), b]   # released call, masked second clip, plain second clip
    p = InferenceIP2PVideo(unet, scheduler="dpmsolver++", num_ddim_steps=4, branch_streams=False)
    seq = [_alone(p, c) for c in calls]
    held = (rel == 4)[:, :, None].expand_as(seq[0]["latent"])
    res = p.run_stacked(calls)
    torch.cuda.synchronize()
    for j, (x, y) in enumerate(zip(seq, res)):
        assert len(y["all_latent"]) == 4 and len(y["all_pred"]) == 4
        report(y["latent"], x["latent"], f"released run_stacked clip {j} vs alone", **STACKED)
        report(y["all_pred"][-1], x["all_pred"][-1], f"released run_stacked clip {j} last x0", **STACKED)
    assert torch.equal(_bits(res[0]["latent"].cpu()[held]), _bits(seq[0]["latent"].cpu()[held])), "held cells differ between alone and stacked"
    _held_is_known(res[0]["latent"], ka, rel, "dpmsolver++", 4, "released run_stacked clip 0")
    pc = InferenceIP2PVideo(unet, scheduler="dpmsolver++", num_ddim_steps=4)
    seq = [_alone(pc, c)["latent"].clone() for c in calls]
    res = pc.run_concurrent(calls)
    torch.cuda.synchronize()
    for j, (x, y) in enumerate(zip(seq, res)):
        report(y["latent"], x, f"released run_concurrent clip {j} vs alone", **STACKED)
    assert torch.equal(_bits(res[0]["latent"].cpu()[held]), _bits(seq[0].cpu()[held]))
    # a batched call slices the release map per entry
    two = [calls[0], dict(calls[0], latent=calls[1]["latent"], source_latent=kb["source_latent"], known_noise=kb["known_noise"], release=rel.flip(1).contiguous())]
    alone = [_alone(p, c)["latent"] for c in two]
    cat = {k: torch.cat([c[k] for c in two], 0) for k in ("latent", "text_cond", "text_uncond", "img_cond", "source_latent", "known_noise", "release")}
    out = p(**cat, text_cfg=7.5, img_cfg=1.5, guidance_rescale=0.5)["latent"]
    for j in range(2):
        report(out[j:j + 1], alone[j], f"released batched __call__ entry {j} vs alone", **STACKED)


# ------------------------------------------------------------------------------------------------------------------ drivers
def _strength_image():
    """[1,T,S,S]: a ramp from 0 to 1 over the columns inside a rectangle that is not aligned to the cells, 0 outside it and on whole frames."""
    m = torch.zeros((1, T, S, S))
    m[:, :, 13:41, 10:45] = torch.linspace(0.05, 1.0, 35)[None, None, None, :]
    m[:, 7:] = 0.0
    m[:, 8, 50:60, 2:9] = 0.5
    return m


def test_edit_video_strength_map_is_the_steps_done_by_hand(tiny_unet, tiny_model):
    from insv2v import ops
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.run_loveu_tgve import split_batch
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4)
    u, smap = _unit("a"), _strength_image()
    img, lat, est = _edit(tiny_model, pipe, u, strength_map=smap, return_mask=True)
    assert img.shape == u["frames"].shape and lat.shape == (1, T, 4, S // 8, S // 8)
    # by hand: the release map and the gate, the two windows with release=, the decode, the composite with G
    model = tiny_model
    z = model.encode_image_to_latent(u["frames"], u["enc_noise"])
    cond = z / model.scale_factor
    rel, G = ops.strength_release(smap[0].to(DEV), 4, "max")
    assert torch.equal(est["release"], rel[None]) and torch.equal(est["gate"], G[None]) and set(est) == {"release", "gate"}
    assert np.array_equal(rel.cpu().numpy(), sr.release_plan(smap[0].numpy(), 4, "max")) and len(rel.unique()) >= 4
    zs, conds, rels = (split_batch(t, **WIN)[0] for t in (z.to(device=DEV, dtype=torch.float32), cond, rel[None]))
    n0, n1 = (x.to(device=DEV, dtype=torch.float32) for x in u["init_noises"])
    common = dict(text_cond=u["text_cond"], text_uncond=u["text_uncond"], text_cfg=7.5, img_cfg=1.5)
    first = pipe(latent=n0, img_cond=conds[0], release=rels[0].contiguous(), source_latent=zs[0], known_noise=n0, **common)["latent"]
    init1 = torch.cat([n0[:, -2:], n1], dim=1)
    second = pipe.second_clip_forward(latent=init1, img_cond=torch.cat([conds[0][:, -2:], conds[1]], dim=1),
                                      release=torch.cat([rels[0][:, -2:], rels[1]], dim=1).contiguous(), source_latent=torch.cat([zs[0][:, -2:], zs[1]], dim=1),
                                      known_noise=init1, latent_ref=first[:, -2:], noise_correct_step=0.5, **common)["latent"]
    want_lat = torch.cat([first, second[:, 2:]], dim=1)
    dec = model.decode_latent_to_image(want_lat)[0].to(torch.float32).contiguous()
    want_img = ops.composite(dec, u["frames"][0].to(device=DEV, dtype=torch.float32).contiguous(), G)[None]
    assert torch.equal(_bits(lat), _bits(want_lat)) and torch.equal(_bits(img), _bits(want_img))
    # where the strength is 0 the delivered pixel is the input's; elsewhere something was edited; never released cells end at `known`
    img, lat = img.cpu(), lat.cpu()
    keep = (smap == 0.0)[:, :, None].expand_as(img)
    assert torch.equal(img[keep], u["frames"][keep]) and (img[~keep] - u["frames"][~keep]).abs().max() > 1e-2 and img.abs().max() <= 1.0
    n = torch.cat(u["init_noises"], dim=1)
    k_src, k_noise = kr.known_coefficients("ddim", 4, kr.timesteps("ddim", 4)[-1])
    held = (rel.cpu() == 4)[None, :, None].expand_as(lat)
    close(lat[held], (k_src * z.cpu().double() + k_noise * n.double())[held], "edit_video: latent of the never released cells")
    # a lower strength stays closer to the source: cells released at step 3 against cells free from step 0, inside the ramp of one frame
    plain = _edit(tiny_model, pipe, u)[1].cpu()
    assert (lat - plain)[held].abs().max() > 0.1
    # a [1,1,H,W] map serves all frames, next to a mask and in "mean" mode: G is the mask where the map is positive
    mask = _image_mask()
    one, _, est1 = _edit(tiny_model, pipe, u, strength_map=smap[:, :1], mask=mask, mask_mode="mean", return_mask=True)
    want_G = sr.gate(smap[:, :1].expand(1, T, S, S)[0].numpy(), mask[0].numpy())
    assert np.array_equal(est1["gate"][0].cpu().numpy(), want_G)
    assert np.array_equal(est1["release"][0].cpu().numpy(), sr.release_plan(smap[:, :1].expand(1, T, S, S)[0].numpy(), 4, "mean"))
    keep1 = torch.from_numpy(want_G == 0)[None, :, None].expand(1, T, 3, S, S)
    assert torch.equal(one.cpu()[keep1], u["frames"][keep1])


def test_strength_map_from_the_feathered_mask(tiny_unet, tiny_model):
    """strength_map="mask" with mask_shape=dict(feather=...): the map is ``shaped`` - bit for bit the edit that is handed ``shaped`` as a
    tensor map - and the latent hold still comes from ``support``."""
    from insv2v.inference import InferenceIP2PVideo
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4)
    u, mask = _unit("a"), _image_mask()
    shape = dict(feather=6.0)
    img, lat, est = _edit(tiny_model, pipe, u, mask=mask, mask_shape=shape, strength_map="mask", return_mask=True)
    assert {"shaped", "support", "release", "gate"} <= set(est)
    shaped = est["shaped"]
    assert ((shaped > 0) & (shaped < 1)).any(), "the feather left no graded edge"
    img2, lat2, est2 = _edit(tiny_model, pipe, u, mask=mask, mask_shape=shape, strength_map=shaped.cpu(), return_mask=True)
    assert torch.equal(_bits(img), _bits(img2)) and torch.equal(_bits(lat), _bits(lat2)) and torch.equal(est["release"], est2["release"])
    assert torch.equal(est["gate"], shaped), "G is the shaped mask where it is positive, 0 elsewhere"
    assert len(est["release"].unique()) >= 3, "the feather became no graded strength"
    hard = _edit(tiny_model, pipe, u, mask=mask, mask_shape=shape)[1]
    assert (lat - hard).abs().max() > 1e-2
    keep = (shaped.cpu() == 0.0)[:, :, None].expand_as(img)
    assert torch.equal(img.cpu()[keep], u["frames"][keep])


def test_edit_videos_two_units_one_mapped(tiny_unet, tiny_model):
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.run_loveu_tgve import edit_videos
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4)
    smap = _strength_image()
    units = [dict(_unit("a"), text_cfg=7.5, video_cfg=1.5, strength_map=smap), dict(_unit("b"), text_cfg=7.5, video_cfg=1.5)]
    outs = edit_videos(tiny_model, pipe, units, return_latent=True, **WIN)
    for j, (u, (img, lat)) in enumerate(zip(units, outs)):
        rimg, rlat = _edit(tiny_model, pipe, u, **({"strength_map": u["strength_map"]} if "strength_map" in u else {}))
        report(lat, rlat.cpu(), f"edit_videos unit {j} latent vs edit_video", **STACKED)
        report(img, rimg.cpu(), f"edit_videos unit {j} frames vs edit_video", **STACKED)
    keep = (smap == 0.0)[:, :, None].expand_as(units[0]["frames"])
    assert torch.equal(outs[0][0].cpu()[keep], units[0]["frames"][keep])
    assert (outs[0][1] - outs[1][1]).abs().max() > 1e-2, "two different units gave the same latent"


def test_keyframes_reduce_the_map_to_the_keys(tiny_unet, tiny_model):
    """keyframes=2: the key frames are bit for bit edit_video(frames[:, keys], strength_map=map[:, keys]); the frames in between are
    composited with the full-rate G, so where the map is 0 they are the input's."""
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.keyfill import key_frames
    from insv2v.run_loveu_tgve import edit_video
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4)
    u, smap = _unit("a"), _strength_image()
    flows = dict(fwd=torch.zeros((T - 1, 2, S, S), device=DEV), bwd=torch.zeros((T - 1, 2, S, S), device=DEV))
    keys = key_frames(T, 2)
    assert len(keys) < T
    args = (tiny_model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5)
    got, est = edit_video(*args, seed=5, unit=0, strength_map=smap, keyframes=2, key_flows=flows, return_mask=True, **WIN)
    sub = edit_video(tiny_model, pipe, u["frames"][:, keys], u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=5, unit=0, strength_map=smap[:, keys], **WIN)
    assert torch.equal(_bits(got[:, keys]), _bits(sub))
    assert est["gate"].shape == (1, T, S, S) and est["release"].shape == (1, len(keys), S // 8, S // 8) and list(est["keys"]) == list(keys)
    assert np.array_equal(est["gate"][0].cpu().numpy(), sr.gate(smap[0].numpy()))
    keep = (smap == 0.0)[:, :, None].expand_as(got)
    assert torch.equal(got.cpu()[keep], u["frames"][keep])
