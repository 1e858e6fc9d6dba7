"""DPM-Solver++ multistep on the GPU: insv2v_cfg_step_ms against a float64 restatement and against insv2v_cfg_step, the closed-form
Gaussian trajectory through the kernel, and the pipelines on the tiny UNet against (a) the golden DDIM latent of the unmodified reference
(order 1 IS DDIM) and (b) the CPU oracle's loops driven by the float64 sampler of tests/multistep_ref.py.

Bounds: kernel level 1e-5 * max|ref| (a handful of fp32 operations per element); 10-step trajectories the project's rel-RMS 3e-2 /
max 1e-1 (tests/test_model_gpu.py); stacked against alone its rel-RMS 1e-2 / max 4e-2 (test_run_stacked_matches_sequential)."""
import math

import numpy as np
import pytest
import torch

import multistep_ref as mr
from test_model_gpu import tiny_unet, _pipe_inputs, report   # noqa: F401  (tiny_unet: the module-scoped fixture, instantiated for this module)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TRAJ = dict(rms_tol=3e-2, max_tol=1e-1)
F, H, W = 3, 5, 7   # odd on purpose: the kernel reads channels-last eps and writes the reference layout


def f32(v):
    return float(np.float32(v))


def _rnd(key, shape):
    from insv2v import synth
    return synth.synth_input(f"multistep.{key}", tuple(shape)).to(DEV)


def close(got, ref64, what):
    """|got - ref| <= 1e-5 * max|ref|, ref in float64 on the host."""
    err = (got.detach().double().cpu() - ref64).abs().max().item()
    mx = ref64.abs().max().item()
    print(f"[parity] {what}: max-abs err {err:.3e}  max|ref| {mx:.3e}  ratio {err / mx:.3e}")
    assert math.isfinite(err) and err <= 1e-5 * mx, f"{what}: {err:.3e} > 1e-5 * {mx:.3e}"


# ------------------------------------------------------------------------------------------------------------------ kernel level
def _step_ref64(e, lat, *, nbranch, tc, ic, sa, s1, coef, c_hist, hist, noise, gr, correct, ref, dq):
    """Float64 restatement of insv2v_cfg_step_ms.  e: [3,F,4,h,w] (nbranch 3) or [F,4,h,w] (nbranch 0), reference layout."""
    e, lat = e.double().cpu(), lat.double().cpu()
    if nbranch == 3:
        n1 = e[0]
        cfg = e[0] + ic * (e[1] - e[0]) + tc * (e[2] - e[1])
        if gr > 0:
            cfg = gr * (cfg * (n1.std() / cfg.std())) + (1 - gr) * cfg
        e = cfg
    if correct:
        ref = ref.double().cpu()
        R = ref.shape[0]
        d = (lat[:R] - sa * ref) / s1 - e[:R]
        q = d.mean(0, keepdim=True) if correct == 1 else dq.double().cpu()
        e = torch.cat([e[:R] + d, e[R:] + q], 0)
    x0 = (lat - s1 * e) / sa
    prev = coef[0] * x0 + coef[1] * e + coef[2] * lat + c_hist * hist.double().cpu() + coef[3] * noise.double().cpu()
    return e, x0, prev


@pytest.mark.parametrize("correct", [0, 1, 2])
@pytest.mark.parametrize("nbranch", [3, 0])
def test_cfg_step_ms_vs_float64(nbranch, correct):
    """Every combination of guidance rescale 0 / 0.5, back-to-back / branch-major stacked eps (clip 1 of 2) and both signs of c_hist, with
    all five terms of the update present, at t = 501 of a 10-step grid."""
    from insv2v import ops
    from insv2v.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(10)
    co = s.coefficients(501, 601)
    sa, s1 = co["sqrt_a"], co["sqrt_1ma"]
    rows1, R = F * H * W, 2
    lat, hist, noise = _rnd("lat", (F, 4, H, W)), _rnd("hist", (F, 4, H, W)), _rnd("noise", (F, 4, H, W))
    ref, dq = _rnd("ref", (R, 4, H, W)), _rnd("dq", (F - R, 4, H, W))
    e = _rnd("eps3", (3, F, 4, H, W)) if nbranch == 3 else _rnd("eps0", (F, 4, H, W))
    coef = (f32(0.83), f32(0.05), f32(0.41), f32(0.3))
    tc, ic = 7.5, 1.5
    for gr in ((0.0, 0.5) if nbranch == 3 else (0.0,)):
        for stacked in ((False, True) if nbranch == 3 else (False,)):
            for c_hist in (f32(-0.37), f32(0.21)):
                bstride = 0
                if nbranch == 3:
                    e_cl = e.permute(0, 1, 3, 4, 2).contiguous()
                    eps_in = e_cl
                    if stacked:   # branch-major stack of n = 2 clips, this one is clip 1
                        big = torch.full((3, 2, rows1 * 4), 1e3, device=DEV)
                        big[:, 1] = e_cl.reshape(3, -1)
                        eps_in, bstride = big.reshape(-1)[rows1 * 4:], 2 * rows1 * 4
                else:
                    eps_in = e
                stats = None
                if gr > 0:
                    stats = torch.empty(2, device=DEV)
                    ops.cfg_stats(eps_in, stats, F, H, W, tc, ic, branch_stride=bstride)
                new, pred, eo = torch.zeros_like(lat), torch.zeros_like(lat), torch.zeros_like(lat)
                ops.cfg_step(eps_in, lat, nbranch=nbranch, text_cfg=tc, img_cfg=ic, sqrt_a=sa, sqrt_1ma=s1, coef=coef, latent_out=new,
                             pred_x0=pred, eps_out=eo, latent_ref=ref if correct else None, correct=correct,
                             delta_q=dq if correct == 2 else None, noise=noise, rescale_stats=stats, guidance_rescale=gr,
                             branch_stride=bstride, x0_hist=hist, c_hist=c_hist)
                we, wx0, wprev = _step_ref64(e, lat, nbranch=nbranch, tc=tc, ic=ic, sa=sa, s1=s1, coef=coef, c_hist=c_hist, hist=hist,
                                             noise=noise, gr=gr, correct=correct, ref=ref, dq=dq)
                tag = f"cfg_step_ms nbranch={nbranch} correct={correct} rescale={gr} stacked={int(stacked)} c_hist={c_hist:+.2f}"
                close(eo, we, tag + " eps")
                close(pred, wx0, tag + " x0")
                close(new, wprev, tag + " prev")
                # the history term reached the output
                plain = torch.zeros_like(lat)
                ops.cfg_step(eps_in, lat, nbranch=nbranch, text_cfg=tc, img_cfg=ic, sqrt_a=sa, sqrt_1ma=s1, coef=coef, latent_out=plain,
                             latent_ref=ref if correct else None, correct=correct, delta_q=dq if correct == 2 else None, noise=noise,
                             rescale_stats=stats, guidance_rescale=gr, branch_stride=bstride)
                assert (new - plain).abs().max() > 0.1, tag + ": the history term did not reach the output"


@pytest.mark.parametrize("strided", [False, True])
def test_ms_entry_without_history_is_cfg_step_and_seeded_noise_is_randn(strided):
    from insv2v import ops, _lib
    from insv2v.rng import stream_id, STEP
    from insv2v.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")
    s.set_timesteps(10)
    co = s.coefficients(501, 601)
    assert co["coef"][3] != 0.0 and co["c_hist"] != 0.0
    rows = F * H * W
    bstride = (rows + 11) * 4 if strided else 0
    eps = _rnd("eq.eps", (3 * (rows + 11) * 4,))
    lat, hist, ref = _rnd("eq.lat", (F, 4, H, W)), _rnd("eq.hist", (F, 4, H, W)), _rnd("eq.ref", (2, 4, H, W))
    seed, stream = 1234567, stream_id(STEP, 5, 1, 2)
    kw = dict(nbranch=3, text_cfg=7.5, img_cfg=1.5, sqrt_a=co["sqrt_a"], sqrt_1ma=co["sqrt_1ma"], coef=co["coef"], latent_ref=ref,
              correct=1, branch_stride=bstride)

    def run(fn, **more):
        out = [torch.zeros_like(lat) for _ in range(3)]
        fn(eps, lat, latent_out=out[0], pred_x0=out[1], eps_out=out[2], **more, **kw)
        return out

    drawn = ops.randn(lat.shape, seed, stream, device=DEV)
    for src in (dict(noise=drawn), dict(noise_seed=seed, noise_stream=stream), dict()):
        a, b = run(ops.cfg_step, **src), run(ops.cfg_step_ms, x0_hist=None, **src)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), sorted(src)
    # with a history: the seeded stream inside the kernel == the same stream passed as a tensor
    a = run(ops.cfg_step, x0_hist=hist, c_hist=co["c_hist"], noise=drawn)
    b = run(ops.cfg_step, x0_hist=hist, c_hist=co["c_hist"], noise_seed=seed, noise_stream=stream)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = run(ops.cfg_step, noise=drawn)
    assert (a[0] - c[0]).abs().max() > 1e-2 and torch.equal(a[1], c[1]) and torch.equal(a[2], c[2])
    # refused before any launch: a coefficient without a history, a history that is an output, both noise sources
    out = torch.zeros_like(lat)
    with pytest.raises(_lib.HipKernelError, match="invalid argument"):
        ops.cfg_step_ms(eps, lat, latent_out=out, x0_hist=None, c_hist=0.5, **kw)
    for alias in ("latent_out", "pred_x0", "eps_out"):
        with pytest.raises(_lib.HipKernelError, match="invalid argument"):
            ops.cfg_step(eps, lat, **{"latent_out": out, alias: hist}, x0_hist=hist, c_hist=0.5, **kw)
    with pytest.raises(_lib.HipKernelError, match="invalid argument"):
        ops.cfg_step(eps, lat, latent_out=out, x0_hist=hist, c_hist=0.5, noise=drawn, noise_seed=seed, noise_stream=stream, **kw)
    with pytest.raises(_lib.HipKernelError):
        ops.cfg_step(eps, lat, latent_out=out, x0_hist=hist[:2], c_hist=0.5, **kw)
    torch.cuda.synchronize()
    assert out.abs().sum() == 0


def _device_gauss(z, n, order):
    """The closed-form case through ops.cfg_step (nbranch = 0): eps* evaluated by torch on the device in fp32."""
    from insv2v import ops
    from insv2v.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(solver_order=order)
    s.set_timesteps(n)
    ac = s.alphas_cumprod.double()
    ts = s.timesteps.tolist()
    a, sg = math.sqrt(float(ac[ts[0]])), math.sqrt(1 - float(ac[ts[0]]))
    lat = torch.from_numpy(mr.gauss_marginal(z, a, sg)).float().reshape(4, 4, 16, 16).to(DEV)
    hist = tl = None
    for t in ts:
        a, sg = math.sqrt(float(ac[t])), math.sqrt(1 - float(ac[t]))
        eps = mr.gauss_eps(lat, a, sg)
        co = s.coefficients(t, tl)
        new, pred = torch.empty_like(lat), torch.empty_like(lat)
        ops.cfg_step(eps, lat, nbranch=0, sqrt_a=co["sqrt_a"], sqrt_1ma=co["sqrt_1ma"], coef=co["coef"], latent_out=new, pred_x0=pred,
                     **(dict(x0_hist=hist, c_hist=co["c_hist"]) if co["c_hist"] != 0.0 else {}))
        lat, hist, tl = new, pred, t
    return lat.double().cpu().numpy().reshape(-1)


def test_closed_form_gaussian_trajectory_on_the_device():
    z = np.random.default_rng(0).standard_normal(4096)
    ref, exact = mr.gauss_trajectory(z, 10, 2)
    got = _device_gauss(z, 10, 2)
    one20 = _device_gauss(z, 20, 1)
    d, e2m, e1 = mr.rel_rms(got, ref), mr.rel_rms(got, exact), mr.rel_rms(one20, exact)
    print(f"[parity] gaussian 2M@10 on the device: rel-rms vs float64 host simulation {d:.3e}; error vs closed form {e2m:.3e}, "
          f"order 1 @20 on the device {e1:.3e}")
    assert d <= 1e-4
    assert e2m < e1


# ------------------------------------------------------------------------------------------------------------------ pipelines
@pytest.fixture(scope="module")
def oracle_unet(tiny_unet):
    import oracle.unet3d as ou
    from insv2v import synth
    o = ou.UNet3DConditionModel(**synth.UNET_TINY).eval()
    o.load_state_dict(tiny_unet[1])
    return o


def _flows(i):
    from insv2v import synth
    return [synth.synth_input(f"pipe.flow{q}", (i["R"], 2, i["h"] * 8, i["w"] * 8), scale=8.0) for q in range(i["F"] - i["R"])]


def test_order_1_is_ddim_vs_golden(tiny_unet, golden):
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    i = _pipe_inputs()
    p = InferenceIP2PVideo(unet, scheduler="dpmsolver++", solver_order=1, num_ddim_steps=10)
    r = p(i["lat"], i["tc"], i["tu"], i["cond"], text_cfg=7.5, img_cfg=1.5)
    report(r["latent"], golden("pipelines_tiny")["ddim10_latent"], "dpmsolver++ order 1, 10 steps vs golden ddim10 latent", **TRAJ)


@pytest.mark.parametrize("case", ["call", "second_clip", "flow", "start_time_3"])
def test_order_2_vs_oracle_driven_restatement(tiny_unet, oracle_unet, case):
    """2M at 10 steps: the product pipe against the CPU oracle's loop (fp32 UNet) stepping with the float64 restatement."""
    import oracle.pipelines as op
    from insv2v.inference import InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow
    unet, _ = tiny_unet
    i = _pipe_inputs()
    flow = case == "flow"
    p = (InferenceIP2PVideoOpticalFlow if flow else InferenceIP2PVideo)(unet, scheduler="dpmsolver++", num_ddim_steps=10)
    o = (op.InferenceIP2PVideoOpticalFlow if flow else op.InferenceIP2PVideo)(oracle_unet, scheduler="ddim", num_ddim_steps=10)
    o.scheduler = mr.RefScheduler(10, solver_order=2)
    a = (i["lat"], i["tc"], i["tu"], i["cond"])
    g = dict(text_cfg=7.5, img_cfg=1.5)
    if case == "call":
        r, w = p(*a, **g), o(*a, **g)
    elif case == "start_time_3":
        r, w = p(*a, start_time=3, **g), o(*a, start_time=3, **g)
        assert len(r["all_latent"]) == 7
    elif case == "second_clip":
        k = dict(latent_ref=i["lref"], noise_correct_step=0.5, **g)
        r, w = p.second_clip_forward(*a, **k), o.second_clip_forward(*a, **k)
    else:
        k = dict(latent_ref=i["lref"], flows=_flows(i), noise_correct_step=0.5, **g)
        r, w = p.second_clip_forward(*a, **k), o.second_clip_forward(*a, **k)
    assert len(r["all_latent"]) == len(w["all_latent"]) == len(r["all_pred"])
    report(r["all_pred"][1], w["all_pred"][1], f"dpmsolver++ 2M {case}: x0 of the first second-order step", **TRAJ)
    report(r["latent"], w["latent"], f"dpmsolver++ 2M {case}: final latent (10-step grid)", **TRAJ)


def _stack_calls(i):
    from insv2v import synth
    lat2 = synth.synth_input("pipe.latent.b", (1, i["F"], 4, i["h"], i["w"]))
    tc2 = synth.synth_input("pipe.tc.b", tuple(i["tc"].shape))
    return [dict(latent=i["lat"], text_cond=i["tc"], text_uncond=i["tu"], img_cond=i["cond"], text_cfg=7.5, img_cfg=1.5, guidance_rescale=0.5),
            dict(latent=lat2, text_cond=tc2, text_uncond=i["tu"], img_cond=i["cond"], latent_ref=i["lref"], noise_correct_step=0.5,
                 text_cfg=5.0, img_cfg=1.2)]


def _alone(p, c, **more):
    c = dict(c, **more)
    return (p.second_clip_forward if "latent_ref" in c else p)(**c)


def test_run_stacked_and_run_concurrent_match_each_call_alone(tiny_unet):
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    calls = _stack_calls(_pipe_inputs())
    p = InferenceIP2PVideo(unet, scheduler="dpmsolver++", num_ddim_steps=4, branch_streams=False)
    seq = [_alone(p, c) for c in calls]
    res = p.run_stacked(calls)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(seq, res)):
        assert len(b["all_latent"]) == 4 and len(b["all_pred"]) == 4
        report(b["latent"], a["latent"], f"dpmsolver++ 2M run_stacked clip {k} vs alone")
        report(b["all_pred"][0], a["all_pred"][0], f"dpmsolver++ 2M run_stacked clip {k} first x0")
    # the history is per clip: interleaved on two stream sets == one after the other, bit for bit
    pc = InferenceIP2PVideo(unet, scheduler="dpmsolver++", num_ddim_steps=4)
    seq = [_alone(pc, c)["latent"].clone() for c in calls]
    res = pc.run_concurrent(calls)
    torch.cuda.synchronize()
    for a, b in zip(seq, res):
        assert torch.equal(a, b["latent"])


def test_sde_seeded_unit_alone_and_stacked(tiny_unet):
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    p = InferenceIP2PVideo(unet, scheduler="sde-dpmsolver++", num_ddim_steps=4, branch_streams=False)
    assert p.scheduler.stochastic
    calls = [dict(c, seed=7, unit=j) for j, c in enumerate(_stack_calls(_pipe_inputs()))]
    alone = [_alone(p, c)["latent"].clone() for c in calls]
    assert torch.equal(_alone(p, calls[0])["latent"], alone[0])
    d = (_alone(p, calls[0], seed=8)["latent"] - alone[0]).pow(2).mean().sqrt() / alone[0].pow(2).mean().sqrt()
    assert d > 0.1, "another seed gave the same latent"
    for order in (calls, calls[::-1]):
        for c, r in zip(order, p.run_stacked(order)):
            report(r["latent"], alone[c["unit"]], f"sde-dpmsolver++ run_stacked unit {c['unit']} vs alone (seed)", rms_tol=1e-2, max_tol=4e-2)


def test_sde_injected_noise_vs_oracle_driven_restatement(tiny_unet, oracle_unet):
    import oracle.pipelines as op
    from insv2v import synth
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    i = _pipe_inputs()
    noises = [synth.synth_input(f"multistep.var.{k}", tuple(i["lat"].shape)) for k in range(10)]
    p = InferenceIP2PVideo(unet, scheduler="sde-dpmsolver++", num_ddim_steps=10)
    p.variance_noises = noises
    o = op.InferenceIP2PVideo(oracle_unet, scheduler="ddim", num_ddim_steps=10)
    o.scheduler = mr.RefScheduler(10, solver_order=2, sde=True, noises=noises)
    a = (i["lat"], i["tc"], i["tu"], i["cond"])
    r, w = p(*a, text_cfg=7.5, img_cfg=1.5), o(*a, text_cfg=7.5, img_cfg=1.5)
    report(r["latent"], w["latent"], "sde-dpmsolver++ 2M, injected noise: final latent (10-step grid)", **TRAJ)
    assert torch.equal(p(*a, text_cfg=7.5, img_cfg=1.5, seed=3)["latent"], r["latent"])   # an injected noise wins over the seed


def test_one_entry_per_executed_step(tiny_unet):
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    i = _pipe_inputs()
    for name in ("dpmsolver++", "sde-dpmsolver++"):
        p = InferenceIP2PVideo(unet, scheduler=name, num_ddim_steps=4)
        for start in (0, 1, 3):
            r = p(i["lat"], i["tc"], i["tu"], i["cond"], text_cfg=7.5, img_cfg=1.5, start_time=start, seed=1)
            assert len(r["all_latent"]) == len(r["all_pred"]) == 4 - start
            assert torch.equal(r["all_latent"][-1], r["latent"]) and torch.isfinite(r["latent"]).all()
            assert len({x.data_ptr() for x in r["all_pred"]}) == 4 - start   # the history is last step's entry, never overwritten
