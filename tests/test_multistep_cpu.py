"""DPM-Solver++ multistep on the host: the scheduler's time grid, its coefficient table against known answers and against the float64
restatement of tests/multistep_ref.py, order selection, and the interfaces the feature adds (C header, ctypes, CLI, pipelines)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import multistep_ref as mr
from conftest import ROOT


def _sched(n, order=2, alg="dpmsolver++"):
    from insv2v.schedulers import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(solver_order=order, algorithm_type=alg, beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear")
    s.set_timesteps(n)
    return s


def _apply(co, x, eps, hist=None, noise=None):
    """The kernel's update in float64 with the scheduler's (fp32-valued) scalars."""
    x0 = (x - co["sqrt_1ma"] * eps) / co["sqrt_a"]
    c_x0, c_eps, c_xt, c_noise = co["coef"]
    prev = c_x0 * x0 + c_eps * eps + c_xt * x
    if co["c_hist"] != 0.0:
        prev = prev + co["c_hist"] * hist
    if c_noise != 0.0:
        prev = prev + c_noise * noise
    return prev, x0


def _alpha_sigma(s, t, n):
    prev = t - 1000 // n
    ac = s.alphas_cumprod.double()
    a_t, a_p = float(ac[t]), float(ac[prev] if prev >= 0 else ac[0])
    return math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_p), math.sqrt(1 - a_p)


@pytest.mark.parametrize("n", [4, 10, 20, 50])
def test_timesteps_are_ddims(n):
    from insv2v.schedulers import DDIMScheduler
    d = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False)
    d.set_timesteps(n)
    for alg in ("dpmsolver++", "sde-dpmsolver++"):
        s = _sched(n, alg=alg)
        assert s.timesteps.tolist() == d.timesteps.tolist() == mr.leading_timesteps(n)
    assert _sched(n).stochastic is False and _sched(n, alg="sde-dpmsolver++").stochastic is True


@pytest.mark.parametrize("n", [4, 10, 20])
def test_order_1_of_the_ode_form_is_ddim(n):
    """c_x0 x0 + c_xt x_t = alpha_prev x0 + sigma_prev eps on random float64 vectors, to 1e-6 relative (the coefficients are fp32),
    at every step of the grid, the end point alpha_bar[0] included; and next to DDIMScheduler's own coefficients."""
    from insv2v.schedulers import DDIMScheduler
    d = DDIMScheduler(set_alpha_to_one=False, steps_offset=1, clip_sample=False)
    d.set_timesteps(n)
    s = _sched(n, order=1)
    g = np.random.default_rng(n)
    for t in s.timesteps.tolist():
        co = s.coefficients(t, None)
        assert co["c_hist"] == 0.0 and co["coef"][1] == 0.0 and co["coef"][3] == 0.0
        cd = d.coefficients(t)
        assert co["sqrt_a"] == cd["sqrt_a"] and co["sqrt_1ma"] == cd["sqrt_1ma"]
        x0, eps = g.standard_normal(512), g.standard_normal(512)
        x = co["sqrt_a"] * x0 + co["sqrt_1ma"] * eps
        prev, px0 = _apply(co, x, eps)
        _, _, alpha_p, sigma_p = _alpha_sigma(s, t, n)
        want = alpha_p * x0 + sigma_p * eps
        assert np.abs(px0 - x0).max() <= 1e-12
        assert np.abs(prev - want).max() <= 1e-6 * np.abs(want).max()
        ddim = cd["coef"][0] * x0 + cd["coef"][1] * eps
        assert np.abs(prev - ddim).max() <= 1e-6 * np.abs(ddim).max()


def test_order_selection():
    for alg in ("dpmsolver++", "sde-dpmsolver++"):
        for n in (10, 20):
            s = _sched(n, alg=alg)
            ts = s.timesteps.tolist()
            assert s.coefficients(ts[0], None)["c_hist"] == 0.0                      # the first executed step
            assert s.coefficients(ts[3], None)["c_hist"] == 0.0                      # ... also after start_time = 3
            assert all(s.coefficients(t, tl)["c_hist"] != 0.0 for tl, t in zip(ts[:-2], ts[1:-1]))
            assert s.coefficients(ts[4], ts[3])["c_hist"] != 0.0
            last = s.coefficients(ts[-1], ts[-2])["c_hist"]
            assert (last == 0.0) if n == 10 else (last != 0.0)                       # lower_order_final below 15 steps
            one = _sched(n, order=1, alg=alg)
            assert all(one.coefficients(t, tl)["c_hist"] == 0.0 for tl, t in zip(ts[:-1], ts[1:]))
            for t in ts:
                assert s.coefficients(t, None)["coef"][1] == 0.0                      # c_eps
    # the sign of the history term: minus in the ODE form (E = expm1(-h) < 0 ... c_hist = alpha E / 2r), minus in the SDE form as well
    assert _sched(20).coefficients(801, 851)["c_hist"] < 0 and _sched(20, alg="sde-dpmsolver++").coefficients(801, 851)["c_hist"] < 0
    from insv2v.schedulers import DPMSolverMultistepScheduler
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler(solver_order=3)
    with pytest.raises(NotImplementedError):
        DPMSolverMultistepScheduler(algorithm_type="dpmsolver")


@pytest.mark.parametrize("order", [1, 2])
def test_sde_known_answer(order):
    """A constant x0 = c and x_t = alpha_t c + sigma_t z: one SDE step gives alpha_prev c + sigma_prev (e^-h z + sqrt(1 - e^-2h) n), at
    both orders (the history of a constant x0 is c, so the second-order term cancels).  Pins the SDE row without any other library."""
    n_steps = 20
    s = _sched(n_steps, order=order, alg="sde-dpmsolver++")
    g = np.random.default_rng(order)
    ts = s.timesteps.tolist()
    for tl, t in zip([None] + ts[:-1], ts):
        if order == 2 and tl is None:
            continue
        co = s.coefficients(t, tl)
        assert (co["c_hist"] != 0.0) == (order == 2)
        c = g.standard_normal(256)
        z, nz = g.standard_normal(256), g.standard_normal(256)
        alpha_t, sigma_t, alpha_p, sigma_p = _alpha_sigma(s, t, n_steps)
        x = alpha_t * c + sigma_t * z
        eps = (x - co["sqrt_a"] * c) / co["sqrt_1ma"]      # the model output for which the kernel's x0 is exactly c
        prev, x0 = _apply(co, x, eps, hist=c, noise=nz)
        h = math.log(alpha_p / sigma_p) - math.log(alpha_t / sigma_t)
        want = alpha_p * c + sigma_p * (math.exp(-h) * z + math.sqrt(1 - math.exp(-2 * h)) * nz)
        assert np.abs(x0 - c).max() <= 1e-9
        # fp32 scalars: each of the four terms carries 6e-8 relative, and alpha_prev c is rebuilt from two terms that cancel (c_xt alpha_t
        # + c_x0 [+ c_hist] = alpha_prev) whose sizes are below 2 |c| here
        assert np.abs(prev - want).max() <= 1e-6 * np.abs(want).max()


def _scheduler_trajectory(z, n, order):
    s = _sched(n, order=order)
    ts = s.timesteps.tolist()
    ac = s.alphas_cumprod.double()
    a, sg = math.sqrt(float(ac[ts[0]])), math.sqrt(1 - float(ac[ts[0]]))
    x = mr.gauss_marginal(z, a, sg)
    hist = tl = None
    for t in ts:
        a, sg = math.sqrt(float(ac[t])), math.sqrt(1 - float(ac[t]))
        x, hist = _apply(s.coefficients(t, tl), x, mr.gauss_eps(x, a, sg), hist=hist)
        tl = t
    return x


def test_closed_form_gaussian_trajectory():
    """Data N(1, 0.25^2): the exact eps is known, and so is the probability-flow solution.  2M at 10 steps lands closer to it than order
    1 (DDIM) at 20 steps, and the scheduler's trajectory is the float64 restatement's.  Relative RMS error at the end point, float64
    simulation of this grid: order 1 7.8e-2 / 4.8e-2 / 2.3e-2 at 10 / 20 / 50 steps, 2M 8.5e-3 at 10.  (No such claim for broad data: at s = 1
    the two tie on this uniform-t grid, DESIGN.md.)"""
    z = np.random.default_rng(0).standard_normal(4096)
    got10 = _scheduler_trajectory(z, 10, 2)
    ref10, exact = mr.gauss_trajectory(z, 10, 2)
    e2m = mr.rel_rms(got10, exact)
    e1 = {n: mr.rel_rms(_scheduler_trajectory(z, n, 1), exact) for n in (10, 20, 50)}
    print(f"[multistep] gaussian end point rel-rms error: 2M@10 {e2m:.3e}; order 1 @10 {e1[10]:.3e} @20 {e1[20]:.3e} @50 {e1[50]:.3e}")
    assert e2m < e1[20]
    assert e1[50] < e1[20] < e1[10]
    assert mr.rel_rms(got10, ref10) <= 1e-5
    for n, order in ((20, 2), (20, 1), (10, 1)):
        assert mr.rel_rms(_scheduler_trajectory(z, n, order), mr.gauss_trajectory(z, n, order)[0]) <= 1e-5


def test_sde_trajectory_equals_the_restatement():
    """Ten SDE steps with a synthetic eps and injected noise, the scheduler's scalars against the D0 / D1 form, start_time = 0 and 3."""
    g = np.random.default_rng(7)
    n = 10
    for order in (1, 2):
        for start in (0, 3):
            s = _sched(n, order=order, alg="sde-dpmsolver++")
            ts = s.timesteps.tolist()[start:]
            noises = [g.standard_normal(300) for _ in ts]
            ref = mr.RefScheduler(n, solver_order=order, sde=True)
            x = xr = g.standard_normal(300)
            hist = tl = None
            for k, t in enumerate(ts):
                eps, epsr = np.tanh(x) * 0.7 + 0.1, np.tanh(xr) * 0.7 + 0.1
                x, hist = _apply(s.coefficients(t, tl), x, eps, hist=hist, noise=noises[k])
                xr, _ = ref.step64(epsr, t, xr, noises[k])
                tl = t
            assert mr.rel_rms(x, xr) <= 1e-5


def test_interfaces():
    from insv2v import _lib
    from insv2v.inference import InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow
    from insv2v.run_loveu_tgve import build_parser
    from insv2v.schedulers import DPMSolverMultistepScheduler
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    assert re.search(r"^int insv2v_cfg_step_ms\(const insv2v_mstep_desc\* d, insv2v_stream_t stream\);", header, flags=re.M)
    assert _lib.ABI_VERSION == 15
    src = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "elementwise.hip")).read()
    assert re.search(r"insv2v_abi_version\(void\) \{ return 15; \}", src)
    step = [("eps_in", "p"), ("latent", "p"), ("latent_ref", "p"), ("delta_q", "p"), ("noise", "p"), ("rescale_stats", "p"),
            ("latent_out", "p"), ("pred_x0", "p"), ("eps_out", "p"), ("nbranch", "i"), ("F", "i"), ("h", "i"), ("w", "i"), ("R", "i"),
            ("correct", "i"), ("text_cfg", "f"), ("img_cfg", "f"), ("sqrt_a", "f"), ("sqrt_1ma", "f"), ("c_x0", "f"), ("c_eps", "f"),
            ("c_xt", "f"), ("c_noise", "f"), ("guidance_rescale", "f"), ("branch_stride", "q"), ("noise_seed", "q"), ("noise_stream", "q"),
            ("noise_on", "i")]
    kind = {ctypes.c_void_p: "p", ctypes.c_int64: "q", ctypes.c_int32: "i", ctypes.c_float: "f"}
    assert [(n, kind[t]) for n, t in _lib.StepDesc._fields_] == step
    assert [(n, kind[t]) for n, t in _lib.MStepDesc._fields_] == step + [("x0_hist", "p"), ("c_hist", "f")]
    # the C struct, field for field (the parser of tests/test_cpu_host.py, on the new struct)
    body = re.search(r"typedef struct insv2v_mstep_desc \{(.*?)\} insv2v_mstep_desc;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(const\s+)?(void|float|int64_t|int32_t)\s*(\*?)\s*(.*)", decl)
        ctype = "p" if m.group(3) else {"float": "f", "int64_t": "q", "int32_t": "i"}[m.group(2)]
        fields += [(v.strip(), ctype) for v in m.group(4).split(",")]
    assert fields == [(n, kind[t]) for n, t in _lib.MStepDesc._fields_]
    assert "insv2v_cfg_step_ms" in _lib.SIGNATURES
    a = build_parser().parse_args(["--scheduler", "dpmsolver++", "--solver-order", "1"])
    assert a.solver_order == 1 and a.scheduler == "dpmsolver++" and build_parser().parse_args([]).solver_order == 2

    class FakeUNet:
        device = torch.device("cpu")
    for cls in (InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow):
        for name in ("dpmsolver++", "sde-dpmsolver++"):
            p = cls(FakeUNet(), scheduler=name, num_ddim_steps=10)
            assert isinstance(p.scheduler, DPMSolverMultistepScheduler) and p.scheduler.solver_order == 2
            assert p.scheduler.algorithm_type == name and p.scheduler.stochastic == (name == "sde-dpmsolver++")
            assert p.scheduler.timesteps.tolist() == [901, 801, 701, 601, 501, 401, 301, 201, 101, 1]
            assert cls(FakeUNet(), scheduler=name, solver_order=1).scheduler.solver_order == 1
        with pytest.raises(NotImplementedError):
            cls(FakeUNet(), scheduler="unipc")


def test_ms_entry_refuses_bad_arguments_before_any_launch():
    """The argument checks of insv2v_cfg_step_ms run on the host in front of the launch, so they are testable without a GPU: the
    addresses below are never dereferenced."""
    from insv2v import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build
        build.build(verbose=False)
    lib = _lib.load()
    n = 3 * 4 * 5 * 7 * 4   # bytes of one [F,4,h,w] fp32 tensor

    def desc(**kw):
        d = _lib.MStepDesc()
        d.eps_in, d.latent, d.latent_out, d.pred_x0, d.eps_out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
        d.nbranch, d.F, d.h, d.w = 3, 3, 5, 7
        d.sqrt_a, d.sqrt_1ma, d.c_x0, d.c_xt = 0.8, 0.6, 0.5, 0.5
        d.x0_hist, d.c_hist = 0x60000, 0.25
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)

    assert lib.insv2v_cfg_step_ms(None, None) == -1
    assert lib.insv2v_cfg_step_ms(desc(x0_hist=None), None) == -1                       # a coefficient without a history
    for out in (0x30000, 0x40000, 0x50000):                                            # the history is an output, or overlaps one
        assert lib.insv2v_cfg_step_ms(desc(x0_hist=out), None) == -1
        assert lib.insv2v_cfg_step_ms(desc(x0_hist=out + n - 4), None) == -1
        assert lib.insv2v_cfg_step_ms(desc(x0_hist=out - n + 4), None) == -1
    assert lib.insv2v_cfg_step_ms(desc(noise=0x70000, noise_on=1, c_noise=0.5), None) == -1   # the checks shared with insv2v_cfg_step
    assert lib.insv2v_cfg_step_ms(desc(nbranch=2), None) == -1
    assert lib.insv2v_cfg_step_ms(desc(correct=1), None) == -1
    assert lib.insv2v_cfg_step_ms(desc(latent_out=None, eps_out=None), None) == -1
    assert lib.insv2v_cfg_step_ms(desc(F=0), None) == -1
