"""The mask estimate on the GPU: the three kernels of csrc/automask.hip against the float64 restatement
(tests/automask_ref.py) and their bit-exact properties, ``InferenceIP2PVideo.estimate_mask`` with a planted UNet, on the tiny UNet
against the CPU oracle and with seeded noise, and the drivers' ``mask="auto"``.

Bounds.  Kernel level: ``close`` of tests/test_multistep_gpu.py, 1e-5 * max|ref| against float64.  For insv2v_eps_absdiff_accum that is
derived: per draw 4 subtractions + 3 additions + 1 fma, so at most 4 * 16 + 12 roundings of 2^-24 reach a cell for n <= 16 draws - about
4.6e-6 relative.  ``mask_latent`` is compared in every cell farther than ``dilate`` from a cell whose float64 soft value is within 1e-5
of the threshold (tests/test_automask_cpu.py shows that at most 2 cells per case are in that band on these very inputs).  The pipe's
raw map against the oracle: see ``test_estimate_mask_tiny_unet_vs_oracle``."""
import math

import numpy as np
import pytest
import torch

import automask_ref as ar
from test_model_gpu import tiny_unet, _pipe_inputs, report   # noqa: F401  (tiny_unet: the module-scoped fixture, instantiated for this module)
from test_multistep_gpu import close, f32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STACKED = dict(rms_tol=1e-2, max_tol=5e-2)
# The pipes of this file run without hipGraph capture.  The launches are the same kernels either way (test_model_gpu.py::
# test_unet_graph_matches_eager), but every graph a test process captures stays parked until the process ends, and the park is bounded
# (inference._GRAVEYARD): a retired graph that is destroyed and whose shape is captured again crashes hipGraphLaunch on ROCm 7.2
# (inference.py, above _GRAVEYARD).  This file shares its shapes with the pipeline tests that follow it, so it adds no graph to the
# process.  The captured-graph form of estimate_mask is what tools/bench_automask.py measures.
EAGER = dict(use_graph=False)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------------------------ 1. the input kernel
@pytest.mark.parametrize("ldo", [8, 16])
@pytest.mark.parametrize("stacked", [False, True])
@pytest.mark.parametrize("source", ["injected", "seeded"])
def test_build_unet_input_noised_is_add_noise_then_build_unet_input_bitwise(source, stacked, ldo):
    """F,h,w = 3,5,7: 105 pixels and 420 elements, no multiple of anything.  Alone, and as clip 1 of a 2-clip branch-major stack; the
    output is prefilled with a sentinel, and the rows the call does not own keep it."""
    from insv2v import ops
    from insv2v.rng import stream_id, MASK
    F, h, w = 3, 5, 7
    z, cond = ar._synth("in.z", (F, 4, h, w)).to(DEV), ar._synth("in.cond", (F, 4, h, w)).to(DEV)
    ka, kb = f32(0.6502932), f32(0.7596833)
    seed, stream = 20250311, stream_id(MASK, 7, 2, 1)
    noise = ar._synth("in.noise", (F, 4, h, w)).to(DEV) if source == "injected" else ops.randn((F, 4, h, w), seed, stream, device=DEV)
    src = dict(noise=noise) if source == "injected" else dict(seed=seed, stream=stream)
    n, c = (2, 1) if stacked else (1, 0)
    rows1 = F * h * w
    lay = dict(branch_rows=n * rows1, t_stride=n) if stacked else {}
    SENT, TSENT = 123.0, -7.0
    out, ref = (torch.full((3 * n * rows1, ldo), SENT, device=DEV, dtype=torch.float16) for _ in range(2))
    t_out, t_ref = (torch.full((3 * n,), TSENT, device=DEV, dtype=torch.float32) for _ in range(2))
    ops.build_unet_input_noised(z, cond, out[c * rows1:], t_out[c:], 401, ka, kb, **src, **lay)
    ops.build_unet_input(ops.add_noise(z, noise, ka, kb), cond, ref[c * rows1:], t_ref[c:], 401, 3, **lay)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16)) and torch.equal(t_out, t_ref)
    o = out.view(3, n, rows1, ldo)
    if stacked:
        assert (o[:, 0] == SENT).all() and (t_out.view(3, n)[:, 0] == TSENT).all()
    assert (t_out.view(3, n)[:, c] == 401.0).all()
    # and it is the noised latent, not the source: float64 of the definition, one fp16 rounding
    want = ar.noised(z.cpu().numpy(), noise.cpu().numpy(), ka, kb).transpose(0, 2, 3, 1).reshape(rows1, 4)
    for br in range(3):
        got = o[br, c].float().cpu().numpy()
        assert np.abs(got[:, :4] - want).max() <= 2.0 ** -10 * np.abs(want).max()
        assert np.array_equal(got[:, 4:8], (cond.cpu().numpy().transpose(0, 2, 3, 1).reshape(rows1, 4) if br else np.zeros((rows1, 4))).astype(np.float16).astype(np.float32))
        assert not got[:, 8:].any()
    assert np.abs(o[1, c].float().cpu().numpy()[:, :4] - z.cpu().numpy().transpose(0, 2, 3, 1).reshape(rows1, 4)).max() > 0.1
    with pytest.raises(Exception):
        ops.build_unet_input_noised(z, cond, out, t_out, 401, ka, kb, noise=noise, seed=seed, stream=stream)
    with pytest.raises(Exception):
        ops.build_unet_input_noised(z, cond, out, t_out, 401, ka, kb)


# ------------------------------------------------------------------------------------------------------------------ 2. the accumulator
def _channels_last(e):
    """[3,F,4,h,w] (reference layout) -> the runner's output [3*F*h*w, 4]."""
    return e.permute(0, 1, 3, 4, 2).contiguous().reshape(-1, 4)


def _accumulate(eps, scale):
    from insv2v import ops
    n, _, F, _, h, w = eps.shape
    acc = torch.full((F, h, w), float("nan"), device=DEV)   # the first draw writes: whatever was there is gone
    for d in range(n):
        ops.eps_absdiff_accum(_channels_last(eps[d]).to(DEV), acc, scale, accumulate=d > 0)
    return acc


def _emulate32(eps, scale):
    """The documented order in fp32: s = (|d0| + |d1|) + (|d2| + |d3|); acc = fma(scale, s, acc), the first draw scale * s.  (The fma
    is one rounding of the exact scale * s + acc: float64 holds that product exactly.)"""
    e = eps.numpy().astype(np.float32)
    acc = None
    for d in range(e.shape[0]):
        a = np.abs(e[d, 2] - e[d, 1])                    # [F,4,h,w], fp32
        s = (a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])
        acc = np.float32(scale) * s if acc is None else (np.float64(np.float32(scale)) * s.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


@pytest.mark.parametrize("shape,n", ar.EPS_CASES)
def test_eps_absdiff_accum_vs_float64(shape, n):
    eps = ar.eps_input(*shape, n)
    scale = f32(1.0 / (4 * n))
    acc = _accumulate(eps, scale)
    close(acc, torch.from_numpy(ar.raw_map(eps.numpy())), f"eps_absdiff_accum {shape} n={n}")
    assert np.array_equal(acc.cpu().numpy().view(np.int32), _emulate32(eps, scale).view(np.int32)), "the documented summation order"


def test_eps_absdiff_accum_stacked_reads_only_its_two_branches():
    """Clip 1 of a 3-clip branch-major stack: branch 0 and every other clip's eps are NaN.  Finite, and the alone result bit for bit."""
    from insv2v import ops
    (F, h, w), n, clips, c = (3, 5, 7), 3, 3, 1
    eps = ar.eps_input(F, h, w, n)
    scale = f32(1.0 / (4 * n))
    alone = _accumulate(eps, scale)
    rows1 = F * h * w
    acc = torch.empty((F, h, w), device=DEV)
    for d in range(n):
        buf = torch.full((3, clips, rows1, 4), float("nan"), device=DEV)
        cl = _channels_last(eps[d]).view(3, rows1, 4).to(DEV)
        buf[1, c], buf[2, c] = cl[1], cl[2]
        ops.eps_absdiff_accum(buf.view(-1, 4)[c * rows1:], acc, scale, accumulate=d > 0, branch_stride=clips * rows1 * 4)
    assert torch.isfinite(acc).all() and _same_bits(acc, alone)


@pytest.mark.parametrize("n", [1, 2, 4])
def test_eps_absdiff_accum_exact(n):
    """eps a multiple of 1/8 with |eps| <= 4 and a power-of-two scale: every intermediate is representable, so the result IS the float64 one."""
    F, h, w = 2, 9, 13
    eps = torch.round(ar._synth(f"eps.exact.{n}", (n, 3, F, 4, h, w), kind="uniform") * 32.0) / 8.0
    assert eps.abs().max() <= 4.0 and (eps * 8 == torch.round(eps * 8)).all()
    acc = _accumulate(eps.float(), 1.0 / (4 * n))
    want = ar.raw_map(eps.numpy())
    assert want.max() > 1.0 and np.array_equal(acc.cpu().numpy().astype(np.float64), want)


# ------------------------------------------------------------------------------------------------------------------ 3. finish
def _check_finish(raw, flags, got, what):
    """soft by ``close``; mask_latent equal outside the excluded band; mask = the 8x8 replication, and mask_to_latent of it in both modes."""
    from insv2v import ops
    smooth, dilate, th = flags
    soft, ml, mask = got
    ref = ar.finish(raw.cpu().numpy(), smooth=smooth, dilate=dilate, threshold=th)
    close(soft, torch.from_numpy(ref["soft"]), what + " soft")
    nband, excluded = ar.near_threshold(ref["soft"], th, dilate)
    assert nband <= 2, what
    differ = (ml.cpu().numpy().astype(np.float64) != ref["mask_latent"]) & ~excluded
    assert not differ.any(), f"{what}: mask_latent differs in {int(differ.sum())} cells outside the threshold band"
    assert set(np.unique(ml.cpu().numpy())) <= {0.0, 1.0}
    assert _same_bits(mask, ml.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2))
    for mode in ("max", "mean"):
        assert _same_bits(ops.mask_to_latent(mask, mode), ml), f"{what}: mask_to_latent({mode}) of the image mask is not mask_latent"


@pytest.mark.parametrize("T,h,w", ar.FINISH_SHAPES)
def test_automask_finish_vs_float64(T, h, w):
    from insv2v import ops
    raw = ar.raw_input(T, h, w).to(DEV)
    for flags in ar.FINISH_FLAGS:
        smooth, dilate, th = flags
        got = ops.automask_finish(raw, clamp_ratio=3.0, threshold=th, smooth=smooth, dilate=dilate)
        _check_finish(raw, flags, got, f"automask_finish {T}x{h}x{w} smooth={int(smooth)} dilate={dilate} thr={th}")
    again = ops.automask_finish(raw, clamp_ratio=3.0, threshold=th, smooth=smooth, dilate=dilate)
    assert all(_same_bits(a, b) for a, b in zip(got, again)), "two runs differ"
    other = ops.automask_finish(raw, clamp_ratio=1.5, threshold=0.5, smooth=True, dilate=1)   # another clamp ratio
    close(other[0], torch.from_numpy(ar.finish(raw.cpu().numpy(), clamp_ratio=1.5)["soft"]), f"automask_finish {T}x{h}x{w} clamp_ratio=1.5 soft")


def test_automask_finish_exact_case_bitwise():
    from insv2v import ops
    raw = torch.from_numpy(ar.exact_raw()).to(DEV)
    for smooth, dilate, th in ar.EXACT_FLAGS:
        soft, ml, mask = ops.automask_finish(raw, clamp_ratio=3.0, threshold=th, smooth=smooth, dilate=dilate)
        ref = ar.finish(ar.exact_raw(), smooth=smooth, dilate=dilate, threshold=th)
        for name, g in (("soft", soft), ("mask_latent", ml), ("mask", mask)):
            assert np.array_equal(g.cpu().numpy().astype(np.float64), ref[name]), (name, smooth, dilate, th)
    assert ref["mask_latent"].sum() > 0


def test_automask_finish_zero_map_and_refusals():
    from insv2v import ops, _lib
    for smooth in (True, False):
        got = ops.automask_finish(torch.zeros((3, 5, 7), device=DEV), smooth=smooth, dilate=2)
        assert all(torch.isfinite(g).all() and not g.any() for g in got)
    raw = ar.raw_input(2, 5, 7).to(DEV)
    for kw in (dict(threshold=0.0), dict(threshold=1.0), dict(threshold=float("nan")), dict(clamp_ratio=0.0), dict(clamp_ratio=-1.0), dict(dilate=-1)):
        with pytest.raises(_lib.HipKernelError):
            ops.automask_finish(raw, **kw)
    for bad in (raw[0], raw.cpu(), raw.double(), raw.transpose(1, 2), torch.zeros((0, 5, 7), device=DEV), torch.zeros((2, 0, 7), device=DEV)):
        with pytest.raises(_lib.HipKernelError):
            ops.automask_finish(bad)
    lib = _lib.load()
    soft, ml = torch.empty_like(raw), torch.empty_like(raw)
    mask = torch.empty((2, 40, 56), device=DEV)
    ws = torch.empty(64, device=DEV)
    args = lambda **kw: [kw.get("raw", raw.data_ptr()), kw.get("soft", soft.data_ptr()), kw.get("ml", ml.data_ptr()), kw.get("mask", mask.data_ptr()),
                         kw.get("ws", ws.data_ptr()), kw.get("wsb", 256), kw.get("T", 2), kw.get("h", 5), kw.get("w", 7), 3.0, 0.5, kw.get("smooth", 1), 1, None]
    assert lib.insv2v_automask_finish(*args()) == 0
    for kw in (dict(raw=None), dict(soft=None), dict(ml=None), dict(mask=None), dict(ws=None), dict(T=0), dict(h=-1), dict(w=0), dict(wsb=0),
               dict(smooth=2), dict(soft=raw.data_ptr()), dict(ml=soft.data_ptr())):
        assert lib.insv2v_automask_finish(*args(**kw)) == -1, kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 4. a planted UNet
class _PlantedRunner:
    """Stands in for the stacked runner: eps is random in branches 0 and 1; branch 2 = branch 1 + ``const`` inside ``rect`` on the frames
    in ``frames``.  A row's frame is read from the video condition it finds in x_in (channel 4 of branch 1 holds the frame index)."""

    def __init__(self, B, F, h, w, m, plant):
        self.B, self.F, self.h, self.w, self.m, self.plant = B, F, h, w, m, plant
        self.x_in = torch.full((B * F * h * w, 8), float("nan"), device=DEV, dtype=torch.float16)
        self.t = torch.full((B,), -1.0, device=DEV)
        self.ctx = None
        self.runs = 0

    def set_context(self, ctx):
        self.ctx = ctx

    def run(self):
        m, rows1 = self.m, self.F * self.h * self.w
        x = self.x_in.float().view(3, m, rows1, 8)
        assert torch.isfinite(x).all() and (self.t == self.plant["t"]).all() and self.ctx.shape[0] == 3 * m
        assert not x[0, :, :, 4:].any() and torch.equal(x[1], x[2]) and torch.equal(x[0, :, :, :4], x[1, :, :, :4])
        assert all((x[1, a, :, :4] - x[1, b, :, :4]).abs().max() > 0.1 for a in range(m) for b in range(a))   # every draw its own noise
        g = torch.Generator().manual_seed(1000 + self.runs)
        self.runs += 1
        eps = torch.randn((3, m, rows1, 4), generator=g).to(DEV)
        frame = x[1, :, :, 4].round().long()                                            # [m, rows1]
        cell = torch.arange(rows1, device=DEV) % (self.h * self.w)
        y, xx = cell // self.w, cell % self.w
        (y0, y1, x0, x1) = self.plant["rect"]
        inside = ((y >= y0) & (y < y1) & (xx >= x0) & (xx < x1))[None] & torch.isin(frame, torch.tensor(self.plant["frames"], device=DEV))
        eps[2] = eps[1] + self.plant["const"] * inside[..., None].float()
        return eps.view(-1, 4)


@pytest.mark.parametrize("const", [0.75, 0.0])
def test_estimate_mask_with_a_planted_unet(monkeypatch, const):
    """T = 5 in chunks of 2 (three chunks, the last of one frame), 6x9 cells, 3 draws: the mask is the planted rectangle grown by one
    cell, on the planted frames only; with branch 2 == branch 1 it is empty."""
    from insv2v import inference
    T, h, w, n = 5, 6, 9, 3
    plant = dict(rect=(2, 4, 3, 7), frames=[1, 4], const=const, t=401.0)
    made = {}

    class Unet:
        device = torch.device(DEV)

    def fake_shared_runner(unet, B, F, H, W, L, slot=0, use_graph=True, branch_streams=True, cfg_clips=0):
        assert cfg_clips * 3 == B and not branch_streams and (H, W, L) == (h, w, 77)
        return made.setdefault((B, F), _PlantedRunner(B, F, H, W, cfg_clips, plant))
    monkeypatch.setattr(inference, "shared_runner", fake_shared_runner)
    pipe = inference.InferenceIP2PVideo(Unet(), scheduler="ddim", num_ddim_steps=10, **EAGER)
    z = ar._synth("planted.z", (1, T, 4, h, w))
    cond = ar._synth("planted.cond", (1, T, 4, h, w))
    cond[0, :, 0] = torch.arange(T, dtype=torch.float32)[:, None, None]               # the frame index, for the planted runner
    tc, tu = ar._synth("planted.tc", (1, 77, 64)), ar._synth("planted.tu", (1, 77, 64))
    r = pipe.estimate_mask(z, tc, tu, cond, n_maps=n, smooth=False, dilate=1, frames_in_batch=2)
    torch.cuda.synchronize()
    assert sorted(made) == [(9, 1), (9, 2)] and made[(9, 2)].runs == 2 and made[(9, 1)].runs == 1
    assert r["raw"].shape == r["soft"].shape == r["mask_latent"].shape == (1, T, h, w) and r["mask"].shape == (1, T, 8 * h, 8 * w)
    want_raw, want = np.zeros((T, h, w)), np.zeros((T, h, w))
    if const:
        want_raw[[1, 4], 2:4, 3:7] = const
        want[[1, 4], 1:5, 2:8] = 1.0
    assert np.array_equal(r["mask_latent"][0].cpu().numpy(), want) and all(torch.isfinite(v).all() for v in r.values())
    assert np.abs(r["raw"][0].cpu().numpy() - want_raw).max() <= 1e-6 and not r["raw"][0].cpu().numpy()[want_raw == 0].any()
    assert _same_bits(r["mask"][0], r["mask_latent"][0].repeat_interleave(8, dim=1).repeat_interleave(8, dim=2))
    assert np.array_equal(r["soft"][0].cpu().numpy(), (want_raw > 0).astype(np.float32))   # 16 of 270 cells: raw >= 3 mu inside


# ------------------------------------------------------------------------------------------------------------------ 5. tiny UNet vs oracle
@pytest.fixture(scope="module")
def oracle_unet(tiny_unet):
    import oracle.unet3d as ou
    from insv2v import synth
    o = ou.UNet3DConditionModel(**synth.UNET_TINY).eval()
    o.load_state_dict(tiny_unet[1])
    return o


def _draws(key, chunks, n, h, w):
    return [[ar._synth(f"{key}.noise.{k}.{d}", (1, b - a, 4, h, w)) for d in range(n)] for k, (a, b) in enumerate(chunks)]


def test_estimate_mask_tiny_unet_vs_oracle(tiny_unet, oracle_unet):
    """F = 8, 16x24, 2 injected draws, DDIM 10 steps (mask_strength 0.5 -> t = 401).  With D = eps3 - eps2 of the oracle and
    rho = rms(eps3) / rms(D), both from the oracle alone:  rms(raw_gpu - raw_ref) / rms(D) <= sqrt(2) * 1e-2 * rho.
    Derivation: 1e-2 is the project's per-forward rel-RMS bound (``report``'s default, used for the first x0 prediction) on each of eps3
    and eps2, i.e. an rms error of 1e-2 * rms(eps) each; the two branches err independently at worst (sqrt 2); |.| and averaging do
    not increase an rms error.  The bound means something only while rho <= 10 (asserted; 3.6 on these inputs).
    soft / mask_latent must be the float64 finish of the GPU's OWN raw.  The binary mask is deliberately not compared with the oracle's:
    a random-init UNet's map is nearly flat, a large share of its cells lies within 0.05 of any threshold, and that comparison is noise."""
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    i = _pipe_inputs()
    F, h, w, n = i["F"], i["h"], i["w"], 2
    noises = _draws("pipe", [(0, F)], n, h, w)
    pipe = InferenceIP2PVideo(unet, scheduler="ddim", num_ddim_steps=10, **EAGER)
    r = pipe.estimate_mask(i["lat"], i["tc"], i["tu"], i["cond"], n_maps=n, noises=noises, threshold=0.3)
    t = int(pipe.scheduler.timesteps[5])
    ka, kb = pipe.scheduler.start_coefficients(t)
    assert t == 401
    es = []
    with torch.no_grad():
        for d in range(n):
            x = ka * i["lat"] + kb * noises[0][d]
            l1, l2 = torch.cat([x, torch.zeros_like(i["cond"])], dim=2), torch.cat([x, i["cond"]], dim=2)
            e = oracle_unet(torch.cat([l1, l2, l2.clone()], dim=0).permute(0, 2, 1, 3, 4), torch.full((3,), t, dtype=torch.long),
                            encoder_hidden_states=torch.cat([i["tu"], i["tu"], i["tc"]], dim=0)).sample
            es.append(e.permute(0, 2, 1, 3, 4))
    e = torch.stack(es).double()                                   # [n,3,F,4,h,w]
    delta = e[:, 2] - e[:, 1]
    rms = lambda v: float(v.pow(2).mean().sqrt())
    rho = rms(e[:, 2]) / rms(delta)
    raw_ref = torch.from_numpy(ar.raw_map(e.numpy()))
    err = rms(r["raw"][0].double().cpu() - raw_ref) / rms(delta)
    bound = math.sqrt(2.0) * 1e-2 * rho
    print(f"[automask] tiny UNet vs oracle: rho {rho:.3f}  rms(raw_gpu - raw_ref) / rms(D) {err:.3e}  bound {bound:.3e}")
    assert rho <= 10.0
    assert err <= bound, f"raw map vs oracle: {err:.3e} > {bound:.3e}"
    raw = r["raw"][0]
    ref = ar.finish(raw.cpu().numpy(), threshold=0.3)
    close(r["soft"][0], torch.from_numpy(ref["soft"]), "estimate_mask soft vs float64 finish of its own raw")
    nband, excluded = ar.near_threshold(ref["soft"], 0.3, 1)
    frac = float(ref["bin"].mean())
    print(f"[automask] tiny UNet: {nband} cells in the threshold band, {frac:.3f} of the cells above 0.3")
    assert nband <= 2 and 0.0 < frac < 1.0
    assert not ((r["mask_latent"][0].cpu().numpy().astype(np.float64) != ref["mask_latent"]) & ~excluded).any()


# ------------------------------------------------------------------------------------------------------------------ 6. seeded
def test_estimate_mask_seeded(tiny_unet):
    """T = 10 in chunks of 8 (a second chunk of 2 frames), 2 draws."""
    from insv2v import ops
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.rng import stream_id, MASK
    unet, _ = tiny_unet
    T, h, w, n, fib, seed = 10, 16, 24, 2, 8, 424242
    z, cond = ar._synth("seeded.z", (1, T, 4, h, w)), ar._synth("seeded.cond", (1, T, 4, h, w))
    i = _pipe_inputs()
    pipe = InferenceIP2PVideo(unet, scheduler="ddim", num_ddim_steps=10, **EAGER)
    kw = dict(n_maps=n, frames_in_batch=fib, threshold=0.3)
    a = pipe.estimate_mask(z, i["tc"], i["tu"], cond, seed=seed, unit=3, **kw)
    a = {k: v.clone() for k, v in a.items()}
    b = pipe.estimate_mask(z, i["tc"], i["tu"], cond, seed=seed, unit=3, **kw)
    assert all(_same_bits(a[k], b[k]) for k in ("raw", "soft", "mask_latent", "mask"))
    c = pipe.estimate_mask(z, i["tc"], i["tu"], cond, seed=seed, unit=4, **kw)
    d = float((c["raw"] - a["raw"]).pow(2).mean().sqrt() / a["raw"].pow(2).mean().sqrt())
    print(f"[automask] seeded: rel-rms distance of another unit's raw map {d:.3e}")
    assert d > 1e-3, "another unit gave the same raw map"
    noises = [[ops.randn((1, q - p, 4, h, w), seed, stream_id(MASK, 3, k, dd), device=DEV) for dd in range(n)] for k, (p, q) in enumerate(ar.chunks(T, fib))]
    e = pipe.estimate_mask(z, i["tc"], i["tu"], cond, noises=noises, seed=seed + 1, unit=9, **kw)   # injected tensors win over the seed
    assert all(_same_bits(a[k], e[k]) for k in ("raw", "soft", "mask_latent", "mask"))
    assert 0 < float(a["mask_latent"].mean()) < 1


# ------------------------------------------------------------------------------------------------------------------ 7. drivers
@pytest.fixture(scope="module")
def tiny_model(tiny_unet):
    from insv2v import synth, shapes
    from insv2v.vae import AutoencoderKL
    from insv2v.model import InstructP2PVideoModel
    vae = AutoencoderKL(**synth.VAE_TINY, device=DEV).load_state_dict(synth.synth_state_dict(shapes.vae_shapes(**synth.VAE_TINY)))
    return InstructP2PVideoModel(tiny_unet[0], vae)


T_DRV, S_DRV, SEED = 20, 64, 77   # two windows: 16 frames, then 4 new ones behind 12 carried over
AUTO = dict(n_maps=2, threshold=0.33, dilate=0)   # a random-init UNet's map is nearly flat around 1/3: this cuts through it


def _unit(key):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"automask.ev.frames.{key}", (1, T_DRV, 3, S_DRV, S_DRV), kind="uniform"),
                text_cond=synth.synth_input(f"automask.ev.tc.{key}", (1, 77, 64)), text_uncond=synth.synth_input("automask.ev.tu", (1, 77, 64)))


def _edit(model, pipe, u, unit, **kw):
    from insv2v.run_loveu_tgve import edit_video
    return edit_video(model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5, seed=SEED, unit=unit, **kw)


@pytest.fixture(scope="module")
def auto_edits(tiny_unet, tiny_model):
    """edit_video(mask="auto") of units a and b, computed once: (frames, estimate) per unit."""
    from insv2v.inference import InferenceIP2PVideo
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4, **EAGER)
    out = {}
    for unit, key in enumerate("ab"):
        img, est = _edit(tiny_model, pipe, _unit(key), unit, mask="auto", auto_mask=AUTO, return_mask=True)
        out[key] = (img.clone(), {k: v.clone() for k, v in est.items()})
    return pipe, out


def test_edit_video_auto_is_edit_video_with_that_mask(tiny_model, auto_edits):
    pipe, out = auto_edits
    u = _unit("a")
    img, est = out["a"]
    frac = float(est["mask_latent"].mean())
    print(f"[automask] edit_video: {frac:.3f} of the latent cells are edited")
    assert est["mask"].shape == (1, T_DRV, S_DRV, S_DRV) and 0.05 < frac < 0.95
    again = _edit(tiny_model, pipe, u, 0, mask=est["mask"])
    assert _same_bits(img, again), "mask=\"auto\" is not the edit with the mask it estimated"
    assert _same_bits(img, _edit(tiny_model, pipe, u, 0, mask=est["mask"], mask_mode="mean")), "mask_mode has an effect on an estimated mask"
    keep = (est["mask"].cpu() == 0.0)[:, :, None].expand_as(u["frames"])
    got = img.cpu()
    assert torch.equal(got[keep], u["frames"][keep]), "frames outside the estimated mask are not the input's"
    assert (got[~keep] - u["frames"][~keep]).abs().max() > 1e-2, "nothing was edited inside the mask"
    plain = _edit(tiny_model, pipe, u, 0)
    assert not torch.equal(plain.cpu()[keep], u["frames"][keep])   # without a mask the same pixels do change
    assert _edit(tiny_model, pipe, u, 0, return_mask=True)[1] is None


def test_edit_video_auto_with_an_instruction_that_changes_nothing(tiny_unet, tiny_model):
    """text_cond == text_uncond: branches 1 and 2 are the same computation, the map is zero, the mask empty - the output is the input."""
    from insv2v.inference import InferenceIP2PVideo
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4, **EAGER)
    u = _unit("a")
    u["text_cond"] = u["text_uncond"]
    img, est = _edit(tiny_model, pipe, u, 0, mask="auto", auto_mask=AUTO, return_mask=True)
    print(f"[automask] identical prompts: max raw {float(est['raw'].max()):.3e}")
    assert not est["raw"].any() and not est["mask"].any() and all(torch.isfinite(v).all() for v in est.values())
    assert torch.equal(img.cpu(), u["frames"].clip(-1, 1))


def test_edit_videos_with_auto_units(tiny_model, auto_edits):
    from insv2v.run_loveu_tgve import edit_videos
    pipe, alone = auto_edits
    ua, ub, uc = _unit("a"), _unit("b"), _unit("c")
    common = dict(text_cfg=7.5, video_cfg=1.5)
    units = [dict(ua, mask="auto", auto_mask=AUTO, unit=0, **common), dict(ub, mask="auto", auto_mask=AUTO, unit=1, **common), dict(uc, unit=2, **common)]
    outs = edit_videos(tiny_model, pipe, units, seed=SEED, return_mask=True)
    assert outs[2][1] is None
    for key, (img, est) in zip("ab", outs[:2]):
        rimg, rest = alone[key]
        assert all(_same_bits(est[k], rest[k]) for k in ("raw", "soft", "mask_latent", "mask")), f"unit {key}: the stacked driver estimated another mask"
        report(img, rimg.cpu(), f"edit_videos auto unit {key} frames vs edit_video", **STACKED)
        keep = (est["mask"].cpu() == 0.0)[:, :, None].expand_as(img)
        assert torch.equal(img.cpu()[keep], units["ab".index(key)]["frames"][keep])
    assert not _same_bits(outs[0][1]["mask_latent"], outs[1][1]["mask_latent"])   # each unit its own mask
    # the plain unit: bit for bit what it is next to the same two units carrying those masks as tensors, and within the stacked bound of alone
    given = [dict(ua, mask=alone["a"][1]["mask"], unit=0, **common), dict(ub, mask=alone["b"][1]["mask"], unit=1, **common), dict(uc, unit=2, **common)]
    ref = edit_videos(tiny_model, pipe, given, seed=SEED)
    assert all(_same_bits(o[0], r) for o, r in zip(outs, ref))
    report(outs[2][0], _edit(tiny_model, pipe, uc, 2).cpu(), "edit_videos plain unit next to two auto units vs edit_video", **STACKED)
