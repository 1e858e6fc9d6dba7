"""Seeded noise on the GPU: insv2v_randn against the numpy reference of the stream definition (tests/philox_ref.py; words bit for bit,
normals within the measured fp32 evaluation error), the fused forms (scheduler step, VAE posterior sample) bit for bit against
insv2v_randn + the unseeded kernel, and the invariances the seed buys at pipeline level on the tiny UNet / VAE."""
import numpy as np
import pytest
import torch

import philox_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SEED, STREAM, N20 = 0x0123456789ABCDEF, 7, 1 << 20
# max |fp32 kernel normal - float64 reference| over the 2^20 case as measured on an MI355X ("Seeded noise"); the bound is four
# times that - other seeds reach |z| = 5.9 against 5.1 in this sample and the error grows with r - and never looser than 2e-4.
MEASURED_MAX_ERR = 5.605e-7
NORMAL_TOL = min(4 * MEASURED_MAX_ERR, 2e-4)


def _cases():
    from insv2v.rng import stream_id, STEP
    return [(0, 0, 0, 4),                                                     # the first Random123 known answer
            (-1, 2 ** 63 - 1, 0, 4099),
            (SEED, STREAM, 3, 1021),                                          # a head of 1 and a ragged tail
            (5, stream_id(STEP, 2 ** 24 - 1, 4095, 65535), 2 ** 34 - 6, 16)]  # crosses the carry of the block index into its high word


def rel_rms(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()).item()


def report(out, ref, what, rms_tol, max_tol):
    """The measure of tests/test_model_gpu.py: rel-RMS and max-abs over max|ref|."""
    out, ref = out.detach().float().cpu(), ref.detach().float().cpu()
    assert out.shape == ref.shape
    rms = ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    mx = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"[seeded noise] {what}: rel-rms {rms:.3e}  max-abs/max-ref {mx:.3e}")
    assert np.isfinite(rms) and rms <= rms_tol and mx <= max_tol, f"{what}: rel-rms {rms:.3e} (tol {rms_tol}), max {mx:.3e} (tol {max_tol})"


@pytest.fixture(scope="module")
def ref20():
    return philox_ref.normals(SEED, STREAM, 0, N20)


# ------------------------------------------------------------------------------------------------------------------ insv2v_randn
@pytest.mark.parametrize("case", range(4))
def test_raw_words_equal_the_reference_bit_for_bit(case):
    from insv2v import ops
    seed, stream, offset, n = _cases()[case]
    got = ops.randn(n, seed, stream, offset=offset, raw=True, device=DEV)
    assert got.dtype == torch.int32 and got.shape == (n,)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), philox_ref.words(seed, stream, offset, n))
    if case == 0:
        assert ["%08x" % w for w in got.cpu().numpy().view(np.uint32)] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]


def test_sub_range_equals_the_same_range_of_a_longer_draw():
    from insv2v import ops
    whole = ops.randn(1000, SEED, STREAM, device=DEV)
    part = ops.randn(763, SEED, STREAM, offset=137, device=DEV)
    assert torch.equal(part, whole[137:900])
    # into caller memory at every 4-byte alignment: the vector store path and the element path write the same values
    buf = torch.zeros(1000 + 8, device=DEV)
    for shift in range(4):
        buf.zero_()
        ops.randn(buf[shift:shift + 763], SEED, STREAM, offset=137)
        assert torch.equal(buf[shift:shift + 763], whole[137:900]) and buf[:shift].abs().sum() == 0 and buf[shift + 763:].abs().sum() == 0
    assert torch.equal(ops.randn((2, 3, 5), SEED, STREAM, device=DEV).reshape(-1), whole[:30])


@pytest.mark.parametrize("case", range(4))
def test_normals_against_the_float64_reference(case):
    from insv2v import ops
    seed, stream, offset, n = _cases()[case]
    got = ops.randn(n, seed, stream, offset=offset, device=DEV).cpu().numpy().astype(np.float64)
    err = np.abs(got - philox_ref.normals(seed, stream, offset, n)).max()
    print(f"[seeded noise] case {case}: max |fp32 kernel - float64 reference| = {err:.3e} (bound {NORMAL_TOL:.1e})")
    assert err <= NORMAL_TOL


def test_normals_2p20_error_and_moments(ref20):
    from insv2v import ops
    got = ops.randn(N20, SEED, STREAM, device=DEV).cpu().numpy().astype(np.float64)
    err = np.abs(got - ref20)
    i = int(err.argmax())
    print(f"[seeded noise] 2^20 normals: max |fp32 kernel - float64 reference| = {err.max():.3e} at element {i} (z = {ref20[i]:.4f}), "
          f"rms {np.sqrt((err ** 2).mean()):.3e} (bound {NORMAL_TOL:.1e})")
    m = philox_ref.moments(got)
    print("[seeded noise] 2^20 normals: moments", m)
    assert err.max() <= NORMAL_TOL
    philox_ref.check_moments(got)


def test_randn_rejects_bad_arguments():
    from insv2v import ops, _lib
    lib = _lib.load()
    buf = torch.zeros(16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.insv2v_randn(None, 4, 0, 0, 0, 0, s) == -1
    assert lib.insv2v_randn(buf.data_ptr(), -1, 0, 0, 0, 0, s) == -1
    assert lib.insv2v_randn(buf.data_ptr(), 4, 0, 0, -4, 0, s) == -1
    assert lib.insv2v_randn(buf.data_ptr(), 4, 0, 0, 0, 2, s) == -1
    assert lib.insv2v_randn(buf.data_ptr(), 4, 0, 0, 2 ** 63 - 2, 0, s) == -1
    assert lib.insv2v_randn(buf.data_ptr() + 2, 4, 0, 0, 0, 0, s) == -1
    assert lib.insv2v_randn(buf.data_ptr(), 0, 0, 0, 0, 0, s) == 0
    torch.cuda.synchronize()
    assert buf.abs().sum() == 0
    with pytest.raises(_lib.HipKernelError):
        ops.randn(torch.zeros(4), 0, 0)


# ------------------------------------------------------------------------------------------------------------------ fused forms
@pytest.mark.parametrize("correct", [0, 1])
@pytest.mark.parametrize("strided", [False, True])
def test_seeded_cfg_step_equals_randn_plus_unseeded_step(strided, correct):
    """A DDPM step with c_noise != 0 at F, h, w = 3, 5, 7 (420 elements, h * w odd), three branches back to back or a branch stride apart."""
    from insv2v import ops, synth, _lib
    from insv2v.rng import stream_id, STEP
    from insv2v.schedulers import DDPMScheduler
    F, h, w = 3, 5, 7
    rows = F * h * w
    sch = DDPMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False)
    sch.set_timesteps(4)
    co = sch.coefficients(int(sch.timesteps[1]))
    assert co["coef"][3] != 0.0
    bstride = (rows + 11) * 4 if strided else 0
    eps = synth.synth_input("seeded.eps", (3 * (rows + 11) * 4,)).to(DEV)
    lat = synth.synth_input("seeded.lat", (F, 4, h, w)).to(DEV)
    ref = synth.synth_input("seeded.ref", (2, 4, h, w)).to(DEV) if correct else None
    seed, stream = 1234567, stream_id(STEP, 5, 1, 2)
    kw = dict(nbranch=3, text_cfg=7.5, img_cfg=1.5, sqrt_a=co["sqrt_a"], sqrt_1ma=co["sqrt_1ma"], coef=co["coef"], latent_ref=ref,
              correct=correct, branch_stride=bstride)
    outs = []
    for seeded in (False, True):
        new, pred = torch.zeros_like(lat), torch.zeros_like(lat)
        src = dict(noise_seed=seed, noise_stream=stream) if seeded else dict(noise=ops.randn(lat.shape, seed, stream, device=DEV))
        ops.cfg_step(eps, lat, latent_out=new, pred_x0=pred, **src, **kw)
        outs.append((new, pred))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    plain = torch.zeros_like(lat)
    ops.cfg_step(eps, lat, latent_out=plain, **kw)
    assert (plain - outs[0][0]).abs().max() > 1e-2, "the variance noise did not reach the step"
    with pytest.raises(_lib.HipKernelError, match="invalid argument"):   # one source of noise, never both
        ops.cfg_step(eps, lat, latent_out=plain, noise=torch.zeros_like(lat), noise_seed=seed, noise_stream=stream, **kw)


def test_seeded_posterior_sample_equals_the_explicit_noise_form():
    from insv2v import ops, synth
    from insv2v.rng import stream_id, ENC
    N, h, w = 5, 3, 5
    mom = synth.synth_input("seeded.moments", (N * h * w, 8)).to(DEV)
    seed, stream = -77, stream_id(ENC, 9)
    noise = ops.randn((N, 4, h, w), seed, stream, device=DEV)
    want = ops.posterior_sample(mom, noise, N, h, w, 0.18215)
    assert torch.equal(ops.posterior_sample(mom, None, N, h, w, 0.18215, seed=seed, stream=stream), want)
    # frames 2 ... 4 on their own, at their offset inside the video
    part = ops.posterior_sample(mom[2 * h * w:], None, 3, h, w, 0.18215, seed=seed, stream=stream, offset=2 * 4 * h * w)
    assert torch.equal(part, want[2:])


@pytest.fixture(scope="module")
def tiny_vae():
    from insv2v import synth, shapes
    from insv2v.vae import AutoencoderKL
    return AutoencoderKL(**synth.VAE_TINY, device=DEV).load_state_dict(synth.synth_state_dict(shapes.vae_shapes(**synth.VAE_TINY)))


def test_vae_encode_with_a_seed_does_not_depend_on_the_frame_chunking(tiny_vae, monkeypatch):
    from insv2v import synth
    x = synth.synth_input("seeded.vae.x", (5, 3, 32, 40), kind="uniform")
    whole = tiny_vae.encode(x, seed=11, unit=3).clone()
    assert whole.shape == (5, 4, 4, 5)
    monkeypatch.setattr(type(tiny_vae), "_frames_per_call", lambda self, H, W: 2)
    assert torch.equal(tiny_vae.encode(x, seed=11, unit=3), whole)
    # a video encoded in two calls, the second at its offset
    tail = tiny_vae.encode(x[2:], seed=11, unit=3, offset=2 * 4 * 4 * 5)
    assert torch.equal(tail, whole[2:])
    assert rel_rms(tiny_vae.encode(x, seed=11, unit=4), whole) > 0.1


# ------------------------------------------------------------------------------------------------------------------ pipeline
@pytest.fixture(scope="module")
def tiny_unet():
    from insv2v import synth, shapes
    from insv2v.unet import UNet3DConditionModel
    sd = synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_TINY))
    return UNet3DConditionModel(**synth.UNET_TINY, device=DEV).load_state_dict(sd)


def _clip(tag, F=4, h=8, w=8):
    from insv2v import synth
    return dict(latent=synth.synth_input(f"seeded.lat.{tag}", (1, F, 4, h, w)), img_cond=synth.synth_input(f"seeded.cond.{tag}", (1, F, 4, h, w)),
                text_cond=synth.synth_input(f"seeded.tc.{tag}", (1, 77, 64)), text_uncond=synth.synth_input("seeded.tu", (1, 77, 64)),
                text_cfg=7.5, img_cfg=1.5)


def test_same_seed_same_latent_other_seed_or_unit_another(tiny_unet):
    from insv2v.inference import InferenceIP2PVideo
    p = InferenceIP2PVideo(tiny_unet, scheduler="ddpm", num_ddim_steps=4)
    c = _clip(0)
    a = p(**c, seed=42)["latent"].clone()
    assert torch.isfinite(a).all()
    assert torch.equal(p(**c, seed=42)["latent"], a)
    assert rel_rms(p(**c, seed=43)["latent"], a) > 0.1
    assert rel_rms(p(**c, seed=42, unit=1)["latent"], a) > 0.1
    assert rel_rms(p(**c, seed=42, window=1)["latent"], a) > 0.1
    # an injected variance noise wins over the seed
    from insv2v import synth
    p.variance_noises = [synth.synth_input(f"seeded.var.{k}", (1, 4, 4, 8, 8)) for k in range(4)]
    inj = p(**c)["latent"].clone()
    assert torch.equal(p(**c, seed=42)["latent"], inj)


def test_run_stacked_units_match_each_unit_alone(tiny_unet):
    """Units 0, 1, 2 stacked into one launch chain against each unit alone, under the shipped stochastic sampler: the tolerance
    tests/test_model_gpu.py::test_run_stacked_matches_sequential asserts for injected noise (B = 9 launches may pick other tiles than B = 3)."""
    from insv2v.inference import InferenceIP2PVideo
    p = InferenceIP2PVideo(tiny_unet, scheduler="ddpm", num_ddim_steps=4, branch_streams=False)
    calls = [dict(_clip(j), seed=7, unit=j) for j in range(3)]
    alone = [p(**c)["latent"].clone() for c in calls]
    for j, (r, a) in enumerate(zip(p.run_stacked(calls), alone)):
        report(r["latent"], a, f"run_stacked unit {j} vs alone (ddpm, seed)", rms_tol=1e-2, max_tol=4e-2)
    # a batched __call__ numbers its entries unit, unit + 1, ...
    b = {k: torch.cat([c[k] for c in calls[1:]], 0) for k in ("latent", "img_cond", "text_cond", "text_uncond")}
    out = p(**b, text_cfg=7.5, img_cfg=1.5, seed=7, unit=1)["latent"]
    for j in (1, 2):
        report(out[j - 1:j], alone[j], f"batched __call__ entry of unit {j} vs alone", rms_tol=1e-2, max_tol=4e-2)


def test_edit_videos_does_not_depend_on_unit_order_or_company(tiny_unet, tiny_vae):
    """edit_videos([u0, u1, u2], seed) against edit_videos([u2, u0], seed) with the units carrying their ids: T = 20 frames = two windows,
    so the INIT / STEP streams of a second window are exercised; the tolerance of test_edit_videos_stacked_matches_edit_video.  (Without a
    seed the two calls differ by O(1) under DDPM: the draws come from one global stream in call order.)"""
    from insv2v import synth
    from insv2v.model import InstructP2PVideoModel
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.run_loveu_tgve import edit_videos, edit_video
    model = InstructP2PVideoModel(tiny_unet, tiny_vae)
    pipe = InferenceIP2PVideo(tiny_unet, scheduler="ddpm", num_ddim_steps=4)
    T, S = 20, 64
    tu = synth.synth_input("seeded.ev.tu", (1, 77, 64))
    u = [dict(frames=synth.synth_input(f"seeded.ev.frames.{j}", (1, T, 3, S, S), kind="uniform"),
              text_cond=synth.synth_input(f"seeded.ev.tc.{j}", (1, 77, 64)), text_uncond=tu, text_cfg=7.5, video_cfg=1.5) for j in range(3)]
    full = edit_videos(model, pipe, u, return_latent=True, seed=99)
    part = edit_videos(model, pipe, [{**u[2], "unit": 2}, {**u[0], "unit": 0}], return_latent=True, seed=99)
    for (img, lat), (rimg, rlat), j in ((part[0], full[2], 2), (part[1], full[0], 0)):
        assert img.shape == u[j]["frames"].shape
        report(lat, rlat, f"edit_videos unit {j} latent, other order and company", rms_tol=1e-2, max_tol=5e-2)
        report(img, rimg, f"edit_videos unit {j} frames, other order and company", rms_tol=1e-2, max_tol=5e-2)
    one = edit_video(model, pipe, u[1]["frames"], u[1]["text_cond"], tu, 7.5, 1.5, return_latent=True, seed=99, unit=1)
    report(one[1], full[1][1], "edit_video unit 1 latent vs edit_videos", rms_tol=1e-2, max_tol=5e-2)
    assert rel_rms(full[0][1], full[1][1]) > 0.1


def test_a_seed_does_not_leak_into_a_deterministic_sampler(tiny_unet, tiny_vae):
    from insv2v import synth
    from insv2v.model import InstructP2PVideoModel
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.run_loveu_tgve import edit_video
    model = InstructP2PVideoModel(tiny_unet, tiny_vae)
    pipe = InferenceIP2PVideo(tiny_unet, scheduler="ddim", num_ddim_steps=4)
    T, S = 20, 64
    frames = synth.synth_input("seeded.ddim.frames", (1, T, 3, S, S), kind="uniform")
    tc, tu = synth.synth_input("seeded.ddim.tc", (1, 77, 64)), synth.synth_input("seeded.ddim.tu", (1, 77, 64))
    inj = dict(init_noises=[synth.synth_input(f"seeded.ddim.n{k}", (1, n, 4, S // 8, S // 8)) for k, n in enumerate((16, 4))],
               enc_noise=synth.synth_input("seeded.ddim.enc", (1, T, 4, S // 8, S // 8)), return_latent=True)
    plain = edit_video(model, pipe, frames, tc, tu, 7.5, 1.5, **inj)
    seeded = edit_video(model, pipe, frames, tc, tu, 7.5, 1.5, seed=5, unit=2, **inj)
    assert torch.equal(plain[1], seeded[1]) and torch.equal(plain[0], seeded[0])
