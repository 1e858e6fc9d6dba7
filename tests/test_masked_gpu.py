"""Masked and partial edits on the GPU: insv2v_cfg_step_mask against the float64 restatement (tests/masked_ref.py) and its bit-exact
properties, the mask reduction / composite / re-noising kernels, the pipelines on the tiny UNet against the CPU oracle's loops stepping
with the float64 restatement, and the drivers' ``mask`` / ``strength`` controls.

Bounds are the project's: kernel level 1e-5 * max|ref| against float64 (``close`` of tests/test_multistep_gpu.py); trajectories ``TRAJ``
(rel-RMS 3e-2 / max 1e-1); stacked against alone rel-RMS 1e-2 / max 4e-2 (``report``'s defaults)."""
import ctypes

import numpy as np
import pytest
import torch

import masked_ref as kr
import philox_ref
from test_model_gpu import tiny_unet, _pipe_inputs, report   # noqa: F401  (tiny_unet: the module-scoped fixture, instantiated for this module)
from test_multistep_gpu import close, f32, _step_ref64, _stack_calls, _alone, _flows, TRAJ

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, H, W = 3, 5, 7   # odd on purpose; 4 * H * W = 140 > one 128-thread block, so the tail block runs
STACKED = dict(rms_tol=1e-2, max_tol=4e-2)


def _rnd(key, shape, kind="normal"):
    from insv2v import synth
    return synth.synth_input(f"masked.{key}", tuple(shape), kind=kind).to(DEV)


def _soft_mask(key, shape):
    """Values in [0,1] with exact zeros and ones among them (about a quarter each)."""
    return (_rnd(key, shape, "uniform") * 1.0 + 0.5).clamp(0.0, 1.0).contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ kernel level
def _operands(nbranch, R):
    lat, hist, noise = _rnd("lat", (F, 4, H, W)), _rnd("hist", (F, 4, H, W)), _rnd("noise", (F, 4, H, W))
    ref, dq = _rnd(f"ref{R}", (R, 4, H, W)), _rnd(f"dq{R}", (F - R, 4, H, W))
    e = _rnd("eps3", (3, F, 4, H, W)) if nbranch == 3 else _rnd("eps0", (F, 4, H, W))
    eps_in = e.permute(0, 1, 3, 4, 2).contiguous() if nbranch == 3 else e
    mask, src, kn = _soft_mask("mask", (F, H, W)), _rnd("src", (F, 4, H, W)), _rnd("kn", (F, 4, H, W))
    return dict(lat=lat, hist=hist, noise=noise, ref=ref, dq=dq, e=e, eps_in=eps_in, mask=mask, src=src, kn=kn)


COEF = (f32(0.83), f32(0.05), f32(0.41), f32(0.3))
SA, S1 = f32(0.8), f32(0.6)
KS, KN = f32(0.93), f32(0.37)
TC, IC = 7.5, 1.5


def _ref64(o, *, nbranch, correct, c_hist, noise, coef=COEF, mask=True):
    """Float64: the step of test_multistep_gpu._step_ref64, then the blend of masked_ref."""
    zeros = torch.zeros_like(o["lat"])
    we, wx0, wprev = _step_ref64(o["e"], o["lat"], nbranch=nbranch, tc=TC, ic=IC, sa=SA, s1=S1, coef=coef, c_hist=c_hist,
                                 hist=o["hist"] if c_hist != 0.0 else zeros, noise=zeros if noise is None else noise, gr=0.0,
                                 correct=correct, ref=o["ref"], dq=o["dq"])
    if mask:
        wprev = kr.blend(wprev, o["src"].double().cpu(), o["kn"].double().cpu(), o["mask"].double().cpu(), KS, KN)
    return we, wx0, wprev


def _launch(o, *, nbranch, correct, c_hist, masked=True, eps_in=None, **more):
    from insv2v import ops
    new, pred, eo = (torch.zeros_like(o["lat"]) for _ in range(3))
    kw = dict(nbranch=nbranch, text_cfg=TC, img_cfg=IC, sqrt_a=SA, sqrt_1ma=S1, coef=COEF, latent_out=new, pred_x0=pred, eps_out=eo,
              latent_ref=o["ref"] if correct else None, correct=correct, delta_q=o["dq"] if correct == 2 else None)
    if c_hist != 0.0:
        kw.update(x0_hist=o["hist"], c_hist=c_hist)
    if masked:
        kw.update(mask=o["mask"], src=o["src"], known_noise=o["kn"], k_src=KS, k_noise=KN)
    kw.update(more)
    ops.cfg_step(o["eps_in"] if eps_in is None else eps_in, o["lat"], **kw)
    return new, pred, eo


@pytest.mark.parametrize("hist", [True, False])
@pytest.mark.parametrize("correct", [0, 1, 2])
@pytest.mark.parametrize("nbranch", [3, 0])
def test_cfg_step_mask_vs_float64(nbranch, correct, hist):
    """All terms of the update present (injected variance noise), a soft random mask, R = 1 and 2 reference frames."""
    c_hist = f32(-0.37) if hist else 0.0
    for R in ((1, 2) if correct else (1,)):
        o = _operands(nbranch, R)
        new, pred, eo = _launch(o, nbranch=nbranch, correct=correct, c_hist=c_hist, noise=o["noise"])
        we, wx0, wprev = _ref64(o, nbranch=nbranch, correct=correct, c_hist=c_hist, noise=o["noise"])
        tag = f"cfg_step_mask nbranch={nbranch} correct={correct} R={R} hist={int(hist)}"
        close(eo, we, tag + " eps")
        close(pred, wx0, tag + " x0")
        close(new, wprev, tag + " latent")
        # the blend reached the output, and only latent_out: pred_x0 / eps_out are bit for bit those of the unmasked call.  (The masked
        # kernel is a separate instantiation of the step body: this equality holds while the compiler contracts the multiply-adds in
        # front of the blend alike in both - which is why mask == NULL dispatches to the unmasked kernels instead of branching at run time.)
        plain = _launch(o, nbranch=nbranch, correct=correct, c_hist=c_hist, noise=o["noise"], masked=False)
        assert (new - plain[0]).abs().max() > 0.1, tag + ": the mask did not reach the output"
        assert torch.equal(pred, plain[1]) and torch.equal(eo, plain[2]), tag + ": pred_x0 / eps_out differ from the unmasked call's"
        one = o["mask"] == 1.0
        assert one.any() and torch.equal(new[one[:, None].expand_as(new)], plain[0][one[:, None].expand_as(new)])   # m == 1: prev itself


@pytest.mark.parametrize("source", ["injected", "seeded", "none"])
def test_cfg_step_mask_variance_noise_sources(source):
    from insv2v import ops
    from insv2v.rng import stream_id, STEP
    o = _operands(3, 2)
    seed, stream = 20240607, stream_id(STEP, 3, 1, 4)
    n = F * 4 * H * W
    if source == "injected":
        more, noise = dict(noise=o["noise"]), o["noise"]
    elif source == "seeded":   # element li of the stream, float64 reference of the stream definition
        more, noise = dict(noise_seed=seed, noise_stream=stream), torch.from_numpy(philox_ref.normals(seed, stream, 0, n)).reshape(F, 4, H, W)
    else:
        more, noise = {}, None
    c_hist = f32(0.21)
    new, pred, eo = _launch(o, nbranch=3, correct=1, c_hist=c_hist, **more)
    we, wx0, wprev = _ref64(o, nbranch=3, correct=1, c_hist=c_hist, noise=noise)
    close(eo, we, f"cfg_step_mask noise={source} eps")
    close(pred, wx0, f"cfg_step_mask noise={source} x0")
    close(new, wprev, f"cfg_step_mask noise={source} latent")
    if source == "seeded":   # ... and bit for bit the same stream passed as a tensor
        drawn = ops.randn((F, 4, H, W), seed, stream, device=DEV)
        again = _launch(o, nbranch=3, correct=1, c_hist=c_hist, noise=drawn)
        assert all(torch.equal(a, b) for a, b in zip((new, pred, eo), again))


def test_cfg_step_mask_branch_stride_inside_sentinel_buffers():
    """Branch-major stacked eps (clip 1 of 2) and every operand carved out of a sentinel-filled buffer: inputs sit between NaNs (a read
    outside an operand poisons the result), outputs between a finite sentinel that must survive."""
    from insv2v import ops
    o = _operands(3, 2)
    rows1, pad = F * H * W, 37

    def carve(t, fill):
        buf = torch.full((t.numel() + 2 * pad,), fill, device=DEV, dtype=torch.float32)
        buf[pad:pad + t.numel()] = t.reshape(-1)
        return buf, buf[pad:pad + t.numel()].view(t.shape)

    nan = float("nan")
    ins = {k: carve(o[k], nan) for k in ("lat", "hist", "noise", "ref", "mask", "src", "kn")}
    big = torch.full((3, 2, rows1 * 4), nan, device=DEV)
    big[:, 1] = o["eps_in"].reshape(3, -1)
    eps_in, bstride = big.reshape(-1)[rows1 * 4:], 2 * rows1 * 4
    outs = [carve(torch.zeros_like(o["lat"]), 12345.0) for _ in range(3)]
    c_hist = f32(-0.37)
    ops.cfg_step(eps_in, ins["lat"][1], nbranch=3, text_cfg=TC, img_cfg=IC, sqrt_a=SA, sqrt_1ma=S1, coef=COEF, latent_out=outs[0][1],
                 pred_x0=outs[1][1], eps_out=outs[2][1], latent_ref=ins["ref"][1], correct=1, noise=ins["noise"][1], branch_stride=bstride,
                 x0_hist=ins["hist"][1], c_hist=c_hist, mask=ins["mask"][1], src=ins["src"][1], known_noise=ins["kn"][1], k_src=KS, k_noise=KN)
    torch.cuda.synchronize()
    we, wx0, wprev = _ref64(o, nbranch=3, correct=1, c_hist=c_hist, noise=o["noise"])
    close(outs[2][1], we, "cfg_step_mask strided eps")
    close(outs[1][1], wx0, "cfg_step_mask strided x0")
    close(outs[0][1], wprev, "cfg_step_mask strided latent")
    for buf, view in outs:
        assert (buf[:pad] == 12345.0).all() and (buf[pad + view.numel():] == 12345.0).all(), "a write outside an output"
    for k, (buf, view) in ins.items():
        assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + view.numel():]).all() and torch.equal(view, o[k]), f"input {k} was written"
    assert torch.isnan(big[:, 0]).all() and torch.equal(big[:, 1], o["eps_in"].reshape(3, -1))


def test_cfg_step_mask_bit_exact_properties():
    from insv2v import ops
    o = _operands(3, 2)
    c_hist = f32(-0.37)
    # where m == 0, latent_out does not depend on the model's prediction: two different eps_in, the same bits
    a = _launch(o, nbranch=3, correct=1, c_hist=c_hist, noise=o["noise"])
    other = (o["eps_in"] * -1.7 + 0.3).contiguous()
    b = _launch(o, nbranch=3, correct=1, c_hist=c_hist, noise=o["noise"], eps_in=other)
    zero = (o["mask"] == 0.0)[:, None].expand_as(a[0])
    assert zero.any() and torch.equal(_bits(a[0][zero]), _bits(b[0][zero]))
    assert (a[0] - b[0])[~zero].abs().max() > 0.1 and (a[1] - b[1]).abs().max() > 0.1
    known = KS * o["src"].double() + KN * o["kn"].double()
    close(a[0][zero], known[zero].cpu(), "latent_out where m == 0 vs k_src z + k_noise n")
    # mask=None through the new keywords == the call without them (the same kernels), with and without a history, all noise sources
    for hist in (c_hist, 0.0):
        for src in (dict(noise=o["noise"]), dict(noise_seed=11, noise_stream=5), dict()):
            x = _launch(o, nbranch=3, correct=1, c_hist=hist, masked=False, **src)
            y = _launch(o, nbranch=3, correct=1, c_hist=hist, masked=False, **src, mask=None, src=None, known_noise=None, k_src=0.0, k_noise=0.0)
            new, pred, eo = (torch.zeros_like(o["lat"]) for _ in range(3))
            ops.cfg_step_mask(o["eps_in"], o["lat"], mask=None, src=o["src"], known_noise=o["kn"], k_src=KS, k_noise=KN, nbranch=3, text_cfg=TC,
                              img_cfg=IC, sqrt_a=SA, sqrt_1ma=S1, coef=COEF, latent_out=new, pred_x0=pred, eps_out=eo, latent_ref=o["ref"],
                              correct=1, **(dict(x0_hist=o["hist"], c_hist=hist) if hist != 0.0 else {}), **src)
            assert all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in zip(x, y, (new, pred, eo))), (hist, sorted(src))


def test_cfg_step_mask_refusals():
    from insv2v import ops, _lib
    o = _operands(3, 2)
    out = torch.zeros_like(o["lat"])
    base = dict(nbranch=3, text_cfg=TC, img_cfg=IC, sqrt_a=SA, sqrt_1ma=S1, coef=COEF, k_src=KS, k_noise=KN)
    full = dict(mask=o["mask"], src=o["src"], known_noise=o["kn"])
    bad = "invalid argument"
    with pytest.raises(_lib.HipKernelError, match=bad):
        ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, mask=o["mask"], src=o["src"], **base)
    with pytest.raises(_lib.HipKernelError, match=bad):
        ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, mask=o["mask"], known_noise=o["kn"], **base)
    with pytest.raises(_lib.HipKernelError, match=bad):                     # a mask blends latent_out: eps_out alone is refused
        ops.cfg_step(o["eps_in"], o["lat"], eps_out=out, **full, **base)
    with pytest.raises(_lib.HipKernelError, match="need a mask"):
        ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, src=o["src"], known_noise=o["kn"], **base)
    # an input that overlaps an output range
    buf = torch.zeros(2 * out.numel(), device=DEV)
    outv = buf[:out.numel()].view(out.shape)
    inside4 = buf[8:8 + out.numel()].view(out.shape)
    inside_m = buf[out.numel() - 4:out.numel() - 4 + F * H * W].view(F, H, W)
    for which in ("latent_out", "pred_x0", "eps_out"):
        outs = {"latent_out": out, which: outv}
        for name, t in (("mask", inside_m), ("src", inside4), ("known_noise", inside4)):
            with pytest.raises(_lib.HipKernelError, match=bad):
                ops.cfg_step(o["eps_in"], o["lat"], **outs, **dict(full, **{name: t}), **base)
        with pytest.raises(_lib.HipKernelError, match=bad):
            ops.cfg_step(o["eps_in"], o["lat"], **outs, x0_hist=inside4, c_hist=0.5, **full, **base)
    with pytest.raises(_lib.HipKernelError):                                 # wrong shapes never reach the kernel
        ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, **dict(full, mask=o["mask"][:2]), **base)
    with pytest.raises(_lib.HipKernelError):
        ops.cfg_step(o["eps_in"], o["lat"], latent_out=out, **dict(full, src=o["src"][:, :3]), **base)
    # F, h, w non-positive: not expressible through ops (they come from the latent's shape) - the entry itself
    lib = _lib.load()
    for k in ("F", "h", "w"):
        d = _lib.MaskStepDesc()
        d.eps_in, d.latent, d.latent_out = o["eps_in"].data_ptr(), o["lat"].data_ptr(), out.data_ptr()
        d.mask, d.src, d.known_noise = o["mask"].data_ptr(), o["src"].data_ptr(), o["kn"].data_ptr()
        d.nbranch, d.F, d.h, d.w, d.sqrt_a, d.sqrt_1ma = 3, F, H, W, SA, S1
        setattr(d, k, 0)
        assert lib.insv2v_cfg_step_mask(ctypes.byref(d), None) == -1
    torch.cuda.synchronize()
    assert out.abs().sum() == 0 and buf.abs().sum() == 0


def _np_reduce(m, mode):
    n, hh, ww = m.shape
    cells = m.reshape(n, hh // 8, 8, ww // 8, 8)
    return cells.max(axis=(2, 4)) if mode == "max" else cells.astype(np.float64).mean(axis=(2, 4))


@pytest.mark.parametrize("N,HH,WW", [(3, 24, 40), (1, 8, 8)])
def test_mask_to_latent(N, HH, WW):
    """Binary masks: exact in both modes (sums of at most 64 ones and the division by 64 are exact in fp32).  A soft mask, mode "mean":
    within 1e-6 absolute of the float64 mean.  Derivation: the kernel adds the 64 fp32 values of a cell pairwise - 6 levels - so every
    value passes through 6 roundings of relative size u = 2^-24 and the sum of nonnegative terms carries a relative error of at most
    (1 + u)^6 - 1 < 6.1 u; the multiplication by 1/64 is exact; the mean of values in [0,1] is at most 1, so the absolute error is
    below 6.1 * 2^-24 = 3.7e-7 < 1e-6.  "max" picks one of the inputs: exact for any mask."""
    from insv2v import ops, _lib
    binary = (_rnd(f"m2l.bin.{HH}", (N, HH, WW), "uniform") > 0.6).float()
    binary[0, :8, :8] = 0.0          # an empty cell, a full cell, a cell with a single pixel
    if HH > 8:
        binary[0, 8:16, 8:16] = 1.0
        binary[0, 16:24, 32:40] = 0.0
        binary[0, 23, 39] = 1.0
    soft = _rnd(f"m2l.soft.{HH}", (N, HH, WW), "uniform").abs().contiguous()
    for mode in ("mean", "max"):
        got = ops.mask_to_latent(binary, mode)
        assert got.shape == (N, HH // 8, WW // 8) and got.dtype == torch.float32
        assert np.array_equal(got.cpu().numpy().astype(np.float64), _np_reduce(binary.cpu().numpy(), mode).astype(np.float64)), mode
        got = ops.mask_to_latent(soft, mode).cpu().numpy().astype(np.float64)
        err = np.abs(got - _np_reduce(soft.cpu().numpy(), mode)).max()
        print(f"[parity] mask_to_latent {mode} soft {N}x{HH}x{WW}: max-abs err {err:.3e}")
        assert err <= (1e-6 if mode == "mean" else 0.0)
    assert ops.mask_to_latent(binary[None], "max").shape == (1, N, HH // 8, WW // 8)   # leading dimensions are kept
    for shape in ((1, 12, 8), (1, 8, 20), (2, 7, 7)):
        with pytest.raises(_lib.HipKernelError, match="invalid argument"):
            ops.mask_to_latent(torch.zeros(shape, device=DEV), "mean")
    with pytest.raises(_lib.HipKernelError):
        ops.mask_to_latent(torch.zeros((1, 8, 8)), "mean")   # not on the GPU: no fallback


def test_composite_exact_where_binary_and_out_may_be_edited():
    """m in {0, 1}: the clipped original / edited frame, bit for bit (0 * x = 0 and 1 * x = x are exact).  Elsewhere within 1e-6 of
    float64: |edited|, |original| <= 1.5, so 1 - m, the two products and the sum carry at most 4 roundings of at most 1.5 * 2^-24 each
    = 3.6e-7."""
    from insv2v import ops, _lib
    N, HH, WW = 2, 24, 40
    edited, orig = _rnd("comp.e", (N, 3, HH, WW), "uniform") * 1.5, _rnd("comp.o", (N, 3, HH, WW), "uniform") * 1.5
    m = _soft_mask("comp.m", (N, HH, WW))
    want = (m.double()[:, None] * edited.double() + (1 - m.double()[:, None]) * orig.double()).clamp(-1, 1).cpu()
    e_clip, o_clip = edited.clamp(-1, 1), orig.clamp(-1, 1)
    fresh = ops.composite(edited, orig, m)
    inplace = edited.clone()
    assert ops.composite(inplace, orig, m, out=inplace) is inplace and torch.equal(inplace, fresh)
    one, zero = (m == 1.0)[:, None].expand_as(fresh), (m == 0.0)[:, None].expand_as(fresh)
    assert one.any() and zero.any() and (~(one | zero)).any()
    assert torch.equal(fresh[one], e_clip[one]) and torch.equal(fresh[zero], o_clip[zero])
    err = (fresh.double().cpu() - want).abs().max().item()
    print(f"[parity] composite: max-abs err {err:.3e}")
    assert err <= 1e-6 and fresh.abs().max() <= 1.0 and (want.abs() == 1.0).any()
    with pytest.raises(_lib.HipKernelError):
        ops.composite(edited, orig, m[:, :8])
    with pytest.raises(_lib.HipKernelError):
        ops.composite(edited[:, :2], orig[:, :2], m)


def test_add_noise_vs_float64():
    from insv2v import ops
    z, n = _rnd("an.z", (F, 4, H, W)), _rnd("an.n", (F, 4, H, W))
    ka, kb = f32(0.6123), f32(0.7906)
    got = ops.add_noise(z, n, ka, kb)
    assert got.shape == z.shape
    close(got, ka * z.double().cpu() + kb * n.double().cpu(), "add_noise")
    big = _rnd("an.big", (3, 1031))                                     # several blocks and a ragged tail
    close(ops.add_noise(big, big.flip(0).contiguous(), ka, kb), ka * big.double().cpu() + kb * big.flip(0).double().cpu(), "add_noise 3x1031")


# ------------------------------------------------------------------------------------------------------------------ pipelines
@pytest.fixture(scope="module")
def oracle_unet(tiny_unet):
    import oracle.unet3d as ou
    from insv2v import synth
    o = ou.UNet3DConditionModel(**synth.UNET_TINY).eval()
    o.load_state_dict(tiny_unet[1])
    return o


def _known(i, key="a"):
    from insv2v import synth
    shape = (1, i["F"], 4, i["h"], i["w"])
    m = (synth.synth_input(f"masked.pipe.mask.{key}", (1, i["F"], i["h"], i["w"]), kind="uniform") + 0.5).clamp(0.0, 1.0)
    return dict(mask=m, source_latent=synth.synth_input(f"masked.pipe.z.{key}", shape), known_noise=i["lat"])


def _kept_is_known(latent, k, kind, n_steps, what):
    """Outside the mask the final latent is k_src z + k_noise n of the last step (kernel bound)."""
    k_src, k_noise = kr.known_coefficients(kind, n_steps, kr.timesteps(kind, n_steps)[-1])
    zero = (k["mask"] == 0.0)[:, :, None].expand_as(latent)
    assert zero.any()
    want = k_src * k["source_latent"].double() + k_noise * k["known_noise"].double()
    close(latent.cpu()[zero], want[zero], what + ": latent outside the mask vs k_src z + k_noise n")


@pytest.mark.parametrize("kind", ["ddim", "dpmsolver++"])
@pytest.mark.parametrize("case", ["call", "second_clip", "flow", "strength_0.5"])
def test_masked_pipelines_vs_oracle_driven_restatement(tiny_unet, oracle_unet, case, kind):
    """10 steps: the product pipe against the CPU oracle's loop (fp32 UNet) stepping with the float64 restatement of masked_ref."""
    import oracle.pipelines as op
    from insv2v import ops
    from insv2v.inference import InferenceIP2PVideo, InferenceIP2PVideoOpticalFlow
    unet, _ = tiny_unet
    i = _pipe_inputs()
    k = _known(i)
    flow = case == "flow"
    p = (InferenceIP2PVideoOpticalFlow if flow else InferenceIP2PVideo)(unet, scheduler=kind, num_ddim_steps=10)
    o = (op.InferenceIP2PVideoOpticalFlow if flow else op.InferenceIP2PVideo)(oracle_unet, scheduler="ddim", num_ddim_steps=10)
    o.scheduler = kr.MaskedScheduler(kind, 10, k["source_latent"], k["known_noise"], k["mask"])
    g = dict(text_cfg=7.5, img_cfg=1.5)
    if case == "call":
        r, w = p(i["lat"], i["tc"], i["tu"], i["cond"], **g, **k), o(i["lat"], i["tc"], i["tu"], i["cond"], **g)
    elif case == "strength_0.5":
        from insv2v.schedulers import strength_to_start
        n_exec, st = strength_to_start(0.5, 10)
        assert (n_exec, st) == (5, 5)
        st64, x64 = kr.start_latent(kind, 10, 0.5, k["source_latent"].double(), k["known_noise"].double())
        start = ops.add_noise(k["source_latent"].to(DEV), k["known_noise"].to(DEV), *p.scheduler.start_coefficients(int(p.scheduler.timesteps[st])))
        close(start, x64, f"masked {kind} strength 0.5: start latent")
        r = p(start, i["tc"], i["tu"], i["cond"], start_time=st, **g, **k)
        w = o(x64.float(), i["tc"], i["tu"], i["cond"], start_time=st64, **g)
        assert len(r["all_latent"]) == 5
    elif case == "second_clip":
        c = dict(latent_ref=i["lref"], noise_correct_step=0.5, **g)
        r = p.second_clip_forward(i["lat"], i["tc"], i["tu"], i["cond"], **c, **k)
        w = o.second_clip_forward(i["lat"], i["tc"], i["tu"], i["cond"], **c)
    else:
        c = dict(latent_ref=i["lref"], flows=_flows(i), noise_correct_step=0.5, **g)
        r = p.second_clip_forward(i["lat"], i["tc"], i["tu"], i["cond"], **c, **k)
        w = o.second_clip_forward(i["lat"], i["tc"], i["tu"], i["cond"], **c)
    assert len(r["all_latent"]) == len(w["all_latent"]) == len(r["all_pred"])
    report(r["all_pred"][1], w["all_pred"][1], f"masked {kind} {case}: x0 of the second executed step", **TRAJ)
    report(r["latent"], w["latent"], f"masked {kind} {case}: final latent", **TRAJ)
    _kept_is_known(r["latent"], k, kind, 10, f"masked {kind} {case}")


def test_masked_ddpm_injected_noise_vs_oracle_driven_restatement(tiny_unet, oracle_unet):
    import oracle.pipelines as op
    from insv2v import synth
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    i = _pipe_inputs()
    k = _known(i)
    noises = [synth.synth_input(f"masked.var.{j}", tuple(i["lat"].shape)) for j in range(3)] + [None]
    p = InferenceIP2PVideo(unet, scheduler="ddpm", num_ddim_steps=4)
    p.variance_noises = noises
    o = op.InferenceIP2PVideo(oracle_unet, scheduler="ddim", num_ddim_steps=4)
    o.scheduler = kr.MaskedScheduler("ddpm", 4, k["source_latent"], k["known_noise"], k["mask"], noises=noises)
    a = (i["lat"], i["tc"], i["tu"], i["cond"])
    r, w = p(*a, text_cfg=7.5, img_cfg=1.5, **k), o(*a, text_cfg=7.5, img_cfg=1.5)
    report(r["all_latent"][0], w["all_latent"][0], "masked ddpm: latent after the first step", **TRAJ)
    report(r["latent"], w["latent"], "masked ddpm, injected noise: final latent", **TRAJ)
    zero = (k["mask"] == 0.0)[:, :, None].expand_as(r["latent"])
    assert torch.equal(r["latent"].cpu()[zero], k["source_latent"][zero])   # DDPM's end point is alpha_bar = 1: (k_src, k_noise) = (1, 0)


def _masked_stack_calls(i):
    a, b = _stack_calls(i)
    ka, kb = _known(i, "a"), _known(i, "b")
    kb["known_noise"] = b["latent"]
    return [dict(a, **ka), b, dict(b, **kb)]   # masked call, unmasked second clip, masked second clip


def test_run_stacked_and_run_concurrent_with_masked_and_unmasked_clips(tiny_unet):
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    calls = _masked_stack_calls(_pipe_inputs())
    p = InferenceIP2PVideo(unet, scheduler="dpmsolver++", num_ddim_steps=4, branch_streams=False)
    seq = [_alone(p, c) for c in calls]
    assert (seq[1]["latent"] - seq[2]["latent"]).abs().max() > 0.1   # the mask matters
    res = p.run_stacked(calls)
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(seq, res)):
        assert len(b["all_latent"]) == 4 and len(b["all_pred"]) == 4
        report(b["latent"], a["latent"], f"masked run_stacked clip {j} vs alone", **STACKED)
        report(b["all_pred"][-1], a["all_pred"][-1], f"masked run_stacked clip {j} last x0", **STACKED)
    pc = InferenceIP2PVideo(unet, scheduler="dpmsolver++", num_ddim_steps=4)
    seq = [_alone(pc, c)["latent"].clone() for c in calls]
    res = pc.run_concurrent(calls)
    torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(seq, res)):
        report(b["latent"], a, f"masked run_concurrent clip {j} vs alone", **STACKED)
    # a batched call slices mask / source_latent / known_noise per entry
    two = [calls[0], dict(calls[0], latent=calls[2]["latent"], **{k: calls[2][k] for k in ("mask", "source_latent", "known_noise")})]
    alone = [_alone(p, c)["latent"] for c in two]
    cat = {k: torch.cat([c[k] for c in two], 0) for k in ("latent", "text_cond", "text_uncond", "img_cond", "mask", "source_latent", "known_noise")}
    out = p(**cat, text_cfg=7.5, img_cfg=1.5, guidance_rescale=0.5)["latent"]
    for j in range(2):
        report(out[j:j + 1], alone[j], f"masked batched __call__ entry {j} vs alone", **STACKED)


def test_sde_seeded_masked_unit_alone_and_stacked(tiny_unet):
    """A seeded masked unit is reproducible bit for bit, alone and inside a stack, in either order of the stack; and where the mask is
    0 its latent is bit for bit the same alone and stacked (it does not depend on the UNet).  Elsewhere a stack runs other UNet kernels
    than a single clip, so alone against stacked holds within the stacked bound, as for every stacked test of the project."""
    from insv2v.inference import InferenceIP2PVideo
    unet, _ = tiny_unet
    p = InferenceIP2PVideo(unet, scheduler="sde-dpmsolver++", num_ddim_steps=4, branch_streams=False)
    calls = [dict(c, seed=7, unit=j) for j, c in enumerate(_masked_stack_calls(_pipe_inputs()))]
    alone = [_alone(p, c)["latent"].clone() for c in calls]
    for c, a in zip(calls, alone):
        assert torch.equal(_alone(p, c)["latent"], a)
    d = (_alone(p, calls[0], seed=8)["latent"] - alone[0]).pow(2).mean().sqrt() / alone[0].pow(2).mean().sqrt()
    assert d > 0.02, "another seed gave the same latent"
    first = None
    for order in (calls, calls[::-1], calls):
        res = {c["unit"]: r["latent"].clone() for c, r in zip(order, p.run_stacked(order))}
        for u, lat in res.items():
            report(lat, alone[u], f"seeded masked sde-dpmsolver++ run_stacked unit {u} vs alone", **STACKED)
            if "mask" in calls[u]:
                zero = (calls[u]["mask"] == 0.0)[:, :, None].expand_as(lat)
                assert torch.equal(lat.cpu()[zero], alone[u].cpu()[zero])
        if first is None:
            first = res
        elif order is calls:
            assert all(torch.equal(res[u], first[u]) for u in res)   # the same stack again: bit for bit


# ------------------------------------------------------------------------------------------------------------------ drivers
@pytest.fixture(scope="module")
def tiny_model(tiny_unet):
    from insv2v import synth, shapes
    from insv2v.vae import AutoencoderKL
    from insv2v.model import InstructP2PVideoModel
    vae = AutoencoderKL(**synth.VAE_TINY, device=DEV).load_state_dict(synth.synth_state_dict(shapes.vae_shapes(**synth.VAE_TINY)))
    return InstructP2PVideoModel(tiny_unet[0], vae)


T, S, NEWS = 10, 64, (6, 4)   # two windows of 6 frames, the second re-using 2
WIN = dict(frames_in_batch=6, num_ref_frames=2)


def _unit(key):
    from insv2v import synth
    return dict(frames=synth.synth_input(f"masked.ev.frames.{key}", (1, T, 3, S, S), kind="uniform"),
                text_cond=synth.synth_input(f"masked.ev.tc.{key}", (1, 77, 64)), text_uncond=synth.synth_input("masked.ev.tu", (1, 77, 64)),
                enc_noise=synth.synth_input(f"masked.ev.enc.{key}", (1, T, 4, S // 8, S // 8)),
                init_noises=[synth.synth_input(f"masked.ev.n.{key}.{j}", (1, n, 4, S // 8, S // 8)) for j, n in enumerate(NEWS)])


def _image_mask():
    m = torch.zeros((1, T, S, S))
    m[:, :, 13:41, 10:45] = 1.0       # not aligned to the 8x8 cells: "max" edits every cell the rectangle touches
    m[:, 7:] = 0.0                    # and whole frames that are kept
    m[:, 8, 50:60, 2:9] = 1.0
    return m


def _edit(model, pipe, u, **kw):
    from insv2v.run_loveu_tgve import edit_video
    return edit_video(model, pipe, u["frames"], u["text_cond"], u["text_uncond"], 7.5, 1.5, init_noises=u["init_noises"], enc_noise=u["enc_noise"],
                      return_latent=True, **WIN, **kw)


def test_edit_video_without_mask_and_full_strength_is_unchanged(tiny_unet, tiny_model):
    from insv2v.inference import InferenceIP2PVideo
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4)
    u = _unit("a")
    plain = _edit(tiny_model, pipe, u)
    explicit = _edit(tiny_model, pipe, u, mask=None, strength=1.0)
    assert torch.equal(plain[0], explicit[0]) and torch.equal(plain[1], explicit[1])


def test_edit_video_two_windows_binary_mask(tiny_unet, tiny_model):
    from insv2v.inference import InferenceIP2PVideo
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4)
    u = _unit("a")
    mask = _image_mask()
    img, lat = _edit(tiny_model, pipe, u, mask=mask)
    assert img.shape == u["frames"].shape and lat.shape == (1, T, 4, S // 8, S // 8)
    img, lat = img.cpu(), lat.cpu()
    keep = (mask == 0.0)[:, :, None].expand_as(img)
    assert torch.equal(img[keep], u["frames"][keep]), "frames outside the mask are not the input's"
    assert (img[~keep] - u["frames"][~keep]).abs().max() > 1e-2, "nothing was edited inside the mask"
    assert img.abs().max() <= 1.0
    # the returned latent outside the reduced mask: the source latent re-noised to the end point of the last step
    small = torch.from_numpy(_np_reduce(mask[0].numpy(), "max"))[None]
    assert 0 < small.sum() < small.numel() and (small[:, :, 1:6, 1:6][:, :7] == 1).all()
    z = tiny_model.encode_image_to_latent(u["frames"], u["enc_noise"]).cpu()
    n = torch.cat(u["init_noises"], dim=1)     # the overlap frames re-use the first window's noise: per frame, the draw it first got
    k_src, k_noise = kr.known_coefficients("ddim", 4, kr.timesteps("ddim", 4)[-1])
    zero = (small == 0.0)[:, :, None].expand_as(lat)
    close(lat[zero], (k_src * z.double() + k_noise * n.double())[zero], "edit_video: latent outside the reduced mask")
    plain = _edit(tiny_model, pipe, u)[1].cpu()
    assert (lat - plain)[zero].abs().max() > 0.1
    # a [1,1,H,W] mask serves all frames; a soft one is accepted; "mean" reduces differently
    one = _edit(tiny_model, pipe, u, mask=mask[:, :1], mask_mode="mean")
    keep1 = (mask[:, :1] == 0.0)[:, :, None].expand(1, T, 3, S, S)
    assert torch.equal(one[0].cpu()[keep1], u["frames"][keep1])


def test_edit_video_strength(tiny_unet, tiny_model):
    """strength 0.5 of 4 steps: two executed steps per window, from the noised source latent; a lighter touch stays closer to it."""
    from insv2v.inference import InferenceIP2PVideo
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4)
    u = _unit("a")
    z = tiny_model.encode_image_to_latent(u["frames"], u["enc_noise"]).cpu()
    full = _edit(tiny_model, pipe, u)[1].cpu()
    half = _edit(tiny_model, pipe, u, strength=0.5)[1].cpu()
    light = _edit(tiny_model, pipe, u, strength=0.25)[1].cpu()
    assert torch.isfinite(half).all() and (half - full).abs().max() > 1e-2
    near = _edit(tiny_model, pipe, u, strength=0.9)[1].cpu()   # round(0.9 * 4) = 4 steps: every step runs, but from the noised source, not from the noise
    assert torch.isfinite(near).all() and (near - full).abs().max() > 1e-2
    d = [float((x - z).pow(2).mean().sqrt()) for x in (light, half, full)]
    print(f"[masked] rms distance to the source latent at strength 0.25 / 0.5 / 1.0: {d[0]:.3f} / {d[1]:.3f} / {d[2]:.3f}")
    assert d[0] < d[1] < d[2]


@pytest.mark.parametrize("steps,s", [(4, 0.9), (10, 0.99)])
def test_strength_below_one_that_rounds_to_all_steps_starts_from_the_noised_source(tiny_unet, tiny_model, steps, s):
    """At s == 1.0 the initial latent is the noise; at EVERY other s it is sqrt(a_t) z + sqrt(1 - a_t) n with t = timesteps[start_time] -
    also where n_exec == steps, i.e. start_time == 0 (a_t at timesteps[0] is small, not zero).  The driver's per-window start latent
    against masked_ref.start_latent, both windows (the overlap takes the carried noise and the previous window's source latent)."""
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.run_loveu_tgve import _EditPlan
    from insv2v.schedulers import strength_to_start
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=steps)
    assert strength_to_start(s, steps) == (steps, 0) == kr.strength_plan(steps, s)
    u = _unit("a")
    z = tiny_model.encode_image_to_latent(u["frames"], u["enc_noise"])
    plan = _EditPlan(tiny_model, pipe, u["frames"], z / tiny_model.scale_factor, None, s, "max", 6, 2, z=z)
    assert plan.active and plan.start_time == 0
    n0, n1 = (x.to(DEV) for x in u["init_noises"])
    inits = [n0, torch.cat([n0[:, -2:], n1], dim=1)]
    zs = [z[:, :6], z[:, 4:10]]
    for k, (init, zk) in enumerate(zip(inits, zs)):
        latent, kw = plan.window(k, 2 if k else 0, init)
        assert kw == {"start_time": 0}
        st, want = kr.start_latent("ddim", steps, s, zk.double().cpu(), init.double().cpu())
        assert st == 0
        close(latent, want, f"strength {s} of {steps} steps, window {k}: start latent vs masked_ref.start_latent")
        assert (latent - init).abs().max() > 1e-2, "the trajectory starts from pure noise"
    full = _EditPlan(tiny_model, pipe, u["frames"], z / tiny_model.scale_factor, None, 1.0, "max", 6, 2, z=z)
    latent, kw = full.window(0, 0, n0)
    assert latent is n0 and kw == {} and not full.active


def test_edit_videos_two_units_one_masked(tiny_unet, tiny_model):
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.run_loveu_tgve import edit_videos
    pipe = InferenceIP2PVideo(tiny_unet[0], scheduler="ddim", num_ddim_steps=4)
    units = [dict(_unit("a"), text_cfg=7.5, video_cfg=1.5, mask=_image_mask()), dict(_unit("b"), text_cfg=7.5, video_cfg=1.5)]
    outs = edit_videos(tiny_model, pipe, units, return_latent=True, **WIN)
    for j, (u, (img, lat)) in enumerate(zip(units, outs)):
        rimg, rlat = _edit(tiny_model, pipe, u, **({"mask": u["mask"]} if "mask" in u else {}))
        report(lat, rlat.cpu(), f"edit_videos unit {j} latent vs edit_video", **STACKED)
        report(img, rimg.cpu(), f"edit_videos unit {j} frames vs edit_video", **STACKED)
    keep = (units[0]["mask"] == 0.0)[:, :, None].expand_as(units[0]["frames"])
    assert torch.equal(outs[0][0].cpu()[keep], units[0]["frames"][keep])
    assert (outs[0][1] - outs[1][1]).abs().max() > 1e-2, "two different units gave the same latent"
