"""Any frame size: latents whose sides are not multiples of 8 through the convolution kernels (nearest-x2 upsample to an explicit output
size, Winograd tiles at odd sizes), the VAE mid-block attention at any h*w, the UNet / VAE / sampling pipelines.

Kernel level: the tolerances of the neighbouring tests in tests/test_kernels_gpu.py - rel 2e-3, abs 1e-3 of a convolution against fp32
F.conv2d on the same fp16-rounded operands, rel 3e-3, abs 2e-3 between two kernel forms.
Model level: the tolerances stated at the top of tests/test_model_gpu.py - single forward / VAE rel-RMS <= 1e-2, max-abs <= 4e-2 max|ref|,
multi-step trajectories rel-RMS <= 3e-2 - against fixtures written by the UNMODIFIED reference (tools/gen_golden_anysize.py).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev():
    return torch.device(DEV)


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).to(dev())


def err_tol(out, ref, rel, abs_):
    out, ref = out.float(), ref.float()
    return (out - ref).abs().max().item(), rel * ref.abs().max().item() + abs_


def close(out, ref, rel=2e-3, abs_=1e-3, what=""):
    err, tol = err_tol(out, ref, rel, abs_)
    print(f"[kernel] {what}: max err {err:.4g} (tol {tol:.4g})")
    assert math.isfinite(err) and err <= tol, f"{what}: max err {err:.4g} > tol {tol:.4g}"


def report(out, ref, what, rms_tol=1e-2, max_tol=4e-2):
    out, ref = out.detach().float().cpu(), torch.as_tensor(ref).float().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    rms = ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    mx = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"[parity] {what}: rel-rms {rms:.3e}  max-abs/max-ref {mx:.3e}")
    assert math.isfinite(rms) and rms <= rms_tol and mx <= max_tol, f"{what}: rel-rms {rms:.3e} (tol {rms_tol}), max {mx:.3e} (tol {max_tol})"


def to_cl(x):  # NCHW -> [N*H*W, C] fp16
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).half().contiguous()


def up_ref(x, wt, b, oh, ow):
    return F.conv2d(F.interpolate(x, size=(oh, ow), mode="nearest"), wt, b, padding=1)


def _conv_case(nb, c1, c2, cout, h, w):
    from insv2v.unet import prep_conv3x3
    x1 = rnd(nb, c1, h, w).half().float()
    x2 = rnd(nb, c2, h, w, seed=2).half().float() if c2 else None
    wt = rnd(cout, c1 + c2, 3, 3, scale=(9 * (c1 + c2)) ** -0.5).half().float()
    b = rnd(cout, seed=4)
    wk, bk = prep_conv3x3({"c.weight": wt.cpu(), "c.bias": b.cpu()}, "c", dev())
    return x1, x2, wt, b, wk, bk


def _check_cropped(out, geom, xin, wt, b, nb, h, w, oh, ow, extra, what):
    """out against conv(interpolate(size)); the last output row / column on its own; and the reference pair "crop, then pad" vs
    "convolve the x2 image, then crop" differs there by far more than the tolerance, so an implementation that crops afterwards fails."""
    cout = wt.shape[0]
    assert geom == (nb, oh, ow)
    ref4 = up_ref(xin, wt, b, oh, ow)
    ref = to_cl(ref4).float() + extra
    close(out, ref, what=what)
    o4, r4 = out.float().reshape(nb, oh, ow, cout), ref.reshape(nb, oh, ow, cout)
    late = to_cl(up_ref(xin, wt, b, 2 * h, 2 * w)[:, :, :oh, :ow]).float().reshape(nb, oh, ow, cout) + extra.reshape(nb, oh, ow, cout)
    tol = 2e-3 * ref.abs().max().item() + 1e-3
    if oh == 2 * h - 1:
        close(o4[:, -1], r4[:, -1], what=what + ", last row")
        gap = (late[:, -1] - r4[:, -1]).abs().max().item()
        assert gap > 10 * tol, f"{what}: crop-after-convolution differs by only {gap:.3g} on the last row (tol {tol:.3g})"
        assert (o4[:, -1] - late[:, -1]).abs().max().item() > 5 * tol
    if ow == 2 * w - 1:
        close(o4[:, :, -1], r4[:, :, -1], what=what + ", last column")
        gap = (late[:, :, -1] - r4[:, :, -1]).abs().max().item()
        assert gap > 10 * tol, f"{what}: crop-after-convolution differs by only {gap:.3g} on the last column (tol {tol:.3g})"
        assert (o4[:, :, -1] - late[:, :, -1]).abs().max().item() > 5 * tol


# ------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("tile", [0, 5, 210, 230, 240])   # dispatched / 128x128 tile (gemm) / gemm_w4 / gemm_q8 / gemm_r8, forced as test_conv3x3_q8 does
@pytest.mark.parametrize("dh,dw", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_conv3x3_upsample_to_size(tile, dh, dw):
    """Nearest-x2 upsample + 3x3 convolution to an explicit output size (2h - dh, 2w - dw) on every gather kernel, with bias and residual,
    against F.conv2d(F.interpolate(x, size=...), padding=1)."""
    from insv2v import ops
    nb, c1, cout, h, w = 6, 128, 320, 8, 16
    oh, ow = 2 * h - dh, 2 * w - dw
    x1, _, wt, b, wk, bk = _conv_case(nb, c1, 0, cout, h, w)
    res = rnd(nb * oh * ow, cout, seed=7).half()
    out, geom = ops.conv3x3(to_cl(x1), (nb, h, w), wk, bk, residual=res, upsample=True, out_size=(oh, ow), tile=tile)
    _check_cropped(out, geom, x1, wt, b, nb, h, w, oh, ow, res.float(), f"upsample conv to {oh}x{ow} tile {tile}")
    if tile:
        out5, _ = ops.conv3x3(to_cl(x1), (nb, h, w), wk, bk, residual=res, upsample=True, out_size=(oh, ow), tile=5)
        close(out, out5, rel=3e-3, abs_=2e-3, what=f"tile {tile} vs the 128x128 tile")
    if (dh, dw) == (0, 0):   # out_size = exactly x2 is the call without out_size
        same, _ = ops.conv3x3(to_cl(x1), (nb, h, w), wk, bk, residual=res, upsample=True, tile=tile)
        assert torch.equal(out, same)


@pytest.mark.parametrize("dh,dw", [(1, 0), (1, 1)])
def test_conv3x3_upsample_to_size_two_sources_and_row_bias(dh, dw):
    """The two-source (x | x2) operand and the per-sample row bias at a cropped target (odd pixel counts per bias group)."""
    from insv2v import ops
    nb, c1, c2, cout, h, w = 4, 128, 64, 192, 5, 7
    oh, ow = 2 * h - dh, 2 * w - dw
    x1, x2, wt, b, wk, bk = _conv_case(nb, c1, c2, cout, h, w)
    rb = rnd(nb // 2, cout, seed=6) * 0.5
    out, geom = ops.conv3x3(to_cl(x1), (nb, h, w), wk, bk, x2=to_cl(x2), row_bias=rb, rows_per_group=2 * oh * ow, upsample=True, out_size=(oh, ow))
    _check_cropped(out, geom, torch.cat([x1, x2], 1), wt, b, nb, h, w, oh, ow, rb.repeat_interleave(2 * oh * ow, 0), f"two-source upsample conv to {oh}x{ow}")


def test_conv3x3_upsample_to_size_split_into_image_ranges():
    """Under a shrunk operand window the launcher cuts the cropped problem into image ranges (opix = OH * OW of the REQUESTED extent):
    bit-identical to the single launch, and right."""
    from insv2v import ops
    nb, c1, cout, h, w = 6, 128, 64, 8, 16
    oh, ow = 2 * h - 1, 2 * w - 1
    x1, _, wt, b, wk, bk = _conv_case(nb, c1, 0, cout, h, w)
    res = rnd(nb * oh * ow, cout, seed=7).half()
    one, geom = ops.conv3x3(to_cl(x1), (nb, h, w), wk, bk, residual=res, upsample=True, out_size=(oh, ow))
    with ops.operand_window(one.numel() * 2 // 3 + 1):   # -> 3 parts of 2 images
        parts, g2 = ops.conv3x3(to_cl(x1), (nb, h, w), wk, bk, residual=res, upsample=True, out_size=(oh, ow))
    assert g2 == geom and torch.equal(one, parts)
    _check_cropped(parts, g2, x1, wt, b, nb, h, w, oh, ow, res.float(), "upsample conv to size, image-range split")


def test_conv3x3_upsample_rejects_other_sizes():
    from insv2v import ops, _lib
    nb, c1, cout, h, w = 2, 64, 64, 8, 12
    x1, _, wt, b, wk, bk = _conv_case(nb, c1, 0, cout, h, w)
    for size in ((2 * h - 2, 2 * w), (2 * h + 1, 2 * w), (2 * h, 2 * w - 2), (2 * h, 2 * w + 1)):
        with pytest.raises(_lib.HipKernelError):
            ops.conv3x3(to_cl(x1), (nb, h, w), wk, bk, upsample=True, out_size=size)
    with pytest.raises(ValueError):   # out_size is the target of the upsample
        ops.conv3x3(to_cl(x1), (nb, h, w), wk, bk, out_size=(h, w))


@pytest.mark.parametrize("H,W", [(5, 7), (23, 40), (12, 21), (45, 80)])
@pytest.mark.parametrize("C1,C2,gn", [(640, 0, False), (640, 0, True), (640, 640, True)])
def test_winograd_conv3x3_odd_sizes(H, W, C1, C2, gn):
    """The body of test_winograd_conv3x3_vs_fp32 at odd sizes: ceil(H/2) x ceil(W/2) tiles, the overhanging row / column reads zeros
    (also under the folded GroupNorm + SiLU) and is not stored; plain, folded norm, two sources; against fp32 and the direct form."""
    from insv2v import ops
    NB, N = 4, 640
    C, M = C1 + C2, NB * H * W
    ips = 2
    x = rnd(M, C1, seed=1).half()
    x2 = rnd(M, C2, seed=2).half() if C2 else None
    w = rnd(N, C, 3, 3, scale=(9 * C) ** -0.5, seed=3)
    b = rnd(N, seed=4)
    assert ops.winograd_ok((NB, H, W), C, C1 if C2 else 0)
    U = ops.winograd_weights(w.cpu(), dev())
    ab = None
    xin = torch.cat([x, x2], 1).float() if C2 else x.float()
    if gn:
        ab = torch.stack([1.0 + 0.2 * rnd(NB // ips, C, seed=5), 0.3 * rnd(NB // ips, C, seed=6)], -1).contiguous()   # (scale, shift)
        sc = ab[..., 0].repeat_interleave(ips * H * W, 0), ab[..., 1].repeat_interleave(ips * H * W, 0)
        xin = F.silu(xin * sc[0] + sc[1])
    xin = xin.half().float()                # the kernel stages the normalised pixels in fp16
    tb = rnd(NB // ips, N, seed=7)
    r = rnd(M, N, seed=8).half()
    out = ops.winograd_conv3x3(x, (NB, H, W), U, b, x2=x2, gn_ab=ab, gn_images_per_sample=ips, gn_silu=gn, row_bias=tb, rows_per_group=ips * H * W, residual=r)
    ref = F.conv2d(xin.reshape(NB, H, W, C).permute(0, 3, 1, 2), w.half().float(), b, padding=1).permute(0, 2, 3, 1).reshape(M, N)
    ref = ref + tb.repeat_interleave(ips * H * W, 0) + r.float()
    close(out, ref, rel=2e-3, abs_=1e-3, what=f"winograd conv {NB}x{H}x{W} {C}->{N} gn={gn}")
    direct, _ = ops.conv3x3(xin.half(), (NB, H, W), w.permute(0, 2, 3, 1).reshape(N, 9 * C).half().contiguous(), b, row_bias=tb, rows_per_group=ips * H * W, residual=r)
    close(out, direct, rel=3e-3, abs_=2e-3, what="winograd vs direct convolution")


def test_winograd_ok_rules():
    from insv2v import ops
    for hw in ((5, 7), (23, 40), (12, 21), (45, 80)):
        assert ops.winograd_ok((4, *hw), 1280) and ops.winograd_ok((4, *hw), 2560, 1280)
    assert ops.winograd_ok((4, 12, 20), 1280, upsample=True) and ops.winograd_ok((4, 12, 20), 1280, upsample=True, out_size=(24, 40))
    for size in ((23, 40), (24, 39), (23, 39)):
        assert not ops.winograd_ok((4, 12, 20), 1280, upsample=True, out_size=size)


@pytest.mark.parametrize("N,H,W,C", [(3, 5, 7, 512), (2, 45, 45, 128)])
def test_vae_attention_any_hw(N, H, W, C):
    """The VAE's mid AttnBlock at h*w = 35 and 2025 (not multiples of 8: padded score rows, the softmax leaves the pad columns zero) against
    an fp32 torch softmax(q k^T / sqrt(C)) v composition of the same fp16-rounded weights; tolerance as test_vae_vs_golden."""
    from insv2v.vae import VAttn
    HW = H * W
    sd = {"a.norm.weight": 1 + 0.1 * rnd(C, seed=1), "a.norm.bias": 0.1 * rnd(C, seed=2)}
    for i, n in enumerate(("q", "k", "v", "proj_out")):
        sd[f"a.{n}.weight"] = rnd(C, C, 1, 1, scale=C ** -0.5, seed=10 + i)
        sd[f"a.{n}.bias"] = 0.1 * rnd(C, seed=20 + i)
    sd = {k: v.cpu() for k, v in sd.items()}
    att = VAttn(sd, "a", C, dev())
    x = (rnd(N, C, H, W, seed=3) * 1.5).half()
    out = att(to_cl(x.float()), (N, H, W))
    xf = x.float()
    n = F.group_norm(xf, 32, sd["a.norm.weight"].to(dev()), sd["a.norm.bias"].to(dev()), 1e-6)
    lin = lambda t, k: F.conv2d(t, sd[f"a.{k}.weight"].to(dev()).half().float(), sd[f"a.{k}.bias"].to(dev()))
    q, k, v = (lin(n, s).reshape(N, C, HW) for s in "qkv")
    p = torch.softmax(torch.bmm(q.permute(0, 2, 1), k) * C ** -0.5, dim=2)
    o = torch.bmm(v, p.permute(0, 2, 1)).reshape(N, C, H, W)
    ref = xf + lin(o, "proj_out")
    report(out.float().reshape(N, H, W, C).permute(0, 3, 1, 2), ref, f"VAE AttnBlock h*w = {HW}")


# ------------------------------------------------------------------------------------------- model level
@pytest.fixture(scope="module")
def tiny_unet():
    from insv2v import synth, shapes
    from insv2v.unet import UNet3DConditionModel
    sd = synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_TINY))
    return UNet3DConditionModel(**synth.UNET_TINY, device=DEV).load_state_dict(sd)


def _case_c():
    from insv2v import synth
    lat = synth.synth_input("anysize.c.latent", (1, 4, 4, 12, 20))   # [b, c, f, h, w]
    cond = synth.synth_input("anysize.c.cond", (1, 4, 4, 12, 20))
    tu, tc = synth.synth_input("anysize.c.tu", (1, 77, 64)), synth.synth_input("anysize.c.tc", (1, 77, 64))
    return lat, cond, torch.cat([tu, tu, tc], 0)


def test_unet_tiny_anysize_vs_golden(tiny_unet, golden):
    from insv2v import synth
    g = golden("unet_tiny_anysize")
    x = synth.synth_input("anysize.a.sample", (2, 8, 4, 20, 14))
    ctx = synth.synth_input("anysize.a.ctx", (2, 77, 64))
    out = tiny_unet(x, torch.full((2,), 481, dtype=torch.long), encoder_hidden_states=ctx).sample
    report(out, g["a"], "unet tiny fwd 20x14 (reference golden)")
    x = synth.synth_input("anysize.b.sample", (1, 8, 5, 18, 22))
    ctx = synth.synth_input("anysize.b.ctx", (1, 77, 64))
    out = tiny_unet(x, torch.full((1,), 481, dtype=torch.long), encoder_hidden_states=ctx, video_start_index=3).sample
    report(out, g["b"], "unet tiny fwd 18x22 start=3 (reference golden)")
    lat, cond, ctx = _case_c()
    x = torch.cat([torch.cat([lat, torch.zeros_like(cond)], 1), torch.cat([lat, cond], 1), torch.cat([lat, cond], 1)], 0)   # [b, c, f, h, w]
    out = tiny_unet(x, torch.full((3,), 481, dtype=torch.long), encoder_hidden_states=ctx).sample
    report(out, g["c"], "unet tiny fwd 12x20 CFG triple (reference golden)")


def test_unet_anysize_graph_and_cfg_prefix(tiny_unet, golden):
    """The CFG triple at 12x20 through GraphedUNet: eager, captured (bit-identical to eager) and with the shared CFG prefix (cfg_clips = 1),
    each against the reference's output."""
    from insv2v.inference import GraphedUNet
    from insv2v import ops
    g = golden("unet_tiny_anysize")["c"]
    lat, cond, ctx = _case_c()
    B, Fr, H, W, L = 3, 4, 12, 20, 77
    outs = []
    for use_graph, cfg_clips in ((False, 0), (True, 0), (False, 1), (True, 1)):
        r = GraphedUNet(tiny_unet, B, Fr, H, W, L, use_graph=use_graph, branch_streams=False, cfg_clips=cfg_clips)
        assert r.cfg_clips == cfg_clips
        r.set_context(ctx)
        ops.build_unet_input(lat[0].permute(1, 0, 2, 3).contiguous().to(DEV), cond[0].permute(1, 0, 2, 3).contiguous().to(DEV), r.x_in, r.t, 481, 3)   # [f, c, h, w]
        e1 = r.run().clone()
        assert torch.equal(e1, r.run())
        outs.append(e1)
        report(e1.reshape(B, Fr, H, W, 4).permute(0, 4, 1, 2, 3), g, f"GraphedUNet 12x20 graph={use_graph} cfg_clips={cfg_clips} (reference golden)")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[2], outs[3]), "hipGraph replay must be bit-identical to eager launches"


def test_unet_anysize_batch_invariance(tiny_unet):
    """A sample alone equals the same sample inside a stack of 3, bit for bit, at a ragged size (the property the
    test_c2_stacked_forward_* tests hold the product to: samples are independent)."""
    from insv2v import synth
    x = synth.synth_input("anysize.inv.sample", (3, 8, 4, 20, 14))
    ctx = synth.synth_input("anysize.inv.ctx", (3, 77, 64))
    x[2], ctx[2] = x[0], ctx[0]
    t = torch.full((3,), 481, dtype=torch.long)
    stack = tiny_unet(x, t, encoder_hidden_states=ctx).sample
    assert torch.equal(stack[0], stack[2]), "equal samples inside one stack differ"
    alone = tiny_unet(x[:1], t[:1], encoder_hidden_states=ctx[:1]).sample
    diff = (alone[0] - stack[0]).abs().max().item()
    print(f"[parity] sample alone vs inside a stack of 3 at 20x14: max |diff| = {diff:.3e}")
    assert torch.equal(alone[0], stack[0]), f"a sample alone differs from the same sample in a stack of 3 by {diff:.3e}"


def test_unet_full_width_anysize_vs_golden(golden):
    """Full width at a ragged size: a branch-major CFG triple of 16 frames at latent 9x8 against the unmodified reference - the row
    kernels without the GroupNorm fold (72 % 32 != 0), the fused temporal / text attention kernels on ragged pixel tiles, every upsampler
    to a cropped target (2 -> 3 -> 5 -> 9 rows); eager and with the shared CFG prefix."""
    from insv2v import synth, shapes, ops
    from insv2v.unet import UNet3DConditionModel
    from insv2v.inference import GraphedUNet
    g = golden("unet_full_anysize")["out"]
    unet = UNet3DConditionModel(**synth.UNET_FULL, device=DEV).load_state_dict(synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_FULL)))
    lat = synth.synth_input("anysize.full.latent", (1, 4, 16, 9, 8))   # [b, c, f, h, w]
    cond = synth.synth_input("anysize.full.cond", (1, 4, 16, 9, 8))
    tu, tc = synth.synth_input("anysize.full.tu", (1, 77, 768)), synth.synth_input("anysize.full.tc", (1, 77, 768))
    ctx = torch.cat([tu, tu, tc], 0)
    x = torch.cat([torch.cat([lat, torch.zeros_like(cond)], 1), torch.cat([lat, cond], 1), torch.cat([lat, cond], 1)], 0)
    out = unet(x, torch.full((3,), 481, dtype=torch.long), encoder_hidden_states=ctx).sample
    report(out, g, "full-width UNet fwd 9x8 CFG triple (reference golden)")
    r = GraphedUNet(unet, 3, 16, 9, 8, 77, use_graph=False, cfg_clips=1)
    r.set_context(ctx)
    ops.build_unet_input(lat[0].permute(1, 0, 2, 3).contiguous().to(DEV), cond[0].permute(1, 0, 2, 3).contiguous().to(DEV), r.x_in, r.t, 481, 3)
    report(r.run().reshape(3, 16, 9, 8, 4).permute(0, 4, 1, 2, 3), g, "full-width UNet fwd 9x8, shared CFG prefix (reference golden)")
    del unet, r
    torch.cuda.empty_cache()


def test_upsample3d_full_width_vs_golden(golden):
    """Upsample3D at 1280 channels, 5x7 -> output_size 9x14 (rows cropped, columns exact), as the UNet's up block issues it."""
    from insv2v import synth, ops
    from insv2v.unet import prep_conv3x3
    g = golden("blocks_anysize")["up1280"]
    conv = torch.nn.Conv2d(1280, 1280, 3, padding=1)
    sd = {"c." + k: synth.synth_tensor("up1280.conv." + k, v) for k, v in conv.state_dict().items()}
    wk, bk = prep_conv3x3(sd, "c", dev())
    x = synth.synth_input("up1280.x", (1, 1280, 1, 5, 7))
    xcl = to_cl(x[:, :, 0].to(DEV))
    assert not ops.winograd_ok((1, 5, 7), 1280, upsample=True, out_size=(9, 14))
    out, geom = ops.conv3x3(xcl, (1, 5, 7), wk, bk, upsample=True, out_size=(9, 14))
    assert geom == (1, 9, 14)
    report(out.float().reshape(1, 9, 14, 1280).permute(0, 3, 1, 2), g[:, :, 0], "Upsample3D 1280 ch 5x7 -> 9x14 (reference golden)")


def test_vae_tiny_anysize_vs_golden(golden):
    from insv2v import synth, shapes, ops
    from insv2v.vae import AutoencoderKL
    g = golden("vae_tiny_anysize")
    sd = synth.synth_state_dict(shapes.vae_shapes(**synth.VAE_TINY))
    vae = AutoencoderKL(**synth.VAE_TINY, device=DEV).load_state_dict(sd)
    x = synth.synth_input("anysize.vae.x", (2, 3, 40, 56), kind="uniform")
    mom, geom = vae.moments(x)
    assert geom == (2, 5, 7)
    report(mom.reshape(2, 5, 7, 8).permute(0, 3, 1, 2), g["moments"], "VAE tiny encoder moments 40x56 (reference golden)")
    z = synth.synth_input("anysize.vae.z", (1, 4, 5, 7))
    report(vae.decode(z), g["dec"], "VAE tiny decode 5x7 -> 40x56 (reference golden)")
    with pytest.raises(ValueError):
        vae.moments(torch.zeros(1, 3, 36, 56))


def _pipe_kw():
    from insv2v import synth
    Fr, h, w, R = 6, 20, 14, 2
    kw = dict(latent=synth.synth_input("anysize.pipe.latent", (1, Fr, 4, h, w)), img_cond=synth.synth_input("anysize.pipe.cond", (1, Fr, 4, h, w)),
              text_cond=synth.synth_input("anysize.pipe.text_cond", (1, 77, 64)), text_uncond=synth.synth_input("anysize.pipe.text_uncond", (1, 77, 64)),
              text_cfg=7.5, img_cfg=1.5)
    return kw, synth.synth_input("anysize.pipe.latent_ref", (1, R, 4, h, w))


def test_pipelines_anysize_vs_golden(tiny_unet, golden):
    from insv2v.inference import InferenceIP2PVideo
    g = golden("pipelines_anysize")
    kw, lref = _pipe_kw()
    tol = dict(rms_tol=3e-2, max_tol=1e-1)
    p = InferenceIP2PVideo(tiny_unet, scheduler="ddim", num_ddim_steps=4)
    r = p(**kw)
    report(r["all_pred"][-1], g["ddim4_pred_last"], "ddim4 20x14 last x0 prediction (reference golden)", **tol)
    report(r["latent"], g["ddim4_latent"], "ddim4 20x14 final latent (reference golden)", **tol)
    r2 = p.second_clip_forward(**kw, latent_ref=lref, noise_correct_step=0.5)
    report(r2["latent"], g["second_clip_latent"], "second_clip_forward 20x14 (reference golden)", **tol)
    rs = p.run_stacked([dict(kw), dict(kw, latent_ref=lref, noise_correct_step=0.5)])
    report(rs[0]["latent"], g["ddim4_latent"], "run_stacked 20x14: __call__ clip (reference golden)", **tol)
    report(rs[1]["latent"], g["second_clip_latent"], "run_stacked 20x14: second_clip_forward clip (reference golden)", **tol)


def _launch_tags(unet, x, ctx):
    from insv2v import ops
    rec = []
    ops.set_launch_recorder(rec)
    try:
        unet(x, torch.full((x.shape[0],), 481, dtype=torch.long), encoder_hidden_states=ctx)
        torch.cuda.synchronize()
    finally:
        ops.set_launch_recorder(None)
    return [t[4] for t in rec if len(t) > 4 and t[4]]


def test_exact_x2_sizes_keep_their_launches(monkeypatch):
    """Regression guard of the dispatch rule, on a tiny UNet whose 256-channel upsamplers carry the Winograd up-form (thresholds lowered):
    a latent whose sides are multiples of 8 issues no cropped-upsample launch and takes the Winograd up-form wherever winograd_ok allows
    it; a ragged latent takes the direct form with an explicit output size exactly where its target is cropped."""
    from insv2v import synth, shapes, unet as U
    monkeypatch.setattr(U, "WINOGRAD_MIN_ROWS", 0)
    monkeypatch.setattr(U, "WINOGRAD_UP_MIN_CIN", 256)
    sd = synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_TINY))
    unet = U.UNet3DConditionModel(**synth.UNET_TINY, device=DEV).load_state_dict(sd)
    assert [blk.get("up_u") is not None for blk in unet.up] == [True, True, False, False]
    B, Fr = 1, 4
    ctx = synth.synth_input("anysize.x2.ctx", (B, 77, 64))
    for (H, W), want_wino, want_direct in (((16, 24), [(4, 6), (8, 12)], [(16, 24)]), ((20, 14), [], [(5, 4), (10, 7), (20, 14)])):
        tags = _launch_tags(unet, synth.synth_input("anysize.x2.sample", (B, 8, Fr, H, W)), ctx)
        up_convs = sorted(t[1] for t in tags if t[0] == "conv" and t[5] == 1)          # output rows of the direct upsample convolutions
        wino_up = sorted(t[1] for t in tags if t[0] == "wino_out")                      # (no ResnetBlock3D of this width takes the Winograd form)
        assert up_convs == sorted(B * Fr * h * w for h, w in want_direct), (H, W, up_convs)
        assert wino_up == sorted(B * Fr * h * w for h, w in want_wino), (H, W, wino_up)
        sizes = U.plan_sizes(H, W)   # (coarsest upsampler first)
        assert sizes["up"] == want_wino + want_direct
