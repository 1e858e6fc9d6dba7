"""The fused row kernels beyond the 2 GiB operand window.

The launchers of insv2v_ffn_fused, insv2v_tattn_fused / _attn and insv2v_xattn_fused / _attn run a problem whose x, out or residual
operands reach beyond one 2 GiB buffer descriptor as ranges of whole units (128-row tiles; samples, with their K / V streams), one launch
each, so every operand may exceed the window; only one unit has to fit.  Every kernel is run on operands above 2 GiB and checked (a) against fp32 torch at the bounds of its
in-window test in tests/test_kernels_gpu.py and (b) bit for bit against the same rows run as a problem of their own: a row's arithmetic
does not depend on its position.  Inputs are a seeded 4096-row block repeated, with the rows around the 2^31-byte mark perturbed so that
they differ from their period (a kernel that wrapped its offsets would read a row with other values).  Then the whole forward and the
pipeline beyond today's stack cap, the split path at small shapes (ops.operand_window) and the refusals.

The temporal and text attention read whole samples (all frames of a pixel / the sample's K, V), so their checks take whole samples: the
first, the one that contains the 2^31-byte mark, and the last.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARK = 2 ** 31


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def close(out, ref, rel=4e-3, abs_=4e-3, what=""):
    out, ref = out.float(), ref.float()
    err = (out - ref).abs().max().item()
    tol = rel * ref.abs().max().item() + abs_
    print(f"[parity] {what}: max err {err:.4g} (tol {tol:.4g})")
    assert math.isfinite(err) and err <= tol, f"{what}: max err {err:.4g} > tol {tol:.4g} (ref max {ref.abs().max().item():.4g})"


def big_rows(M, C, seed, scale=1.3, shift=0.2):
    """[M, C] fp16 beyond 2 GiB: a seeded 4096-row block repeated; 1000 rows around byte 2^31 differ from their period.  Returns the
    tensor and the row that holds the mark."""
    assert M * C * 2 > MARK
    g = torch.Generator(device="cpu").manual_seed(seed)
    blk = (torch.randn(4096, C, generator=g) * scale + shift).half().to(DEV)
    x = blk.repeat(M // 4096 + 1, 1)[:M].contiguous()
    mark = MARK // (C * 2)
    x[mark - 500:mark + 500] += 0.25
    return x, mark


def layernorm32(xf, eps=1e-5):
    return (xf - xf.mean(1, keepdim=True)) * (xf.var(1, unbiased=False, keepdim=True) + eps).rsqrt()


# ------------------------------------------------------------------------------------------------ T1: feed-forward
def test_ffn_fused_operands_beyond_2gib():
    """T1: insv2v_ffn_fused, plain and with the trailing projection (post), at M = 3 400 037 x 320: x, out and post_residual are 2.18 GB
    each (the 2^31-byte mark is in row 3 355 443).  Bounds of test_ffn_fused_vs_fp32."""
    from insv2v import ops
    from insv2v.fused import pack_ffn_stream
    from insv2v.unet import fold_layernorm
    M, C, NH = 3400037, 320, 1280
    x, mark = big_rows(M, C, seed=5)
    assert mark == 3355443
    w1, b1 = rnd(2 * NH, C, scale=C ** -0.5), rnd(2 * NH, seed=1) * 0.3
    w2, b2 = rnd(C, NH, scale=NH ** -0.5, seed=2).half(), rnd(C, seed=3) * 0.3
    gamma, beta = 1 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    wp, bp = rnd(C, C, scale=C ** -0.5, seed=6).half(), rnd(C, seed=7) * 0.3
    wf, _, bf = fold_layernorm(w1.cpu(), gamma.cpu(), beta.cpu(), b1.cpu())
    stream = pack_ffn_stream(wf.float(), bf, w2.float().cpu(), b2.cpu()).to(DEV)
    stream_p = pack_ffn_stream(wf.float(), bf, w2.float().cpu(), b2.cpu(), post=(wp.float().cpu(), bp.cpu())).to(DEV)
    out = ops.ffn_fused(x, stream, NH)
    r2 = out                                   # a > 2 GiB post_residual
    outp = ops.ffn_fused(x, stream_p, NH, post_residual=r2)
    for lo, hi in [(0, 512), (3355000, 3356000), (M - 300, M)]:
        xf = x[lo:hi].float()
        y = layernorm32(xf) @ wf.float().to(DEV).t() + bf.to(DEV)
        h, g = y.chunk(2, dim=-1)
        ref = (h * F.gelu(g)).half().float() @ w2.float().t() + b2 + xf
        close(out[lo:hi], ref, what=f"ffn_fused rows {lo}:{hi} of a 2.18 GB operand")
        refp = ref.half().float() @ wp.float().t() + bp + r2[lo:hi].float()
        close(outp[lo:hi], refp, what=f"ffn_fused + proj_out rows {lo}:{hi}")
    lo = mark - mark % 128 - 1024              # the tile-aligned 2048-row block around the mark as a problem of its own
    xs = x[lo:lo + 2048].contiguous()
    assert torch.equal(ops.ffn_fused(xs, stream, NH), out[lo:lo + 2048])
    assert torch.equal(ops.ffn_fused(xs, stream_p, NH, post_residual=r2[lo:lo + 2048].contiguous()), outp[lo:lo + 2048])
    del out, outp, r2, x
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ T2: the attention kernels
def _tattn_ref(xs, wqkv, table, samples, F_, HW, H, wo=None, bo=None):
    """fp32 torch temporal attention of whole samples (rows (sample, frame, pixel)), as test_tattn_fused_vs_fp32."""
    M, C = xs.shape
    D = C // H
    xf = xs.float()
    frame = (torch.arange(M, device=xs.device) // HW) % F_
    qkv = (layernorm32(xf) @ wqkv.float().t() + table[frame]).half().float().reshape(samples, F_, HW, 3, H, D)
    q, k, v = (qkv[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))
    a = F.scaled_dot_product_attention(q, k, v).permute(0, 3, 1, 2, 4).reshape(M, C)
    if wo is None:
        return a
    return a.half().float() @ wo.float().t() + bo + xf


@pytest.mark.parametrize("F_,samples", [(16, 140), (24, 93)])
def test_tattn_fused_operands_beyond_2gib(F_, samples):
    """T2: insv2v_tattn_fused at HW = 1531 (odd: with 16 frame slots a wave's pixel pair straddles two samples, the last tile of every range
    is ragged).
    F = 16, 140 samples = 3 429 440 rows: fp32 bounds of test_tattn_fused_vs_fp32 and bit identity.  F = 24 (32 frame slots, one pixel
    per wave), 93 samples: bit identity only."""
    from insv2v import ops
    from insv2v.fused import pack_tattn_stream
    C, H, HW = 320, 8, 1531
    R = F_ * HW
    M = samples * R
    x, mark = big_rows(M, C, seed=7)
    wqkv = rnd(3 * C, C, scale=C ** -0.5).half()
    table = rnd(F_, 3 * C, seed=1) * 0.4
    wo, bo = rnd(C, C, scale=C ** -0.5, seed=2).half(), rnd(C, seed=3) * 0.3
    stream = pack_tattn_stream(wqkv.float().cpu(), table.cpu(), wo.float().cpu(), bo.cpu()).to(DEV)
    out = ops.tattn_fused(x, stream, samples, HW, H, F_)
    sm = mark // R
    assert 0 < sm < samples - 1
    if F_ == 16:
        for s in (0, sm, samples - 1):
            ref = _tattn_ref(x[s * R:(s + 1) * R], wqkv, table, 1, F_, HW, H, wo, bo)
            close(out[s * R:(s + 1) * R], ref, what=f"tattn_fused sample {s} of {samples} (2.19 GB operands)")
    for s in (sm, samples - 1):                # the sample that contains the mark and the last one, each run alone
        alone = ops.tattn_fused(x[s * R:(s + 1) * R].contiguous(), stream, 1, HW, H, F_)
        assert torch.equal(alone, out[s * R:(s + 1) * R]), f"tattn_fused F={F_}: sample {s} differs from the same sample run alone"
    del out, x
    torch.cuda.empty_cache()


def test_tattn_attn_640_operands_beyond_2gib():
    """T2: insv2v_tattn_attn (C = 640), 70 samples x 16 frames x 1531 pixels = 1 714 720 rows (mark in row 1 677 721).  Bounds of
    test_tattn_attn_640_vs_fp32."""
    from insv2v import ops
    from insv2v.fused import pack_tattn_qkv_stream
    C, H, HW, F_, samples = 640, 8, 1531, 16, 70
    R = F_ * HW
    M = samples * R
    assert M == 1714720
    x, mark = big_rows(M, C, seed=9)
    assert mark == 1677721
    wqkv = rnd(3 * C, C, scale=C ** -0.5).half()
    table = rnd(F_, 3 * C, seed=1) * 0.4
    stream = pack_tattn_qkv_stream(wqkv.float().cpu(), table.cpu()).to(DEV)
    out = ops.tattn_attn(x, stream, samples, HW, H, F_)
    sm = mark // R
    assert 0 < sm < samples - 1
    for s in (0, sm, samples - 1):
        close(out[s * R:(s + 1) * R], _tattn_ref(x[s * R:(s + 1) * R], wqkv, table, 1, F_, HW, H), what=f"tattn_attn sample {s} of {samples} (2.19 GB operands)")
    for s in (sm, samples - 1):
        alone = ops.tattn_attn(x[s * R:(s + 1) * R].contiguous(), stream, 1, HW, H, F_)
        assert torch.equal(alone, out[s * R:(s + 1) * R]), f"tattn_attn: sample {s} differs from the same sample run alone"
    del out, x
    torch.cuda.empty_cache()


def _xattn_ref(xs, kv1, wq, bq, H, L, wo=None, bo=None):
    """fp32 torch text cross-attention of ONE sample's rows against its [L, 2 C] K / V, as test_xattn_fused_vs_fp32."""
    M, C = xs.shape
    D = C // H
    xf = xs.float()
    xn = layernorm32(xf).half().float()
    q = (xn @ wq.float().t() + bq).half().float().reshape(1, M, H, D).permute(0, 2, 1, 3)
    k = kv1[:, :C].float().reshape(1, L, H, D).permute(0, 2, 1, 3)
    v = kv1[:, C:].float().reshape(1, L, H, D).permute(0, 2, 1, 3)
    a = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(M, C)
    if wo is None:
        return a
    return a.half().float() @ wo.float().t() + bo + xf


def test_xattn_fused_operands_beyond_2gib():
    """T2: insv2v_xattn_fused, plain and with the leading out-projection (pre_residual), 140 samples x 24 496 rows (= 16 x 1531: ragged
    128-row tiles per sample) = 3 429 440 rows; x, out and pre_residual are 2.19 GB each.  Bounds of test_xattn_fused_vs_fp32."""
    from insv2v import ops
    from insv2v.fused import pack_xattn_stream, pack_xattn_kv
    C, H, L, samples, R = 320, 8, 77, 140, 16 * 1531
    M = samples * R
    assert M == 3429440
    x, mark = big_rows(M, C, seed=11)
    wq, bq = rnd(C, C, scale=C ** -0.5).half(), rnd(C, seed=5) * 0.3
    wo, bo = rnd(C, C, scale=C ** -0.5, seed=2).half(), rnd(C, seed=3) * 0.3
    wo1, bo1 = rnd(C, C, scale=C ** -0.5, seed=11).half(), rnd(C, seed=12) * 0.3
    kv = (rnd(samples * L, 2 * C, seed=4) * 1.5).half()
    stream = pack_xattn_stream(wq.float().cpu(), bq.cpu(), wo.float().cpu(), bo.cpu()).to(DEV)
    pre_stream = pack_xattn_stream(wq.float().cpu(), bq.cpu(), wo.float().cpu(), bo.cpu(), pre=(wo1.float().cpu(), bo1.cpu())).to(DEV)
    kvs = pack_xattn_kv(kv, samples, L, C, H)
    out = ops.xattn_fused(x, stream, kvs, R, H, L)
    hres = out                                 # a > 2 GiB pre_residual; x doubles as the self-attention output of the second form
    out_pre = ops.xattn_fused(x, pre_stream, kvs, R, H, L, pre_residual=hres)
    sm = mark // R
    assert 0 < sm < samples - 1
    for s in (0, sm, samples - 1):
        rows, kv1 = slice(s * R, (s + 1) * R), kv[s * L:(s + 1) * L]
        close(out[rows], _xattn_ref(x[rows], kv1, wq, bq, H, L, wo, bo), what=f"xattn_fused sample {s} of {samples} (2.19 GB operands)")
        x1 = (x[rows].float() @ wo1.float().t() + bo1 + hres[rows].float()).half()
        close(out_pre[rows], _xattn_ref(x1, kv1, wq, bq, H, L, wo, bo), what=f"xattn_fused with leading out-projection, sample {s}")
    for s in (sm, samples - 1):                # each run alone, with its own K / V stream
        rows, kv1 = slice(s * R, (s + 1) * R), kvs[s:s + 1].contiguous()
        assert torch.equal(ops.xattn_fused(x[rows].contiguous(), stream, kv1, R, H, L), out[rows]), f"xattn_fused: sample {s} differs from the same sample run alone"
        assert torch.equal(ops.xattn_fused(x[rows].contiguous(), pre_stream, kv1, R, H, L, pre_residual=hres[rows].contiguous()), out_pre[rows]), \
            f"xattn_fused (pre): sample {s} differs from the same sample run alone"
    del out, out_pre, hres, x
    torch.cuda.empty_cache()


def test_xattn_attn_640_operands_beyond_2gib():
    """T2: insv2v_xattn_attn (C = 640), 70 samples x 24 496 rows = 1 714 720 rows (mark in row 1 677 721).  Bounds of
    test_xattn_attn_640_vs_fp32."""
    from insv2v import ops
    from insv2v.fused import pack_xattn_q_stream, pack_xattn640_kv
    C, H, L, samples, R = 640, 8, 77, 70, 16 * 1531
    M = samples * R
    x, mark = big_rows(M, C, seed=13)
    assert M == 1714720 and mark == 1677721
    wq, bq = rnd(C, C, scale=C ** -0.5).half(), rnd(C, seed=5) * 0.3
    kv = (rnd(samples * L, 2 * C, seed=4) * 1.5).half()
    stream = pack_xattn_q_stream(wq.float().cpu(), bq.cpu()).to(DEV)
    kvs = pack_xattn640_kv(kv, samples, L, C, H)
    out = ops.xattn_attn(x, stream, kvs, R, H, L)
    sm = mark // R
    assert 0 < sm < samples - 1
    for s in (0, sm, samples - 1):
        rows = slice(s * R, (s + 1) * R)
        close(out[rows], _xattn_ref(x[rows], kv[s * L:(s + 1) * L], wq, bq, H, L), what=f"xattn_attn sample {s} of {samples} (2.19 GB operands)")
    for s in (sm, samples - 1):
        rows = slice(s * R, (s + 1) * R)
        assert torch.equal(ops.xattn_attn(x[rows].contiguous(), stream, kvs[s:s + 1].contiguous(), R, H, L), out[rows]), \
            f"xattn_attn: sample {s} differs from the same sample run alone"
    del out, x
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ T3 / T4: the forward and the pipeline
@pytest.fixture(scope="module")
def full_unet():
    from insv2v import synth, shapes
    from insv2v.unet import UNet3DConditionModel
    sd = synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_FULL))
    return UNet3DConditionModel(**synth.UNET_FULL, device=DEV).load_state_dict(sd)


def report(out, ref, what, rms_tol, max_tol):
    out, ref = out.detach().float().cpu(), torch.as_tensor(np.asarray(ref)).float().cpu()
    assert out.shape == ref.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(ref.shape)}"
    rms = ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    mx = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"[parity] {what}: rel-rms {rms:.3e}  max-abs/max-ref {mx:.3e}")
    assert math.isfinite(rms) and rms <= rms_tol and mx <= max_tol, f"{what}: rel-rms {rms:.3e} (tol {rms_tol}), max {mx:.3e} (tol {max_tol})"


def test_c2_forward_46_clips_beyond_every_cap(full_unet):
    """T3: one eager full-width forward of 46 clips' CFG triples (B = 138): the level-0 token matrix is 3 391 488 x 320 = 2.17 GB, one clip
    more than the row kernels took while they addressed whole operands.  Every triple carries the C2 reference golden's inputs: each is
    pinned by value (the bounds of test_c2_stacked_forward_vs_reference_golden) and all must agree bit for bit."""
    from insv2v import synth
    g = np.load(os.path.join(GOLD, "c2_unet_fwd.npz"))["out"]
    n = 46
    x = synth.synth_input("c2.sample", (3, 8, 16, 32, 48)).repeat(n, 1, 1, 1, 1)
    ctx = synth.synth_input("c2.ctx", (3, 77, 768)).repeat(n, 1, 1)
    assert 3 * n * 16 * 32 * 48 * 320 * 2 > MARK
    out = full_unet(x, torch.full((3 * n,), 981, dtype=torch.long), encoder_hidden_states=ctx).sample
    assert out.shape == (3 * n, 4, 16, 32, 48) and torch.isfinite(out).all()
    report(out[:3], g, f"C2 stacked forward (B = {3 * n}), clip 0 (reference golden)", 1e-2, 4e-2)
    for i in range(1, n):                      # equal to clip 0, which is pinned by value: every triple is within the same bounds
        assert torch.equal(out[:3], out[3 * i:3 * i + 3]), f"clip {i} differs from clip 0: samples are not independent"
    del out
    torch.cuda.empty_cache()


def test_run_stacked_max_clips_20_at_45x80(full_unet):
    """T4: run_stacked(calls, max_clips=20) at the 45 x 80 latent size (360 x 640 frames): 20 clips in ONE launch chain, where the default
    cap splits them at 9.  2 DDIM steps, three distinct clips repeated: twins inside the stack are bit-equal, and clips 0 - 2 agree with
    the default grouping (max_clips=None) at the bounds of test_run_stacked_10_clips_full_width_vs_sequential."""
    from insv2v import synth
    from insv2v.inference import InferenceIP2PVideo, max_clips_in_flight, stack_groups
    n, Fc, h, w = 20, 16, 45, 80
    assert max_clips_in_flight(Fc, h, w) == 9
    assert stack_groups(n, max_clips_in_flight(Fc, h, w)) == [7, 7, 6] and stack_groups(n, 20) == [20]
    pipe = InferenceIP2PVideo(full_unet, scheduler="ddim", num_ddim_steps=2)
    calls = []
    for k in range(n):
        j = k % 3
        calls.append(dict(latent=synth.synth_input(f"sc.lat.{j}", (1, Fc, 4, h, w)), img_cond=synth.synth_input(f"sc.cond.{j}", (1, Fc, 4, h, w)),
                          text_cond=synth.synth_input(f"sc.tc.{j}", (1, 77, 768)), text_uncond=synth.synth_input("sc.tu", (1, 77, 768)),
                          text_cfg=7.5, img_cfg=1.5))
    res = pipe.run_stacked(calls, max_clips=20)
    assert len(res) == n
    for k in range(3, n):
        assert torch.equal(res[k]["latent"], res[k % 3]["latent"]), f"stacked clip {k} differs from its twin {k % 3}"
    base = pipe.run_stacked(calls, max_clips=None)
    for j in range(3):
        report(res[j]["latent"], base[j]["latent"].cpu(), f"run_stacked(max_clips=20) clip {j} vs the default grouping, 2 steps", 1e-2, 5e-2)
    del res, base
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ T5: refusal
def test_split_path_at_small_shapes_and_refusal_below_one_unit():
    """T5: with the window shrunk (ops.operand_window) small problems take the range path of all five launchers: bit-identical to one
    launch, ragged last tiles and the K / V stream offsets included; a window below ONE unit (a 128-row tile; a sample) is refused with
    INSV2V_EUNSUPPORTED, never run wrongly."""
    from insv2v import ops, _lib
    from insv2v.fused import pack_ffn_stream, pack_tattn_stream, pack_tattn_qkv_stream, pack_xattn_stream, pack_xattn_kv, pack_xattn_q_stream, pack_xattn640_kv
    from insv2v.unet import fold_layernorm
    H, L = 8, 77
    # feed-forward: 1000 rows = 8 tiles -> 3 ranges of 3 + 3 + 2 tiles
    C, NH, M = 320, 1280, 1000
    x, r2 = (rnd(M, C) * 1.3 + 0.2).half(), rnd(M, C, seed=8).half()
    wf, _, bf = fold_layernorm(rnd(2 * NH, C, scale=C ** -0.5).cpu(), (1 + 0.1 * rnd(C, seed=4)).cpu(), (0.1 * rnd(C, seed=5)).cpu(), (rnd(2 * NH, seed=1) * 0.3).cpu())
    w2, b2 = rnd(C, NH, scale=NH ** -0.5, seed=2).half().float().cpu(), (rnd(C, seed=3) * 0.3).cpu()
    wp, bp = rnd(C, C, scale=C ** -0.5, seed=6).half().float().cpu(), (rnd(C, seed=7) * 0.3).cpu()
    st, stp = pack_ffn_stream(wf.float(), bf, w2, b2).to(DEV), pack_ffn_stream(wf.float(), bf, w2, b2, post=(wp, bp)).to(DEV)
    whole, wholep = ops.ffn_fused(x, st, NH), ops.ffn_fused(x, stp, NH, post_residual=r2)
    with ops.operand_window(3 * 128 * C * 2 + 1):
        assert torch.equal(ops.ffn_fused(x, st, NH), whole) and torch.equal(ops.ffn_fused(x, stp, NH, post_residual=r2), wholep)
    with ops.operand_window(128 * C * 2):
        with pytest.raises(_lib.HipKernelError, match="unsupported"):
            ops.ffn_fused(x, st, NH)
    # temporal attention: 5 samples of an odd pixel count, 16 and 32 frame slots, masked windows -> ranges of 2 + 2 + 1 samples
    for C, F_, HW in ((320, 16, 13), (320, 9, 13), (320, 24, 13), (640, 16, 13), (640, 20, 13)):
        samples = 5
        x = (rnd(samples * F_ * HW, C, seed=F_) * 1.3 + 0.2).half()
        wqkv, table = rnd(3 * C, C, scale=C ** -0.5).half().float().cpu(), (rnd(F_, 3 * C, seed=1) * 0.4).cpu()
        if C == 320:
            stream = pack_tattn_stream(wqkv, table, rnd(C, C, scale=C ** -0.5, seed=2).half().float().cpu(), (rnd(C, seed=3) * 0.3).cpu()).to(DEV)
            fn = lambda: ops.tattn_fused(x, stream, samples, HW, H, F_)
        else:
            stream = pack_tattn_qkv_stream(wqkv, table).to(DEV)
            fn = lambda: ops.tattn_attn(x, stream, samples, HW, H, F_)
        whole = fn()
        with ops.operand_window(2 * F_ * HW * C * 2 + 1):
            assert torch.equal(fn(), whole), f"tattn C={C} F={F_}: sample ranges differ from one launch"
        with ops.operand_window(F_ * HW * C * 2):
            with pytest.raises(_lib.HipKernelError, match="unsupported"):
                fn()
    # text cross-attention: 5 samples of 300 rows (ragged third tile), each with its own K / V -> ranges of 2 + 2 + 1 samples
    for C in (320, 640):
        samples, R = 5, 300
        x, hres = (rnd(samples * R, C) * 1.3 + 0.2).half(), (rnd(samples * R, C, seed=14) * 1.1).half()
        wq, bq = rnd(C, C, scale=C ** -0.5).half().float().cpu(), (rnd(C, seed=5) * 0.3).cpu()
        wo, bo = rnd(C, C, scale=C ** -0.5, seed=2).half().float().cpu(), (rnd(C, seed=3) * 0.3).cpu()
        kv = (rnd(samples * L, 2 * C, seed=4) * 1.5).half()
        if C == 320:
            stream, pre = pack_xattn_stream(wq, bq, wo, bo).to(DEV), pack_xattn_stream(wq, bq, wo, bo, pre=(wo, bo)).to(DEV)
            kvs = pack_xattn_kv(kv, samples, L, C, H)
            fns = [lambda: ops.xattn_fused(x, stream, kvs, R, H, L), lambda: ops.xattn_fused(x, pre, kvs, R, H, L, pre_residual=hres)]
        else:
            stream, kvs = pack_xattn_q_stream(wq, bq).to(DEV), pack_xattn640_kv(kv, samples, L, C, H)
            fns = [lambda: ops.xattn_attn(x, stream, kvs, R, H, L)]
        for fn in fns:
            whole = fn()
            with ops.operand_window(2 * R * C * 2 + 1):
                assert torch.equal(fn(), whole), f"xattn C={C}: sample ranges differ from one launch"
            with ops.operand_window(R * C * 2):
                with pytest.raises(_lib.HipKernelError, match="unsupported"):
                    fn()
    torch.cuda.synchronize()


def test_sample_beyond_the_window_is_refused():
    """T5 at its real size: the temporal attention cannot split a sample.  One sample of 32 frames x 240 x 224 pixels (1920 x 1792 frames)
    at C = 640 is 2.2 GB: insv2v_tattn_attn answers INSV2V_EUNSUPPORTED before it launches anything, and the Python check that runs in
    front of every forward raises ValueError, naming the kernel, for the same geometry (a UNet whose first level is 640 wide; at the
    default widths that level is 320 wide and a sample is 1.1 GB, which runs)."""
    from insv2v import ops, _lib
    from insv2v.fused import check_operand_windows, OPERAND_WINDOW
    C, H, F_, h, w = 640, 8, 32, 240, 224
    HW = h * w
    assert F_ * HW * C * 2 >= OPERAND_WINDOW > F_ * HW * 320 * 2
    with pytest.raises(ValueError, match="insv2v_tattn_attn"):
        check_operand_windows(1, F_, h, w, channels=(640, 1280))
    check_operand_windows(1, F_, h, w)
    x = torch.zeros((F_ * HW, C), device=DEV, dtype=torch.float16)
    out = torch.empty_like(x)
    stream = torch.zeros(int(_lib.load().insv2v_tattn_attn_stream_elems(C, H, F_)), device=DEV, dtype=torch.float16)
    with pytest.raises(_lib.HipKernelError, match="insv2v_tattn_attn: unsupported"):
        ops.tattn_attn(x, stream, 1, HW, H, F_, out=out)
    torch.cuda.synchronize()
    del x, out
    torch.cuda.empty_cache()
