"""The text cross-attention kernels (insv2v_xattn_fused, C = 320; insv2v_xattn_attn, C = 640) and the GroupNorm fold of insv2v_rowlin at
token counts that do not line up with their tiles: rows_per_sample not a multiple of 128, gn_rows not a multiple of 32 - the frame sizes
whose latent sides are not multiples of 8 (480x480: 3600 / 900 pixels per frame; the 9x8 golden: 72 / 20).

References and tolerances are those of the aligned tests in tests/test_kernels_gpu.py (test_xattn_fused_vs_fp32, test_xattn_attn_640_vs_fp32,
test_rowlin_fused_groupnorm): rel 4e-3 + abs 4e-3 against fp32 torch on the same fp16-rounded operands and between the fused and unfused
forms, rel 3e-3 + abs 3e-3 of the fused GroupNorm against GroupNorm kernel + row Linear.  The per-row arithmetic does not depend on the
row schedule, so ragged shapes get no wider margin.  Model level: the bounds of test_unet_full_width_anysize_vs_golden."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.25   # exactly representable in fp16; not a value any case produces in a whole row


def dev():
    return torch.device(DEV)


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).to(dev())


def close(out, ref, rel, abs_, what=""):
    out, ref = out.float(), ref.float()
    err, tol = (out - ref).abs().max().item(), rel * ref.abs().max().item() + abs_
    print(f"[kernel] {what}: max err {err:.4g} (tol {tol:.4g})")
    assert math.isfinite(err) and err <= tol, f"{what}: max err {err:.4g} > tol {tol:.4g}"


def guarded(M, N, extra=160):
    """out = the first M rows of a larger buffer filled with a sentinel; check_guard: the rows beyond M kept it."""
    buf = torch.full((M + extra, N), SENTINEL, device=dev(), dtype=torch.float16)
    return buf, buf[:M]


def check_guard(buf, M, what):
    assert bool((buf[M:] == SENTINEL).all()), f"{what}: rows beyond M = {M} were written"


def layernorm_rows(xf):
    return ((xf - xf.mean(1, keepdim=True)) * (xf.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()).half().float()


# ------------------------------------------------------------------------------------------- insv2v_xattn_fused, C = 320
def _xattn320_case(samples, rows, L):
    from insv2v.fused import pack_xattn_stream, pack_xattn_kv
    C, H = 320, 8
    M = samples * rows
    x = (rnd(M, C) * 1.3 + 0.2).half()
    wq, bq = rnd(C, C, scale=C ** -0.5).half(), rnd(C, seed=5) * 0.3
    wo, bo = rnd(C, C, scale=C ** -0.5, seed=2).half(), rnd(C, seed=3) * 0.3
    kv = (rnd(samples * L, 2 * C, seed=4) * 1.5).half()   # distinct K / V per sample: a row on its neighbour's stream fails by value
    stream = pack_xattn_stream(wq.float().cpu(), bq.cpu(), wo.float().cpu(), bo.cpu()).to(dev())
    kvs = pack_xattn_kv(kv, samples, L, C, H)
    return x, wq, bq, wo, bo, kv, stream, kvs


@pytest.mark.parametrize("samples,rows,L", [(3, 72, 77), (3, 129, 77), (2, 200, 77), (3, 320, 77), (3, 128, 77), (2, 200, 96)])
def test_xattn_fused_ragged(samples, rows, L):
    """insv2v_xattn_fused at rows_per_sample below one tile, one row into the second tile, 200, the 9x8 golden's level-1 count and the
    aligned control: against fp32, against the unfused three launches, the form with the leading out-projection, deterministic, and no
    row beyond M written."""
    from insv2v import ops
    from insv2v.fused import pack_xattn_stream, pack_linear_stream
    C, H, D = 320, 8, 40
    M = samples * rows
    x, wq, bq, wo, bo, kv, stream, kvs = _xattn320_case(samples, rows, L)
    assert ops.xattn_fused_supported(C, H, L, rows)
    buf, out = guarded(M, C)
    ops.xattn_fused(x, stream, kvs, rows, H, L, out=out)
    check_guard(buf, M, "xattn_fused")
    xf = x.float()
    q = (layernorm_rows(xf) @ wq.float().t() + bq).half().float().reshape(samples, rows, H, D).permute(0, 2, 1, 3)
    k = kv[:, :C].float().reshape(samples, L, H, D).permute(0, 2, 1, 3)
    v = kv[:, C:].float().reshape(samples, L, H, D).permute(0, 2, 1, 3)
    a = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(M, C).half().float()
    ref = a @ wo.float().t() + bo + xf
    close(out, ref, 4e-3, 4e-3, what=f"xattn_fused samples={samples} rows={rows} L={L}")
    q2 = ops.rowlin(x, pack_linear_stream(wq.float().cpu(), bq.cpu()).to(dev()), C, layernorm=True)
    a2 = torch.empty((M, C), device=dev(), dtype=torch.float16)
    kp = kv.data_ptr()
    ops.attention(q2.data_ptr(), kp, kp + 2 * C, a2, batch=samples, heads=H, head_dim=D, seq_q=rows, seq_k=L, scale=D ** -0.5,
                  q_rs=C, k_rs=2 * C, v_rs=2 * C, o_rs=C, q_addr=(1, rows * C, 0), kv_addr=(1, L * 2 * C, 0), o_addr=(1, rows * C, 0))
    two = ops.rowlin(a2, pack_linear_stream(wo.float().cpu(), bo.cpu()).to(dev()), C, residual=x)
    close(out, two, 4e-3, 4e-3, what=f"xattn_fused vs unfused samples={samples} rows={rows} L={L}")
    assert torch.equal(out, ops.xattn_fused(x, stream, kvs, rows, H, L)), "not deterministic"
    # + the preceding self-attention's output projection in the same launch
    wo1, bo1 = rnd(C, C, scale=C ** -0.5, seed=11).half(), rnd(C, seed=12) * 0.3
    a1, hres = (rnd(M, C, seed=13) * 0.8).half(), (rnd(M, C, seed=14) * 1.1 + 0.1).half()
    pre_stream = pack_xattn_stream(wq.float().cpu(), bq.cpu(), wo.float().cpu(), bo.cpu(), pre=(wo1.float().cpu(), bo1.cpu())).to(dev())
    bufp, out_pre = guarded(M, C)
    ops.xattn_fused(a1, pre_stream, kvs, rows, H, L, pre_residual=hres, out=out_pre)
    check_guard(bufp, M, "xattn_fused with leading out-projection")
    x1 = ops.rowlin(a1, pack_linear_stream(wo1.float().cpu(), bo1.cpu()).to(dev()), C, residual=hres)
    close(out_pre, ops.xattn_fused(x1, stream, kvs, rows, H, L), 4e-3, 4e-3, what=f"xattn_fused with leading out-projection samples={samples} rows={rows}")
    assert torch.equal(out_pre, ops.xattn_fused(a1, pre_stream, kvs, rows, H, L, pre_residual=hres)), "not deterministic"


# ------------------------------------------------------------------------------------------- insv2v_xattn_attn, C = 640
def _xattn640_case(samples, rows, L):
    from insv2v.fused import pack_xattn_q_stream, pack_xattn640_kv
    C, H = 640, 8
    x = (rnd(samples * rows, C) * 1.3 + 0.2).half()
    wq, bq = rnd(C, C, scale=C ** -0.5).half(), rnd(C, seed=5) * 0.3
    kv = (rnd(samples * L, 2 * C, seed=4) * 1.5).half()
    stream = pack_xattn_q_stream(wq.float().cpu(), bq.cpu()).to(dev())
    kvs = pack_xattn640_kv(kv, samples, L, C, H)
    return x, wq, bq, kv, stream, kvs


@pytest.mark.parametrize("samples,rows", [(3, 72), (3, 320), (2, 200), (1, 128)])
def test_xattn_attn_640_ragged(samples, rows):
    """insv2v_xattn_attn at ragged rows_per_sample (and the aligned control) against fp32 and the unfused route."""
    from insv2v import ops
    from insv2v.fused import pack_linear_stream
    C, H, D, L = 640, 8, 80, 77
    M = samples * rows
    x, wq, bq, kv, stream, kvs = _xattn640_case(samples, rows, L)
    assert ops.xattn_attn_supported(C, H, L, rows)
    buf, out = guarded(M, C)
    ops.xattn_attn(x, stream, kvs, rows, H, L, out=out)
    check_guard(buf, M, "xattn_attn")
    q = (layernorm_rows(x.float()) @ wq.float().t() + bq).half().float().reshape(samples, rows, H, D).permute(0, 2, 1, 3)
    k = kv[:, :C].float().reshape(samples, L, H, D).permute(0, 2, 1, 3)
    v = kv[:, C:].float().reshape(samples, L, H, D).permute(0, 2, 1, 3)
    ref = F.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3).reshape(M, C)
    close(out, ref, 4e-3, 4e-3, what=f"xattn_attn samples={samples} rows={rows}")
    q2 = ops.rowlin(x, pack_linear_stream(wq.float().cpu(), bq.cpu()).to(dev()), C, layernorm=True)
    a2 = torch.empty((M, C), device=dev(), dtype=torch.float16)
    kp = kv.data_ptr()
    ops.attention(q2.data_ptr(), kp, kp + 2 * C, a2, batch=samples, heads=H, head_dim=D, seq_q=rows, seq_k=L, scale=D ** -0.5,
                  q_rs=C, k_rs=2 * C, v_rs=2 * C, o_rs=C, q_addr=(1, rows * C, 0), kv_addr=(1, L * 2 * C, 0), o_addr=(1, rows * C, 0))
    close(out, a2, 4e-3, 4e-3, what=f"xattn_attn vs unfused samples={samples} rows={rows}")
    assert torch.equal(out, ops.xattn_attn(x, stream, kvs, rows, H, L)), "not deterministic"


# ------------------------------------------------------------------------------------------- position invariance
def test_xattn_position_invariance():
    """At rows_per_sample = 200 a sample launched alone equals the same sample as the third of three, bit for bit, on both kernels (the
    stacked forwards rely on samples being independent of their position)."""
    from insv2v import ops
    rows, L, H = 200, 77, 8
    x, _, _, _, _, _, stream, kvs = _xattn320_case(3, rows, L)
    stack = ops.xattn_fused(x, stream, kvs, rows, H, L)
    alone = ops.xattn_fused(x[2 * rows:].contiguous(), stream, kvs[2:].contiguous(), rows, H, L)
    assert torch.equal(alone, stack[2 * rows:]), "xattn_fused: the third sample of three differs from the same sample alone"
    x, _, _, _, stream, kvs = _xattn640_case(3, rows, L)
    stack = ops.xattn_attn(x, stream, kvs, rows, H, L)
    alone = ops.xattn_attn(x[2 * rows:].contiguous(), stream, kvs[2:].contiguous(), rows, H, L)
    assert torch.equal(alone, stack[2 * rows:]), "xattn_attn: the third sample of three differs from the same sample alone"


# ------------------------------------------------------------------------------------------- insv2v_rowlin(gn_ab=...)
@pytest.mark.parametrize("K,nsamples,rows", [(320, 5, 72), (320, 4, 20), (320, 3, 33), (640, 3, 225), (320, 6, 96)])
def test_rowlin_fused_groupnorm_ragged(K, nsamples, rows):
    """The GroupNorm fold at gn_rows that are no multiple of a wave's 32 rows (scale and shift distinct per sample) == GroupNorm kernel +
    row kernel, == fp32 torch; no row beyond M written."""
    from insv2v import ops
    from insv2v.fused import pack_linear_stream
    M, N, G = nsamples * rows, K, 32
    x = (rnd(M, K) * 1.7 + 0.4).half()
    gamma, beta = 1 + 0.1 * rnd(K, seed=1), 0.1 * rnd(K, seed=2)
    w, b = rnd(N, K, scale=K ** -0.5, seed=3).half(), rnd(N, seed=4) * 0.3
    st = pack_linear_stream(w.float().cpu(), b.cpu()).to(dev())
    ab = ops.groupnorm_stats(x, nsamples, rows, gamma, beta, G, 1e-6)
    buf, out = guarded(M, N)
    ops.rowlin(x, st, N, gn_ab=ab, gn_rows=rows, out=out)
    check_guard(buf, M, "rowlin with the GroupNorm fold")
    two = ops.rowlin(ops.groupnorm(x, nsamples, rows, gamma, beta, G, 1e-6), st, N)
    close(out, two, 3e-3, 3e-3, what=f"fused GroupNorm vs GroupNorm kernel + rowlin K={K} {nsamples}x{rows}")
    xr = x.float().reshape(nsamples, rows, K).permute(0, 2, 1)
    ref = F.group_norm(xr, G, gamma, beta, 1e-6).permute(0, 2, 1).reshape(M, K) @ w.float().t() + b
    close(out, ref, 4e-3, 4e-3, what=f"fused GroupNorm + rowlin vs fp32 K={K} {nsamples}x{rows}")
    assert torch.equal(out, ops.rowlin(x, st, N, gn_ab=ab, gn_rows=rows)), "not deterministic"


# ------------------------------------------------------------------------------------------- model level
def test_unet_full_width_ragged_uses_fused_rows(golden):
    """The full-width UNet on the CFG triple at latent 9x8 (72 and 20 pixels per frame at the two row-kernel levels; inputs and bounds of
    test_unet_full_width_anysize_vs_golden) takes the aligned shapes' routes: the C = 640 cross-attention as insv2v_xattn_attn, every
    C = 320 / 640 transformer and motion GroupNorm as statistics + fold, no generic attention over the text at levels 0 and 1."""
    from insv2v import synth, shapes, ops
    from insv2v.unet import UNet3DConditionModel
    g = golden("unet_full_anysize")["out"]
    unet = UNet3DConditionModel(**synth.UNET_FULL, device=DEV).load_state_dict(synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_FULL)))
    lat = synth.synth_input("anysize.full.latent", (1, 4, 16, 9, 8))   # [b, c, f, h, w]
    cond = synth.synth_input("anysize.full.cond", (1, 4, 16, 9, 8))
    tu, tc = synth.synth_input("anysize.full.tu", (1, 77, 768)), synth.synth_input("anysize.full.tc", (1, 77, 768))
    ctx = torch.cat([tu, tu, tc], 0)
    x = torch.cat([torch.cat([lat, torch.zeros_like(cond)], 1), torch.cat([lat, cond], 1), torch.cat([lat, cond], 1)], 0)
    rec = []
    ops.set_launch_recorder(rec)
    try:
        out = unet(x, torch.full((3,), 481, dtype=torch.long), encoder_hidden_states=ctx).sample
    finally:
        ops.set_launch_recorder(None)
    torch.cuda.synchronize()
    o, r = out.detach().float().cpu(), torch.as_tensor(g).float()
    rms = ((o - r).pow(2).mean().sqrt() / r.pow(2).mean().sqrt()).item()
    mx = ((o - r).abs().max() / r.abs().max()).item()
    print(f"[parity] full-width UNet fwd 9x8 CFG triple, fused row kernels: rel-rms {rms:.3e}  max-abs/max-ref {mx:.3e}")
    assert o.shape == r.shape and math.isfinite(rms) and rms <= 1e-2 and mx <= 4e-2, (rms, mx)
    tags = [e[4] for e in rec if len(e) > 4]
    # level 0: 3 x 16 x 72 = 3456 rows at C = 320; level 1: 3 x 16 x 20 = 960 rows at C = 640
    assert any(t[0] == "xattn_attn" and t[1] == 960 for t in tags), "no insv2v_xattn_attn launch with M = 960"
    assert any(t[0] == "xattn" and t[1] == 3456 for t in tags), "no insv2v_xattn_fused launch with M = 3456"
    # GroupNorm of a transformer / motion module: per (sample, frame) over HW pixels; the ResnetBlock norms span all frames of a sample
    copies = [t for t in tags if t[0] == "gn" and t[2] in (72, 20) and t[3] in (320, 640)]
    assert not copies, f"GroupNorm launches that write a normalised copy in front of a C = 320 / 640 proj_in: {copies}"
    for hw, c in ((72, 320), (20, 640)):
        assert any(t[0] == "gnstats" and t[2:] == (hw, c) for t in tags), f"no statistics-only GroupNorm over {hw} pixels at C = {c}"
    text = [t for t in tags if t[0] == "attn" and t[5] == 77 and t[3] in (40, 80)]
    assert not text, f"generic attention over the text tokens at levels 0 / 1: {text}"
    del unet
    torch.cuda.empty_cache()
