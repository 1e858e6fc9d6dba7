"""The fused temporal-attention kernels at every window length 1 .. 32 frames (insv2v_tattn_fused at C = 320, insv2v_tattn_attn at C = 640):
against fp32 torch and the unfused path, masked padding keys, padded frame slots never written, and the motion modules at 24, 8 and 20
frames against the fp32 oracle with the launch sequence they take."""
import math

import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WINDOWS = [1, 7, 8, 12, 16, 17, 24, 31, 32]


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def close(out, ref, rel=4e-3, abs_=4e-3, what=""):
    out, ref = out.float(), ref.float()
    err = (out - ref).abs().max().item()
    tol = rel * ref.abs().max().item() + abs_
    assert math.isfinite(err) and err <= tol, f"{what}: max err {err:.4g} > tol {tol:.4g} (ref max {ref.abs().max().item():.4g})"


def _problem(C, F_, samples, HW, seed=0, negative=False):
    M = samples * F_ * HW
    x = (rnd(M, C, seed=seed) * 1.3 + 0.2).half()
    wqkv = rnd(3 * C, C, scale=C ** -0.5, seed=seed + 1).half()
    table = rnd(F_, 3 * C, seed=seed + 2) * 0.4
    if negative:
        # q = +u, k = -u per head on top of the data: every valid score is strongly negative, so a padding key (score 0) left in the
        # softmax would set its shift and swamp the valid keys
        u = torch.ones(C, device=DEV) * 1.5
        table[:, :C] += u
        table[:, C:2 * C] -= u
    return x, wqkv, table


def _reference(x, wqkv, table, samples, F_, HW, H):
    M, C = x.shape
    D = C // H
    xf = x.float()
    xn = (xf - xf.mean(1, keepdim=True)) * (xf.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    frame = (torch.arange(M, device=DEV) // HW) % F_
    qkv = (xn @ wqkv.float().t() + table[frame]).half().float().reshape(samples, F_, HW, 3, H, D)
    q, k, v = (qkv[:, :, :, i].permute(0, 2, 3, 1, 4) for i in range(3))         # [b, pixel, head, frame, d]
    return Fn.scaled_dot_product_attention(q, k, v).permute(0, 3, 1, 2, 4).reshape(M, C)


def _unfused_attention(x, wqkv, table, samples, F_, HW, H):
    """LayerNorm-ed row Linear for q/k/v, the per-frame table added in torch, the generic attention kernel."""
    from insv2v import ops
    from insv2v.fused import pack_linear_stream
    M, C = x.shape
    D = C // H
    qkv = ops.rowlin(x, pack_linear_stream(wqkv.float().cpu(), None).to(DEV), 3 * C, layernorm=True)
    frame = (torch.arange(M, device=DEV) // HW) % F_
    qkv = (qkv.float() + table[frame]).half()
    a = torch.empty((M, C), device=DEV, dtype=torch.float16)
    p = qkv.data_ptr()
    addr = (HW, F_ * HW * 3 * C, 3 * C)
    ops.attention(p, p + 2 * C, p + 4 * C, a, batch=samples * HW, heads=H, head_dim=D, seq_q=F_, seq_k=F_, scale=D ** -0.5,
                  q_rs=HW * 3 * C, k_rs=HW * 3 * C, v_rs=HW * 3 * C, o_rs=HW * C, q_addr=addr, kv_addr=addr, o_addr=(HW, F_ * HW * C, C))
    return a


@pytest.mark.parametrize("F_", WINDOWS)
def test_tattn_fused_windows_vs_fp32(F_):
    """C = 320: 3 samples x 13 pixels = 39 pixels (ragged last tile of 8 or 4 pixels)."""
    from insv2v import ops
    from insv2v.fused import pack_tattn_stream, pack_linear_stream
    C, H, samples, HW = 320, 8, 3, 13
    assert ops.tattn_fused_supported(C, H, F_)
    x, wqkv, table = _problem(C, F_, samples, HW, seed=F_)
    wo, bo = rnd(C, C, scale=C ** -0.5, seed=2).half(), rnd(C, seed=3) * 0.3
    stream = pack_tattn_stream(wqkv.float().cpu(), table.cpu(), wo.float().cpu(), bo.cpu()).to(DEV)
    out = ops.tattn_fused(x, stream, samples, HW, H, F_)
    ref = _reference(x, wqkv, table, samples, F_, HW, H).half().float() @ wo.float().t() + bo + x.float()
    close(out, ref, what=f"tattn_fused F={F_}")
    a2 = _unfused_attention(x, wqkv, table, samples, F_, HW, H)
    two = ops.rowlin(a2, pack_linear_stream(wo.float().cpu(), bo.cpu()).to(DEV), C, residual=x)
    close(out, two, what=f"tattn_fused vs unfused F={F_}")
    assert torch.equal(out, ops.tattn_fused(x, stream, samples, HW, H, F_)), "not deterministic"


@pytest.mark.parametrize("F_", WINDOWS)
def test_tattn_attn_640_windows_vs_fp32(F_):
    """C = 640: 2 samples x 11 pixels = 22 pixels (ragged last tile)."""
    from insv2v import ops
    from insv2v.fused import pack_tattn_qkv_stream
    C, H, samples, HW = 640, 8, 2, 11
    assert ops.tattn_attn_supported(C, H, F_)
    x, wqkv, table = _problem(C, F_, samples, HW, seed=F_)
    stream = pack_tattn_qkv_stream(wqkv.float().cpu(), table.cpu()).to(DEV)
    out = ops.tattn_attn(x, stream, samples, HW, H, F_)
    close(out, _reference(x, wqkv, table, samples, F_, HW, H), what=f"tattn_attn F={F_}")
    close(out, _unfused_attention(x, wqkv, table, samples, F_, HW, H), what=f"tattn_attn vs unfused F={F_}")
    assert torch.equal(out, ops.tattn_attn(x, stream, samples, HW, H, F_)), "not deterministic"


@pytest.mark.parametrize("F_", [8, 24])
def test_tattn_windows_mask_padding_keys(F_):
    """Every valid score strongly negative: an unmasked padding key (score 0) would take over the softmax."""
    from insv2v import ops
    from insv2v.fused import pack_tattn_stream, pack_tattn_qkv_stream
    samples, HW, H = 2, 9, 8
    x, wqkv, table = _problem(320, F_, samples, HW, seed=40 + F_, negative=True)
    wo, bo = rnd(320, 320, scale=320 ** -0.5, seed=5).half(), rnd(320, seed=6) * 0.3
    out = ops.tattn_fused(x, pack_tattn_stream(wqkv.float().cpu(), table.cpu(), wo.float().cpu(), bo.cpu()).to(DEV), samples, HW, H, F_)
    a = _reference(x, wqkv, table, samples, F_, HW, H)
    close(out, a.half().float() @ wo.float().t() + bo + x.float(), what=f"tattn_fused negative scores F={F_}")
    x, wqkv, table = _problem(640, F_, samples, HW, seed=50 + F_, negative=True)
    out = ops.tattn_attn(x, pack_tattn_qkv_stream(wqkv.float().cpu(), table.cpu()).to(DEV), samples, HW, H, F_)
    close(out, _reference(x, wqkv, table, samples, F_, HW, H), what=f"tattn_attn negative scores F={F_}")


@pytest.mark.parametrize("F_", [7, 12, 20])
def test_tattn_windows_never_write_padded_slots(F_):
    """A padded slot's row (b F + fr) HW + p, fr >= F, lies in the next sample's rows or past the tensor: `out` is a view of the first M rows
    of a sentinel-filled buffer (and once with ldo > C); the tail and the extra columns stay untouched, every sample's rows are right."""
    from insv2v import ops
    from insv2v.fused import pack_tattn_stream, pack_tattn_qkv_stream
    samples, HW, H = 3, 5, 8
    for C in (320, 640):
        x, wqkv, table = _problem(C, F_, samples, HW, seed=60 + F_ + C)
        M = x.shape[0]
        if C == 320:
            wo, bo = rnd(C, C, scale=C ** -0.5, seed=7).half(), rnd(C, seed=8) * 0.3
            stream = pack_tattn_stream(wqkv.float().cpu(), table.cpu(), wo.float().cpu(), bo.cpu()).to(DEV)
            ref = _reference(x, wqkv, table, samples, F_, HW, H).half().float() @ wo.float().t() + bo + x.float()
            run = ops.tattn_fused
        else:
            stream = pack_tattn_qkv_stream(wqkv.float().cpu(), table.cpu()).to(DEV)
            ref = _reference(x, wqkv, table, samples, F_, HW, H)
            run = ops.tattn_attn
        for extra_cols in (0, 64):
            buf = torch.full((M + 32 * HW, C + extra_cols), -777.0, device=DEV, dtype=torch.float16)
            out = buf[:M, :C]
            assert run(x, stream, samples, HW, H, F_, out=out) is out
            torch.cuda.synchronize()
            assert bool((buf[M:] == -777.0).all()), f"C={C} F={F_}: rows past the tensor written"
            if extra_cols:
                assert bool((buf[:M, C:] == -777.0).all()), f"C={C} F={F_}: columns past C written"
            close(out, ref, what=f"C={C} F={F_} ldo={C + extra_cols}")


def _motion_pair(C, F_):
    from insv2v import synth, shapes, unet as U
    import oracle.unet3d as ou
    mkw = synth.UNET_FULL["motion_module_kwargs"]
    d = {}
    shapes._motion(d, f"mmw{C}", C, mkw)
    sd = synth.synth_state_dict(d)
    mm = U.MotionModule(sd, f"mmw{C}", C, 32, DEV, **mkw)
    ora = ou.MotionModule(C, 32, **mkw).eval()
    ora.load_state_dict({k[len(f"mmw{C}."):]: v for k, v in sd.items()})
    return mm, ora


def _to_cl(x):
    from insv2v.unet import Act
    b, c, f, h, w = x.shape
    return Act(x.permute(0, 2, 3, 4, 1).reshape(b * f * h * w, c).to(device=DEV, dtype=torch.float16).contiguous(), b, f, h, w)


@pytest.mark.parametrize("C", [320, 640])
def test_motion_module_windows_vs_oracle(C):
    """Full-width motion modules at 24 frames, 8 frames and 20 frames starting at positional-encoding row 12, against the fp32 oracle; the
    launches: the fused kernel and no generic attention or LayerNorm-statistics launch for 24 / 20 frames, the route DESIGN.md section 9 records
    (row-linear q/k/v + the short attention kernel) for 8."""
    from insv2v import ops, synth
    mm, ora = _motion_pair(C, 24)
    B, H, W = 2, 4, 6
    fused_kind = "tattn" if C == 320 else "tattn_attn"
    for F_, start in ((24, 0), (8, 0), (20, 12)):
        x = synth.synth_input(f"mmw{C}.x{F_}", (B, C, F_, H, W))
        rec = []
        ops.set_launch_recorder(rec)
        try:
            a = mm(_to_cl(x), start)
            torch.cuda.synchronize()
        finally:
            ops.set_launch_recorder(None)
        kinds = [t[4][0] for t in rec if len(t) > 4 and t[4]]
        if F_ > 16:
            assert kinds.count(fused_kind) == 2 and "attn" not in kinds and "lnstats" not in kinds, kinds
        else:
            assert fused_kind not in kinds and kinds.count("attn") == 2 and "lnstats" not in kinds, kinds
        out = a.t.float().reshape(B, F_, H, W, C).permute(0, 4, 1, 2, 3).cpu()
        with torch.no_grad():
            ref = ora(x.float(), start)
        rms = ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
        mx = ((out - ref).abs().max() / ref.abs().max()).item()
        print(f"[parity] motion module C={C} F={F_} start={start}: rel-rms {rms:.3e}  max-abs/max-ref {mx:.3e}")
        assert math.isfinite(rms) and rms <= 1e-2 and mx <= 4e-2, (C, F_, start, rms, mx)
        assert (out - x).abs().max() > 1e-2   # the temporal path is live
