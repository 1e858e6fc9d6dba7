"""Flash attention for the VAE's 512-channel mid block: insv2v_attention at head_dim = 512, VAttn without its score matrix, the VAE at
frame sizes whose score matrix no longer fits one operand window.

Tolerances
  kernel level   that of the attention tests in tests/test_kernels_gpu.py: max err <= 4e-3 max|ref| + 2e-3 ("P in fp16");
  block / VAE    rel-RMS <= 1e-2, max-abs <= 4e-2 max|ref| (tests/test_model_gpu.py, test_vae_attention_any_hw).
The reference is always fp32 / float64 torch softmax(q k^T scale) v on the same fp16-rounded operands, never the code under test.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 512
SENTINEL = 0x5A5A          # fp16 bit pattern (205.25) of every output element the kernel must not touch
PAD_ROWS = 37              # rows behind every problem's keys: k = 30, v = 1000


def dev():
    return torch.device(DEV)


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).to(dev())


def close(out, ref, rel=4e-3, abs_=2e-3, what=""):
    out, ref = out.float(), ref.float()
    err, tol = (out - ref).abs().max().item(), rel * ref.abs().max().item() + abs_
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


# ------------------------------------------------------------------------------------------- kernel level
def run_d512(q, k, v, scale, ref_dtype=torch.float32, what=""):
    """q [B, Sq, 512], k / v [B, Sk, 512] (CPU or device, any float type) through ops.attention in the hostile layout:
      * q | k | v are column ranges of ONE [rows, 1536] fp16 matrix with max(Sq, Sk) + 37 rows per problem behind 3 leading rows; every
        row that is not a key of its problem holds k = 30, v = 1000 (one key read past the end moves the result by far more than the
        tolerance), every row that is not a query holds q = 30;
      * the output goes into a sentinel-filled buffer with 5 spare rows per problem, 2 leading rows and 8 + 16 spare columns; everything
        outside [Sq, 512] of each problem must keep the sentinel's bit pattern.
    Checked against softmax(q k^T scale) v in ref_dtype on the fp16-rounded operands."""
    from insv2v import ops
    B, Sq, _ = q.shape
    Sk = k.shape[1]
    R, lead = max(Sq, Sk) + PAD_ROWS, 3
    qh, kh, vh = (t.to(dev()).half() for t in (q, k, v))
    m = torch.empty((lead + B * R, 3 * D), device=dev(), dtype=torch.float16)
    m[:, :2 * D] = 30.0
    m[:, 2 * D:] = 1000.0
    body = m[lead:].view(B, R, 3 * D)
    body[:, :Sq, :D] = qh
    body[:, :Sk, D:2 * D] = kh
    body[:, :Sk, 2 * D:] = vh
    OR, OC, olead, ocol = Sq + 5, D + 24, 2, 8
    obuf = torch.full((olead + B * OR + 1, OC), SENTINEL, device=dev(), dtype=torch.int16).view(torch.float16)
    p = m.data_ptr() + lead * 3 * D * 2
    o_view = obuf[olead:, ocol:]             # data_ptr = first element of problem 0
    ops.attention(p, p + 2 * D, p + 4 * D, o_view, batch=B, heads=1, head_dim=D, seq_q=Sq, seq_k=Sk, scale=scale,
                  q_rs=3 * D, k_rs=3 * D, v_rs=3 * D, o_rs=OC, q_addr=(1, R * 3 * D, 0), kv_addr=(1, R * 3 * D, 0), o_addr=(1, OR * OC, 0))
    torch.cuda.synchronize()
    res = obuf[olead:olead + B * OR].view(B, OR, OC)
    out = res[:, :Sq, ocol:ocol + D]
    untouched = torch.ones_like(obuf, dtype=torch.bool)
    untouched[olead:olead + B * OR].view(B, OR, OC)[:, :Sq, ocol:ocol + D] = False
    bits = obuf.view(torch.int16)
    assert bool((bits[untouched] == SENTINEL).all()), f"{what}: the kernel wrote outside [seq_q, 512] of a problem"
    assert torch.isfinite(out).all(), f"{what}: non-finite output"
    w = torch.softmax(qh.to(ref_dtype) @ kh.to(ref_dtype).transpose(1, 2) * scale, -1)
    close(out, w @ vh.to(ref_dtype), what=what)
    return out


SEQS = [(1, 1), (1, 33), (15, 17), (16, 32), (17, 31), (33, 65), (63, 64), (64, 63), (65, 129), (127, 33), (129, 257), (257, 1)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("seq_q,seq_k", SEQS)
def test_d512_sequence_lengths(seq_q, seq_k, batch):
    """+-1 around every multiple of 16 / 32 / 64 / 128 a tile plan could use: one partial tile, a ragged last tile, a partial last query
    block / workgroup (the kernel: 16 query rows per wave, 64 per workgroup, 32-key tiles)."""
    q, k, v = rnd(batch, seq_q, D, seed=1), rnd(batch, seq_k, D, seed=2), rnd(batch, seq_k, D, seed=3)
    run_d512(q, k, v, D ** -0.5, what=f"d=512 seq_q={seq_q} seq_k={seq_k} batch={batch}")


@pytest.mark.parametrize("seq_q,seq_k,batch", [(40, 40, 2), (70, 31, 4), (5, 97, 2)])
def test_d512_poison_and_strided_operands(seq_q, seq_k, batch):
    """Queries that line up with the poison rows: q = +|q| makes q . (30, 30, ...) the largest logit by hundreds, so a single poison key
    inside the softmax turns the output into v = 1000.  Layout and sentinel check: run_d512."""
    q, k, v = rnd(batch, seq_q, D, seed=4).abs(), rnd(batch, seq_k, D, seed=5), rnd(batch, seq_k, D, seed=6)
    out = run_d512(q, k, v, D ** -0.5, what=f"d=512 poison seq_q={seq_q} seq_k={seq_k} batch={batch}")
    assert out.float().abs().max().item() < 10.0


@pytest.mark.parametrize("case", ["rising", "falling"])
@pytest.mark.parametrize("seq", [257, 100])
def test_d512_running_maximum_rescale(case, seq):
    """Key j scaled by 1 + 6 j / seq_k: the maximum rises tile by tile (the accumulators are rescaled again and again); the mirror, where
    the first keys dominate and everything later is far below the maximum.  q is scaled so that the logits reach about +-60; float64
    reference; all finite."""
    B = 2
    q, k, v = rnd(B, seq, D, seed=7) * 2.5, rnd(B, seq, D, seed=8), rnd(B, seq, D, seed=9)
    j = torch.arange(seq, device=dev()).float().view(1, seq, 1)
    if case == "falling":
        j = seq - 1 - j
    k = k * (1 + j / seq * 6)
    logits = (q.half().double() @ k.half().double().transpose(1, 2)) * D ** -0.5
    print(f"[kernel] logits in [{logits.min().item():.1f}, {logits.max().item():.1f}]")
    assert 40 < logits.abs().max().item() < 120
    run_d512(q, k, v, D ** -0.5, ref_dtype=torch.float64, what=f"d=512 {case} maximum seq={seq}")


def test_d512_two_heads():
    """heads = 2 x 512 in fused qkv rows (row stride 3 * 1024), seq 65: head addressing."""
    from insv2v import ops
    BF, HW, heads = 2, 65, 2
    C = heads * D
    qkv = rnd(BF * HW, 3 * C).half()
    out = torch.empty((BF * HW, C), device=dev(), dtype=torch.float16)
    p = qkv.data_ptr()
    ops.attention(p, p + 2 * C, p + 4 * C, out, batch=BF, heads=heads, head_dim=D, seq_q=HW, seq_k=HW, scale=D ** -0.5,
                  q_rs=3 * C, k_rs=3 * C, v_rs=3 * C, o_rs=C, q_addr=(1, HW * 3 * C, 0), kv_addr=(1, HW * 3 * C, 0), o_addr=(1, HW * C, 0))
    t = qkv.reshape(BF, HW, 3, heads, D).permute(2, 0, 3, 1, 4).float()
    ref = (torch.softmax(t[0] @ t[1].transpose(-1, -2) * D ** -0.5, -1) @ t[2]).permute(0, 2, 1, 3).reshape(BF * HW, C)
    close(out, ref, what="d=512 two heads")


def _plain_call(head_dim, seq=20, **kw):
    from insv2v import ops
    C = head_dim
    qkv = rnd(seq, 3 * C).half()
    out = torch.zeros((seq, C), device=dev(), dtype=torch.float16)
    p = qkv.data_ptr()
    ops.attention(p, p + 2 * C, p + 4 * C, out, batch=1, heads=1, head_dim=head_dim, seq_q=seq, seq_k=seq, scale=C ** -0.5,
                  q_rs=3 * C, k_rs=3 * C, v_rs=3 * C, o_rs=C, q_addr=(1, 0, 0), kv_addr=(1, 0, 0), o_addr=(1, 0, 0), **kw)
    torch.cuda.synchronize()
    return out


def test_d512_refusals():
    """causal or bias tables with d = 512: INSV2V_EUNSUPPORTED, never silently ignored; head_dim = 256 stays INSV2V_EINVAL."""
    from insv2v._lib import HipKernelError
    with pytest.raises(HipKernelError, match="unsupported configuration"):
        _plain_call(512, causal=True)
    with pytest.raises(HipKernelError, match="unsupported configuration"):
        _plain_call(512, seq=16, qkv_bias=torch.zeros((16, 3 * 512), device=dev(), dtype=torch.float16))
    with pytest.raises(HipKernelError, match="unsupported configuration"):
        _plain_call(512, seq=40, qkv_bias=torch.zeros((40, 3 * 512), device=dev(), dtype=torch.float16))
    with pytest.raises(HipKernelError, match="invalid argument"):
        _plain_call(256)
    assert torch.isfinite(_plain_call(512)).all()      # the same call without the flags runs


# ------------------------------------------------------------------------------------------- block level
def _attn_sd(C):
    sd = {"a.norm.weight": 1 + 0.1 * rnd(C, seed=1), "a.norm.bias": 0.1 * rnd(C, seed=2)}
    for i, n in enumerate(("q", "k", "v", "proj_out")):
        sd[f"a.{n}.weight"] = rnd(C, C, 1, 1, scale=C ** -0.5, seed=10 + i)
        sd[f"a.{n}.bias"] = 0.1 * rnd(C, seed=20 + i)
    return {k: v.cpu() for k, v in sd.items()}


def _block_ref(sd, x, chunk=2048):
    """fp32 composition of the AttnBlock on the device (x [N, C, H, W] fp32 of fp16-rounded values, fp16-rounded weights), the
    softmax over query chunks so that no more than chunk x h*w scores exist at a time."""
    N, C, H, W = x.shape
    HW = H * W
    n = F.group_norm(x, 32, sd["a.norm.weight"].to(dev()), sd["a.norm.bias"].to(dev()), 1e-6)
    lin = lambda t, k: F.conv2d(t, sd[f"a.{k}.weight"].to(dev()).half().float(), sd[f"a.{k}.bias"].to(dev()))
    q, k, v = (lin(n, s).reshape(N, C, HW) for s in "qkv")
    o = torch.empty((N, C, HW), device=dev(), dtype=torch.float32)
    for i in range(0, HW, chunk):
        p = torch.softmax(torch.bmm(q[:, :, i:i + chunk].permute(0, 2, 1), k) * C ** -0.5, dim=2)
        o[:, :, i:i + chunk] = torch.bmm(v, p.permute(0, 2, 1))
    return x + lin(o.reshape(N, C, H, W), "proj_out")


class _Counter:
    def __init__(self, monkeypatch):
        from insv2v import ops
        self.n = {"attention": 0, "softmax_rows": 0}
        for name in self.n:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def f(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return f

    def take(self):
        got, self.n = (self.n["attention"], self.n["softmax_rows"]), {"attention": 0, "softmax_rows": 0}
        return got


def _from_cl(t, N, H, W, C):
    return t.float().reshape(N, H, W, C).permute(0, 3, 1, 2)


@pytest.mark.parametrize("N,H,W,C", [(3, 5, 7, 512), (2, 45, 45, 128), (1, 9, 29, 512)])
def test_vattn_three_paths(N, H, W, C, monkeypatch):
    """flash=True against the fp32 composition and against flash=False; flash=None takes the score path below the threshold."""
    from insv2v.vae import VAttn
    sd = _attn_sd(C)
    x = (rnd(N, C, H, W, seed=3) * 1.5).half()
    xcl = to_cl(x.float())
    cnt = _Counter(monkeypatch)
    fl = VAttn(sd, "a", C, dev(), flash=True)(xcl, (N, H, W))
    assert cnt.take() == (1, 0), "flash=True must launch insv2v_attention and no softmax over scores"
    sc = VAttn(sd, "a", C, dev(), flash=False)(xcl, (N, H, W))
    assert cnt.take() == (0, 1)
    df = VAttn(sd, "a", C, dev())(xcl, (N, H, W))
    assert cnt.take() == (0, 1), "h*w <= 4096: the default is the score path"
    assert torch.equal(df, sc)
    ref = _block_ref(sd, x.float())
    report(_from_cl(fl, N, H, W, C), ref, f"VAttn flash C = {C} h*w = {H * W} vs fp32")
    report(_from_cl(sc, N, H, W, C), ref, f"VAttn scores C = {C} h*w = {H * W} vs fp32")
    report(fl, sc, f"VAttn flash vs scores C = {C} h*w = {H * W}")


def test_vattn_first_default_flash_size(monkeypatch):
    """(1, 64, 66, 512), h*w = 4224: the first multiple-of-8 frame side past the threshold; the default is the flash path."""
    from insv2v.vae import VAttn
    N, H, W, C = 1, 64, 66, 512
    sd = _attn_sd(C)
    x = (rnd(N, C, H, W, seed=3) * 1.5).half()
    cnt = _Counter(monkeypatch)
    out = VAttn(sd, "a", C, dev())(to_cl(x.float()), (N, H, W))
    assert cnt.take() == (1, 0)
    report(_from_cl(out, N, H, W, C), _block_ref(sd, x.float()), "VAttn default at h*w = 4224 vs fp32")


def test_vattn_beyond_the_window():
    """(1, 128, 264, 512), h*w = 33 792: one frame's scores (2.28 GB) no longer fit the window of the batched score GEMM.  All rows against
    the chunked fp32 reference; peak memory above the pre-call baseline <= 8 x N h*w C 2 bytes (the path holds the normalised input,
    q | k | v = 3, the attention output and the result = 6 of that size, 4 at a time; 8 leaves room for allocator rounding; the score
    path would need 66 x)."""
    from insv2v.vae import VAttn, attn_plan
    N, H, W, C = 1, 128, 264, 512
    HW = H * W
    with pytest.raises(ValueError):
        attn_plan(C, HW, flash=False)
    sd = _attn_sd(C)
    att = VAttn(sd, "a", C, dev())
    warm = (rnd(1, C, 5, 7, seed=5)).half()
    VAttn(sd, "a", C, dev(), flash=True)(to_cl(warm.float()), (1, 5, 7))    # the library's one-time workspace is not this call's memory
    x = (rnd(N, C, H, W, seed=3) * 1.5).half()
    xcl = to_cl(x.float())
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = att(xcl, (N, H, W))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    unit = N * HW * C * 2
    print(f"[memory] VAttn flash h*w = {HW}: peak {peak} bytes above the baseline = {peak / unit:.2f} x N h*w C 2")
    assert peak <= 8 * unit, f"peak {peak} bytes = {peak / unit:.2f} x {unit}"
    report(_from_cl(out, N, H, W, C), _block_ref(sd, x.float()), "VAttn flash at h*w = 33792 vs fp32 (all rows)")


# ------------------------------------------------------------------------------------------- VAE level
@pytest.fixture(scope="module")
def vaes():
    from insv2v import synth, shapes
    from insv2v.vae import AutoencoderKL
    sd = synth.synth_state_dict(shapes.vae_shapes(**synth.VAE_FULL))
    made = {}

    def get(flash):
        if flash not in made:
            made[flash] = AutoencoderKL(**synth.VAE_FULL, device=DEV, attn_flash=flash).load_state_dict(sd)
        return made[flash]
    return get


def test_vae_flash_vs_golden(vaes, golden, monkeypatch):
    from insv2v import synth
    vae = vaes(True)
    cnt = _Counter(monkeypatch)
    g = golden("vae_full")
    x = synth.synth_input("vae.x", (2, 3, 64, 96), kind="uniform")
    noise = synth.synth_input("vae.noise", (2, 4, 8, 12))
    report(vae.encode(x, noise), g["enc_sample"], "VAE encode, flash mid block (sampled, injected noise)")
    z = synth.synth_input("vae.z", (1, 4, 8, 12))
    report(vae.decode(z), g["dec"], "VAE decode, flash mid block")
    assert cnt.take() == (2, 0)


def test_vae_flash_on_by_default(vaes, monkeypatch):
    """One frame of 512 x 528 (latent 64 x 66 = 4224 tokens): the default setting takes the flash kernel and agrees with attn_flash=False
    within the bound test_vae_full_size_frame_batching_invariance uses between two launch forms."""
    from insv2v import synth
    cnt = _Counter(monkeypatch)
    x = synth.synth_input("vae.flash.x", (1, 3, 512, 528), kind="uniform")
    noise = synth.synth_input("vae.flash.noise", (1, 4, 64, 66))
    z = vaes(None).encode(x, noise)
    img = vaes(None).decode(z)
    assert cnt.take() == (2, 0), "the default path at h*w = 4224 is the flash kernel"
    z0 = vaes(False).encode(x, noise)
    img0 = vaes(False).decode(z)
    assert cnt.take() == (0, 2)
    assert z.shape == (1, 4, 64, 66) and img.shape == (1, 3, 512, 528)
    dz, di = ((z - z0).abs().max() / z0.abs().max()).item(), ((img - img0).abs().max() / img0.abs().max()).item()
    print(f"[parity] flash vs scores at 512 x 528: encode {dz:.3e}, decode {di:.3e} of the maximum")
    assert dz <= 5e-3 and di <= 5e-3


def test_vae_large_frame_decodes(vaes):
    """One latent of 128 x 264 (a 1024 x 2112 frame, 33 792 mid-block tokens), run once: right shape, all finite."""
    from insv2v import synth
    z = synth.synth_input("vae.large.z", (1, 4, 128, 264))
    img = vaes(None).decode(z)
    assert img.shape == (1, 3, 1024, 2112)
    assert torch.isfinite(img).all()
