"""KL-VAE encode/decode on the HIP kernels (drop-in for modules/kl_autoencoder/autoencoder.py:89-100
over modules/vqvae/model.py Encoder/Decoder).  Same ``ddconfig``/``embed_dim`` kwargs and state-dict
keys (encoder.*, decoder.*, quant_conv.*, post_quant_conv.*).

Channels-last fp16 throughout; frames are batched (the reference decodes one frame at a time,
instruct_p2p_video.py:73-76 -- same values, fewer launches).  The mid AttnBlock (model.py:145-197,
single head, C=512) has two forms, chosen by ``attn_plan``:
  "scores"  three batched GEMMs + a row softmax: S = q k^T / sqrt(C), P = softmax(S), O = P v, with v^T
            produced directly by a GEMM so no transpose kernel is needed.  The [N, h*w, h*w] scores live in
            memory: every geometry up to h*w = 4096 (all that is benched or pinned by a golden) runs this form;
  "flash"   q | k | v row GEMMs into one [N*h*w, 3C] matrix + insv2v_attention (one head of C channels, online
            softmax): nothing of size (h*w)^2 exists, so a frame of any size runs.  C = 128 and 512 only.
"""
import torch

from . import ops
from .fused import OPERAND_WINDOW
from .rng import stream_id, ENC
from .unet import prep_conv3x3, prep_linear, prep_norm, _dev

EPS = 1e-6
GROUPS = 32
# The score tensor of one chunk of frames passes half a GB from here on (15 frames x 4096^2 x 2 B at 512 x 512): a memory rule, not a
# measured crossover.  Every geometry with a golden or a bench number lies below it and launches what it always launched.
FLASH_MIN_HW = 4096
FLASH_WIDTHS = (128, 512)   # head dims insv2v_attention dispatches that a VAE mid block can have (VAE_TINY, full width)
# insv2v_gemm refuses a BATCHED problem with an operand beyond one window (gemm.hip beyond_window(); its default window keeps 1 MiB
# of headroom below 2 GiB): the score matrix of ONE frame, HW x HWp fp16, has to stay below this
SCORE_WINDOW = OPERAND_WINDOW - 2 ** 20


def attn_plan(C, HW, flash=None):
    """Which form the mid AttnBlock of C channels takes at h*w = HW tokens: "scores" or "flash".  flash=None: the memory rule above;
    True / False force a form.  Raises ValueError, before anything is launched, for a form that cannot run.  Pure arithmetic."""
    C, HW = int(C), int(HW)
    if flash is None:
        flash = C in FLASH_WIDTHS and HW > FLASH_MIN_HW
    if flash:
        if C not in FLASH_WIDTHS:
            raise ValueError(f"VAE attention of C = {C} channels at h*w = {HW}: the flash form takes C in {FLASH_WIDTHS} only "
                             f"(the score form would hold {HW * ((HW + 7) // 8 * 8) * 2} bytes of scores per frame)")
        return "flash"
    HWp = (HW + 7) // 8 * 8
    if HW * HWp * 2 >= SCORE_WINDOW:
        raise ValueError(f"VAE attention of C = {C} channels at h*w = {HW}: one frame's score matrix is {HW * HWp * 2} bytes, and the batched "
                         f"score GEMM addresses it through one window of {SCORE_WINDOW} bytes"
                         + ("" if C in FLASH_WIDTHS else f"; the flash form takes C in {FLASH_WIDTHS} only"))
    return "scores"


class VResBlock:
    def __init__(self, sd, key, cin, cout, dev):
        self.n1, self.n2 = prep_norm(sd, key + ".norm1", dev), prep_norm(sd, key + ".norm2", dev)
        self.c1, self.c2 = prep_conv3x3(sd, key + ".conv1", dev), prep_conv3x3(sd, key + ".conv2", dev)
        self.sc = prep_linear(sd, key + ".nin_shortcut", dev) if cin != cout else None

    def __call__(self, x, geom):
        N, H, W = geom
        n = ops.groupnorm(x, N, H * W, *self.n1, GROUPS, EPS, silu=True)
        h, _ = ops.conv3x3(n, geom, *self.c1)
        n = ops.groupnorm(h, N, H * W, *self.n2, GROUPS, EPS, silu=True)
        res = ops.gemm(x, *self.sc) if self.sc is not None else x
        out, _ = ops.conv3x3(n, geom, *self.c2, residual=res)
        return out


class VAttn:
    def __init__(self, sd, key, ch, dev, flash=None):
        self.ch = ch
        self.flash = flash   # None: attn_plan's memory rule; True / False: force the form
        self.norm = prep_norm(sd, key + ".norm", dev)
        self.wqk = _dev(torch.cat([sd[f"{key}.{n}.weight"].reshape(ch, ch).float() for n in "qk"], 0), torch.float16, dev)
        self.bqk = _dev(torch.cat([sd[f"{key}.{n}.bias"].float() for n in "qk"], 0), torch.float32, dev)
        self.wv, self.bv = prep_linear(sd, key + ".v", dev)
        self.proj = prep_linear(sd, key + ".proj_out", dev)

    def __call__(self, x, geom):
        N, H, W = geom
        C, HW = self.ch, H * W
        if attn_plan(C, HW, self.flash) == "flash":
            return self._flash(x, N, HW)
        # The batched GEMMs want 16-byte leading dimensions (ldc = HW of the scores, K = HW of P.v): for an h*w that is not a multiple of 8
        # the score rows and v^T rows are padded to HWp columns.  The softmax writes the pad columns of P as exact zeros and v^T's pad
        # columns are zero, so contracting over HWp adds nothing.  HW % 8 == 0: HWp = HW, the launches of before.
        HWp = (HW + 7) // 8 * 8
        n = ops.groupnorm(x, N, HW, *self.norm, GROUPS, EPS)
        qk = ops.gemm(n, self.wqk, self.bqk)  # [N*HW, 2C]
        s = torch.empty((N, HW, HWp), device=x.device, dtype=torch.float16)
        # S_f = q_f k_f^T * C^-0.5 (alpha applied in the epilogue keeps fp16 in range)
        ops.gemm(qk, qk[:, C:], out=s, alpha=float(C) ** -0.5, batch=N, M=HW, N=HW, K=C, lda=2 * C, ldw=2 * C, ldc=HWp,
                 a_bs=HW * 2 * C, w_bs=HW * 2 * C, c_bs=HW * HWp)
        ops.softmax_rows(s, valid=HW)
        # v^T_f [C, HW] = Wv n_f^T ; the v bias is added after P.v (softmax rows sum to 1)
        vt = (torch.empty if HWp == HW else torch.zeros)((N, C, HWp), device=x.device, dtype=torch.float16)
        ops.gemm(self.wv, n, out=vt, batch=N, M=C, N=HW, K=C, lda=C, ldw=C, ldc=HWp, a_bs=0, w_bs=HW * C, c_bs=C * HWp)
        o = torch.empty((N * HW, C), device=x.device, dtype=torch.float16)
        ops.gemm(s.reshape(N * HW, HWp), vt.reshape(N * C, HWp), self.bv, out=o, batch=N, M=HW, N=C, K=HWp, lda=HWp, ldw=HWp,
                 ldc=C, a_bs=HW * HWp, w_bs=C * HWp, c_bs=HW * C)
        return ops.gemm(o, *self.proj, residual=x)

    def _flash(self, x, N, HW):
        """q | k and v (bias in its GEMM) as column ranges of one [N*HW, 3C] matrix, so that one problem stride serves all three operands of
        insv2v_attention; one head of C channels per frame."""
        C = self.ch
        n = ops.groupnorm(x, N, HW, *self.norm, GROUPS, EPS)
        qkv = torch.empty((N * HW, 3 * C), device=x.device, dtype=torch.float16)
        ops.gemm(n, self.wqk, self.bqk, out=qkv[:, :2 * C])
        ops.gemm(n, self.wv, self.bv, out=qkv[:, 2 * C:])
        del n
        o = torch.empty((N * HW, C), device=x.device, dtype=torch.float16)
        p = qkv.data_ptr()
        ops.attention(p, p + 2 * C, p + 4 * C, o, batch=N, heads=1, head_dim=C, seq_q=HW, seq_k=HW, scale=float(C) ** -0.5,
                      q_rs=3 * C, k_rs=3 * C, v_rs=3 * C, o_rs=C, q_addr=(1, HW * 3 * C, 0), kv_addr=(1, HW * 3 * C, 0), o_addr=(1, HW * C, 0))
        del qkv
        return ops.gemm(o, *self.proj, residual=x)


class AutoencoderKL:
    def __init__(self, ddconfig, embed_dim=4, device="cuda", attn_flash=None, **unused):
        self.dd = dict(ddconfig)
        self.attn_flash = attn_flash   # the mid AttnBlocks' form: None = attn_plan's rule, True / False force it
        self.embed_dim = embed_dim
        self.device = torch.device(device)
        if len(self.dd.get("attn_resolutions", [])):
            raise NotImplementedError("attn_resolutions is empty in the InsV2V config")
        self.loaded = False

    def load_state_dict(self, sd, strict=True):
        dd, dev = self.dd, self.device
        ch, mult, nres = dd["ch"], list(dd["ch_mult"]), dd["num_res_blocks"]
        # encoder
        e = "encoder"
        self.e_in = prep_conv3x3(sd, e + ".conv_in", dev)
        self.e_in_pad = self.e_in[0].shape[1] // 9
        self.e_down = []
        cur = ch
        in_mult = [1] + mult
        for lvl in range(len(mult)):
            blocks = []
            cur = ch * in_mult[lvl]
            for j in range(nres):
                blocks.append(VResBlock(sd, f"{e}.down.{lvl}.block.{j}", cur, ch * mult[lvl], dev))
                cur = ch * mult[lvl]
            ds = prep_conv3x3(sd, f"{e}.down.{lvl}.downsample.conv", dev) if lvl != len(mult) - 1 else None
            self.e_down.append((blocks, ds))
        self.e_mid = (VResBlock(sd, e + ".mid.block_1", cur, cur, dev), VAttn(sd, e + ".mid.attn_1", cur, dev, self.attn_flash),
                      VResBlock(sd, e + ".mid.block_2", cur, cur, dev))
        self.e_norm = prep_norm(sd, e + ".norm_out", dev)
        self.e_out = prep_conv3x3(sd, e + ".conv_out", dev)
        self.quant = prep_linear(sd, "quant_conv", dev)
        # decoder
        d = "decoder"
        self.post_quant = prep_linear(sd, "post_quant_conv", dev)
        cur = ch * mult[-1]
        self.d_in = prep_conv3x3(sd, d + ".conv_in", dev)
        self.d_in_pad = self.d_in[0].shape[1] // 9
        self.d_mid = (VResBlock(sd, d + ".mid.block_1", cur, cur, dev), VAttn(sd, d + ".mid.attn_1", cur, dev, self.attn_flash),
                      VResBlock(sd, d + ".mid.block_2", cur, cur, dev))
        self.d_up = []
        for lvl in reversed(range(len(mult))):
            blocks = []
            for j in range(nres + 1):
                blocks.append(VResBlock(sd, f"{d}.up.{lvl}.block.{j}", cur, ch * mult[lvl], dev))
                cur = ch * mult[lvl]
            us = prep_conv3x3(sd, f"{d}.up.{lvl}.upsample.conv", dev) if lvl != 0 else None
            self.d_up.append((blocks, us))
        self.d_norm = prep_norm(sd, d + ".norm_out", dev)
        self.d_out = prep_conv3x3(sd, d + ".conv_out", dev)
        self.loaded = True
        return self

    # ---------------------------------------------------------------------------------------------
    def _frames_per_call(self, H, W):
        """Frames whose largest activation ([N*H*W, C] fp16 at image resolution) stays inside the 2 GiB descriptor
        window of the LDS-DMA operand loads (insv2v_gemm rejects larger operands): e.g. 21 frames at 384x512."""
        cmax = self.dd["ch"] * max(self.dd["ch_mult"][:2])  # widest feature map held at full / half resolution
        return max(1, int((2 ** 31 - 2 ** 24) // (H * W * cmax * 2)))

    @torch.no_grad()
    def moments(self, x):
        """x [N,3,H,W] float -> channels-last fp32 moments [N*h*w, 2*embed_dim], (N,h,w)."""
        N, C, H, W = x.shape
        down = 2 ** (len(self.dd["ch_mult"]) - 1)
        if H % down or W % down:   # the (0,1,0,1)-padded stride-2 stages and the decoder's exact x2 (model.py:67-71,46-52) round-trip only these
            raise ValueError(f"AutoencoderKL: image height and width must be multiples of {down}, got {H}x{W}")
        attn_plan(self.dd["ch"] * self.dd["ch_mult"][-1], (H // down) * (W // down), self.attn_flash)   # refuse up front what the mid block cannot run
        step = self._frames_per_call(H, W)
        if N > step:  # frames are independent: chunk so every operand fits the addressing window
            parts = [self.moments(x[i:i + step]) for i in range(0, N, step)]
            return torch.cat([p[0] for p in parts], 0), (N, *parts[0][1][1:])
        t = ops.nchw_to_nhwc_f16(x.to(device=self.device, dtype=torch.float32), self.e_in_pad)
        geom = (N, H, W)
        t, geom = ops.conv3x3(t, geom, *self.e_in)
        for blocks, ds in self.e_down:
            for b in blocks:
                t = b(t, geom)
            if ds is not None:
                t, geom = ops.conv3x3(t, geom, *ds, stride=2, pad=(0, 0))  # F.pad (0,1,0,1) + stride 2 (model.py:67-71)
        r1, at, r2 = self.e_mid
        t = r2(at(r1(t, geom), geom), geom)
        n = ops.groupnorm(t, geom[0], geom[1] * geom[2], *self.e_norm, GROUPS, EPS, silu=True)
        t, _ = ops.conv3x3(n, geom, *self.e_out)
        return ops.gemm(t, *self.quant, out_fp32=True), geom

    @torch.no_grad()
    def encode(self, x, noise=None, scale=1.0, seed=None, unit=0, offset=0):
        """Posterior SAMPLE (autoencoder.py:89-95); ``noise`` [N,4,h,w] defaults to a CPU randn like the
        reference (autoencoder.py:22).  Returns fp32 [N,4,h,w] times ``scale``.
        ``seed`` (without ``noise``, which wins): the noise is generated inside the sampling kernel from the unit's ENC stream
        (insv2v/rng.py), element = ``offset`` + flat index of [N,4,h,w]; a video encoded in several calls passes each call's first
        frame times 4*h*w as ``offset`` and gets the sample of one call."""
        mom, (N, h, w) = self.moments(x)
        if noise is None and seed is not None:
            return ops.posterior_sample(mom, None, N, h, w, scale, seed=seed, stream=stream_id(ENC, unit), offset=offset)
        if noise is None:
            noise = torch.randn((N, self.embed_dim, h, w))
        noise = noise.to(device=self.device, dtype=torch.float32)
        return ops.posterior_sample(mom, noise, N, h, w, scale)

    @torch.no_grad()
    def decode(self, z, scale=1.0):
        """z [N,4,h,w] float -> image [N,3,8h,8w] fp32 (autoencoder.py:97-100); z is multiplied by ``scale`` first."""
        N, C, h, w = z.shape
        attn_plan(self.dd["ch"] * self.dd["ch_mult"][-1], h * w, self.attn_flash)   # refuse up front what the mid block cannot run
        step = self._frames_per_call(8 * h, 8 * w)
        if N > step:
            return torch.cat([self.decode(z[i:i + step], scale) for i in range(0, N, step)], 0)
        t = ops.nchw_to_nhwc_f16(z.to(device=self.device, dtype=torch.float32), 8, scale)  # 4 latent ch + zero pad
        wp, bp = self._post_quant_padded()
        t = ops.gemm(t, wp, bp)  # [N*h*w, d_in_pad]; channels >= z_channels are exactly zero
        geom = (N, h, w)
        t, geom = ops.conv3x3(t, geom, *self.d_in)
        r1, at, r2 = self.d_mid
        t = r2(at(r1(t, geom), geom), geom)
        for blocks, us in self.d_up:
            for b in blocks:
                t = b(t, geom)
            if us is not None:
                t, geom = ops.conv3x3(t, geom, *us, upsample=True)
        n = ops.groupnorm(t, geom[0], geom[1] * geom[2], *self.d_norm, GROUPS, EPS, silu=True)
        t, _ = ops.conv3x3(n, geom, *self.d_out, out_fp32=True)
        return ops.nhwc_to_nchw_f32(t, geom[0], self.dd["out_ch"], geom[1], geom[2])

    def _post_quant_padded(self):
        """post_quant_conv weight [z, embed] zero-padded to K=8 (GEMM K granularity) and to d_in_pad rows,
        so its output is directly the zero-padded channels-last input of decoder.conv_in."""
        if not hasattr(self, "_pq"):
            w, b = self.post_quant
            wp = torch.zeros((self.d_in_pad, 8), device=w.device, dtype=torch.float16)
            wp[:w.shape[0], :w.shape[1]] = w
            bp = torch.zeros((self.d_in_pad,), device=w.device, dtype=torch.float32)
            bp[:b.shape[0]] = b
            self._pq = (wp, bp)
        return self._pq

    def to(self, *a, **k):
        return self

    def eval(self):
        return self
