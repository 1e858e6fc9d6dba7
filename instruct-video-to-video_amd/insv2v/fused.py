"""Host side of the register-resident fused kernels (csrc/rows_ffn.hip, rows_tattn.hip, rows_xattn.hip): weight packing into MFMA-fragment streams.

A *fragment* is the A operand of one ``v_mfma_f32_32x32x16_f16``: 64 lanes x 8 halfs = 1 KiB, lane ``l`` holding
``W[row0 + (l & 31)][k(half = l >> 5, jj = 0..7)]``.  The kernels keep activations in registers as B operands whose k order is
the C layout of the MFMA that produced them, so the k index of slot (half, jj) of k-step ``s`` is

    k(s, half, jj) = 16 s + 4 half + (jj & 3) + 8 (jj >> 2)

(lane half ``half`` of a 32x32 accumulator tile owns rows (r & 3) + 8 (r >> 2) + 4 half, registers r = 8 s' + jj).  Applying that
permutation to the weight columns here is what lets one MFMA's output feed the next without any data movement.  A layer that reads
its input from memory loads 16 bytes per lane instead, i.e. the natural order k(s, half, jj) = 16 s + 8 half + jj (``_kperm_nat``).
Biases ride in an extra k-step against a constant fragment that is 1 in slots 0 and 1 of the lower lane half: slot 0 carries
the fp16 rounding of the bias, slot 1 the fp16 rounding of the remainder (together exact to ~2^-22 relative).
"""
import torch

FRAG = 512  # halfs per fragment


def _kperm(nsteps):
    """[nsteps, 2, 8] -> k index of slot (half, jj) of k-step s."""
    s = torch.arange(nsteps).view(-1, 1, 1)
    half = torch.arange(2).view(1, -1, 1)
    jj = torch.arange(8).view(1, 1, -1)
    return 16 * s + 4 * half + (jj & 3) + 8 * (jj >> 2)


def _kperm_nat(nsteps):
    """[nsteps, 2, 8] -> k index of slot (half, jj) of k-step s for an operand loaded from memory 16 bytes per lane: 16 s + 8 half + jj."""
    s = torch.arange(nsteps).view(-1, 1, 1)
    half = torch.arange(2).view(1, -1, 1)
    jj = torch.arange(8).view(1, 1, -1)
    return 16 * s + 8 * half + jj


def _frags(w_rows, kidx):
    """w_rows [32, K] (one 32-row block), kidx [S, 2, 8] -> fragments [S, 64, 8]: lane = half * 32 + row."""
    g = w_rows[:, kidx]                      # [32, S, 2, 8]
    return g.permute(1, 2, 0, 3).reshape(kidx.shape[0], 64, 8)


def _bias_frag(b_rows):
    """fp32 bias of one 32-row block -> [64, 8] fragment (hi in slot 0, lo in slot 1 of the lower lane half)."""
    f = torch.zeros(64, 8)
    hi = b_rows.half().float()
    f[:32, 0] = hi
    f[:32, 1] = (b_rows - hi).half().float()
    return f


def pack_ffn_stream(w1f, b1f, w2, b2, post=None):
    """Weight stream of insv2v_ffn_fused (C = 320).
    w1f [2*NH, C]: first projection with the LayerNorm gamma folded in, ALREADY rounded to fp16 values (rows 0..NH-1 = h, NH.. = gate,
    the diffusers GEGLU chunk order); b1f [2*NH] fp32 = W1 @ beta + b1; w2 [C, NH]; b2 [C] fp32.
    Layout in fragments (the order the kernel consumes): prologue section [b2: CT][W1(0): 42][pad to 64]; for chunk k = 0..NCH-2 a
    stage [W1(k+1): 42][W2(k): 20][pad 2]; final section [W2(NCH-1): 20][pad to 32].  W1(c) = for k-step s = 0..KS (KS = bias step):
    (h block c, gate block c); W2(c) = for s2 = 0,1: for output tile ct.  post = (Wp [C, C], bp [C]): the transformer module's trailing
    Linear appended for insv2v_ffn_fused(post=1)."""
    w1f, b1f, w2, b2 = w1f.detach().float().cpu(), b1f.detach().float().cpu(), w2.detach().float().cpu(), b2.detach().float().cpu()
    C = w2.shape[0]
    NH = w2.shape[1]
    assert w1f.shape == (2 * NH, C) and C % 32 == 0 and NH % 32 == 0
    KS, CT, NCH = C // 16, C // 32, NH // 32
    k1 = _kperm_nat(KS)   # the first projection reads x from memory; the second (k2 below) consumes the first's MFMA result

    def W1(c):
        h = _frags(w1f[32 * c:32 * c + 32], k1)                         # [KS, 64, 8]
        g = _frags(w1f[NH + 32 * c:NH + 32 * c + 32], k1)
        hb = _bias_frag(b1f[32 * c:32 * c + 32])[None]
        gb = _bias_frag(b1f[NH + 32 * c:NH + 32 * c + 32])[None]
        return torch.stack([torch.cat([h, hb], 0), torch.cat([g, gb], 0)], dim=1).reshape(2 * (KS + 1), 64, 8)

    k2 = _kperm(2)

    def W2(c):
        cols = 32 * c + k2                                                # [2, 2, 8] hidden units of this chunk
        out = []
        for s2 in range(2):
            for ct in range(CT):
                out.append(_frags(w2[32 * ct:32 * ct + 32], cols[s2:s2 + 1])[0])
        return torch.stack(out, 0)                                        # [2*CT, 64, 8]

    def pad(n):
        return torch.zeros(n, 64, 8)

    parts = [torch.stack([_bias_frag(b2[32 * ct:32 * ct + 32]) for ct in range(CT)], 0), W1(0)]
    parts.append(pad(64 - CT - 2 * (KS + 1)))
    for k in range(NCH - 1):
        parts += [W1(k + 1), W2(k), pad(64 - 2 * (KS + 1) - 2 * CT)]
    parts += [W2(NCH - 1), pad(32 - 2 * CT)]
    if post is not None:
        # trailing Linear [C, C] (+ bias) consuming the feed-forward result in registers: C-layout k order; output tiles in pairs
        # interleaved over the k-steps (k-step KS = bias), padded to a whole number of 32-fragment slots
        wp, bp = post[0].detach().float().cpu().reshape(C, C), post[1].detach().float().cpu()
        kc = _kperm(KS)
        n = 0
        for p in range(CT // 2):
            t = [torch.cat([_frags(wp[32 * (2 * p + j):32 * (2 * p + j) + 32], kc), _bias_frag(bp[32 * (2 * p + j):32 * (2 * p + j) + 32])[None]], 0) for j in range(2)]
            parts.append(torch.stack(t, dim=1).reshape(-1, 64, 8))
            n += 2 * (KS + 1)
        parts.append(pad((n + 31) // 32 * 32 - n))
    return torch.cat(parts, 0).reshape(-1).half()


def _frame_frag(table_rows, step=0):
    """Per-frame bias table restricted to one 32-row block, [F <= 32, 32] fp32 -> [64, 8] fragment for one-hot-of-frame k-step ``step``
    (frames 16 step .. 16 step + 15): lane (row i, half), slot jj = table[16 step + 8 half + jj][i] (fp16), zero beyond F."""
    F = table_rows.shape[0]
    f = torch.zeros(2, 32, 8)
    for fr in range(16 * step, min(F, 16 * step + 16)):
        f[(fr >> 3) & 1, :, fr & 7] = table_rows[fr].half().float()
    return f.reshape(64, 8)


def _tattn_frame_slots(table):
    """Frame slots of the fused temporal-attention kernels for a window of table.shape[0] frames: 16 (1 .. 16 frames) or 32 (17 .. 32)."""
    F = table.shape[0]
    assert 1 <= F <= 32, F
    return 16 if F <= 16 else 32


def _tattn_tile(w_rows, table_rows, kn, nb):
    """[KS + nb, 64, 8]: the fragments of one q / k / v channel tile - the weight k-steps, then nb one-hot frame-bias steps."""
    return torch.cat([_frags(w_rows, kn)] + [_frame_frag(table_rows, j)[None] for j in range(nb)], 0)


def pack_linear_stream(w, bias=None, table=None):
    """Weight stream of insv2v_rowlin for a [N, K = 320] Linear.  w: fp16-valued weights (LayerNorm gamma already folded in when the
    op normalises); bias [N] fp32 (plain bias, carried exactly as hi + lo fp16 parts) OR table [F <= 16, N] fp32 (per-frame bias,
    fp16).  Layout: per pair of 32-row output tiles (2p, 2p+1) one section = for k-step s = 0..KS (KS = bias step): (tile 2p, tile 2p+1),
    padded to a whole number of 16-fragment ring slots (K = 320: 42 -> 48 fragments, K = 640: 82 -> 96)."""
    w = w.detach().float().cpu()
    N, K = w.shape
    assert N % 64 == 0 and K % 16 == 0
    KS = K // 16
    kp = _kperm_nat(KS)
    if table is not None:
        table = table.detach().float().cpu()
        assert table.shape[0] <= 16 and table.shape[1] == N
    else:
        bias = torch.zeros(N) if bias is None else bias.detach().float().cpu()
    parts = []
    for p in range(N // 64):
        tiles = []
        for t in range(2):
            rows = slice(64 * p + 32 * t, 64 * p + 32 * t + 32)
            bf = _frame_frag(table[:, rows]) if table is not None else _bias_frag(bias[rows])
            tiles.append(torch.cat([_frags(w[rows], kp), bf[None]], 0))           # [KS + 1, 64, 8]
        parts.append(torch.stack(tiles, dim=1).reshape(2 * (KS + 1), 64, 8))
        parts.append(torch.zeros((2 * (KS + 1) + 15) // 16 * 16 - 2 * (KS + 1), 64, 8))
    return torch.cat(parts, 0).reshape(-1).half()


def pack_tattn_stream(wqkv, table, wo, bo):
    """Weight stream of insv2v_tattn_fused (C = 320, 8 heads x 40, a window of F = 1 .. 32 frames).
    wqkv [3C, C]: fused to_q / to_k / to_v weights with the LayerNorm gamma folded in (fp16-valued); table [F, 3C] fp32: per-frame bias
    (positional-encoding rows pushed through the weights + W beta); wo [C, C], bo [C]: output projection.
    F <= 16: 16 frame slots, NB = 1 frame-bias step per q/k/v tile; 17 <= F <= 32: 32 frame slots, NB = 2; table rows beyond F are zero.
    Layout (fragments; the kernel's ta_op schedule): for head group G = 0, 1 (channel tiles c = 5G .. 5G+4):
    [for tile c: for k-step s = 0..19+NB: (q, k)] [v tiles (5G, 5G+1) interleaved over s] [v tiles (5G+2, 5G+3)] [v tile 5G+4]
    [pad to a multiple of 16: 5 / 6]; then [output tiles in pairs, interleaved over s = 0..20] [pad 14].  s >= 20 are the bias steps
    (frame table for q/k/v, hi + lo bias for the output).  q/k/v read x from memory (natural k order); the output projection consumes the
    attention result in the C-layout order."""
    wqkv, table, wo, bo = wqkv.detach().float().cpu(), table.detach().float().cpu(), wo.detach().float().cpu(), bo.detach().float().cpu()
    C = wo.shape[0]
    assert wqkv.shape == (3 * C, C) and table.shape[1] == 3 * C and C == 320
    nb = _tattn_frame_slots(table) // 16
    KS = C // 16
    kn, kc = _kperm_nat(KS), _kperm(KS)

    def tile(which, c):      # [KS + nb, 64, 8]: the fragments of q (0) / k (1) / v (2) channel tile c
        rows = slice(which * C + 32 * c, which * C + 32 * c + 32)
        return _tattn_tile(wqkv[rows], table[:, rows], kn, nb)

    def inter(a, b):         # interleave two tiles' fragments over the k-steps
        return torch.stack([a, b], dim=1).reshape(-1, 64, 8)

    sec = 15 * (KS + nb)
    parts = []
    for G in range(2):
        for tl in range(5):
            parts.append(inter(tile(0, 5 * G + tl), tile(1, 5 * G + tl)))
        parts.append(inter(tile(2, 5 * G), tile(2, 5 * G + 1)))
        parts.append(inter(tile(2, 5 * G + 2), tile(2, 5 * G + 3)))
        parts.append(tile(2, 5 * G + 4))
        parts.append(torch.zeros((sec + 15) // 16 * 16 - sec, 64, 8))
    for p in range(5):
        t = [torch.cat([_frags(wo[32 * (2 * p + j):32 * (2 * p + j) + 32], kc), _bias_frag(bo[32 * (2 * p + j):32 * (2 * p + j) + 32])[None]], 0) for j in range(2)]
        parts.append(inter(t[0], t[1]))
    parts.append(torch.zeros(14, 64, 8))
    out = torch.cat(parts, 0)
    assert out.shape[0] == (864 if nb == 1 else 896)
    return out.reshape(-1).half()


def pack_tattn_qkv_stream(wqkv, table):
    """Weight stream of insv2v_tattn_attn (C = 640, 8 heads x 80, a window of F = 1 .. 32 frames): wqkv [3C, C] fused to_q / to_k / to_v with
    the LayerNorm gamma folded in (fp16-valued); table [F, 3C] fp32 per-frame bias (F <= 16: NB = 1 frame-bias step per tile, 17 .. 32:
    NB = 2).  Layout (fragments; the kernel's tb_op schedule), for head group G = 0..3 (2 heads = channel tiles c = 5G .. 5G+4):
    [for tile c: for k-step s = 0..39+NB: (q, k)] [v tiles (5G, 5G+1) interleaved over s] [v tiles (5G+2, 5G+3)] [v tile 5G+4]
    [pad 9 / 10]; s >= 40 are the frame-table steps; natural k order (x is read from memory)."""
    wqkv, table = wqkv.detach().float().cpu(), table.detach().float().cpu()
    C = wqkv.shape[1]
    assert wqkv.shape == (3 * C, C) and table.shape[1] == 3 * C and C == 640
    nb = _tattn_frame_slots(table) // 16
    kn = _kperm_nat(C // 16)

    def tile(which, c):      # [40 + nb, 64, 8]
        rows = slice(which * C + 32 * c, which * C + 32 * c + 32)
        return _tattn_tile(wqkv[rows], table[:, rows], kn, nb)

    def inter(a, b):
        return torch.stack([a, b], dim=1).reshape(-1, 64, 8)

    sec = 15 * (C // 16 + nb)
    parts = []
    for G in range(4):
        for tl in range(5):
            parts.append(inter(tile(0, 5 * G + tl), tile(1, 5 * G + tl)))
        parts.append(inter(tile(2, 5 * G), tile(2, 5 * G + 1)))
        parts.append(inter(tile(2, 5 * G + 2), tile(2, 5 * G + 3)))
        parts.append(tile(2, 5 * G + 4))
        parts.append(torch.zeros((sec + 15) // 16 * 16 - sec, 64, 8))
    out = torch.cat(parts, 0)
    assert out.shape[0] == 4 * (624 if nb == 1 else 640)
    return out.reshape(-1).half()


# ------------------------------------------------------------------------------------------------ text cross-attention block
XA_Q_FR, XA_KV_FR, XA_O_FR = 224, 176, 224


def pack_xattn_stream(wq, bq, wo, bo, pre=None):
    """Shared weight stream of insv2v_xattn_fused (C = 320): wq [C, C] to_q with the LayerNorm gamma folded in (fp16-valued), bq [C] = Wq beta,
    wo [C, C] / bo [C] the output projection.  Layout: [q tiles in pairs interleaved over the 21 k-steps (natural k order, k-step 20 = hi + lo
    bias): 210][pad 14][output tiles in pairs (C-layout k order): 210][pad 14].  pre = (Wo1 [C, C], bo1 [C]): the output projection of the
    preceding self-attention in front, same form as the q section (its operand is read from memory: natural k order)."""
    wq, bq, wo, bo = wq.detach().float().cpu(), bq.detach().float().cpu(), wo.detach().float().cpu(), bo.detach().float().cpu()
    C = wo.shape[0]
    assert wq.shape == (C, C) and wo.shape == (C, C) and C == 320
    KS = C // 16
    parts = []
    secs = [(wq, bq, _kperm_nat(KS)), (wo, bo, _kperm(KS))]
    if pre is not None:
        secs.insert(0, (pre[0].detach().float().cpu().reshape(C, C), pre[1].detach().float().cpu(), _kperm_nat(KS)))
    for w, b, kp in secs:
        for p in range(C // 64):
            t = [torch.cat([_frags(w[32 * (2 * p + j):32 * (2 * p + j) + 32], kp), _bias_frag(b[32 * (2 * p + j):32 * (2 * p + j) + 32])[None]], 0) for j in range(2)]
            parts.append(torch.stack(t, dim=1).reshape(-1, 64, 8))
        parts.append(torch.zeros(14, 64, 8))
    out = torch.cat(parts, 0)
    assert out.shape[0] == XA_Q_FR + XA_O_FR + (224 if pre is not None else 0)
    return out.reshape(-1).half()


def _xa_kstep(h, st):
    """Group-local k-step of step st of head h (4 heads x 40 channels = 160 channels = 10 k-steps): two full k-steps + the unpaired octet."""
    lo = 5 * h
    if st < 2:
        return (lo + 1) // 2 + st if lo & 1 else lo // 2 + st
    return (lo if lo & 1 else lo + 4) >> 1


_XA_INDEX = {}


def xattn_kv_index(C, heads, ctx_len, device):
    """Gather index [XA_KV_FR * 512] into one sample's flattened text K/V ([ctx_len, 2C] row-major: K in columns 0..C-1, V in C..2C-1; index
    ctx_len*2C = a zero) giving its fragment stream for insv2v_xattn_fused: for head gh = 0..7 (group G = gh // 4, h = gh % 4):
    [K: step st = 0..2 x key tile kt = 0..2: lane (key row, half), slot jj = K[32 kt + row][160 G + 16 kst(h, st) + 4 half + (jj & 3) + 8 (jj >> 2)]]
    [V: key k-step 0..5 x tile select 0..1: lane (channel row of tile (40 h) // 32 + select, half), slot jj = V[16 kst + 4 half + (jj & 3) + 8 (jj >> 2)][...]],
    every entry outside the head's 40 channels or beyond ctx_len = zero; then 8 zero fragments."""
    key = (C, heads, ctx_len, str(device))
    if key in _XA_INDEX:
        return _XA_INDEX[key]
    assert C == 320 and heads == 8 and 64 < ctx_len <= 96
    zero = ctx_len * 2 * C
    row = torch.arange(32).view(1, 32, 1)
    half = torch.arange(2).view(2, 1, 1)
    jj = torch.arange(8).view(1, 1, 8)
    kin = 4 * half + (jj & 3) + 8 * (jj >> 2)            # [2, 1, 8] position inside a 16-wide k-step
    frs = []
    for gh in range(8):
        G, h = gh // 4, gh % 4
        for st in range(3):
            for kt in range(3):
                cl = 16 * _xa_kstep(h, st) + kin                                    # [2, 1, 8] group-local channel
                keyi = 32 * kt + row                                                # [1, 32, 1]
                ok = (cl >= 40 * h) & (cl < 40 * h + 40) & (keyi < ctx_len)
                frs.append(torch.where(ok, keyi * (2 * C) + 160 * G + cl, zero).reshape(64, 8))
        for kst in range(6):
            for sel in range(2):
                cl = 32 * ((40 * h) // 32 + sel) + row                              # [1, 32, 1]
                keyi = 16 * kst + kin                                               # [2, 1, 8]
                ok = (cl >= 40 * h) & (cl < 40 * h + 40) & (keyi < ctx_len)
                frs.append(torch.where(ok, keyi * (2 * C) + C + 160 * G + cl, zero).reshape(64, 8))
    frs.append(torch.full((8 * 64, 8), zero).reshape(8, 64, 8).reshape(-1, 8))
    idx = torch.cat([f.reshape(-1) for f in frs]).to(torch.int64)
    assert idx.numel() == XA_KV_FR * 512
    _XA_INDEX[key] = idx.to(device)
    return _XA_INDEX[key]


def pack_xattn_kv(kv, samples, ctx_len, C, heads):
    """kv [samples * ctx_len, 2C] fp16 (the fused to_k / to_v projection of the text context) -> [samples, XA_KV_FR * 512] fragment streams.
    One gather on the tensor's device (data movement only; loop-invariant over the sampling loop)."""
    flat = torch.cat([kv.reshape(samples, ctx_len * 2 * C), kv.new_zeros((samples, 1))], dim=1)
    return flat.index_select(1, xattn_kv_index(C, heads, ctx_len, kv.device)).contiguous()


# ------------------------------------------------------------------------------------------------ text cross-attention, C = 640 (no out-proj)
XB_Q_FR, XB_KV_FR = 208, 80


def pack_xattn_q_stream(wq, bq):
    """q weight stream of insv2v_xattn_attn (C = 640): wq [C, C] to_q with the LayerNorm gamma folded in (fp16-valued), bq [C] = Wq beta.
    Per head group G = 0..3 (channel tiles 5G .. 5G+4): [tiles (5G, 5G+1) interleaved over the 41 k-steps][tiles (5G+2, 5G+3)][tile 5G+4][pad 3];
    natural k order, k-step 40 = hi + lo bias."""
    wq, bq = wq.detach().float().cpu(), bq.detach().float().cpu()
    C = wq.shape[0]
    assert wq.shape == (C, C) and C == 640
    kn = _kperm_nat(C // 16)

    def tile(c):
        return torch.cat([_frags(wq[32 * c:32 * c + 32], kn), _bias_frag(bq[32 * c:32 * c + 32])[None]], 0)

    parts = []
    for G in range(4):
        for p in range(2):
            parts.append(torch.stack([tile(5 * G + 2 * p), tile(5 * G + 2 * p + 1)], dim=1).reshape(-1, 64, 8))
        parts += [tile(5 * G + 4), torch.zeros(3, 64, 8)]
    out = torch.cat(parts, 0)
    assert out.shape[0] == 4 * XB_Q_FR
    return out.reshape(-1).half()


def xattn640_kv_index(C, heads, ctx_len, device):
    """Gather index [4 * XB_KV_FR * 512] into one sample's flattened text K/V ([ctx_len, 2C], K | V; index ctx_len*2C = a zero) for
    insv2v_xattn_attn: for head group G = 0..3, head h = 0, 1 (80 channels = k-steps 5h .. 5h+4 of the group):
    [K: step st = 0..4 x key tile kt = 0..2] [V: key k-step 0..5 x tile 2h + (0..2), zero outside the head's channels]; pad to 80 fragments."""
    key = ("640", C, heads, ctx_len, str(device))
    if key in _XA_INDEX:
        return _XA_INDEX[key]
    assert C == 640 and heads == 8 and 64 < ctx_len <= 96
    zero = ctx_len * 2 * C
    row = torch.arange(32).view(1, 32, 1)
    half = torch.arange(2).view(2, 1, 1)
    jj = torch.arange(8).view(1, 1, 8)
    kin = 4 * half + (jj & 3) + 8 * (jj >> 2)
    frs = []
    for G in range(4):
        for h in range(2):
            for st in range(5):
                for kt in range(3):
                    cl = 16 * (5 * h + st) + kin
                    keyi = 32 * kt + row
                    frs.append(torch.where((keyi < ctx_len) & (cl >= 0), keyi * (2 * C) + 160 * G + cl, zero).reshape(64, 8))
            for kst in range(6):
                for sel in range(3):
                    cl = 32 * (2 * h + sel) + row
                    keyi = 16 * kst + kin
                    ok = (cl >= 80 * h) & (cl < 80 * h + 80) & (keyi < ctx_len)
                    frs.append(torch.where(ok, keyi * (2 * C) + C + 160 * G + cl, zero).reshape(64, 8))
        frs.append(torch.full((14 * 64, 8), zero))
    idx = torch.cat([f.reshape(-1) for f in frs]).to(torch.int64)
    assert idx.numel() == 4 * XB_KV_FR * 512
    _XA_INDEX[key] = idx.to(device)
    return _XA_INDEX[key]


def pack_xattn640_kv(kv, samples, ctx_len, C, heads):
    """kv [samples * ctx_len, 2C] fp16 -> [samples, 4 * XB_KV_FR * 512] fragment streams of insv2v_xattn_attn (one gather)."""
    flat = torch.cat([kv.reshape(samples, ctx_len * 2 * C), kv.new_zeros((samples, 1))], dim=1)
    return flat.index_select(1, xattn640_kv_index(C, heads, ctx_len, kv.device)).contiguous()


def row_units(M, seg_rows, unit):
    """The segmented row schedule of the kernels whose work unit must stay inside one segment of the token rows: the text cross-attention
    kernels (segment = a sample's rows_per_sample rows, unit = a 128-row tile: one K / V stream per tile) and the GroupNorm fold of
    insv2v_rowlin (segment = the gn_rows rows of one (sample, frame) group, unit = a wave's 32 rows: one (scale, shift) table per wave).
    Every segment gets ceil(seg_rows / unit) units of its own; the overhang of its last unit reads zeros and is never stored.
    -> (units_per_segment, n_units).  With seg_rows % unit == 0 this is the plain tiling: n_units == M // unit."""
    if M <= 0 or seg_rows <= 0 or unit <= 0 or M % seg_rows:
        raise ValueError(f"row_units: {M} rows are not whole segments of {seg_rows}")
    ups = -(-seg_rows // unit)
    return ups, (M // seg_rows) * ups


def unit_rows(q, seg_rows, unit):
    """Unit q of the schedule of row_units -> (segment, first real row, number of real rows)."""
    ups = -(-seg_rows // unit)
    s, u = divmod(q, ups)
    return s, s * seg_rows + u * unit, min(unit, seg_rows - u * unit)


# ---- the operand window of the row kernels ------------------------------------------------------------------------------------------------
# A kernel addresses an operand through a buffer descriptor of 2 GiB.  insv2v_rowlin bases its descriptors per row tile; the launchers of
# the fused kernels run a problem whose operands reach beyond one window as ranges of whole units, one launch each (csrc/rows_common.h
# launch_unit_ranges): 128-row tiles for the feed-forward, samples for the temporal and text attention.  So an operand may be of any
# size, and what has to fit one window is ONE unit.  The arithmetic below is the launchers', restated so that a forward that cannot run
# is refused before its first launch.
OPERAND_WINDOW = 2 ** 31
XATTN_KV_BYTES = {320: 176 * 1024, 640: 4 * 80 * 1024}   # one sample's K / V fragment stream (XA_KV_FR, 4 XB_KV_FR fragments of 1 KiB)


def row_kernel_extents(samples, frames, HW, C, ctx_len=77):
    """[(entry point, what has to fit one window, bytes)] of the row kernels that serve a transformer level of C channels with
    `samples` x `frames` x `HW` token rows: widths 320 and 640 have fused kernels, the others none (their GEMMs run oversize problems as
    ranges, insv2v_attention rebases its descriptors)."""
    if C not in (320, 640):
        return []
    sample = f"one sample of {frames} frames x {HW} pixels x {C} channels"
    out = [("insv2v_rowlin", f"a 256-row tile of the fused q/k/v rows ({3 * C} channels)", 256 * 3 * C * 2)]
    if C == 320:
        out.append(("insv2v_ffn_fused", "a 128-row tile", 128 * C * 2))
    if 1 <= frames <= 32:
        out.append(("insv2v_tattn_fused" if C == 320 else "insv2v_tattn_attn", sample, frames * HW * C * 2))
    if 64 < ctx_len <= 96:
        xa = "insv2v_xattn_fused" if C == 320 else "insv2v_xattn_attn"
        out.append((xa, sample, frames * HW * C * 2))
        out.append((xa, f"the K / V streams of {samples} samples", samples * XATTN_KV_BYTES[C]))
    return out


def check_operand_windows(samples, frames, h, w, channels=(320, 640, 1280, 1280), ctx_len=77):
    """Raise ValueError, naming the first operand that does not fit one 2 GiB window, if a UNet forward of `samples` samples x `frames`
    frames of h x w latents cannot run on the row kernels; return None otherwise.  `channels`: the UNet's block_out_channels (level l works
    on ceil(h / 2^l) x ceil(w / 2^l) pixels).  Pure arithmetic: nothing is loaded or launched."""
    samples, frames, h, w = int(samples), int(frames), int(h), int(w)
    if samples < 1 or frames < 1 or h < 1 or w < 1:
        raise ValueError(f"check_operand_windows: {samples} samples x {frames} frames of {h} x {w} latents is not a geometry")
    for level, C in enumerate(channels):
        for entry, what, nbytes in row_kernel_extents(samples, frames, h * w, C, ctx_len):
            if nbytes >= OPERAND_WINDOW:
                raise ValueError(f"{samples} samples x {frames} frames of {h} x {w} latents (level {level}, {C} channels) cannot run: {entry} "
                                 f"addresses {what} = {nbytes} bytes through one buffer descriptor, and that has to stay below "
                                 f"{OPERAND_WINDOW} (2 GiB); use fewer frames per window or a smaller frame")
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
