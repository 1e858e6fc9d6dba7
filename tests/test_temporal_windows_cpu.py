"""CPU tests of the fused temporal-attention streams for windows of 1 .. 32 frames (csrc/rows_tattn.hip insv2v_tattn_fused / insv2v_tattn_attn):
the packers against the library's stream sizes, the 16-frame streams byte-for-byte as before, and a lane-level emulation of the 32-slot
and the masked 16-slot wave schedules over the packed stream against fp32 attention."""
import hashlib
import os
import sys

import pytest
import torch

from conftest import PKG


def _lib():
    from insv2v import _lib as L
    if not os.path.exists(L.LIB_PATH):
        sys.path.insert(0, PKG)
        import build
        build.build(verbose=False)
    return L.load()


def _inputs(C, F):
    g = torch.Generator().manual_seed(1234 + C)
    wqkv = (torch.randn(3 * C, C, generator=g) * C ** -0.5).half().float()
    table = torch.randn(16, 3 * C, generator=g) * 0.3
    wo = (torch.randn(C, C, generator=g) * C ** -0.5).half().float()
    bo = torch.randn(C, generator=g) * 0.1
    if F != 16:
        table = torch.randn(F, 3 * C, generator=torch.Generator().manual_seed(F)) * 0.3
    return wqkv, table, wo, bo


# sha256 of the packed 16-frame streams before windows other than 16 frames existed (the kernels' 16-frame layout is unchanged)
SHA16_320 = "2d5794f642e8a2a836ceb5081eab8c3f26cb53fb6802e415f4e3e2af8425be2b"
SHA16_640 = "14e124aaa3bdaae515463126da1ce2f52a56620a815b691f3ff781f96df96149"


def test_sixteen_frame_streams_are_unchanged():
    from insv2v import fused
    wqkv, table, wo, bo = _inputs(320, 16)
    assert hashlib.sha256(fused.pack_tattn_stream(wqkv, table, wo, bo).numpy().tobytes()).hexdigest() == SHA16_320
    wqkv, table, _, _ = _inputs(640, 16)
    assert hashlib.sha256(fused.pack_tattn_qkv_stream(wqkv, table).numpy().tobytes()).hexdigest() == SHA16_640


@pytest.mark.parametrize("F", [1, 8, 16, 24, 32])
def test_stream_sizes_match_the_library(F):
    from insv2v import fused
    lib = _lib()
    wqkv, table, wo, bo = _inputs(320, F)
    st = fused.pack_tattn_stream(wqkv, table, wo, bo)
    assert st.numel() == int(lib.insv2v_tattn_stream_elems(320, 8, F)) == (864 if F <= 16 else 896) * 512
    wqkv, table, _, _ = _inputs(640, F)
    st = fused.pack_tattn_qkv_stream(wqkv, table)
    assert st.numel() == int(lib.insv2v_tattn_attn_stream_elems(640, 8, F)) == 4 * (624 if F <= 16 else 640) * 512


def test_stream_sizes_reject_other_windows():
    lib = _lib()
    for F in (0, 33, -1):
        assert int(lib.insv2v_tattn_stream_elems(320, 8, F)) == 0
        assert int(lib.insv2v_tattn_attn_stream_elems(640, 8, F)) == 0
    assert int(lib.insv2v_tattn_stream_elems(320, 4, 24)) == 0 and int(lib.insv2v_tattn_stream_elems(640, 8, 24)) == 0
    assert int(lib.insv2v_tattn_attn_stream_elems(640, 16, 24)) == 0 and int(lib.insv2v_tattn_attn_stream_elems(320, 8, 24)) == 0


def test_short_table_pads_with_zero_rows():
    """A table of F < 16 rows packs exactly like the 16-row table whose rows F .. 15 are zero."""
    from insv2v import fused
    wqkv, table, wo, bo = _inputs(320, 16)
    t8 = table[:8]
    pad = torch.cat([t8, torch.zeros(8, table.shape[1])], 0)
    assert torch.equal(fused.pack_tattn_stream(wqkv, t8, wo, bo), fused.pack_tattn_stream(wqkv, pad, wo, bo))


def _emulate_tattn640(FP, F_, seed):
    """fused.pack_tattn_qkv_stream against a lane-level emulation of the schedule insv2v_tattn_attn runs for FP frame slots (tb_op<FP / 16>): a
    wave = 32 / FP pixels x FP slots, slots >= F_ are zero rows (not loaded); q / k tiles with the weights as the A operand and NB = FP / 16
    one-hot frame-bias k-steps; S^T = K . Q^T; softmax in the C layout over the query's pixel, keys >= F_ masked; V with the operands swapped
    so its packed tile is the A operand of O^T = V^T . P^T."""
    from insv2v import fused
    torch.manual_seed(seed)
    C, H, D = 640, 8, 80
    nb, ppw = FP // 16, 32 // FP
    lane = torch.arange(64)
    col, half = lane & 31, lane >> 5

    def mfma(a, b, acc):            # acc [rows of a, rows of b] += A . B^T
        A, B = torch.zeros(32, 16), torch.zeros(32, 16)
        for jj in range(8):
            A[col, 8 * half + jj] = a[:, jj]
            B[col, 8 * half + jj] = b[:, jj]
        return acc + A @ B.T

    def pack_tile(acc):
        out = []
        for u in range(2):
            f = torch.zeros(64, 8)
            for jj in range(8):
                r = 8 * u + jj
                f[:, jj] = acc[(r & 3) + 8 * (r >> 2) + 4 * half, col]
            out.append(f.half().float())
        return out

    x = torch.randn(ppw, F_, C)
    xv = torch.nn.functional.layer_norm(x, (C,)).half().float()
    xn = torch.zeros(ppw, FP, C)
    xn[:, :F_] = xv                                             # wave token = FP * pixel + slot; slots >= F_ read nothing
    xn = xn.reshape(32, C)
    wqkv = (torch.randn(3 * C, C) * C ** -0.5).half().float()
    table = (torch.randn(F_, 3 * C) * 0.3).half().float()
    stream = fused.pack_tattn_qkv_stream(wqkv, table)
    gfr = stream.numel() // (4 * 512)
    assert gfr == (624 if nb == 1 else 640)
    st = stream.float().reshape(4, gfr, 64, 8)
    xf = [torch.stack([xn[col, 16 * s + 8 * half + e] for e in range(8)], 1) for s in range(40)]
    slot, pix = col % FP, col // FP
    fhot = []
    for j in range(nb):
        f = torch.zeros(64, 8)
        for e in range(8):
            f[:, e] = ((2 * j + half == (slot >> 3)) & (e == (slot & 7))).float()
        fhot.append(f)
    tok = torch.arange(32)
    keyok = ((tok[:, None] // FP) == (tok[None, :] // FP)) & ((tok[:, None] % FP) < F_)        # [key, query]
    scale = D ** -0.5
    out = torch.zeros(32, C)
    for G in range(4):
        qs, ks, f = [None] * 10, [None] * 10, 0
        for tl in range(5):
            aq, ak = torch.zeros(32, 32), torch.zeros(32, 32)
            for s in range(40 + nb):
                b = xf[s] if s < 40 else fhot[s - 40]
                aq = mfma(st[G, f], b, aq); ak = mfma(st[G, f + 1], b, ak); f += 2
            qs[2 * tl], qs[2 * tl + 1] = pack_tile(aq)
            ks[2 * tl], ks[2 * tl + 1] = pack_tile(ak)
        PB, invl = [], []
        for h in range(2):
            S = torch.zeros(32, 32)                               # [key token, query token]
            for s5 in range(5):
                S = mfma(ks[5 * h + s5], qs[5 * h + s5], S)
            mx = torch.where(keyok, S, torch.tensor(-1e30)).max(0).values
            e = (torch.exp((S - mx[None, :]) * scale) * keyok).half().float()
            invl.append(1.0 / e.sum(0))
            PB.append(pack_tile(e))                               # B operand: rows = query tokens, k = key tokens in C-layout order
        tiles = []
        for grp in ((0, 1), (2, 3), (4,)):
            accs = [torch.zeros(32, 32) for _ in grp]
            for s in range(40 + nb):
                a = xf[s] if s < 40 else fhot[s - 40]
                for i in range(len(grp)):
                    accs[i] = mfma(a, st[G, f], accs[i]); f += 1  # operands swapped: [token, channel]
            tiles += accs
        assert f == 15 * (40 + nb)
        assert not st[G, f:].any(), "padding fragments"
        for tl, accV in enumerate(tiles):
            v0, v1 = pack_tile(accV)                              # A operand of O^T: rows = channels, k = tokens
            o = torch.zeros(32, 32)
            for qd in range(4):
                h = (32 * tl + 8 * qd) // 80
                O = mfma(v1, PB[h][1], mfma(v0, PB[h][0], torch.zeros(32, 32)))
                rows = [(r & 3) + 8 * (r >> 2) + 4 * hh for hh in range(2) for r in range(4 * qd, 4 * qd + 4)]
                o[rows] = O[rows] * invl[h][None, :]
            out[:, 160 * G + 32 * tl:160 * G + 32 * tl + 32] = o.T
    qkv = (xv @ wqkv.T + table[None]).half().float().reshape(ppw, F_, 3, H, D)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))        # [pixel, head, frame, d]
    ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).permute(0, 2, 1, 3)      # [pixel, frame, head, d]
    got = out.reshape(ppw, FP, C)[:, :F_]
    err = (got - ref.reshape(ppw, F_, C)).abs().max().item()
    assert err < 3e-3 * ref.abs().max().item(), err


@pytest.mark.parametrize("FP,F_", [(32, 24), (32, 20), (16, 8)])
def test_tattn_window_fragment_stream_computes_the_temporal_attention(FP, F_):
    """The 32-slot layout at 24 and 20 frames (one pixel per wave, the whole 32 x 32 score block, two frame-bias k-steps) and the masked
    16-slot layout at 8 frames (two pixels per wave, keys 8 .. 15 of each pixel's block masked)."""
    _emulate_tattn640(FP, F_, seed=F_)
