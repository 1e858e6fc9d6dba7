"""Kernel-level parity of the 4-wave persistent GEMM / implicit-GEMM convolution (csrc/gemm_w4.hip), forced with tile= as the gemm_q8
tests force theirs: 210 = 128x256 tile, 4 waves; 211 = 256x128, 4 waves; 212 = 128x256, 8 waves; 213 = 256x128, 8 waves.

Every case is compared
  * with fp32 torch on the SAME fp16-rounded operands, at the tolerances of tests/test_kernels_gpu.py: 2e-3 * max|ref| + 2e-3 for a GEMM or
    a convolution, 4e-3 * max|ref| + 4e-3 where a LayerNorm is folded in or GEGLU is applied;
  * with the 128x128 tile kernel (tile=5) on the same arguments, element by element: at most one fp16 rounding step, no element outside
    (one_ulp_close, the assertion of test_wide_store_kernels_under_co_residency);
  * with itself: two forced calls are bit-identical.

Conditions on the inputs (need_gap): for every feature a case exercises there is a reference computed WITHOUT it - the row bias of the
neighbouring group, the -mean * col_sum term dropped, gate and value halves swapped, the second K source zeroed, the residual omitted, the
rows of A of the tile the workgroup computed before - and that reference differs from the true one by more than 10 x the tolerance of the
comparison, so a kernel that skips the feature cannot pass.  The conditions involve the references only (they hold on a CPU as well).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TILES = [210, 211, 212, 213]
BM = {210: 128, 211: 256, 212: 128, 213: 256}   # rows / columns of an output tile
BN = {210: 256, 211: 128, 212: 256, 213: 128}


def dev():
    return torch.device(DEV)


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).to(dev())


def tol_of(ref, ln=False):
    r = 4e-3 if ln else 2e-3
    return r * ref.float().abs().max().item() + r


def close(out, ref, ln=False, what=""):
    err, tol = (out.float() - ref.float()).abs().max().item(), tol_of(ref, ln)
    print(f"[gemm_w4] {what}: max err {err:.4g} (tol {tol:.4g})")
    assert math.isfinite(err) and err <= tol, f"{what}: max err {err:.4g} > tol {tol:.4g}"


def one_ulp_close(out, ref, what):
    d = (out.float() - ref.float()).abs()
    tol = ref.float().abs() * 2.0 ** -9 + 2.0 ** -12   # two fp16 ulps of slack for values straddling a binade
    bad = int((d > tol).sum())
    print(f"[gemm_w4] {what}: {bad} elements beyond one fp16 rounding step, worst {d.max().item():.4g}")
    assert bad == 0, f"{what}: {bad} elements beyond one fp16 rounding step, worst {d.max().item():.4g}"


def need_gap(ref, alt, tol, what):
    """A reference computed without the feature under test must be far from the true one (a condition on the INPUTS of the test)."""
    gap = (alt.float() - ref.float()).abs().max().item()
    assert gap > 10 * tol, f"input condition, {what}: that reference differs from the true one by only {gap:.3g} (tolerance {tol:.3g})"


def run_and_check(run, tile, ref, ln, what, blocks=()):
    """run(tile) -> output.  Forced twice (bit-identical), against fp32 as a whole and on each of `blocks` (name, row slice) on its own,
    against the 128x128 tile kernel."""
    out = run(tile)
    assert torch.equal(out, run(tile)), f"{what}: two calls differ"
    assert out.shape == ref.shape
    close(out, ref, ln, what)
    for name, rows in blocks:
        close(out[rows], ref[rows], ln, f"{what}, {name}")
    one_ulp_close(out, run(5), f"{what} vs the 128x128 tile")
    return out


def num_cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count if dev().type == "cuda" else 2


def conv_ref(x_nchw, w, b, stride, upsample):
    if upsample:
        x_nchw = F.interpolate(x_nchw, scale_factor=2.0, mode="nearest")
    return F.conv2d(x_nchw, w, b, stride=stride, padding=1)


def to_cl(x):  # NCHW -> [N*H*W, C] fp16
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).half().contiguous()


# ------------------------------------------------------------------------------------------- 1. linear
def plain_case(M, N, K, res):
    a, w, b = rnd(M, K).half(), rnd(N, K, scale=K ** -0.5).half(), rnd(N)
    r = rnd(M, N, seed=5).half() if res else None
    prod = a.float() @ w.float().t()
    ref = prod + b + (r.float() if res else 0)
    need_gap(ref, prod + (r.float() if res else 0), tol_of(ref), "bias omitted")
    if res:
        need_gap(ref, prod + b, tol_of(ref), "residual omitted")
    return a, w, b, r, ref


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,N,K,res", [(100, 64, 64, False), (1000, 328, 192, True), (258, 640, 64, False)])
def test_w4_plain_and_partial_tiles(tile, M, N, K, res):
    """Less than one tile (grid == 1, two K tiles, N far below the tile's width); a partial last column tile (N % 128 != 0) with a
    residual and a ragged M; 2.5 / 5 column tiles with two rows in the last row tile."""
    from insv2v import ops
    a, w, b, r, ref = plain_case(M, N, K, res)
    run_and_check(lambda t: ops.gemm(a, w, b, residual=r, tile=t), tile, ref, False, f"gemm_w4 tile {tile} {M}x{N}x{K}")


def identity_case():
    M = N = K = 256
    a = torch.eye(M, device=dev()).half()
    w = (torch.arange(N * K, device=dev()).reshape(N, K).float() % 97 / 97).half()
    ref = w.float().t().contiguous()
    need_gap(ref, ref.t(), tol_of(ref), "rows and columns swapped")
    need_gap(ref, ref.reshape(M, N // 16, 2, 8).flip(2).reshape(M, N), tol_of(ref), "the two 8-column halves of a permlane32 pair swapped")
    need_gap(ref, ref.reshape(M // 64, 2, 32, N).flip(1).reshape(M, N), tol_of(ref), "32-row blocks swapped")
    return a, w, ref


@pytest.mark.parametrize("tile", TILES)
def test_w4_transpose_detecting(tile):
    """A = identity, asymmetric W (test_gemm_transpose_detecting): row / column swaps in the MFMA C layout, swapped permlane32 pairs."""
    from insv2v import ops
    a, w, ref = identity_case()
    run_and_check(lambda t: ops.gemm(a, w, tile=t), tile, ref, False, f"gemm_w4 tile {tile} identity")


def xcd_remap(bid, nwg):   # csrc/common.h
    if nwg < 16:
        return bid
    q, r, xcd, idx = nwg // 8, nwg % 8, bid % 8, bid // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def row_tile_of(v, tiles_m, tiles_n):
    """The row tile of the v-th tile of the persistent stream (gemm_w4's tile_origin: XCD remap, then groups of 8 tile rows)."""
    bid = xcd_remap(v, tiles_m * tiles_n)
    per_group = 8 * tiles_n
    gidx = bid // per_group
    first_m = gidx * 8
    gsz, rin = min(8, tiles_m - first_m), bid - gidx * per_group
    return first_m + rin - (rin // gsz) * gsz


def ring_case(tile, K, cus):
    bm, N = BM[tile], BN[tile]
    grid = 2 * cus
    M = bm * grid + bm + 8                       # grid + 2 row tiles of one column tile: two workgroups take a second tile
    a, w, b = rnd(M, K).half(), rnd(N, K, scale=K ** -0.5).half(), rnd(N)
    ref = a.float() @ w.float().t() + b
    tiles_m = (M + bm - 1) // bm
    assert tiles_m == grid + 2 and tiles_m > 2 * cus
    blocks = [("last row tile", slice((tiles_m - 1) * bm, M))]
    for v in (grid, grid + 1):                   # second pass over the grid: the ring slot and the park parity carry over from tile v - grid
        t2, t1 = row_tile_of(v, tiles_m, 1), row_tile_of(v - grid, tiles_m, 1)
        rows2, rows1 = slice(t2 * bm, min(M, (t2 + 1) * bm)), slice(t1 * bm, t1 * bm + min(M, (t2 + 1) * bm) - t2 * bm)
        blocks.append((f"tile {v} of the stream (row tile {t2})", rows2))
        need_gap(ref[rows2], a[rows1].float() @ w.float().t() + b, tol_of(ref[rows2]), f"rows of A of the workgroup's previous tile ({t1} for {t2})")
    return a, w, b, ref, blocks, tiles_m


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("K", [64, 96, 160])
def test_w4_ring_carries_over_tile_boundaries(tile, K):
    """2, 3 and 5 K tiles (the documented minimum, an odd count, counts that are no multiple of the 3 ring slots) with more tiles than
    2 x CUs: the K-tile stream crosses tile boundaries, the ring slot index and the park-buffer parity carry over into a workgroup's second
    tile, stage_park runs for a non-first tile.  Whole output; every row tile against ITS OWN max|ref| (a wrong tile is not averaged
    away); the last (8-row) tile and the two second-pass tiles by name."""
    from insv2v import ops
    a, w, b, ref, blocks, tiles_m = ring_case(tile, K, num_cus())
    what = f"gemm_w4 tile {tile} K={K} {tiles_m} row tiles"
    out = run_and_check(lambda t: ops.gemm(a, w, b, tile=t), tile, ref, False, what, blocks)
    bm, full = BM[tile], tiles_m - 1
    err = (out[:full * bm].float() - ref[:full * bm]).abs().reshape(full, -1).amax(1)
    tol = 2e-3 * ref[:full * bm].abs().reshape(full, -1).amax(1) + 2e-3
    bad = (err > tol).nonzero().flatten().tolist()
    assert not bad, f"{what}: row tiles {bad[:16]} beyond their own tolerance (worst {(err - tol).max().item():.4g} over)"


def layernorm_case(a, N, seed=0):
    """Folded LayerNorm (no affine: col_sum = row sums of w) on rows with non-zero means."""
    M, K = a.shape
    w, b = rnd(N, K, scale=K ** -0.5, seed=seed).half(), rnd(N, seed=seed)
    col = w.float().sum(1).contiguous()
    x = a.float()
    mean, rstd = x.mean(1, keepdim=True), (x.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    ref = F.layer_norm(x, (K,)) @ w.float().t() + b
    need_gap(ref, ref + rstd * mean * col, tol_of(ref, True), "-mean * col_sum dropped")
    need_gap(ref, x @ w.float().t() + b, tol_of(ref, True), "LayerNorm not applied")
    return w, b, col, ref


def producer_operands(M, K):
    return rnd(M, 64, seed=21).half(), rnd(K, 64, scale=64 ** -0.5, seed=22).half(), rnd(K, seed=23) * 0.2 + 0.3


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stats", ["pass", "producer"])
def test_w4_folded_layernorm_ragged_m(tile, stats):
    """Folded LayerNorm with a ragged, even M (the parked (mean, rstd) pairs of the last tile are fetched two rows per lane).  'pass':
    statistics from insv2v_layernorm_stats; 'producer': a RowStats object of partial sums from the GEMM that produced the rows, which the
    library finalises into gemm_w4's parked pairs with an internal launch."""
    from insv2v import ops
    M, N, K = 2 * 4096 + 78, 960, 320
    if stats == "pass":
        a, st = (rnd(M, K) * 1.2 + 0.3).half(), None
    else:
        a, st = ops.gemm(*producer_operands(M, K), emit_stats=True, tile=5)
        assert isinstance(st, ops.RowStats) and st.nparts > 0
    w, b, col, ref = layernorm_case(a, N)
    st = ops.layernorm_stats(a) if st is None else st
    run_and_check(lambda t: ops.gemm(a, w, b, row_stats=st, col_sum=col, tile=t), tile, ref, True, f"gemm_w4 tile {tile} folded LayerNorm, {stats} statistics",
                  [("last row tile", slice(M - M % BM[tile], M))])


def row_bias_case(kind, ln):
    N, K = 320, 64
    if kind == "frame":      # per-frame table, groups wrap: row m takes table[(m // HW) % Fr]
        Fr, rpg = 5, 256
        M, rb_mod, ngroups = 3 * Fr * rpg + 256, Fr, Fr
    else:                    # per-sample table: row m takes table[m // 512]
        rpg, rb_mod, ngroups = 512, 0, 4
        M = 4 * rpg
    a = (rnd(M, K) * 1.2 + 0.3).half()
    table = rnd(ngroups, N, seed=9) * 0.5
    if ln:
        w, b, col, ref = layernorm_case(a, N)
    else:
        w, b, col = rnd(N, K, scale=K ** -0.5).half(), rnd(N), None
        ref = a.float() @ w.float().t() + b
    g = (torch.arange(M, device=dev()) // rpg) % ngroups
    full = ref + table[g]
    need_gap(full, ref + table[(g + 1) % ngroups], tol_of(full, ln), "row bias of the neighbouring group")
    need_gap(full, ref, tol_of(full, ln), "row bias omitted")
    if ln:
        x = a.float()
        need_gap(full, full + (x.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt() * x.mean(1, keepdim=True) * col, tol_of(full, True), "-mean * col_sum dropped")
    return a, w, b, col, table, rpg, rb_mod, full


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kind,ln", [("frame", False), ("frame", True), ("sample", False)])
def test_w4_row_bias(tile, kind, ln):
    """The row-bias vector is parked once per tile from row_group(first row): a per-frame table whose groups wrap (rb_mod = Fr = 5,
    256 rows per group, 16 groups), alone and together with the folded LayerNorm; a per-sample table (rb_mod = 0, 512 rows per group)."""
    from insv2v import ops
    a, w, b, col, table, rpg, rb_mod, ref = row_bias_case(kind, ln)
    kw = dict(row_stats=ops.layernorm_stats(a), col_sum=col) if ln else {}
    run_and_check(lambda t: ops.gemm(a, w, b, row_bias=table, rows_per_group=rpg, rb_mod=rb_mod, tile=t, **kw), tile, ref, ln,
                  f"gemm_w4 tile {tile} {kind} row bias, LayerNorm {ln}")


def two_source_case(split):
    M, N, K = 4096, 320, 960
    a, w, b = rnd(M, K).half(), rnd(N, K, scale=K ** -0.5).half(), rnd(N)
    ref = a.float() @ w.float().t() + b
    need_gap(ref, a[:, :split].float() @ w[:, :split].float().t() + b, tol_of(ref), "second K source zeroed")
    need_gap(ref, a[:, split:].float() @ w[:, split:].float().t() + b, tol_of(ref), "first K source zeroed")
    return a, w, b, ref


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("split", [640, 64])
def test_w4_two_source_k(tile, split):
    """[a | a2] as two operands, split at 640 and at 64 - the smallest split insv2v_gemm accepts (k_split % 64, checked before any kernel
    is chosen: a split at 32 is refused for every tile).  Same K tiles in the same order as the single-source call: bit-identical to it."""
    from insv2v import ops, _lib
    a, w, b, ref = two_source_case(split)
    a1, a2 = a[:, :split].contiguous(), a[:, split:].contiguous()
    out = run_and_check(lambda t: ops.gemm(a1, w, b, a2=a2, tile=t), tile, ref, False, f"gemm_w4 tile {tile} two-source K split at {split}")
    assert torch.equal(out, ops.gemm(a, w, b, tile=tile)), "two-source K differs from the single-source call"
    with pytest.raises(_lib.HipKernelError):
        ops.gemm(a[:, :32].contiguous(), w, b, a2=a[:, 32:].contiguous(), tile=tile)


# ------------------------------------------------------------------------------------------- 2. GEGLU
def geglu_case(M, C, NH):
    from insv2v.unet import fold_layernorm, interleave32
    x = (rnd(M, C) * 1.3 + 0.2).half()
    w1, b1 = rnd(2 * NH, C, scale=C ** -0.5), rnd(2 * NH, seed=1) * 0.3
    gamma, beta = 1 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    wf, col, bf = (t.to(dev()) for t in fold_layernorm(w1.cpu(), gamma.cpu(), beta.cpu(), b1.cpu()))
    xf = x.float()
    mean, rstd = xf.mean(1, keepdim=True), (xf.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    y = F.layer_norm(xf, (C,)) @ wf.float().t() + bf        # == rstd * (x @ wf^T - mean * col) + bf, the operands the kernel gets
    h, g = y.chunk(2, dim=-1)
    ref = h * F.gelu(g)
    need_gap(ref, g * F.gelu(h), tol_of(ref, True), "gate and value halves swapped")
    need_gap(ref, h * F.gelu(h), tol_of(ref, True), "the gate read from the value's accumulator")
    hd, gd = (y + rstd * mean * col).chunk(2, dim=-1)
    need_gap(ref, hd * F.gelu(gd), tol_of(ref, True), "-mean * col_sum dropped")
    args = (x, interleave32(wf).contiguous(), interleave32(bf).contiguous())
    return args, interleave32(col).contiguous(), ref


@pytest.mark.parametrize("tile", [210, 211])
@pytest.mark.parametrize("M,C,NH", [(2 * 4096 + 78, 320, 640), (300, 64, 160), (8192, 320, 1280)])
def test_w4_geglu(tile, M, C, NH):
    """GEGLU on the [32 value | 32 gate] interleaved projection with the folded LayerNorm in front: ragged M; N = 320 (a partial column
    tile, a problem smaller than one tile, two K tiles); the level-0 FF1 shape, which the dispatch (tile=0) runs on the 128x256 tile."""
    from insv2v import ops
    args, col, ref = geglu_case(M, C, NH)
    st = ops.layernorm_stats(args[0])
    out = run_and_check(lambda t: ops.gemm(*args, act=ops.ACT_GEGLU, row_stats=st, col_sum=col, tile=t), tile, ref, True, f"gemm_w4 tile {tile} GEGLU {M}x{2 * NH}x{C}")
    assert out.shape == (M, NH)
    if (M, C, NH) == (8192, 320, 1280) and tile == 210:
        assert torch.equal(ops.gemm(*args, act=ops.ACT_GEGLU, row_stats=st, col_sum=col, tile=0), out), "the dispatched level-0 FF1 is not the 128x256 gemm_w4 tile"


# ------------------------------------------------------------------------------------------- 3. convolution
CONV_GEOMS = [(6, 16, 16, 1, False, False), (6, 8, 16, 1, True, False), (6, 32, 32, 2, False, True), (6, 16, 32, 1, False, True),
              (3, 5, 7, 1, False, False)]   # the last: 35 pixels per image (odd), M = 105 < one tile, a zero-padding border in every row


def conv_case(nb, h, w, stride, ups, cat):
    from insv2v.unet import prep_conv3x3
    c1, c2, cout = 128, 64 if cat else 0, 320
    x1 = rnd(nb, c1, h, w).half().float()
    x2 = rnd(nb, c2, h, w, seed=2).half().float() if cat else None
    xin = torch.cat([x1, x2], 1) if cat else x1
    wt = rnd(cout, c1 + c2, 3, 3, scale=(9 * (c1 + c2)) ** -0.5).half().float()
    b = rnd(cout, seed=4)
    wk, bk = prep_conv3x3({"c.weight": wt.cpu(), "c.bias": b.cpu()}, "c", dev())
    conv = to_cl(conv_ref(xin, wt, b, stride, ups)).float()
    oh, ow = (2 * h, 2 * w) if ups else ((h - 1) // stride + 1, (w - 1) // stride + 1)
    assert conv.shape[0] == nb * oh * ow
    # per-sample row bias.  Every tile must lie inside one bias group: oh * ow is a multiple of 256 in the first four geometries; the
    # 5 x 7 one (35 pixels per image) keeps a row bias as ONE group over all 105 rows
    groups, rpg = (nb, oh * ow) if (oh * ow) % 256 == 0 else (1, nb * oh * ow)
    rb = rnd(groups, cout, seed=6) * 0.5
    res = rnd(nb * oh * ow, cout, seed=7).half()
    g = torch.arange(nb * oh * ow, device=dev()) // rpg
    ref = conv + rb[g] + res.float()
    tol = tol_of(ref)
    need_gap(ref, conv + rb[g], tol, "residual omitted")
    need_gap(ref, conv + res.float(), tol, "row bias omitted")
    if groups > 1:
        need_gap(ref, conv + rb[(g + 1) % groups] + res.float(), tol, "row bias of the neighbouring sample")
    if cat:
        wz = wt.clone()
        wz[:, c1:] = 0
        need_gap(ref, to_cl(conv_ref(xin, wz, b, stride, ups)).float() + rb[g] + res.float(), tol, "second channel source zeroed")
    need_gap(ref, to_cl(conv_ref(xin, wt.flip(3), b, stride, ups)).float() + rb[g] + res.float(), tol, "taps mirrored")
    kw = dict(x2=to_cl(x2) if cat else None, row_bias=rb, rows_per_group=rpg, residual=res, stride=stride, upsample=ups)
    return to_cl(x1), wk, bk, kw, (nb, oh, ow), ref


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("nb,h,w,stride,ups,cat", CONV_GEOMS)
def test_w4_conv3x3(tile, nb, h, w, stride, ups, cat):
    """The gathered 3x3 convolution on gemm_w4 (test_conv3x3_q8's cases): zero padding, stride 2, nearest x2 upsample by index, two-source
    channel concat, per-sample row bias, residual; and 3 images of 5 x 7."""
    from insv2v import ops
    x, wk, bk, kw, geom, ref = conv_case(nb, h, w, stride, ups, cat)

    def run(t):
        out, g = ops.conv3x3(x, (nb, h, w), wk, bk, tile=t, **kw)
        assert g == geom
        return out
    run_and_check(run, tile, ref, False, f"conv3x3 on gemm_w4 tile {tile} {nb}x{h}x{w} stride {stride} upsample {ups} concat {cat}")


# ------------------------------------------------------------------------------------------- 4. dispatch boundaries
# pick_persistent() sends a LINEAR problem without activation, residual or second source to gemm_w4 (128x256 tile) when
# N >= 960 and K <= 640 and M >= 4096 - at K == 640 only from M >= 12288.  One (inside, outside) pair per condition.
@pytest.mark.parametrize("M,N,K,inside", [(4096, 960, 320, True), (4095 + 1 - 8, 960, 320, False), (4096, 952, 320, False),
                                          (4096, 960, 672, False), (12288, 960, 640, True), (12288 - 8, 960, 640, False),
                                          (4096, 1280, 64, True)])
def test_w4_dispatch_boundaries(M, N, K, inside):
    from insv2v import ops
    a, w, b, _, ref = plain_case(M, N, K, False)
    out = ops.gemm(a, w, b)
    close(out, ref, False, f"dispatched gemm {M}x{N}x{K}")
    if inside:
        assert torch.equal(out, ops.gemm(a, w, b, tile=210)), f"{M}x{N}x{K} was not dispatched to the 128x256 gemm_w4 tile"
    one_ulp_close(out, ops.gemm(a, w, b, tile=5), f"dispatched gemm {M}x{N}x{K} vs the 128x128 tile")


# ------------------------------------------------------------------------------------------- 5. the gate
def deinterleaved_geglu(y):   # y: [M, N] of [32 value | 32 gate] column blocks
    M, N = y.shape
    y = y.reshape(M, N // 64, 2, 32)
    return (y[:, :, 0] * F.gelu(y[:, :, 1])).reshape(M, N // 2)


def gate_call(name, tile):
    """One argument set gemm_w4 cannot run.  Returns (output, fp32 reference, LayerNorm / GEGLU tolerance?)."""
    from insv2v import ops, _lib
    M, N, K = 256, 64, 128
    if name == "K=32":
        K = 32
    elif name == "K=80":
        K = 80
    elif name == "N=324":
        N = 324
    elif name in ("geglu+residual", "geglu on 8 waves"):
        N = 128
    elif name == "geglu N=96":
        N = 96
    elif name == "row_stats, odd M":
        M = 255
    elif name == "row bias group":
        M = 320
    elif name == "split_k=2":
        K = 2048
    a, w, b = (rnd(M, K) * 1.2 + 0.3).half(), rnd(N, K, scale=K ** -0.5).half(), rnd(N)
    prod = a.float() @ w.float().t()
    if name in ("K=32", "K=80", "N=324"):
        return ops.gemm(a, w, b, tile=tile), prod + b, False
    if name == "out_fp32":
        out = ops.gemm(a, w, b, out_fp32=True, tile=tile)
        assert out.dtype == torch.float32
        return out, prod + b, False
    if name == "act=SILU":
        return ops.gemm(a, w, b, act=ops.ACT_SILU, tile=tile), F.silu(prod + b), False
    if name == "batch=2":
        a2, w2 = rnd(2, M, K).half(), rnd(2, N, K, scale=K ** -0.5).half()
        out = torch.empty((2, M, N), device=dev(), dtype=torch.float16)
        ops.gemm(a2.reshape(2 * M, K), w2.reshape(2 * N, K), out=out, batch=2, M=M, N=N, K=K, lda=K, ldw=K, ldc=N, a_bs=M * K, w_bs=N * K, c_bs=M * N, tile=tile)
        return out, torch.bmm(a2.float(), w2.float().transpose(1, 2)), False
    if name == "split_k=2":
        return ops.gemm(a, w, b, split_k=2, tile=tile), prod + b, False
    if name == "row_stats, odd M":
        out = ops.gemm(a, w, b, row_stats=ops.layernorm_stats(a), col_sum=w.float().sum(1).contiguous(), tile=tile)
        return out, F.layer_norm(a.float(), (K,)) @ w.float().t() + b, True
    if name == "geglu+residual":
        r = rnd(M, N // 2, seed=5).half()
        return ops.gemm(a, w, b, act=ops.ACT_GEGLU, residual=r, tile=tile), deinterleaved_geglu(prod + b) + r.float(), True
    if name in ("geglu on 8 waves", "geglu N=96"):
        return ops.gemm(a, w, b, act=ops.ACT_GEGLU, tile=tile), deinterleaved_geglu(prod + b) if N % 64 == 0 else None, True
    if name == "row bias group":   # 80 rows per group: a 128- or 256-row tile would span groups
        rb = rnd(4, N, seed=9)
        return ops.gemm(a, w, b, row_bias=rb, rows_per_group=80, tile=tile), prod + b + rb.repeat_interleave(80, 0), False
    if name == "k_split=48":
        return ops.gemm(a[:, :48].contiguous(), w, b, a2=a[:, 48:].contiguous(), tile=tile), prod + b, False
    if name == "conv Cin=48":
        x = rnd(2, 48, 8, 8).half()
        wk = rnd(N, 9 * 48, scale=(9 * 48) ** -0.5).half()
        out, _ = ops.conv3x3(to_cl(x), (2, 8, 8), wk, b, tile=tile)
        return out, None, False
    if name == "emit_stats":
        if tile == 0:
            out, st = ops.gemm(a, w, b, emit_stats=True)
            assert isinstance(st, ops.RowStats)
            s = st.parts.double().sum(0)
            assert (s[:, 0] - out.double().sum(1)).abs().max().item() <= 1e-3 + 1e-5 * out.double().sum(1).abs().max().item()
            return out, prod + b, False
        # the descriptor ops.gemm(emit_stats=True) would build if it did not ask insv2v_gemm_stats_parts first (the wrapper retries without
        # statistics): a forced gemm_w4 call that is to emit statistics is refused by insv2v_gemm itself
        out = torch.empty((M, N), device=dev(), dtype=torch.float16)
        parts = torch.empty(((N + 63) // 64, M, 2), device=dev(), dtype=torch.float32)
        ws = ops._workspace(a.device)
        d = _lib.GemmDesc()
        d.a, d.w, d.c, d.bias = a.data_ptr(), w.data_ptr(), out.data_ptr(), b.data_ptr()
        d.lda, d.ldw, d.ldc = a.stride(0), w.stride(0), out.stride(0)
        d.M, d.N, d.K, d.act, d.c_fp32, d.alpha, d.tile, d.batch = M, N, K, ops.ACT_NONE, 0, 1.0, tile, 1
        d.workspace, d.workspace_bytes, d.split_k = ws.data_ptr(), ws.numel() * 4, 0
        d.stats_out, d.ln_eps = parts.data_ptr(), 1e-5
        _lib.check(_lib.load().insv2v_gemm(ops._byref(d), ops._stream()), "insv2v_gemm")
        return out, prod + b, False
    raise AssertionError(name)


GATE = ["K=32", "K=80", "N=324", "out_fp32", "act=SILU", "batch=2", "split_k=2", "row_stats, odd M", "geglu+residual", "geglu N=96", "geglu on 8 waves",
        "row bias group", "k_split=48", "conv Cin=48", "emit_stats"]
NOT_FOR_INSV2V_GEMM = {"geglu N=96", "k_split=48", "conv Cin=48"}   # refused for every tile: GEGLU needs N % 64, a K split and Cin multiples of 64


# (GEGLU exists on the 4-wave tiles, test_w4_geglu: that refusal is the 8-wave tiles')
@pytest.mark.parametrize("tile,name", [(t, n) for t in TILES for n in GATE if not (n == "geglu on 8 waves" and t in (210, 211))])
def test_w4_gate_refuses(tile, name):
    """What gemm_w4 cannot do it refuses (no launch, no wrong result): every forced call raises."""
    from insv2v import _lib
    with pytest.raises(_lib.HipKernelError):
        gate_call(name, tile)


@pytest.mark.parametrize("name", [n for n in GATE if n not in NOT_FOR_INSV2V_GEMM])
def test_w4_gate_cases_run_by_dispatch(name):
    """... and where the argument set is legal for insv2v_gemm as such, the dispatched call (tile=0) succeeds and is right."""
    out, ref, ln = gate_call(name, 0)
    close(out, ref, ln, f"dispatched gemm, {name}")


# ------------------------------------------------------------------------------------------- 6. the plan names the dispatch
# One problem per kernel family plan_gemm (csrc/gemm_plan.h) can choose: the dispatched call (tile=0) is bit-equal to the call forced to
# the plan's own tile code.  The first eight shapes are the smallest that were named for the rules when the planner was introduced; on
# 256 CUs two of them stay below their rule's threshold (8192 x 640 x 256 and the 2 x 16 x 16 convolution run on the tile kernel), so
# the smallest problems that do reach gemm_r8's linear form and the patch-tiled kernel follow them.  The convolution that reaches
# gemm_r8's channel-block-major form is searched for with the plan itself.
def plan_of_call(run):
    """The plan (for this device) of the first insv2v_gemm descriptor run() issues, and run()'s result."""
    import ctypes
    from insv2v import _lib
    lib, seen = _lib.load(), []
    real = lib.insv2v_gemm

    def spy(ref, stream):
        if not seen:
            seen.append(_lib.GemmPlan())
            assert lib.insv2v_gemm_plan(ref, 0, ctypes.byref(seen[0])) == 0
        return real(ref, stream)
    lib.insv2v_gemm = spy
    try:
        out = run()
    finally:
        lib.insv2v_gemm = real
    return seen[0], out


def smallest_cim_conv():
    """(NB, Cout) of the smallest 16 x 16, 64-channel convolution that plan_gemm sends to gemm_r8's CIM form on this device."""
    import ctypes
    from insv2v import _lib
    lib, best, p = _lib.load(), None, _lib.GemmPlan()
    for cout in (320, 640, 960, 1280, 1920, 2560):
        for nb in range(1, 400):
            d = _lib.GemmDesc()
            d.a = d.w = d.c = 16
            d.M, d.N, d.K, d.mode, d.lda, d.ldw, d.ldc = nb * 256, cout, 576, 1, 64, 576, cout
            d.NB, d.IH, d.IW, d.OH, d.OW, d.Cin, d.stride, d.pad_t, d.pad_l = nb, 16, 16, 16, 16, 64, 1, 1, 1
            assert lib.insv2v_gemm_plan(ctypes.byref(d), 0, ctypes.byref(p)) == 0
            if p.rc == 0 and p.family == 4 and p.cim:
                if best is None or nb * cout < best[0] * best[1]:
                    best = (nb, cout)
                break
    return best


PLAN_CASES = ["lin 8192x640x256", "geglu 8192x5120x640", "lin 4096x1024x640", "geglu 8192x2560x320", "lin 1152x1280x1280", "lin 128x128x4096",
              "conv 2x16x16 64->128", "conv cim", "lin 16384x1280x256", "conv 100x16x16 64->128"]
PLAN_FAMILIES = {}


@pytest.mark.parametrize("case", PLAN_CASES)
def test_dispatch_equals_the_plans_forced_tile(case):
    from insv2v import ops
    from insv2v.unet import prep_conv3x3
    kind, _, shape = case.partition(" ")
    if kind == "conv":
        nb, cout = smallest_cim_conv() if shape == "cim" else (int(shape.split("x")[0]), 128)
        x = rnd(nb, 64, 16, 16).half().float()
        wt, b = rnd(cout, 64, 3, 3, scale=576 ** -0.5).half().float(), rnd(cout, seed=4)
        wk, bk = prep_conv3x3({"c.weight": wt.cpu(), "c.bias": b.cpu()}, "c", dev())
        xcl = to_cl(x)
        run = lambda t: ops.conv3x3(xcl, (nb, 16, 16), wk, bk, tile=t)[0]
        if nb * cout <= 1 << 16:
            close(run(0), to_cl(conv_ref(x, wt, b, 1, False)), False, case)
    else:
        M, N, K = map(int, shape.split("x"))
        a, w = rnd(M, K).half(), rnd(N, K, scale=K ** -0.5).half()
        run = lambda t: ops.gemm(a, w, act=ops.ACT_GEGLU if kind == "geglu" else ops.ACT_NONE, tile=t)
    plan, out = plan_of_call(lambda: run(0))
    print(f"[plan] {case}: family {plan.family} variant {plan.variant} ring {plan.ring} split_k {plan.split_k} cim {plan.cim} forced tile {plan.forced_tile}")
    assert plan.rc == 0 and plan.parts == 1 and plan.forced_tile > 0
    assert torch.equal(out, run(plan.forced_tile)), f"{case}: tile=0 differs from tile={plan.forced_tile}, the plan's own code"
    assert shape != "cim" or (plan.family == 4 and plan.cim == 1)
    PLAN_FAMILIES[case] = plan.family
    if len(PLAN_FAMILIES) == len(PLAN_CASES) and num_cus() == 256:   # every family the planner can choose was reached
        assert set(PLAN_FAMILIES.values()) == {1, 2, 3, 4, 5}, PLAN_FAMILIES
        assert PLAN_FAMILIES["geglu 8192x5120x640"] == 4 and PLAN_FAMILIES["lin 4096x1024x640"] == 3 and PLAN_FAMILIES["geglu 8192x2560x320"] == 5
        assert PLAN_FAMILIES["lin 16384x1280x256"] == 4 and PLAN_FAMILIES["conv 100x16x16 64->128"] == 2
