"""Kernel-level parity of the 8-wave ping-pong GEMM / implicit-GEMM convolution engines, forced with tile=: 230 = gemm_q8 (256 x 256
tile, LDS-DMA requests inside the MFMA segments), 231 = gemm_q8 with the requests in the load segments, 240 = gemm_r8 (256 x 320 tile).
The cases and their fp64 references come from tests/gemm_engine_ref.py, which asserts a need_gap condition per feature (a kernel that
skips the feature cannot pass; tests/test_gemm_engines_cpu.py asserts the same conditions without a GPU).

Every case is compared (run_and_check)
  * with itself: two forced calls are bit-identical;
  * with the fp64 reference on the SAME fp16-rounded operands, as a whole and on every named block against the block's OWN max|ref|:
    2e-3 * max|ref| + 2e-3 for a GEMM or a convolution, 4e-3 for both terms where a LayerNorm is folded in or GEGLU is applied;
  * with the 128x128 tile kernel (tile=5) on the same arguments, element by element: no element beyond |ref| * 2^-9 + 2^-12.
The exact-rounding case has tolerance zero: the output equals the fp32 value rounded to nearest even, bit for bit.

One-line mutations of the kernels that turn these tests red.  Tried on scratch builds of csrc/gemm_q8.hip / gemm_r8.hip (not committed):
  * pack_h2 returning __builtin_amdgcn_cvt_pkrtz(x, y) (round toward zero): test_exact_rounding fails on 230 / 231 / 240 with 35 763 of
    81 920 elements off (32 284 with the residual), every one of them equal to the toward-zero value; every other test stays green;
  * `m < p.M ? ... : OOB_OFFSET` of offc dropped (rows beyond M are stored): test_masked_stores, 83 312 sentinel elements below the
    LINEAR output and 58 560 below the convolution's overwritten;
  * gemm_r8's CIM validity `oh > 0` -> `(oh > 0 || nb > 0)` and `oh + 1 < p.IH` -> `(oh + 1 < p.IH || nb + 1 < p.NB)` (the image edge
    ignored between images - `vh` forced to 7 without reads outside the batch): test_conv_odd_grids 5x9x13 on 240 and
    test_conv_stream_crosses_tile_boundaries fail with max err 2.5 ... 3.1 against a tolerance of 0.02;
  * the factors 8 and 4 of `pc` (gemm_r8) / `pr` (gemm_q8) exchanged: test_layout fails on all three tiles (max err 0.80, tol 0.004),
    test_geglu on 230 / 231 (gemm_r8's GEGLU has its own map);
  * row_group(bm0) -> row_group(0) in stage_park: test_row_bias fails in all nine cases.
Worked out from the code only (their stores or reads would leave the tensors of the test): `okc` forced true in the epilogue's store
(test_masked_stores: columns 328 .. 391 of the sentinel rows), `par` not carried into the next tile (test_stream_crosses_tile_boundaries
at K = 64: the second-pass tiles read the other ring buffer).
"""
import math

import pytest
import torch

import gemm_engine_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TILES = list(R.TILES)
TAG = "[gemm_engines]"


def close(out, ref, ln=False, what=""):
    err, tol = (out.double() - ref).abs().max().item(), R.tol_of(ref, ln)
    print(f"{TAG} {what}: max err {err:.4g} (tol {tol:.4g})")
    assert math.isfinite(err) and err <= tol, f"{what}: max err {err:.4g} > tol {tol:.4g}"


def close_groups(out, ref, dim, size, ln, what):
    """Every group of `size` consecutive rows (dim 0) / columns (dim 1) against ITS OWN max|ref| (only whole groups)."""
    n = ref.shape[dim] // size
    if dim == 0:
        o, r = out[:n * size].double().reshape(n, -1), ref[:n * size].reshape(n, -1)
    else:
        o, r = out[:, :n * size].double().reshape(-1, n, size).transpose(0, 1).reshape(n, -1), ref[:, :n * size].reshape(-1, n, size).transpose(0, 1).reshape(n, -1)
    rel = 4e-3 if ln else 2e-3
    err, tol = (o - r).abs().amax(1), rel * r.abs().amax(1) + rel
    worst = (err - tol).argmax().item()
    print(f"{TAG} {what}: {n} groups, worst group {worst}: max err {err[worst].item():.4g} (tol {tol[worst].item():.4g})")
    bad = (~(err <= tol)).nonzero().flatten().tolist()
    assert not bad, f"{what}: groups {bad[:16]} beyond their own tolerance (worst {(err - tol).max().item():.4g} over)"


def one_ulp_close(out, ref, what):
    d = (out.float() - ref.float()).abs()
    tol = ref.float().abs() * 2.0 ** -9 + 2.0 ** -12   # two fp16 ulps of slack for values straddling a binade
    bad = int((d > tol).sum())
    print(f"{TAG} {what}: {bad} elements beyond one fp16 rounding step, worst {d.max().item():.4g}")
    assert bad == 0, f"{what}: {bad} elements beyond one fp16 rounding step, worst {d.max().item():.4g}"


def run_and_check(run, tile, ref, ln, what, blocks=()):
    """run(tile) -> output.  Forced twice (bit-identical), against fp64 as a whole and on each of `blocks` (name, index) on its own,
    against the 128x128 tile kernel."""
    out = run(tile)
    assert torch.equal(out, run(tile)), f"{what}: two calls differ"
    assert out.shape == ref.shape
    close(out, ref, ln, what)
    for name, idx in blocks:
        close(out[idx], ref[idx], ln, f"{what}, {name}")
    one_ulp_close(out, run(5), f"{what} vs the 128x128 tile")
    return out


def num_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


# ------------------------------------------------------------------------------------------- 1. plain and partial tiles
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,N,K,res", R.PLAIN_SHAPES)
def test_plain_and_partial_tiles(M, N, K, res, tile):
    """Less than one tile with one K tile; two rows in the last row tile and 8 live columns in gemm_r8's last column tile, with a
    residual; 2.5 column tiles of gemm_q8 / 2 of gemm_r8 with an even K-tile count."""
    from insv2v import ops
    a, w, b, r, ref, blocks = R.plain_case(M, N, K, res, DEV)
    run_and_check(lambda t: ops.gemm(a, w, b, residual=r, tile=t), tile, ref, False, f"tile {tile} {M}x{N}x{K}", blocks)


# ------------------------------------------------------------------------------------------- 2. layout
@pytest.mark.parametrize("tile", TILES)
def test_layout(tile):
    """A = identity, asymmetric W: the W source-row maps (pr of gemm_q8, pc of gemm_r8), the MFMA C layout, wm / wn of the waves."""
    from insv2v import ops
    a, w, ref = R.layout_case(DEV)
    out = run_and_check(lambda t: ops.gemm(a, w, tile=t), tile, ref, False, f"tile {tile} identity")
    close_groups(out, ref, 1, 8, False, f"tile {tile} identity, 8-column groups")
    close_groups(out, ref, 0, 16, False, f"tile {tile} identity, 16-row blocks")


# ------------------------------------------------------------------------------------------- 3. exact rounding
@pytest.mark.parametrize("tile", [5, 210, 211, 230, 231, 240])
@pytest.mark.parametrize("res", [False, True])
def test_exact_rounding(res, tile):
    """One non-zero product per accumulator and exact fp32 sums with bits below the fp16 ulp: the stored fp16 value must equal the fp32
    value rounded to nearest even (v_cvt_pk_f16_f32; v_cvt_pkrtz rounds toward zero and differs on more than a third of the elements)."""
    from insv2v import ops
    a, w, b, r, ref32, share, ties = R.exact_case(res, DEV)
    out = ops.gemm(a, w, b, residual=r, tile=tile)
    want = ref32.half()
    bad = out != want
    nbad, toward_zero = int(bad.sum()), int((out == R.round_toward_zero_f16(ref32))[bad].sum())
    print(f"{TAG} exact rounding, tile {tile}, residual {res}: {nbad} of {want.numel()} elements differ from nearest-even ({toward_zero} of them equal toward-zero; "
          f"the inputs tell the two apart on {share:.3f} of the elements, {ties} ties tell nearest-even from half-away)")
    assert nbad == 0, f"tile {tile}: {nbad} elements are not the fp32 value rounded to nearest even ({toward_zero} of them are it rounded toward zero)"
    assert torch.equal(out, ops.gemm(a, w, b, residual=r, tile=tile))


# ------------------------------------------------------------------------------------------- 4. masked stores
SENTINEL = -77.0


def sentinel_intact(big, M, N, what):
    s = torch.full((), SENTINEL, dtype=torch.float16, device=big.device).view(torch.int16)
    below, right = int((big[M:].view(torch.int16) != s).sum()), int((big[:M, N:].view(torch.int16) != s).sum())
    print(f"{TAG} {what}: {below} elements written below row {M}, {right} right of column {N}")
    assert below == 0 and right == 0, f"{what}: {below} elements below the output and {right} right of it were overwritten"


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kind", ["linear", "conv"])
def test_masked_stores(kind, tile):
    """The output is the view big[:M, :N] of a sentinel-filled [M + 256, N + 64] tensor (ldc = N + 64), the residual a strided view too:
    rows beyond M (which read a copy of the last row / zero fill) and columns beyond N (zero-filled bias) leave the memory behind the
    output alone."""
    from insv2v import ops
    if kind == "linear":
        M, N, K, _ = R.MASKED_LINEAR_SHAPE
        a, w, b, r, ref, blocks = R.plain_case(*R.MASKED_LINEAR_SHAPE, DEV)
    else:
        x, wk, bk, kw, geom, ref, blocks = R.conv_case(5, 9, 13, 1, False, 64, DEV)
        M, N, r = ref.shape[0], ref.shape[1], kw["residual"]
    rbig = torch.zeros((M, N + 64), dtype=torch.float16, device=DEV)
    rbig[:, :N] = r
    rbig[:, N:] = 1000.0            # a residual read beyond column N would show
    bigs = {}

    def run(t):
        big = bigs[t] = torch.full((M + 256, N + 64), SENTINEL, dtype=torch.float16, device=DEV)
        if kind == "linear":
            out = ops.gemm(a, w, b, residual=rbig[:, :N], out=big[:M, :N], tile=t)
        else:
            out, g = ops.conv3x3(x, (5, 9, 13), wk, bk, tile=t, out=big[:M, :N], **dict(kw, residual=rbig[:, :N]))
            assert g == geom
        assert out.data_ptr() == big.data_ptr() and out.stride(0) == N + 64
        return out
    what = f"tile {tile} masked stores, {kind}"
    run_and_check(run, tile, ref, False, what, blocks)
    sentinel_intact(bigs[tile], M, N, what)


# ------------------------------------------------------------------------------------------- 5. the stream crosses tile boundaries
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("K", [64, 192, 320])
def test_stream_crosses_tile_boundaries(K, tile):
    """1, 3 and 5 K tiles with three tiles more than CUs: the K-tile stream crosses tile boundaries, the ring parity `par` and the park
    buffer carry over into a workgroup's second tile.  Whole output; every row tile against ITS OWN max|ref|; the last (8-row) tile and
    the second-pass tiles by name."""
    from insv2v import ops
    a, w, b, ref, blocks, tiles_m = R.stream_case(tile, K, num_cus(), DEV)
    what = f"tile {tile} K={K} {tiles_m} row tiles"
    out = run_and_check(lambda t: ops.gemm(a, w, b, tile=t), tile, ref, False, what, blocks)
    close_groups(out, ref, 0, R.BM, False, f"{what}, every full row tile")


# ------------------------------------------------------------------------------------------- 6. folded LayerNorm, row bias, two-source K
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("stats", ["pass", "producer"])
def test_folded_layernorm_ragged_m(stats, tile):
    """Folded LayerNorm with a ragged, even M = 590.  'pass': statistics from insv2v_layernorm_stats; 'producer': a RowStats object of
    partial sums from the GEMM that produced the rows, finalised into the engines' parked (mean, rstd) pairs by an internal launch."""
    from insv2v import ops
    M, N, K = R.LN_SHAPE
    if stats == "pass":
        a, st = R.layernorm_rows(M, K, DEV), None
    else:
        a, st = ops.gemm(*R.producer_operands(M, K, DEV), emit_stats=True, tile=5)
        assert isinstance(st, ops.RowStats) and st.nparts > 0
    w, b, col, ref = R.layernorm_case(a, N)
    st = ops.layernorm_stats(a) if st is None else st
    run_and_check(lambda t: ops.gemm(a, w, b, row_stats=st, col_sum=col, tile=t), tile, ref, True, f"tile {tile} folded LayerNorm, {stats} statistics",
                  [("last row tile", slice(M - M % R.BM, M))])


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kind,ln", [("frame", False), ("frame", True), ("sample", False)])
def test_row_bias(kind, ln, tile):
    """The row-bias vector is parked once per tile from row_group(first row): a per-frame table whose groups wrap (rb_mod = 5, 256 rows
    per group, 16 groups), alone and together with the folded LayerNorm; a per-sample table (rb_mod = 0, 512 rows per group)."""
    from insv2v import ops
    a, w, b, col, table, rpg, rb_mod, ref, blocks = R.row_bias_case(kind, ln, DEV)
    kw = dict(row_stats=ops.layernorm_stats(a), col_sum=col) if ln else {}
    run_and_check(lambda t: ops.gemm(a, w, b, row_bias=table, rows_per_group=rpg, rb_mod=rb_mod, tile=t, **kw), tile, ref, ln,
                  f"tile {tile} {kind} row bias, LayerNorm {ln}", blocks)


@pytest.mark.parametrize("tile", TILES)
def test_row_bias_group_inside_a_tile_is_refused(tile):
    """117 rows per group and M = 585: a 256-row tile would span two groups (row_bias_fits_tiles) - the forced engines refuse, the
    dispatched call (tile=0) is right."""
    from insv2v import ops, _lib
    a, w, b, col, table, rpg, rb_mod, ref, blocks = R.row_bias_case("odd", False, DEV)
    assert rpg == 117 and a.shape[0] > rpg
    with pytest.raises(_lib.HipKernelError):
        ops.gemm(a, w, b, row_bias=table, rows_per_group=rpg, tile=tile)
    out = ops.gemm(a, w, b, row_bias=table, rows_per_group=rpg, tile=0)
    close(out, ref, False, "dispatched gemm, 117 rows per bias group")
    for name, idx in blocks:
        close(out[idx], ref[idx], False, f"dispatched gemm, 117 rows per bias group, {name}")


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("split", [640, 64])
def test_two_source_k(split, tile):
    """[a | a2] as two operands, split at 640 and at 64 (the smallest split insv2v_gemm accepts; a split at 32 is refused).  Same K
    tiles in the same order as the single-source call: bit-identical to it."""
    from insv2v import ops, _lib
    a, w, b, ref, blocks = R.two_source_case(split, DEV)
    a1, a2 = a[:, :split].contiguous(), a[:, split:].contiguous()
    out = run_and_check(lambda t: ops.gemm(a1, w, b, a2=a2, tile=t), tile, ref, False, f"tile {tile} two-source K split at {split}", blocks)
    assert torch.equal(out, ops.gemm(a, w, b, tile=tile)), "two-source K differs from the single-source call"
    with pytest.raises(_lib.HipKernelError):
        ops.gemm(a[:, :32].contiguous(), w, b, a2=a[:, 32:].contiguous(), tile=tile)


# ------------------------------------------------------------------------------------------- 7. GEGLU and output statistics
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("M,C,NH", R.GEGLU_SHAPES)
def test_geglu(M, C, NH, tile):
    """GEGLU on the [32 value | 32 gate] interleaved projection with the folded LayerNorm in front: gemm_q8's permuted W halves,
    gemm_r8's source-row map (16 values and their 16 gates in every fragment).  Less than one tile (N = 320) and 3 column tiles of
    gemm_r8 / 3.75 of gemm_q8; every 16-output-column group (one gemm_r8 fragment) against its own tolerance."""
    from insv2v import ops
    args, col, ref = R.geglu_case(M, C, NH, DEV)
    st = ops.layernorm_stats(args[0])
    what = f"tile {tile} GEGLU {M}x{2 * NH}x{C}"
    out = run_and_check(lambda t: ops.gemm(*args, act=ops.ACT_GEGLU, row_stats=st, col_sum=col, tile=t), tile, ref, True, what,
                        [("last row tile", slice(M - M % R.BM, M))])
    assert out.shape == (M, NH)
    close_groups(out, ref, 1, 16, True, f"{what}, 16-output-column groups")


@pytest.mark.parametrize("M,N,K,res", R.STATS_SHAPES)
def test_r8_output_statistics_per_part(M, N, K, res):
    """emit_stats=True on gemm_r8: N // 160 parts, each part's (sum, sum of squares) against the fp64 sums of the values BEFORE their
    fp16 rounding over that part's 160 columns - per part, so two exchanged parts cannot cancel."""
    from insv2v import ops
    a, w, b, r, ref, sums = R.stats_case(M, N, K, res, DEV)
    got = {}

    def run(t):
        if t != 240:
            return ops.gemm(a, w, b, residual=r, tile=t)
        out, got["st"] = ops.gemm(a, w, b, residual=r, emit_stats=True, tile=t)
        return out
    what = f"tile 240 emit_stats {M}x{N}x{K} residual {res}"
    out = run_and_check(run, 240, ref, False, what)
    assert torch.equal(out, ops.gemm(a, w, b, residual=r, tile=240)), "the output changes when statistics are emitted"
    st = got["st"]
    assert isinstance(st, ops.RowStats) and st.nparts == N // 160 and st.parts.shape == (N // 160, M, 2)
    for p in range(N // 160):
        for j, name in enumerate(("sum", "sum of squares")):
            want = sums[p, :, j]
            err, tol = (st.parts[p, :, j].double() - want).abs().max().item(), R.stats_tol(want)
            print(f"{TAG} {what}, part {p} {name}: max err {err:.4g} (tol {tol:.4g})")
            assert math.isfinite(err) and err <= tol, f"{what}, part {p} {name}: max err {err:.4g} > tol {tol:.4g}"


# ------------------------------------------------------------------------------------------- 8. convolutions at odd grids
def check_conv(x, in_geom, wk, bk, kw, geom, ref, blocks, tile, what):
    from insv2v import ops

    def run(t):
        out, g = ops.conv3x3(x, in_geom, wk, bk, tile=t, **kw)
        assert g == geom
        return out
    return run_and_check(run, tile, ref, False, what, blocks)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("c2", [0, 64])
@pytest.mark.parametrize("nb,h,w,stride,ups", R.CONV_GEOMS)
def test_conv_odd_grids(nb, h, w, stride, ups, c2, tile):
    """The gathered 3x3 convolution at grids where a 256-row tile straddles images and image rows (117 pixels per image: gemm_r8's
    channel-block-major CIM path with and without a second channel source), one-row and one-column images, stride 2 (tap-major), nearest
    x2 upsample; bias, residual and one row-bias group.  Each image and the first / last image rows of all images on their own."""
    x, wk, bk, kw, geom, ref, blocks = R.conv_case(nb, h, w, stride, ups, c2, DEV)
    check_conv(x, (nb, h, w), wk, bk, kw, geom, ref, blocks, tile, f"conv3x3 tile {tile} {nb}x{h}x{w} stride {stride} upsample {ups} c2 {c2}")


@pytest.mark.parametrize("c2", [0, 64])
def test_conv_stream_crosses_tile_boundaries(c2):
    """9 x 13 images for CUs + 2 row tiles on gemm_r8's CIM path: the per-tile (image, row, column) and validity bits are recomputed for
    a workgroup's second tile while the stream crosses into it.  Second-pass tiles by name, every row tile and every image on its own."""
    cus = num_cus()
    nb = R.stream_conv_images(cus)
    x, wk, bk, kw, geom, ref, blocks = R.conv_case(nb, 9, 13, 1, False, c2, DEV)
    sblocks, tiles_m = R.stream_conv_blocks(ref, kw["residual"], nb, cus)
    what = f"conv3x3 tile 240 {nb}x9x13 c2 {c2} {tiles_m} row tiles"
    out = check_conv(x, (nb, 9, 13), wk, bk, kw, geom, ref, blocks + sblocks, 240, what)
    close_groups(out, ref, 0, R.BM, False, f"{what}, every full row tile")
    close_groups(out, ref, 0, 117, False, f"{what}, every image")
