"""The inputs of tests/test_gemm_engines_gpu.py judged without a GPU: every case of tests/gemm_engine_ref.py is built on the CPU (the
stream cases for 4 and for 256 CUs), which asserts every input condition (need_gap: a reference computed without the feature under test
is more than 10 x the tolerance away from the true one); the references are finite; the exact-rounding case tells round-to-nearest-even
from round-toward-zero on more than a third of its elements; the stream's tile map visits every tile exactly once."""
import pytest
import torch

import gemm_engine_ref as R

CPU = torch.device("cpu")


def finite(*refs):
    for r in refs:
        assert torch.isfinite(r).all()


@pytest.mark.parametrize("M,N,K,res", R.PLAIN_SHAPES + [R.MASKED_LINEAR_SHAPE])
def test_plain_inputs(M, N, K, res):
    a, w, b, r, ref, blocks = R.plain_case(M, N, K, res, CPU)
    finite(ref)
    assert ref.shape == (M, N) and all(ref[idx].numel() > 0 for _, idx in blocks)
    assert (M > R.BM) == bool(blocks)


def test_layout_inputs():
    a, w, ref = R.layout_case(CPU)
    finite(ref)
    assert torch.equal(a.float(), torch.eye(320)) and ref.shape == (320, 320)
    # the helper of the wm condition exchanges whole 64-row blocks and nothing else
    rows = torch.arange(320.0)[:, None].expand(320, 2)
    assert torch.equal(R.swap_rows64(rows)[:, 0], torch.cat([torch.arange(64.0, 128), torch.arange(0.0, 64), torch.arange(192.0, 256), torch.arange(128.0, 192), torch.arange(256.0, 320)]))


@pytest.mark.parametrize("res", [False, True])
def test_exact_rounding_inputs(res):
    a, w, b, r, ref32, share, ties = R.exact_case(res, CPU)
    finite(ref32)
    print(f"[gemm_engines] exact rounding, residual {res}: {share:.4f} of the elements differ between nearest-even and toward-zero, {ties} ties differ from half-away")
    assert share > 1 / 3 and ties > 0
    assert ref32.shape == (256, 320) and ref32.dtype == torch.float32
    # the three roundings agree wherever the value is fp16-exact and differ by exactly one step elsewhere
    rne, rtz = ref32.half(), R.round_toward_zero_f16(ref32)
    assert (rtz.float().abs() <= ref32.abs()).all() and ((rne.view(torch.int16) - rtz.view(torch.int16)).abs() <= 1).all()
    exact = rne.float() == ref32
    assert torch.equal(rne[exact], rtz[exact]) and not (rne.float() == ref32).all()
    if res:
        assert ((r.float() >= 1) & (r.float() < 2)).all() and torch.equal((r.float() * 1024) % 1, torch.zeros_like(r.float()))


def test_rounding_helpers():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 1.0 + 2.0 ** -12, 1.0 + 3 * 2.0 ** -12, 0.0, 2.0 ** -13])
    assert R.round_toward_zero_f16(x).tolist() == [1.0, 1.0 + 2.0 ** -10, -1.0, 1.0, 1.0, 0.0, 2.0 ** -13]
    rha, tie = R.round_half_away_f16(x)
    assert rha.tolist() == [1.0 + 2.0 ** -10, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -10), 1.0, 1.0 + 2.0 ** -10, 0.0, 2.0 ** -13]
    assert tie.tolist() == [True, True, True, False, False, False, False]
    assert x.half().tolist() == [1.0, 1.0 + 2.0 ** -9, -1.0, 1.0, 1.0 + 2.0 ** -10, 0.0, 2.0 ** -13]   # nearest even


@pytest.mark.parametrize("tiles_m,tiles_n,grid", [(7, 1, 4), (259, 1, 256), (258, 1, 256), (3, 3, 4), (19, 2, 16), (33, 5, 64), (8, 2, 256), (1, 1, 1)])
def test_tile_map_visits_every_tile_once(tiles_m, tiles_n, grid):
    """row_tile_of / tile_of against a direct enumeration: over the streams of all workgroups (v = b, b + grid, ...) every (row tile,
    column tile) appears exactly once."""
    n = tiles_m * tiles_n
    grid = min(grid, n)
    seen = sorted(R.tile_of(v, tiles_m, tiles_n) for b in range(grid) for v in range(b, n, grid))
    assert seen == [(tm, tn) for tm in range(tiles_m) for tn in range(tiles_n)]
    assert all(R.row_tile_of(v, tiles_m, tiles_n) == R.tile_of(v, tiles_m, tiles_n)[0] for v in range(n))
    assert sorted(R.xcd_remap(v, n) for v in range(n)) == list(range(n))


@pytest.mark.parametrize("tile", R.TILES)
@pytest.mark.parametrize("K", [64, 192, 320])
@pytest.mark.parametrize("cus", [4, 256])
def test_stream_inputs(cus, K, tile):
    a, w, b, ref, blocks, tiles_m = R.stream_case(tile, K, cus, CPU)
    finite(ref)
    assert tiles_m == cus + 3 and ref.shape == (R.BM * (cus + 2) + 8, R.BN[tile])
    assert len(blocks) == 4 and blocks[0][1] == slice((cus + 2) * R.BM, ref.shape[0])
    rows = [idx for _, idx in blocks[1:]]
    assert len({s.start for s in rows}) == 3 and sum(s.stop - s.start == 8 for s in rows) <= 1


@pytest.mark.parametrize("stats", ["pass", "producer"])
def test_folded_layernorm_inputs(stats):
    M, N, K = R.LN_SHAPE
    if stats == "pass":
        a = R.layernorm_rows(M, K, CPU)
    else:   # the rows the producing GEMM stores
        pa, pw, pb = R.producer_operands(M, K, CPU)
        a = (pa.float() @ pw.float().t() + pb).half()
    w, b, col, ref = R.layernorm_case(a, N)
    finite(ref)
    assert M % 2 == 0 and M % R.BM and ref.shape == (M, N)


@pytest.mark.parametrize("kind,ln", [("frame", False), ("frame", True), ("sample", False), ("odd", False)])
def test_row_bias_inputs(kind, ln):
    a, w, b, col, table, rpg, rb_mod, ref, blocks = R.row_bias_case(kind, ln, CPU)
    finite(ref)
    M = ref.shape[0]
    assert sum(int(idx.sum()) for _, idx in blocks) == M
    if kind == "odd":
        assert rpg % R.BM and M > rpg      # a tile would span two groups: row_bias_fits_tiles refuses
    else:
        assert rpg % R.BM == 0
    if kind == "frame":
        assert M // rpg > rb_mod > 0       # the groups wrap


@pytest.mark.parametrize("split", [640, 64])
def test_two_source_inputs(split):
    a, w, b, ref, blocks = R.two_source_case(split, CPU)
    finite(ref)
    assert split % 64 == 0 and ref.shape == R.TWO_SOURCE_SHAPE[:2]


@pytest.mark.parametrize("M,C,NH", R.GEGLU_SHAPES)
def test_geglu_inputs(M, C, NH):
    args, col, ref = R.geglu_case(M, C, NH, CPU)
    finite(ref)
    assert ref.shape == (M, NH) and args[1].shape == (2 * NH, C) and (2 * NH) % 320 == 0 and NH % 16 == 0


@pytest.mark.parametrize("M,N,K,res", R.STATS_SHAPES)
def test_stats_inputs(M, N, K, res):
    a, w, b, r, ref, sums = R.stats_case(M, N, K, res, CPU)
    finite(ref, sums)
    assert sums.shape == (N // 160, M, 2)
    assert torch.allclose(sums[:, :, 0].sum(0), ref.sum(1)) and torch.allclose(sums[:, :, 1].sum(0), (ref * ref).sum(1))


@pytest.mark.parametrize("c2", [0, 64])
@pytest.mark.parametrize("nb,h,w,stride,ups", R.CONV_GEOMS)
def test_conv_inputs(nb, h, w, stride, ups, c2):
    x, wk, bk, kw, geom, ref, blocks = R.conv_case(nb, h, w, stride, ups, c2, CPU)
    finite(ref)
    assert geom[0] == nb and ref.shape == (geom[0] * geom[1] * geom[2], R.CONV_COUT) and wk.shape == (R.CONV_COUT, 9 * (R.CONV_C1 + c2))
    assert len(blocks) == nb + 1 and kw["rows_per_group"] == ref.shape[0]
    if (nb, h, w) == (5, 9, 13):   # the tile boundaries fall mid image and mid image row
        assert all((t * R.BM) % 117 and (t * R.BM) % 13 for t in (1, 2)) and ref.shape[0] == 585


@pytest.mark.parametrize("c2", [0, 64])
@pytest.mark.parametrize("cus", [4, 256])
def test_stream_conv_inputs(cus, c2):
    nb = R.stream_conv_images(cus)
    x, wk, bk, kw, geom, ref, blocks = R.conv_case(nb, 9, 13, 1, False, c2, CPU)
    finite(ref)
    sblocks, tiles_m = R.stream_conv_blocks(ref, kw["residual"], nb, cus)
    assert tiles_m == cus + 2 and len(sblocks) == 3
