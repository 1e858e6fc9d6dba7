"""The float64 reference of the Winograd transform stages (tests/winograd_ref.py) and the inputs of the bit-exact GPU cases
(tests/test_winograd_stages_gpu.py), checked without a GPU and without a kernel:
  * input_ref -> float64 products with G g G^T -> output_ref IS the convolution (to 1e-10), in both forms, at odd sizes: the tile order and
    the k = i*4 + j / g = ci*3 + cj conventions are pinned independently of the kernels;
  * on the exact cases every staged pixel and every reference value is an fp16 number, so the GPU comparison can be bit for bit;
  * the exact cases can tell a wrong kernel from a right one: a reference computed with the neighbouring sample's table, a normalised
    padding, x read for x2 or the neighbouring row-bias group differs from the true one;
  * the geometries meet the launch regimes of insv2v_winograd_input they are listed for."""
import pytest
import torch
import torch.nn.functional as F

import winograd_ref as wr

F64 = torch.float64
SIZES = [(1, 1), (2, 2), (5, 7), (4, 6), (3, 5)]


def rnd64(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed + sum(shape)), dtype=F64)


def to_nchw(rows, NB, H, W):
    return rows.reshape(NB, H, W, -1).permute(0, 3, 1, 2)


def to_rows(nchw):
    n, c, h, w = nchw.shape
    return nchw.permute(0, 2, 3, 1).reshape(n * h * w, c)


@pytest.mark.parametrize("upsample", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("H,W", SIZES)
def test_reference_is_the_convolution(H, W, norm, upsample):
    NB, C, Cout, ips = 3, 5, 4, 2
    x = rnd64(NB * H * W, C, seed=1).half().to(F64)
    ab = torch.stack([1 + 0.2 * rnd64(2, C, seed=2), 0.3 * rnd64(2, C, seed=3)], -1) if norm else None
    w, b = rnd64(Cout, C, 3, 3, seed=4), rnd64(Cout, seed=5)
    up = 4 if upsample else 1
    rpg = ips * H * W * up
    rb, res = rnd64(2, Cout, seed=6), rnd64(NB * H * W * up, Cout, seed=7)
    V = wr.input_ref(x, NB, H, W, ab, ips, norm, upsample)
    U = wr.weights_ref(w, upsample)
    ng = 9 if upsample else 16
    assert V.shape == (ng, wr.tiles_of(NB, H, W, upsample), C) and U.shape == (ng, Cout, C)
    M = torch.einsum("ktc,koc->kto", V, U)
    y = wr.output_ref(M, NB, H, W, b, rb, rpg, res, upsample)
    img = to_nchw(wr.stage_ref(x, NB, H, W, ab, ips, norm), NB, H, W)
    if upsample:
        img = F.interpolate(img, scale_factor=2.0, mode="nearest")
    ref = to_rows(F.conv2d(img, w, b, padding=1)) + rb.repeat_interleave(rpg, 0)[:res.shape[0]] + res
    assert y.shape == ref.shape
    assert (y - ref).abs().max().item() <= 1e-10
    # ... and each addend on its own is what the convolution alone lacks
    assert (wr.output_ref(M, NB, H, W, None, None, 0, None, upsample) - to_rows(F.conv2d(img, w, None, padding=1))).abs().max().item() <= 1e-10


def test_upsample_form_drops_only_zero_matrices():
    """Row / column 2 of B^T d B vanish on the nearest-x2 grid: the 9 matrices are the whole transform."""
    NB, H, W, C = 2, 3, 5, 4
    d = wr.stage_ref(rnd64(NB * H * W, C), NB, H, W)
    v = torch.einsum("ir,ntxrcC,jc->ijntxC", wr.BT, wr._patches(d, NB, H, W, True), wr.BT)
    assert v[2].abs().max().item() == 0 and v[:, 2].abs().max().item() == 0
    assert v[wr.UP_IDX][:, wr.UP_IDX].abs().min().item() > 0


def test_stage_rounds_once_to_fp16():
    NB, H, W, C = 2, 3, 3, 8
    x = rnd64(NB * H * W, C).half().to(F64)
    ab = torch.stack([1 + 0.2 * rnd64(2, C, seed=2), 0.3 * rnd64(2, C, seed=3)], -1)
    d = wr.stage_ref(x, NB, H, W, ab, 1, True)
    t = ab[torch.arange(NB * H * W) // (H * W)]
    assert torch.equal(d, F.silu(x * t[..., 0] + t[..., 1]).half().to(F64))
    assert torch.equal(wr.stage_ref(x, NB, H, W), x)


# ---------------------------------------------------------------------------------------------------------------- the exact cases
@pytest.mark.parametrize("geom", wr.GEOMS, ids=wr.geom_id)
@pytest.mark.parametrize("norm", [False, True])
def test_exact_input_cases_are_exact(geom, norm):
    (NB, H, W, ips), up = geom
    x, ab = wr.exact_input_case(NB, H, W, ips, up, norm)
    assert wr.is_fp16(x) and x.abs().max().item() <= (2 if norm else 4)
    d = x
    if norm:
        t = ab[torch.arange(NB * H * W) // (ips * H * W)]
        d = x * t[..., 0] + t[..., 1]               # NOT rounded: the staged pixel itself must be an fp16 number
        assert ab.shape == (-(-NB // ips), wr.C_IN, 2) and d.abs().max().item() <= 5
    assert wr.is_fp16(d) and torch.equal(wr.stage_ref(x, NB, H, W, ab, ips), d)
    V = wr.input_ref(x, NB, H, W, ab, ips, False, up)
    assert wr.is_fp16(V) and V.abs().max().item() <= (20 if norm else 16)
    assert V.shape == (9 if up else 16, wr.tiles_of(NB, H, W, up), wr.C_IN)

    # distinguishability: what a subtly wrong kernel would compute differs from the reference
    assert not torch.equal(x[:, :wr.C1_IN], x[:, wr.C1_IN:])
    xx = torch.cat([x[:, :wr.C1_IN], x[:, :wr.C1_IN]], 1)
    assert not torch.equal(wr.input_ref(xx, NB, H, W, ab, ips, False, up)[:, :, wr.C1_IN:], V[:, :, wr.C1_IN:]), "x read for x2"
    if norm:
        assert (ab[..., 1] != 0).all()
        if ab.shape[0] > 1:
            assert (ab[1:] != ab[:-1]).all()
            assert not torch.equal(wr.input_ref(x, NB, H, W, ab.roll(1, 0), ips, False, up), V), "the neighbouring sample's table"
        # a kernel that normalises the padding sees `shift` where the reference sees 0
        border = wr.input_ref(torch.zeros_like(x), NB, H, W, ab, ips, False, up)
        assert border.abs().max().item() > 0


@pytest.mark.parametrize("geom", wr.GEOMS, ids=wr.geom_id)
@pytest.mark.parametrize("Cout", [16, 8])
def test_exact_output_cases_are_exact(geom, Cout):
    (NB, H, W, ips), up = geom
    M, bias, rb, rpg, res = wr.exact_output_case(NB, H, W, ips, up, Cout)
    pixels = NB * H * W * (4 if up else 1)
    assert rpg % (H * W * (4 if up else 1)) == 0 and rb.shape[0] * rpg >= pixels and res.shape == (pixels, Cout)
    for t in (M, bias, rb, res):
        assert wr.is_fp16(t) and t.abs().max().item() <= 4 and torch.equal(t * 8, (t * 8).round())
    if rb.shape[0] > 1:
        assert (rb[1:] != rb[:-1]).all()
    full = wr.output_ref(M, NB, H, W, bias, rb, rpg, res, up)
    for use_res in (False, True):
        for use_rb in (False, True):
            for use_b in (False, True):
                y = wr.output_ref(M, NB, H, W, bias if use_b else None, rb if use_rb else None, rpg, res if use_res else None, up)
                assert y.shape == (pixels, Cout) and wr.is_fp16(y) and y.abs().max().item() <= 48
                if not (use_res and use_rb and use_b):
                    assert not torch.equal(y, full)
    if rb.shape[0] > 1:
        assert not torch.equal(wr.output_ref(M, NB, H, W, bias, rb.roll(1, 0), rpg, res, up), full), "the neighbouring row-bias group"


# ---------------------------------------------------------------------------------------------------------------- launch regimes
def launch_regime(H, W, upsample):
    """The launch arithmetic of insv2v_winograd_input (csrc/winograd.hip), restated: (images per workgroup, bands, tile rows per band,
    LDS bytes)."""
    HW = H * W
    ntile = HW if upsample else ((H + 1) // 2) * ((W + 1) // 2)
    slots = HW if upsample else (HW + 1) & ~1
    trows = H if upsample else (H + 1) // 2
    band_tr, ipb = trows, 1
    if slots * 128 <= 65536:
        ipb = max(1, 32 // ntile)
        while ipb > 1 and ipb * slots * 128 > 65536:
            ipb -= 1
    else:
        max_rows = 65536 // (W * 128)
        band_tr = max_rows - 2 if upsample else (max_rows - 2) // 2
        if band_tr < 1:
            return None
    nbands = -(-trows // band_tr)
    srows = H if nbands == 1 else (band_tr + 2 if upsample else 2 * band_tr + 2)
    s = srows * W
    return ipb, nbands, band_tr, ipb * (s if upsample else (s + 1) & ~1) * 128


def test_geometries_meet_their_regimes():
    want = {("direct", 7, 4, 6): (5, 1), ("direct", 3, 2, 2): (32, 1), ("direct", 5, 1, 1): (32, 1), ("direct", 3, 1, 7): (8, 1), ("direct", 3, 7, 1): (8, 1),
            ("direct", 3, 5, 7): (2, 1), ("direct", 2, 16, 32): (1, 1), ("direct", 2, 19, 27): (1, 2), ("direct", 1, 13, 80): (1, 4),
            ("direct", 1, 8, 103): (1, 4), ("direct", 1, 9, 128): (1, 5),
            ("up", 7, 2, 3): (5, 1), ("up", 3, 1, 1): (32, 1), ("up", 2, 1, 5): (6, 1), ("up", 3, 3, 5): (2, 1), ("up", 2, 16, 32): (1, 1),
            ("up", 1, 19, 27): (1, 2), ("up", 1, 5, 128): (1, 3)}
    for (NB, H, W, ips), up in wr.GEOMS:
        ipb, nbands, band_tr, lds = launch_regime(H, W, up)
        assert (ipb, nbands) == want[("up" if up else "direct", NB, H, W)], (NB, H, W, up, ipb, nbands)
        assert lds <= 65536
        if ipb > 1 and NB > ipb:
            assert NB % ipb, "a partial last workgroup is the point of this geometry"
        if ipb > 1 and NB > 1:
            first = min(ipb, NB)
            assert (first - 1) // ips > 0, "a GroupNorm sample boundary must fall inside the first workgroup's images"
    assert launch_regime(16, 32, False)[3] == 65536 and launch_regime(16, 32, True)[3] == 65536      # whole image at the limit
    assert launch_regime(9, 128, False) == (1, 5, 1, 65536) and launch_regime(5, 128, True) == (1, 3, 2, 65536)
    assert launch_regime(8, 103, False)[2] == 1 and launch_regime(13, 80, False)[2] == 2 and 13 // 2 + 1 == 7  # 7 tile rows in bands of 2
    assert launch_regime(5, 7, False)[3] == 2 * 36 * 128                                                  # 35 pixels -> 36 slots
    assert launch_regime(8, 129, False) is None
