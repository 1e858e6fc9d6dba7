"""The float64 references of the optical-flow kernels (tests/flow_ref.py) and the inputs of the bit-exact GPU cases
(tests/test_flow_stages_gpu.py), checked without a GPU and without a kernel:
  * every function of flow_ref equals its counterpart in float64 to 1e-10 (1e-9 where the counterpart normalises coordinates to [-1, 1] and
    the sampler maps them back: CorrBlock.index_pyramid and warp_image): oracle/raft.py, oracle/flow.py, F.conv2d, F.instance_norm,
    F.avg_pool2d - at the grids 17x23, 16x16, 19x40 and 45x80, whose pyramids drop a row or a column at up to three levels;
  * on the exact cases every intermediate of the kernels' fp32 arithmetic is representable, so the GPU comparison can be bit for bit;
  * the exact cases can tell a wrong kernel from a right one: a reference with x and y offsets swapped, level sizes taken as ceil, border
    samples clamped instead of zeroed, neighbour k read as kx*3 + ky, or x2 read for x differs from the true one;
  * the flow-correction inputs keep the float64 coverage sum away from the 0.5 threshold and contain masked and covered pixels."""
import pytest
import torch
import torch.nn.functional as F

import flow_ref as fr

F64 = torch.float64
GRID_IDS = [f"{h}x{w}" for h, w in fr.GRIDS]


def rnd64(*shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed + sum(shape)), dtype=F64)


def maxdiff(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item()


def to_rows(nchw):
    n, c, h, w = nchw.shape
    return nchw.permute(0, 2, 3, 1).reshape(n * h * w, c)


def pyramid_of(corr, h, w, levels=4):
    pyr = [corr]
    for _ in range(levels - 1):
        pyr.append(fr.avgpool_ref(pyr[-1]))
    return pyr


# ---------------------------------------------------------------------------------------------------------------- pins
# every geometry from one source, and from two (C1 channels | the rest) wherever there is more than one 8-channel chunk
CONV_PINS = [(g[:4] + (0,)) for g in fr.CONV_GEOMS] + [(g[:4] + (g[4] or g[0] // 2,)) for g in fr.CONV_GEOMS if g[0] >= 16]


@pytest.mark.parametrize("C,kh,kw,stride,C1", CONV_PINS)
def test_im2col_then_matmul_is_conv2d(C, kh, kw, stride, C1):
    N, (IH, IW) = 2, ((34, 46) if stride == 2 else (17, 23))
    x = rnd64(N, C, IH, IW, seed=kh)
    w, b = rnd64(5, C, kh, kw, seed=1), rnd64(5, seed=2)
    pad = ((kh - 1) // 2, (kw - 1) // 2)
    rows = to_rows(x)
    cols, g = fr.im2col_ref(rows[:, :C1] if C1 else rows, rows[:, C1:] if C1 else None, (N, IH, IW), kh, kw, stride, pad)
    ref = F.conv2d(x, w, b, stride=stride, padding=pad)
    assert g == (N, ref.shape[2], ref.shape[3]) and g[1:] == (17, 23)
    out = cols @ w.permute(0, 2, 3, 1).reshape(5, -1).T + b
    assert maxdiff(out, to_rows(ref)) <= 1e-10


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("HW,C", [(391, 8), (64, 24), (7, 96)])
def test_instance_norm_ref_is_instance_norm(HW, C, relu):
    N = 3
    x = rnd64(N * HW, C) * 0.5 + 30 * rnd64(1, C, seed=1)
    ref = F.instance_norm(x.reshape(N, HW, C).permute(0, 2, 1).reshape(N, C, HW, 1), eps=1e-5)
    ref = ref.reshape(N, C, HW).permute(0, 2, 1).reshape(N * HW, C)
    assert maxdiff(fr.instance_norm_ref(x, N, HW, relu, 1e-5), F.relu(ref) if relu else ref) <= 1e-10


def test_ew_ref():
    a, b, c = rnd64(40, 16), rnd64(40, 16, seed=1), torch.sigmoid(rnd64(40, 16, seed=2))
    assert torch.equal(fr.ew_ref("relu", a), F.relu(a)) and torch.equal(fr.ew_ref("add_relu", a, b), F.relu(a + b))
    assert maxdiff(fr.ew_ref("tanh", a), (torch.exp(2 * a) - 1) / (torch.exp(2 * a) + 1)) <= 1e-12
    assert torch.equal(fr.ew_ref("gru_rh", a, b), a * b)                         # a = r, b = h
    assert torch.equal(fr.ew_ref("gru_out", a, b, c), (1 - c) * b + c * a)        # a = q, b = h, c = z
    assert fr.EW_OPS == ("relu", "add_relu", "tanh", "gru_rh", "gru_out")


@pytest.mark.parametrize("h,w", fr.GRIDS, ids=GRID_IDS)
def test_pyramid_is_the_oracles(h, w):
    """avgpool_ref chained == F.avg_pool2d chained == CorrBlock.build_pyramid: floor sizes at every level."""
    from oracle.raft import CorrBlock
    B, C = (1, 16) if h * w > 1000 else (2, 16)
    f1, f2 = rnd64(B, C, h, w, seed=1), rnd64(B, C, h, w, seed=2)
    cb = CorrBlock(4, 4)
    cb.build_pyramid(f1, f2)
    corr = torch.einsum("bcp,bcq->bpq", f1.reshape(B, C, h * w), f2.reshape(B, C, h * w)).reshape(B * h * w, h, w) / 4.0
    pyr = pyramid_of(corr, h, w)
    x = corr[:, None]
    for l in range(4):
        assert pyr[l].shape == (B * h * w, h >> l, w >> l)
        assert maxdiff(pyr[l], cb.pyramid[l][:, 0]) <= 1e-10 and maxdiff(pyr[l], x[:, 0]) <= 1e-10
        x = F.avg_pool2d(x, 2, 2)
    if (h, w) == (17, 23):
        assert [tuple(p.shape[1:]) for p in pyr] == [(17, 23), (8, 11), (4, 5), (2, 2)]
    if (h, w) == (45, 80):
        assert [tuple(p.shape[1:]) for p in pyr] == [(45, 80), (22, 40), (11, 20), (5, 10)]


@pytest.mark.parametrize("h,w", fr.GRIDS, ids=GRID_IDS)
def test_corr_lookup_ref_is_index_pyramid(h, w):
    """On random operands with large displacements, and on the exact case (integers, border lines, +-10^4).  1e-9: the oracle normalises
    the sample positions to [-1, 1] and grid_sample maps them back."""
    from oracle.raft import CorrBlock, coords_grid
    B = 1
    cb = CorrBlock(4, 4)
    corr = rnd64(B * h * w, h, w, seed=3)
    cb.pyramid = [p[:, None] for p in pyramid_of(corr, h, w)]
    coords = coords_grid(B, h, w).to(F64) + 6 * rnd64(B, 2, h, w, seed=4)
    assert torch.equal(coords_grid(B, h, w).to(F64), fr.grid_xy(B, h, w))
    ref = to_rows(cb.index_pyramid(coords))
    out = fr.corr_lookup_ref([p[:, 0] for p in cb.pyramid], coords, 4, 328)
    assert maxdiff(out[:, :324], ref) <= 1e-9 and out[:, 324:].abs().max().item() == 0
    pyr, coords = fr.corr_case(B, h, w, 4)
    cb.pyramid = [p[:, None] for p in pyr]
    assert maxdiff(fr.corr_lookup_ref(pyr, coords, 4, 324), to_rows(cb.index_pyramid(coords))) <= 1e-9
    if h * w < 1000:
        cb2 = CorrBlock(2, 1)
        cb2.pyramid = cb.pyramid[:2]
        out = fr.corr_lookup_ref(pyr[:2], coords, 1, 24)
        assert maxdiff(out[:, :18], to_rows(cb2.index_pyramid(coords))) <= 1e-9 and out[:, 18:].abs().max().item() == 0


@pytest.mark.parametrize("h,w", fr.GRIDS, ids=GRID_IDS)
def test_convex_upsample_ref_is_upsample_flow(h, w):
    from oracle.raft import upsample_flow, coords_grid
    B = 2
    coords = fr.grid_xy(B, h, w) + 5 * rnd64(B, 2, h, w, seed=5)
    mask = rnd64(B, 576, h, w, seed=6) * 3
    ref = upsample_flow(coords - coords_grid(B, h, w).to(F64), mask)
    assert maxdiff(fr.convex_upsample_ref(coords, to_rows(mask)), ref) <= 1e-10
    coords, mask, _ = fr.upsample_case(B, h, w)
    ref = upsample_flow(coords - coords_grid(B, h, w).to(F64), mask.reshape(B, h, w, 576).permute(0, 3, 1, 2))
    assert torch.equal(fr.convex_upsample_ref(coords, mask), ref)


def test_flow_rows_ref():
    from oracle.raft import coords_grid
    B, h, w = 2, 5, 7
    c, d = fr.grid_xy(B, h, w) + rnd64(B, 2, h, w), rnd64(B * h * w, 8, seed=1)
    c2, rows = fr.flow_rows_ref(c, d, 8)
    want = c + d[:, :2].reshape(B, h, w, 2).permute(0, 3, 1, 2)
    assert torch.equal(c2, want) and torch.equal(rows[:, :2], to_rows(want - coords_grid(B, h, w).to(F64))) and rows[:, 2:].abs().max().item() == 0
    c3, rows = fr.flow_rows_ref(c, None, 2)
    assert torch.equal(c3, c) and rows.shape == (B * h * w, 2)


@pytest.mark.parametrize("H,W", [(17, 23), (45, 80), (5, 7), (2, 2)])
def test_warp_ref_is_warp_image(H, W):
    """1e-9: both normalise to [-1, 1] and back, the oracle inside grid_sample."""
    from oracle.flow import warp_image
    img, flow = fr.warp_case(2, 3, H, W)
    ref = warp_image(img, flow)
    assert ref.dtype == F64 and maxdiff(fr.warp_ref(img, flow), ref) <= 1e-9
    assert maxdiff(fr.warp_ref(img, torch.zeros_like(flow)), img) <= 1e-12


@pytest.mark.parametrize("src,dst", fr.RESIZE_PAIRS)
def test_resize_flow_ref_is_resize_flow(src, dst):
    from oracle.flow import resize_flow
    flow = fr.resize_case(2, *src)
    ref = resize_flow(flow, dst)
    assert ref.dtype == F64 and maxdiff(fr.resize_flow_ref(flow, dst), ref) <= 1e-10


@pytest.mark.parametrize("h,w,R,Q", fr.CORRECTION_SETS)
def test_flow_correction_ref_and_its_inputs(h, w, R, Q):
    """The reference is the pipe's formula on the oracle's warp (1e-9: the warp's), and the inputs keep msum off the 0.5 threshold."""
    from oracle.flow import warp_image
    eps, lat, ref, flows = fr.correction_case(h, w, R, Q)
    assert all(fr.is_fp32(t) for t in (eps, lat, ref, flows)) and flows.shape == (Q, R, 2, h, w)
    out, msum = fr.flow_correction_ref(eps, lat, ref, flows, fr.SQRT_A, fr.SQRT_1MA)
    delta = (lat[:R] - fr.SQRT_A * ref) / fr.SQRT_1MA - eps[:R]
    for q in range(Q):
        wd, m = warp_image(delta, flows[q]).sum(0), warp_image(torch.ones_like(delta[:, :1]), flows[q]).sum(0)
        want = torch.where(m > 0.5, wd / m, torch.zeros((), dtype=F64))
        near = (msum[q] - 0.5).abs() <= 1e-3
        assert maxdiff(msum[q], m[0]) <= 1e-9 and maxdiff(out[q][:, ~near], want[:, ~near]) <= 1e-9
    share = ((msum - 0.5).abs() <= 1e-3).double().mean().item()
    masked, covered = (msum <= 0.5).double().mean().item(), (msum >= R - 1e-9).double().mean().item()
    print(f"[flow stages] flow-correction inputs {h}x{w} R={R}: {100 * share:.2f} % of pixels within 1e-3 of msum = 0.5, "
          f"{100 * masked:.1f} % masked, {100 * covered:.1f} % fully covered")
    assert share <= 0.01
    assert masked > 0 and covered > 0 and (out[(msum <= 0.5)[:, None].expand_as(out)] == 0).all()
    assert msum.reshape(Q, -1)[:, 0].abs().max().item() == 0 and (msum.reshape(Q, -1)[:, 1] - R).abs().max().item() <= 1e-12
    for q in range(Q):           # reference 0 is sampled on column 0, on column w - 1, on row h - 1, half a pixel outside and far outside
        ix, iy = fr.warp_coords_ref(flows[q, :1])
        assert (ix.abs() < 1e-9).any() and ((ix - (w - 1)).abs() < 1e-9).any() and ((iy - (h - 1)).abs() < 1e-9).any()
        assert (((ix + 0.5).abs() < 1e-9) & ((iy + 0.5).abs() < 1e-9)).any() and (ix.abs() > 1000).any()


# ---------------------------------------------------------------------------------------------------------------- the exact cases
@pytest.mark.parametrize("h,w", fr.GRIDS, ids=GRID_IDS)
@pytest.mark.parametrize("levels,radius", [(4, 4), (2, 1)])
def test_corr_case_is_exact(h, w, levels, radius):
    B = 1 if h * w > 1000 else 2
    pyr, coords = fr.corr_case(B, h, w, levels)
    assert len(pyr) == levels and all(p.shape == (B * h * w, h >> l, w >> l) for l, p in enumerate(pyr))
    assert all(torch.equal(p, p.round()) and p.abs().max().item() <= 8 and (p != 0).all() for p in pyr)
    assert fr.is_fp32(coords) and torch.equal(coords * 8, (coords * 8).round())
    side = 2 * radius + 1
    ref = fr.corr_lookup_ref(pyr, coords, radius, levels * side * side)
    # multiples of 2^-12 below 8: 15 bits; and the same arithmetic carried out in fp32 rounds nowhere
    assert torch.equal(ref * 4096, (ref * 4096).round()) and ref.abs().max().item() <= 8
    assert torch.equal(fr.corr_lookup_ref(pyr, coords, radius, levels * side * side, dtype=torch.float32).to(F64), ref)
    assert fr.is_fp16(ref) == (levels == 2), "4 levels: the final rounding to fp16 matters; 2 levels (multiples of 2^-8): it cannot"
    # what the cases contain
    cx, cy = coords[0, 0].reshape(-1), coords[0, 1].reshape(-1)
    n = len(fr.corr_specials(h, w))
    assert [(x, y) for x, y in zip(cx[:n].tolist(), cy[:n].tolist())] == fr.corr_specials(h, w)
    on_int = (cx == cx.round()) & (cy == cy.round())
    assert on_int.sum().item() >= 5
    assert ((cx > -1) & (cx < 0)).any() and ((cx > w - 1) & (cx < w)).any() and ((cy > -1) & (cy < 0)).any() and ((cy > h - 1) & (cy < h)).any()
    assert (cx.abs() >= fr.FAR).sum().item() >= 2 and (cy.abs() >= fr.FAR).sum().item() >= 2
    far = (cx.abs() >= fr.FAR) | (cy.abs() >= fr.FAR)
    assert ref[:h * w][far].abs().max().item() == 0 and (radius < 4 or (ref[:h * w][~far].abs().amax(1) > 0).all())


@pytest.mark.parametrize("h,w", fr.GRIDS, ids=GRID_IDS)
def test_corr_case_tells_a_wrong_kernel(h, w):
    pyr, coords = fr.corr_case(1, h, w, 4)
    ref = fr.corr_lookup_ref(pyr, coords, 4, 324)
    n = len(fr.corr_specials(h, w))
    for name in ("swap_xy", "clamp") + (("ceil_levels",) if (h, w) != (16, 16) else ()):
        bad = fr.corr_lookup_ref(pyr, coords, 4, 324, mutate=name)
        assert not torch.equal(bad, ref), name
        assert not torch.equal(bad[:n], ref[:n]), f"{name}: the named pixels alone must show it"
        for l in range(4):
            differs = not torch.equal(bad[:, 81 * l:81 * (l + 1)], ref[:, 81 * l:81 * (l + 1)])
            same_size = name == "ceil_levels" and (fr.level_size(h, l, "ceil_levels"), fr.level_size(w, l, "ceil_levels")) == (h >> l, w >> l)
            assert differs != same_size, f"{name} at level {l}"
    if (h, w) == (16, 16):       # even at every level: floor and ceil agree
        assert torch.equal(fr.corr_lookup_ref(pyr, coords, 4, 324, mutate="ceil_levels"), ref)


@pytest.mark.parametrize("h,w", [(17, 23), (45, 80), (8, 11), (5, 10)])
def test_avgpool_case(h, w):
    x = fr.avgpool_case(3, h, w)
    assert torch.equal(x * 16, (x * 16).round()) and x.abs().max().item() <= 8
    y = fr.avgpool_ref(x)
    assert y.shape == (3, h // 2, w // 2) and fr.is_fp32(y) and torch.equal(y * 64, (y * 64).round())
    if (h & 1) or (w & 1):
        bad = fr.avgpool_ref(x, mutate="ceil_levels")
        assert bad.shape != y.shape or not torch.equal(bad, y)
        # a kernel that took the output row length from ceil(w / 2) would shift every row after the first
        assert bad.shape[2] == y.shape[2] or not torch.equal(bad.reshape(3, -1)[:, :y[0].numel()], y.reshape(3, -1))


@pytest.mark.parametrize("C,kh,kw,stride,C1", fr.CONV_GEOMS)
def test_im2col_case_tells_a_wrong_kernel(C, kh, kw, stride, C1):
    N, (IH, IW) = 2, ((34, 46) if stride == 2 else (17, 23))
    C1 = C1 or (C // 2 if C >= 16 else 0)
    x, x2 = fr.im2col_case(N, IH, IW, C, C1)
    assert fr.is_fp16(x) and (x != 0).all() and (x2 is None or (fr.is_fp16(x2) and (x2 != 0).all()))
    pad = ((kh - 1) // 2, (kw - 1) // 2)
    ref, g = fr.im2col_ref(x, x2, (N, IH, IW), kh, kw, stride, pad)
    assert g == (N, 17, 23) and ref.shape == (N * 17 * 23, kh * kw * C) and fr.is_fp16(ref)
    if kh * kw > 1:
        assert (ref == 0).any(), "the padding is visible"
    if x2 is not None:
        bad, _ = fr.im2col_ref(x, x2, (N, IH, IW), kh, kw, stride, pad, mutate="x2_for_x")
        assert not torch.equal(bad, ref), "x2 read for x"


def test_flow_rows_case_is_exact():
    B, h, w = 2, 17, 23
    coords, delta = fr.flow_rows_case(B, h, w, 6)
    c2, rows = fr.flow_rows_ref(coords, delta, 8)
    assert fr.is_fp32(coords) and fr.is_fp32(delta) and fr.is_fp32(c2) and fr.is_fp32(rows)
    assert torch.equal(c2 * 64, (c2 * 64).round()) and c2.abs().max().item() < 128           # 13 bits
    assert not fr.is_fp16(rows), "the rounding to fp16 should matter somewhere"
    assert (delta[:, 2:] != 0).any(), "columns of delta past the second must be ignored"


@pytest.mark.parametrize("h,w", fr.GRIDS, ids=GRID_IDS)
def test_upsample_case_is_exact_and_tells_a_wrong_kernel(h, w):
    B = 2
    coords, mask, sel = fr.upsample_case(B, h, w)
    flow = coords - fr.grid_xy(B, h, w)
    assert fr.is_fp32(coords) and fr.is_fp16(mask) and torch.equal(flow * 8, (flow * 8).round()) and (flow != 0).all() and flow.abs().max().item() <= 16
    m = mask.reshape(B, h, w, 9, 64)
    assert ((m == 0).sum(3) == 1).all() and ((m == -60000).sum(3) == 8).all() and torch.equal(m.argmax(3), sel)
    assert torch.exp(torch.tensor(-60000.0, dtype=torch.float32)).item() == 0
    for k in range(9):           # every neighbour at every pixel: on every border and in every corner
        assert ((sel == k).sum(3) >= 7).all()
    ref = fr.convex_upsample_ref(coords, mask)
    # the reference IS 8 x the selected neighbour's flow, 0 outside
    sub = ref.reshape(B, 2, h, 8, w, 8).permute(0, 1, 2, 4, 3, 5).reshape(B, 2, h, w, 64)
    ys, xs = torch.arange(h).reshape(1, h, 1, 1) + sel // 3 - 1, torch.arange(w).reshape(1, 1, w, 1) + sel % 3 - 1
    inside = (ys >= 0) & (ys < h) & (xs >= 0) & (xs < w)
    for c in range(2):
        picked = flow[torch.arange(B).reshape(B, 1, 1, 1), c, ys.clamp(0, h - 1), xs.clamp(0, w - 1)]
        assert torch.equal(sub[:, c], torch.where(inside, 8 * picked, torch.zeros((), dtype=F64)))
    assert (~inside).any() and fr.is_fp32(ref)
    for name in ("k_transposed", "clamp"):
        assert not torch.equal(fr.convex_upsample_ref(coords, mask, mutate=name), ref), name


@pytest.mark.parametrize("H,W", [(17, 23), (45, 80), (5, 7), (2, 2)])
def test_warp_case_reaches_the_border_and_tells_clamping(H, W):
    img, flow = fr.warp_case(2, 3, H, W)
    assert fr.is_fp32(img) and fr.is_fp32(flow)
    ix, iy = fr.warp_coords_ref(flow)
    assert ((ix - 0).abs() < 1e-9).any() and ((ix - (W - 1)).abs() < 1e-9).any() and ((iy - 0).abs() < 1e-9).any() and ((iy - (H - 1)).abs() < 1e-9).any()
    assert ((ix + 0.5).abs() < 1e-9).any() and ((ix - (W - 0.5)).abs() < 1e-9).any() and (ix.abs() > 1000).any()
    ref = fr.warp_ref(img, flow)
    assert (ref[1, :, H - 1, W - 1] == 0).all()
    assert not torch.equal(fr.warp_ref(img, flow, mutate="clamp"), ref)


@pytest.mark.parametrize("HW,C", [(391, 8), (3600, 24), (64, 96), (7, 256)])
def test_instance_norm_case(HW, C):
    N = 2
    x = fr.instance_norm_case(N, HW, C)
    assert fr.is_fp16(x) and x.abs().max().item() < 40
    v = x.reshape(N, HW, C)
    assert (v[:, :, 3] == v[:, :1, 3]).all()
    y = fr.instance_norm_ref(x, N, HW).reshape(N, HW, C)
    assert (y[:, :, 3] == 0).all() and torch.isfinite(y).all()
    off = (v[:, 0] - v[:, 1:].mean(1)).abs() / v[:, 1:].std(1).clamp_min(1e-3)
    keep = torch.arange(C) != 3
    if HW >= 64:
        assert (off[:, keep] > 5).all(), "row 0 is an outlier in every channel"
