"""Float64 restatements of the optical-flow kernels (csrc/raft.hip: im2col, instance_norm, ew, avgpool2x2, corr_lookup, raft_flow_rows,
convex_upsample; csrc/elementwise.hip: warp_image, resize_flow, flow_correction) for the stage tests (tests/test_flow_stages_cpu.py,
tests/test_flow_stages_gpu.py), and the inputs of their bit-exact cases.

Every function is written from the operation's definition in plain index arithmetic with torch on the CPU: no F.grid_sample, no F.unfold,
no F.interpolate, no oracle and no project code - a second, independent reading (tests/test_flow_stages_cpu.py pins it to the first).

Layouts (the C header's): activations are channels-last rows [n*h*w, C]; correspondences / flows are [B, 2, h, w] with channel 0 = x,
1 = y; pixel index = (b*h + y)*w + x; pyramid level l is [B*h*w, h >> l, w >> l].

The keyword arguments named `mutate` compute what a subtly wrong kernel would: the CPU file checks that each one differs from the true
reference on the exact cases, i.e. that the cases can tell such a kernel from a right one."""
import functools

import torch

F64 = torch.float64
EW_OPS = ("relu", "add_relu", "tanh", "gru_rh", "gru_out")      # INSV2V_EW_RELU .. INSV2V_EW_GRU_OUT = 1 .. 5, in this order
GRIDS = [(17, 23), (16, 16), (19, 40), (45, 80)]
# the estimator's convolution geometries: (C, kh, kw, stride, channels of the first source when split, else 0)
CONV_GEOMS = [(8, 7, 7, 2, 0), (64, 3, 3, 1, 0), (96, 3, 3, 2, 0), (64, 1, 1, 2, 0), (384, 1, 5, 1, 0), (384, 5, 1, 1, 128)]
RESIZE_PAIRS = [((136, 184), (17, 23)), ((360, 640), (45, 80)), ((50, 70), (17, 23))]
FAR = 1.0e4


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def is_fp16(t):
    return bool(torch.equal(t.half().to(F64), t))


def is_fp32(t):
    return bool(torch.equal(t.float().to(F64), t))


def ulp16(v):
    """The spacing of fp16 numbers at |v|, elementwise (float64 tensor; the subnormal spacing 2^-24 below 2^-14)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def first_diff(got, ref, names):
    """'' if equal, else the first differing index of two equal-shaped tensors, named."""
    ne = (got != ref).nonzero()
    if ne.numel() == 0:
        return ""
    i = ne[0].tolist()
    where = ", ".join(f"{n} {v}" for n, v in zip(names, i))
    return f"{ne.shape[0]} of {got.numel()} elements differ; first at ({where}): got {got[tuple(i)].item()!r}, reference {ref[tuple(i)].item()!r}"


def grid_xy(B, h, w):
    """The pixel grid [B, 2, h, w] float64: channel 0 = x (column), 1 = y (row)."""
    ys = torch.arange(h, dtype=F64)[:, None].expand(h, w)
    xs = torch.arange(w, dtype=F64)[None, :].expand(h, w)
    return torch.stack([xs, ys], 0)[None].repeat(B, 1, 1, 1)


def _bilinear(flat, base, hl, wl, X, Y, clamp=False):
    """Bilinear samples at (X, Y) (float64, any common shape) of the hl x wl images stored row-major at flat[base + y*wl + x] (base an int64
    tensor that broadcasts against X): the four neighbours of (floor X, floor Y), each ZERO outside [0, wl) x [0, hl).  clamp=True (a
    mutation) reads the nearest border pixel instead.  Indices past the end of `flat` (only a mutated level size produces them) read 0."""
    x0, y0 = torch.floor(X), torch.floor(Y)
    ax, ay = X - x0, Y - y0
    x0, y0 = x0.long(), y0.long()
    zero = torch.zeros((), dtype=flat.dtype)

    def at(yy, xx):
        yc, xc = yy.clamp(0, hl - 1), xx.clamp(0, wl - 1)
        idx = base + yc * wl + xc
        v = torch.where(idx < flat.numel(), flat[idx.clamp(max=flat.numel() - 1)], zero)
        if clamp:
            return v
        ok = (yy >= 0) & (yy < hl) & (xx >= 0) & (xx < wl)
        return torch.where(ok, v, zero)
    return (1 - ay) * ((1 - ax) * at(y0, x0) + ax * at(y0, x0 + 1)) + ay * ((1 - ax) * at(y0 + 1, x0) + ax * at(y0 + 1, x0 + 1))


# ---------------------------------------------------------------------------------------------------------------- csrc/raft.hip
def im2col_ref(x, x2, geom, kh, kw, stride, pad, mutate=None):
    """x [N*IH*IW, C1] (+ x2 [N*IH*IW, C - C1], the channels after x's) -> [N*OH*OW, kh*kw*C], column (ky*kw + kx)*C + c =
    input[n][oh*stride + ky - pad_h][ow*stride + kx - pad_w][c], zeros outside the image.  mutate="x2_for_x": the sources swapped."""
    N, IH, IW = geom
    src = [x] if x2 is None else ([x2, x] if mutate == "x2_for_x" else [x, x2])
    img = torch.cat([s.to(F64) for s in src], 1)
    C = img.shape[1]
    img = img.reshape(N, IH, IW, C)
    OH, OW = (IH + 2 * pad[0] - kh) // stride + 1, (IW + 2 * pad[1] - kw) // stride + 1
    out = torch.zeros((N, OH, OW, kh * kw, C), dtype=F64)
    for oh in range(OH):
        for ky in range(kh):
            ih = oh * stride + ky - pad[0]
            if not 0 <= ih < IH:
                continue
            for kx in range(kw):
                ows = [ow for ow in range(OW) if 0 <= ow * stride + kx - pad[1] < IW]
                if ows:
                    iws = [ow * stride + kx - pad[1] for ow in ows]
                    out[:, oh, ows, ky * kw + kx] = img[:, ih, iws]
    return out.reshape(N * OH * OW, kh * kw * C), (N, OH, OW)


def instance_norm_ref(x, N, HW, relu=False, eps=1e-5):
    """x [N*HW, C]: per image and channel (x - mean) / sqrt(var + eps) over the HW rows, biased variance; then ReLU."""
    v = x.to(F64).reshape(N, HW, -1)
    mean = v.sum(1, keepdim=True) / HW
    var = ((v - mean) ** 2).sum(1, keepdim=True) / HW
    y = (v - mean) / torch.sqrt(var + eps)
    if relu:
        y = torch.where(y > 0, y, torch.zeros((), dtype=F64))
    return y.reshape(N * HW, -1)


def ew_ref(op, a, b=None, c=None):
    a = a.to(F64)
    b = None if b is None else b.to(F64)
    c = None if c is None else c.to(F64)
    zero = torch.zeros((), dtype=F64)
    if op == "relu":
        return torch.where(a > 0, a, zero)
    if op == "add_relu":
        return torch.where(a + b > 0, a + b, zero)
    if op == "tanh":
        return torch.tanh(a)
    if op == "gru_rh":
        return b * a
    if op == "gru_out":
        return (1 - c) * b + c * a
    raise ValueError(op)


def level_size(n, l, mutate=None):
    return -((-n) >> l) if mutate == "ceil_levels" else n >> l


def avgpool_ref(x, mutate=None):
    """[n, h, w] -> [n, h // 2, w // 2]: the mean of each 2x2 block; the last row / column of an odd size is dropped.
    mutate="ceil_levels": [n, ceil(h/2), ceil(w/2)], the missing row / column read as zero."""
    n, h, w = x.shape
    x = x.to(F64)
    if mutate == "ceil_levels":
        p = torch.zeros((n, h + (h & 1), w + (w & 1)), dtype=F64)
        p[:, :h, :w] = x
        x, h, w = p, p.shape[1], p.shape[2]
    oh, ow = h // 2, w // 2
    return 0.25 * (x[:, 0:2 * oh:2, 0:2 * ow:2] + x[:, 0:2 * oh:2, 1:2 * ow:2] + x[:, 1:2 * oh:2, 0:2 * ow:2] + x[:, 1:2 * oh:2, 1:2 * ow:2])


def corr_lookup_ref(pyramid, coords, radius, ldo, mutate=None, dtype=F64):
    """pyramid[l] [B*h*w, h >> l, w >> l], coords [B, 2, h, w] -> [B*h*w, ldo]: channel l*side^2 + i*side + j is the bilinear sample, zero
    outside, of the pixel's level-l image at (x / 2^l + i - radius, y / 2^l + j - radius); columns from levels*side^2 on are zero.
    mutate: "swap_xy" (i goes to y, j to x), "ceil_levels" (level l taken as ceil(h / 2^l) x ceil(w / 2^l)), "clamp".
    dtype=torch.float32 runs the same arithmetic in fp32 (the CPU file uses it to show that the exact cases round nowhere)."""
    B, _, h, w = coords.shape
    npix, side = B * h * w, 2 * radius + 1
    assert ldo >= len(pyramid) * side * side
    cx = coords[:, 0].reshape(npix, 1, 1).to(dtype)
    cy = coords[:, 1].reshape(npix, 1, 1).to(dtype)
    d = torch.arange(side, dtype=dtype) - radius
    di, dj = d.reshape(1, side, 1), d.reshape(1, 1, side)
    if mutate == "swap_xy":
        di, dj = dj, di
    out = torch.zeros((npix, ldo), dtype=dtype)
    pix = torch.arange(npix).reshape(npix, 1, 1)
    for l, lv in enumerate(pyramid):
        assert tuple(lv.shape) == (npix, h >> l, w >> l)
        hl, wl = level_size(h, l, mutate), level_size(w, l, mutate)
        X = (cx / 2 ** l + di).expand(npix, side, side)
        Y = (cy / 2 ** l + dj).expand(npix, side, side)
        v = _bilinear(lv.to(dtype).reshape(-1), pix * (hl * wl), hl, wl, X, Y, clamp=mutate == "clamp")
        out[:, l * side * side:(l + 1) * side * side] = v.reshape(npix, side * side)
    return out


def flow_rows_ref(coords1, delta, ncols):
    """coords1 [B, 2, h, w] += (delta[pix][0], delta[pix][1]) (delta [B*h*w, >= 2] or None); rows [B*h*w, ncols]: columns 0 / 1 = the new
    coords1 - pixel grid, the rest zero.  Returns (coords1, rows)."""
    B, _, h, w = coords1.shape
    c = coords1.to(F64).clone()
    if delta is not None:
        c = c + delta.to(F64)[:, :2].reshape(B, h, w, 2).permute(0, 3, 1, 2)
    rows = torch.zeros((B * h * w, ncols), dtype=F64)
    rows[:, :2] = (c - grid_xy(B, h, w)).permute(0, 2, 3, 1).reshape(B * h * w, 2)
    return c, rows


def convex_upsample_ref(coords1, mask, mutate=None):
    """coords1 [B, 2, h, w], mask [B*h*w, 576] (logit k*64 + i*8 + j) -> [B, 2, 8h, 8w]: out[b][c][8y + i][8x + j] =
    sum_k softmax_k(mask)[k, i, j] * 8 * flow[b][c][y + k // 3 - 1][x + k % 3 - 1], flow = coords1 - pixel grid, zero outside the grid.
    mutate: "k_transposed" (neighbour k read as kx*3 + ky), "clamp"."""
    B, _, h, w = coords1.shape
    flow = 8 * (coords1.to(F64) - grid_xy(B, h, w))
    m = mask.to(F64).reshape(B, h, w, 9, 8, 8)
    m = m - m.max(3, keepdim=True).values
    e = torch.exp(m)
    p = e / e.sum(3, keepdim=True)
    out = torch.zeros((B, 2, h, 8, w, 8), dtype=F64)
    ys, xs = torch.arange(h), torch.arange(w)
    for k in range(9):
        dy, dx = (k % 3 - 1, k // 3 - 1) if mutate == "k_transposed" else (k // 3 - 1, k % 3 - 1)
        yy, xx = ys + dy, xs + dx
        nb = flow[:, :, yy.clamp(0, h - 1)][:, :, :, xx.clamp(0, w - 1)]                   # [B, 2, h, w]
        if mutate != "clamp":
            ok = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
            nb = torch.where(ok, nb, torch.zeros((), dtype=F64))
        out += p[:, :, :, k].permute(0, 1, 3, 2, 4)[:, None] * nb[:, :, :, None, :, None]  # p: [B, h, 8, w, 8]
    return out.reshape(B, 2, 8 * h, 8 * w)


# ---------------------------------------------------------------------------------------------------------------- csrc/elementwise.hip
def warp_coords_ref(flow):
    """Sample positions [N, H, W] x 2 of warp_image: the pixel grid + flow, through the reference's normalisation to [-1, 1]
    (2 (g / (W - 1) - 0.5)) and the sampler's way back (((n + 1) / 2) (W - 1)), in float64."""
    N, _, H, W = flow.shape
    g = grid_xy(N, H, W) + flow.to(F64)
    xn, yn = 2 * (g[:, 0] / (W - 1) - 0.5), 2 * (g[:, 1] / (H - 1) - 0.5)
    return ((xn + 1) / 2) * (W - 1), ((yn + 1) / 2) * (H - 1)


def warp_ref(img, flow, mutate=None):
    """img [N, C, H, W], flow [N, 2, H, W] -> out[n][c][y][x] = the bilinear sample of img[n][c] at (x + u, y + v), zero padding.
    mutate="clamp": border padding."""
    N, C, H, W = img.shape
    ix, iy = warp_coords_ref(flow)
    base = (torch.arange(N * C) * (H * W)).reshape(N, C, 1, 1)
    return _bilinear(img.to(F64).reshape(-1), base, H, W, ix[:, None].expand(N, C, H, W), iy[:, None].expand(N, C, H, W), clamp=mutate == "clamp")


def resize_flow_ref(flow, size):
    """flow [N, 2, h, w] -> [N, 2, H, W]: u scaled by W / w, v by H / h, then bilinear with half-pixel centres (align_corners=False): source
    position (X + 0.5) w / W - 0.5 clamped at 0, the second neighbour clamped at the last pixel."""
    N, _, h, w = flow.shape
    H, W = size
    f = flow.to(F64).clone()
    f[:, 0] *= W / w
    f[:, 1] *= H / h
    sx = ((torch.arange(W, dtype=F64) + 0.5) * w / W - 0.5).clamp_min(0)
    sy = ((torch.arange(H, dtype=F64) + 0.5) * h / H - 0.5).clamp_min(0)
    x0, y0 = torch.floor(sx).long(), torch.floor(sy).long()
    x1, y1 = (x0 + 1).clamp(max=w - 1), (y0 + 1).clamp(max=h - 1)
    lx, ly = (sx - x0)[None, None, None, :], (sy - y0)[None, None, :, None]
    top = (1 - lx) * f[:, :, y0][:, :, :, x0] + lx * f[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * f[:, :, y1][:, :, :, x0] + lx * f[:, :, y1][:, :, :, x1]
    return (1 - ly) * top + ly * bot


def flow_correction_ref(eps, lat, ref, flows, sa, sb):
    """eps, lat [F, 4, h, w], ref [R, 4, h, w], flows [F - R, R, 2, h, w]: delta_r = (lat[r] - sa ref[r]) / sb - eps[r]; for query q the
    warped deltas and the warped all-ones coverage are summed over r; out[q] = sum / msum where msum > 0.5, else 0.
    Returns (out [F - R, 4, h, w], msum [F - R, h, w]), float64."""
    R = ref.shape[0]
    delta = (lat.to(F64)[:R] - sa * ref.to(F64)) / sb - eps.to(F64)[:R]
    outs, msums = [], []
    for q in range(flows.shape[0]):
        wd = warp_ref(delta, flows[q]).sum(0)
        ms = warp_ref(torch.ones_like(delta[:, :1]), flows[q]).sum(0)[0]
        outs.append(torch.where(ms > 0.5, wd / ms.clamp_min(1e-30), torch.zeros((), dtype=F64)))
        msums.append(ms)
    return torch.stack(outs), torch.stack(msums)


# ---------------------------------------------------------------------------------------------------------------- exact cases
@functools.lru_cache(maxsize=None)
def im2col_case(N, IH, IW, C, C1):
    """fp16 inputs of a pure copy: x [N*IH*IW, C1 or C], x2 [.., C - C1] or None; no two channels alike."""
    g = _gen(N, IH, IW, C, C1, 1)
    v = (torch.randint(-2047, 2048, (N * IH * IW, C), generator=g).to(F64) / 256)
    v[v == 0] = 1 / 512        # a zero could pass for padding
    if C1:
        return v[:, :C1].contiguous(), v[:, C1:].contiguous()
    return v, None


@functools.lru_cache(maxsize=None)
def avgpool_case(n, h, w):
    """Multiples of 2^-4 with |x| <= 8: a 2x2 sum is a multiple of 2^-4 below 32, its quarter a multiple of 2^-6: exact in fp32."""
    return torch.randint(-128, 129, (n, h, w), generator=_gen(n, h, w, 2)).to(F64) / 16


@functools.lru_cache(maxsize=None)
def corr_case(B, h, w, levels):
    """Inputs on which insv2v_corr_lookup is exact.  Pyramid values are integers in [-8, 8], independent per level (no level can stand in
    for another).  Coordinates are k / 8: at level l <= 3 the sample position is a multiple of 2^-6, so the weights are multiples of 2^-6,
    (1 - ax) a + ax b is a multiple of 2^-6 below 8 and the result a multiple of 2^-12 below 8 - 15 bits, exact in fp32 in any order, so
    the kernel's output is the fp16 rounding of the exact value.  The first pixels of every batch entry are the named edge cases
    (CORR_SPECIALS); the rest are spread over [-2, w + 1] x [-2, h + 1].  Returns (pyramid list of [B*h*w, h >> l, w >> l], coords)."""
    g = _gen(B, h, w, levels, 3)
    npix = B * h * w
    pyr = []
    for l in range(levels):
        v = torch.randint(-8, 9, (npix, h >> l, w >> l), generator=g).to(F64)
        v[v == 0] = 3.0        # a zero could pass for padding
        pyr.append(v)
    cx = torch.randint(-16, 8 * (w + 1) + 1, (B, h, w), generator=g).to(F64) / 8
    cy = torch.randint(-16, 8 * (h + 1) + 1, (B, h, w), generator=g).to(F64) / 8
    coords = torch.stack([cx, cy], 1)
    for b in range(B):
        flat = coords[b].reshape(2, h * w)
        for n, (x, y) in enumerate(corr_specials(h, w)):
            flat[0, n], flat[1, n] = x, y
    return pyr, coords


def corr_specials(h, w):
    """(x, y) of the named cases: on integers (inside, the corners, the last row / column of level 0, which an odd size drops at level 1);
    in (-1, 0) and (w - 1, w) / (h - 1, h): partly inside at every level once the radius is added; +-10^4 away."""
    return [(5.0, 3.0), (0.0, 0.0), (w - 1.0, h - 1.0), (w - 1.0, 0.0), (0.0, h - 1.0),
            (-0.375, 2.0), (2.0, -0.625), (-0.125, -0.875), (w - 0.5, 4.0), (4.0, h - 0.25), (w - 0.875, h - 0.125),
            (FAR + 0.125, 3.0), (3.0, -FAR - 0.5), (-FAR, FAR), (2 * ((w - 1) // 2) + 0.5, 2 * ((h - 1) // 2) + 0.5)]


@functools.lru_cache(maxsize=None)
def flow_rows_case(B, h, w, ldd):
    """coords1 and delta multiples of 2^-6, |coords1| < 64 + 2^-6 * 2^12, |delta| <= 8: the sum and the difference to the pixel grid are
    exact in fp32 (at most 13 bits); the fp16 flow is its one rounding."""
    g = _gen(B, h, w, ldd, 4)
    coords = grid_xy(B, h, w) + torch.randint(-2048, 2049, (B, 2, h, w), generator=g).to(F64) / 64
    delta = torch.randint(-512, 513, (B * h * w, ldd), generator=g).to(F64) / 64
    return coords, delta


@functools.lru_cache(maxsize=None)
def upsample_case(B, h, w):
    """Inputs on which insv2v_convex_upsample is exact: flows are non-zero multiples of 1/8 with |flow| <= 16; for sub-pixel s = i*8 + j of
    pixel (y, x) logit k = (s + x + 2 y) % 9 is 0 and the other eight are -60000 (an fp16 number: 1875 * 32): exp(-60000) underflows to
    0 in fp32 and in float64, the softmax is exactly one-hot and the output 8 * that neighbour's flow, or 0 outside the grid.  Every pixel -
    every border and corner pixel too - selects each of the 9 neighbours in at least 7 of its 64 sub-pixels.
    Returns (coords1 [B, 2, h, w], mask [B*h*w, 576], selected k [B, h, w, 64])."""
    g = _gen(B, h, w, 5)
    f = torch.randint(1, 129, (B, 2, h, w), generator=g).to(F64) / 8 * (torch.randint(0, 2, (B, 2, h, w), generator=g) * 2 - 1).to(F64)
    coords = grid_xy(B, h, w) + f
    s = torch.arange(64).reshape(1, 1, 1, 64)
    sel = (s + torch.arange(w).reshape(1, 1, w, 1) + 2 * torch.arange(h).reshape(1, h, 1, 1)) % 9
    sel = sel.expand(B, h, w, 64)
    mask = torch.full((B, h, w, 9, 64), -60000.0, dtype=F64)
    mask.scatter_(3, sel[:, :, :, None, :], 0.0)
    return coords, mask.reshape(B * h * w, 576), sel


# ---------------------------------------------------------------------------------------------------------------- other inputs
@functools.lru_cache(maxsize=None)
def instance_norm_case(N, HW, C):
    """fp16 rows [N*HW, C]: per-channel means up to +-30, standard deviation 0.5; channel 3 constant within each image (output exactly 0);
    row 0 of each image 8 standard deviations off (the kernel shifts by row 0)."""
    g = _gen(N, HW, C, 6)
    mean = torch.rand((N, 1, C), generator=g, dtype=F64) * 60 - 30
    x = mean + 0.5 * torch.randn((N, HW, C), generator=g, dtype=F64)
    x[:, 0] = mean[:, 0] + 4.0
    x[:, :, 3] = mean[:, :, 3]
    return x.reshape(N * HW, C).half().to(F64)


def warp_specials(H, W):
    """(y, x, u, v) for the first pixels: the sample lands on column 0, on column W - 1, on row 0, on row H - 1, half a pixel outside
    (left, right, top / left corner), and far outside."""
    y, x = H // 2, W // 2
    return [(y, x, -float(x), 0.25), (y, x - 1, W - 1.0 - (x - 1), -0.25), (y - 1, x, 0.5, -float(y - 1)), (y - 1, x - 1, -0.5, H - 1.0 - (y - 1)),
            (0, 0, -0.5, 0.0), (0, W - 1, 0.5, 0.0), (H - 1, 0, -0.5, 0.5), (H - 1, W - 1, FAR, -FAR)]


@functools.lru_cache(maxsize=None)
def warp_case(N, C, H, W):
    """img [N, C, H, W], flow [N, 2, H, W], both fp32 numbers; flow ~ 3 px with warp_specials() at their pixels in every image (an image
    of fewer than 16 pixels: the first four in the even images, the last four in the odd ones)."""
    g = _gen(N, C, H, W, 7)
    img = torch.randn((N, C, H, W), generator=g).to(F64)
    flow = (3 * torch.randn((N, 2, H, W), generator=g)).to(F64)
    for k, (y, x, u, v) in enumerate(warp_specials(H, W)):
        n0, step = (0, 1) if H * W >= 16 else (k // 4, 2)
        flow[n0::step, 0, y, x], flow[n0::step, 1, y, x] = u, v
    return img, flow


@functools.lru_cache(maxsize=None)
def resize_case(N, h, w):
    return (8 * torch.randn((N, 2, h, w), generator=_gen(N, h, w, 8))).to(F64)


SQRT_A, SQRT_1MA = 0.8125, 0.5625      # fp32 numbers
CORRECTION_SETS = [(45, 80, 3, 1), (17, 23, 1, 2), (17, 23, 3, 2), (5, 7, 3, 2), (5, 7, 1, 2), (2, 2, 1, 1), (2, 2, 3, 2)]   # (h, w, R, Q)


@functools.lru_cache(maxsize=None)
def correction_case(h, w, R, Q):
    """eps, lat [R + Q, 4, h, w], ref [R, 4, h, w], flows [Q, R, 2, h, w] ~ 3 px, fp32 numbers.  In every query frame pixel 0 has every
    reference frame out of view (msum = 0: fully masked), pixel 1 has zero flows (msum = R: fully covered), pixel 2 samples reference 0 on
    the border line x = 0, pixel 3 samples reference 0 half a pixel outside in x and in y (its coverage 0.25, never 0.5), pixel 4 samples
    reference 0 at the corner (w - 1, h - 1): on the last column and the last row (2x2 has no pixel 4: there the zero flows of pixel 1 land on
    column w - 1 and the sample of pixel 2 on row h - 1)."""
    g = _gen(h, w, R, Q, 9)
    F = R + Q
    eps, lat = torch.randn((F, 4, h, w), generator=g).to(F64), torch.randn((F, 4, h, w), generator=g).to(F64)
    ref = torch.randn((R, 4, h, w), generator=g).to(F64)
    flows = (3 * torch.randn((Q, R, 2, h, w), generator=g)).to(F64)
    fl = flows.reshape(Q, R, 2, h * w)
    fl[:, :, 0, 0], fl[:, :, 1, 0] = -FAR, FAR
    fl[:, :, :, 1] = 0.0
    fl[:, 0, 0, 2], fl[:, 0, 1, 2] = -float(2 % w), 0.0
    fl[:, 0, 0, 3], fl[:, 0, 1, 3] = -float(3 % w) - 0.5, -float(3 // w) - 0.5
    if h * w > 4:
        fl[:, 0, 0, 4], fl[:, 0, 1, 4] = w - 1.0 - 4 % w, h - 1.0 - 4 // w
    return eps, lat, ref, flows
