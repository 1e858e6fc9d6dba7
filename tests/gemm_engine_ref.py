"""Case builders and fp64 references for the kernel-level parity tests of the 8-wave ping-pong GEMM engines (csrc/gemm_q8.hip: tile codes
230 / 231, 256 x 256 output tiles; csrc/gemm_r8.hip: tile code 240, 256 x 320 tiles).  Device-agnostic: every builder takes `device`,
draws its operands with a CPU generator (the same numbers everywhere) and returns the fp16 operands, the fp64 reference computed on the
SAME fp16-rounded operands with plain torch (matmul, F.conv2d, F.layer_norm, F.gelu) and the blocks of the output to be judged on their
own (name, index) - a wrong tile must not be averaged away by the global max|ref|.

Every builder asserts the conditions on its own inputs with need_gap: for each feature a case exercises there is a reference computed
WITHOUT it, and that reference differs from the true one by more than 10 x the tolerance of the comparison, so a kernel that skips the
feature cannot pass.  The conditions involve references only; tests/test_gemm_engines_cpu.py asserts them without a GPU.

Tile geometry: BM = 256 for the three codes, BN = 256 for 230 / 231 and 320 for 240; the persistent grid is min(tiles, CUs).
"""
import torch
import torch.nn.functional as F

TILES = (230, 231, 240)
BM = 256
BN = {230: 256, 231: 256, 240: 320}


def rnd(*shape, scale=1.0, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(shape, generator=g) * scale).to(device)


def randint(hi, *shape, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randint(0, hi, shape, generator=g).to(device)


def tol_of(ref, ln=False):
    """The project's tolerances: 2e-3 * max|ref| + 2e-3; 4e-3 for both terms where a LayerNorm is folded in or GEGLU is applied."""
    r = 4e-3 if ln else 2e-3
    return r * ref.abs().max().item() + r


def need_gap(ref, alt, tol, what):
    """A reference computed without the feature under test must be far from the true one (a condition on the INPUTS of the test)."""
    gap = (alt.float() - ref.float()).abs().max().item()
    assert gap > 10 * tol, f"input condition, {what}: that reference differs from the true one by only {gap:.3g} (tolerance {tol:.3g})"


def xcd_remap(bid, nwg):   # csrc/common.h
    if nwg < 16:
        return bid
    q, r, xcd, idx = nwg // 8, nwg % 8, bid % 8, bid // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + idx


def tile_of(v, tiles_m, tiles_n):
    """(row tile, column tile) of the v-th tile of the persistent stream (tile_origin of the engines: XCD remap, then groups of 8 tile rows)."""
    bid = xcd_remap(v, tiles_m * tiles_n)
    per_group = 8 * tiles_n
    gidx = bid // per_group
    first_m = gidx * 8
    gsz, rin = min(8, tiles_m - first_m), bid - gidx * per_group
    tn = rin // gsz
    return first_m + rin - tn * gsz, tn


def row_tile_of(v, tiles_m, tiles_n):
    return tile_of(v, tiles_m, tiles_n)[0]


def cached(fn):
    """Builders are called once per (case, device) and shared by the tests of that case (the engines' tile code varies fastest): the
    last two results are kept, nothing mutates them."""
    memo = {}

    def wrapper(*args):
        key = tuple(str(a) if isinstance(a, torch.device) else a for a in args)
        if key not in memo:
            while len(memo) >= 2:
                memo.pop(next(iter(memo)))
            memo[key] = fn(*args)
        return memo[key]
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


def to_cl(x):  # NCHW -> [N*H*W, C]
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


# ------------------------------------------------------------------------------------------- 1. plain and partial tiles
PLAIN_SHAPES = [(100, 64, 64, False), (258, 328, 192, True), (514, 640, 128, False)]
MASKED_LINEAR_SHAPE = (258, 328, 64, True)   # the LINEAR case of the masked-store test: one K tile, partial row and column tiles, residual


@cached
def plain_case(M, N, K, res, device):
    a, w, b = rnd(M, K, device=device).half(), rnd(N, K, scale=K ** -0.5, device=device).half(), rnd(N, device=device)
    r = rnd(M, N, seed=5, device=device).half() if res else None
    prod = a.double() @ w.double().t()
    ref = prod + b.double() + (r.double() if res else 0)
    need_gap(ref, prod + (r.double() if res else 0), tol_of(ref), "bias omitted")
    if res:
        need_gap(ref, prod + b.double(), tol_of(ref), "residual omitted")
    blocks = [("last row tile", slice((M - 1) // BM * BM, M))] if M > BM else []
    return a, w, b, r, ref, blocks


# ------------------------------------------------------------------------------------------- 2. layout
def swap_rows64(ref):
    """64-row blocks 2 i and 2 i + 1 exchanged (the engines' wm index); a trailing odd block stays."""
    M = ref.shape[0]
    idx = torch.arange(M, device=ref.device)
    pair_end = M // 128 * 128
    idx = torch.where(idx < pair_end, idx ^ 64, idx)
    return ref[idx]


@cached
def layout_case(device):
    """A = identity, asymmetric W: the output IS W^T, every misplaced row / column / lane group shows."""
    M = N = K = 320
    a = torch.eye(M, device=device).half()
    w = (torch.arange(N * K, device=device).reshape(N, K).float() % 97 / 97).half()
    ref = w.double().t().contiguous()
    tol = tol_of(ref)
    need_gap(ref, ref.t(), tol, "rows and columns swapped")
    need_gap(ref, ref.reshape(M, N // 32, 2, 2, 8).flip(3).reshape(M, N), tol, "8-column groups swapped within a 32-column fragment")
    need_gap(ref, ref.reshape(M, N // 32, 2, 16).flip(2).reshape(M, N), tol, "the two 16-column halves of a fragment swapped")
    need_gap(ref, ref.reshape(M, N // 64, 2, 32).flip(2).reshape(M, N), tol, "32-column fragments p and p + 1 swapped")
    need_gap(ref, ref.reshape(M, 2, 160).flip(1).reshape(M, N), tol, "the two 160-column halves swapped (wn)")
    need_gap(ref, swap_rows64(ref), tol, "64-row blocks swapped (wm)")
    return a, w, ref


# ------------------------------------------------------------------------------------------- 3. exact rounding
def round_toward_zero_f16(x32):
    """fp32 -> fp16 by truncation (what v_cvt_pkrtz does)."""
    h = x32.half()
    over = h.float().abs() > x32.abs()            # nearest-even went away from zero: one step back (sign-magnitude bit pattern)
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h)


def round_half_away_f16(x32):
    """fp32 -> fp16, ties away from zero."""
    lo = round_toward_zero_f16(x32)
    up = (lo.view(torch.int16) + 1).view(torch.float16)
    x, l, u = x32.double().abs(), lo.double().abs(), up.double().abs()
    tie = (x - l == u - x) & (l != x)
    return torch.where(tie, up, x32.half()), tie


@cached
def exact_case(res, device):
    """A = identity, so every accumulator holds ONE non-zero product; W = s * (1 + i / 1024), bias = (n % 8) / 8192, residual
    1 + r / 1024: every fp32 sum is exact and carries bits below the fp16 ulp, so the stored value must EQUAL the fp32 value rounded to
    nearest even.  Returns (a, w, bias, residual, the exact fp32 values)."""
    M = K = 256
    N = 320
    a = torch.eye(M, device=device).half()
    i = randint(1024, N, K, seed=1, device=device)
    # s = -1 for a quarter of the elements: with the residual a negative product cancels it, the sum lands in a binade whose ulp is at
    # or below the bias step and is fp16-exact - with half the signs negative only 0.32 of the elements would tell the two roundings apart
    s = 1.0 - 2.0 * (randint(4, N, K, seed=2, device=device) == 0).float()
    w = (s * (1.0 + i.float() / 1024.0)).half()
    assert torch.equal(w.double(), s.double() * (1.0 + i.double() / 1024.0))                 # fp16-exact
    b = (torch.arange(N, device=device) % 8).float() / 8192.0
    r = (1.0 + randint(1024, M, N, seed=3, device=device).float() / 1024.0).half() if res else None
    ref64 = w.double().t() + b.double() + (r.double() if res else 0)
    ref32 = w.float().t() + b
    if res:
        ref32 = ref32 + r.float()
    assert torch.equal(ref32.double(), ref64), "the fp32 sums of the exact-rounding case are not exact"
    rne, rtz = ref32.half(), round_toward_zero_f16(ref32)
    share = (rne != rtz).float().mean().item()
    assert share > 1 / 3, f"input condition: only {share:.3f} of the elements tell nearest-even from toward-zero"
    rha, tie = round_half_away_f16(ref32)
    assert int((rha != rne).sum()) > 0, "input condition: no exact tie whose nearest-even result differs from round-half-away"
    return a, w, b, r, ref32.contiguous(), share, int((rha != rne).sum())


# ------------------------------------------------------------------------------------------- 5. the stream crosses tile boundaries
@cached
def stream_case(tile, K, cus, device):
    """One column tile, CUs + 3 row tiles (the last of 8 rows): every workgroup of the first three takes a second tile.  K = 64 is ONE K
    tile (the prologue's second stage already belongs to the workgroup's next tile, the ring parity flips every tile), 192 and 320 are
    odd counts."""
    N = BN[tile]
    M = BM * (cus + 2) + 8
    a, w, b = rnd(M, K, device=device).half(), rnd(N, K, scale=K ** -0.5, device=device).half(), rnd(N, device=device)
    ref = a.double() @ w.double().t() + b.double()
    tiles_m = (M + BM - 1) // BM
    grid = min(tiles_m, cus)
    assert tiles_m == cus + 3 and grid == cus
    blocks = [("last row tile", slice((tiles_m - 1) * BM, M))]
    for v in range(grid, tiles_m):               # second pass over the grid: ring parity and park buffer carry over from tile v - grid
        t2, t1 = row_tile_of(v, tiles_m, 1), row_tile_of(v - grid, tiles_m, 1)
        n2 = min(M, (t2 + 1) * BM) - t2 * BM
        rows2, rows1 = slice(t2 * BM, t2 * BM + n2), slice(t1 * BM, t1 * BM + n2)
        blocks.append((f"tile {v} of the stream (row tile {t2})", rows2))
        need_gap(ref[rows2], a[rows1].double() @ w.double().t() + b.double(), tol_of(ref[rows2]), f"rows of A of the workgroup's previous tile ({t1} for {t2})")
    return a, w, b, ref, blocks, tiles_m


# ------------------------------------------------------------------------------------------- 6. folded LayerNorm, row bias, two-source K
def layernorm_terms(a):
    x = a.double()
    return x, x.mean(1, keepdim=True), (x.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()


def layernorm_case(a, N, seed=0):
    """Folded LayerNorm (no affine: col_sum = row sums of w) on the rows `a` (non-zero means)."""
    M, K = a.shape
    device = a.device
    w, b = rnd(N, K, scale=K ** -0.5, seed=seed, device=device).half(), rnd(N, seed=seed, device=device)
    col = w.float().sum(1).contiguous()
    x, mean, rstd = layernorm_terms(a)
    ref = F.layer_norm(x, (K,)) @ w.double().t() + b.double()
    need_gap(ref, ref + rstd * mean * col.double(), tol_of(ref, True), "-mean * col_sum dropped")
    need_gap(ref, x @ w.double().t() + b.double(), tol_of(ref, True), "LayerNorm not applied")
    return w, b, col, ref


LN_SHAPE = (590, 960, 320)


def layernorm_rows(M, K, device):
    return (rnd(M, K, device=device) * 1.2 + 0.3).half()


def producer_operands(M, K, device):
    """The GEMM whose output rows (and their emitted statistics) feed the folded LayerNorm in the 'producer' form."""
    return rnd(M, 64, seed=21, device=device).half(), rnd(K, 64, scale=64 ** -0.5, seed=22, device=device).half(), rnd(K, seed=23, device=device) * 0.2 + 0.3


@cached
def row_bias_case(kind, ln, device):
    N, K = 320, 64
    if kind == "frame":      # per-frame table, groups wrap: row m takes table[(m // 256) % 5]
        rpg, rb_mod, ngroups, M = 256, 5, 5, 4096
    elif kind == "sample":   # per-sample table: row m takes table[m // 512]
        rpg, rb_mod, ngroups, M = 512, 0, 4, 2048
    else:                    # "odd": 117 rows per group - a 256-row tile would span groups, the engines refuse, the dispatch does not
        rpg, rb_mod, ngroups, M = 117, 0, 5, 585
    a = layernorm_rows(M, K, device)
    table = rnd(ngroups, N, seed=9, device=device) * 0.5
    if ln:
        w, b, col, ref = layernorm_case(a, N)
    else:
        w, b, col = rnd(N, K, scale=K ** -0.5, device=device).half(), rnd(N, device=device), None
        ref = a.double() @ w.double().t() + b.double()
    g = (torch.arange(M, device=device) // rpg) % ngroups
    full = ref + table.double()[g]
    need_gap(full, ref + table.double()[(g + 1) % ngroups], tol_of(full, ln), "row bias of the neighbouring group")
    need_gap(full, ref, tol_of(full, ln), "row bias omitted")
    if ln:
        _, mean, rstd = layernorm_terms(a)
        need_gap(full, full + rstd * mean * col.double(), tol_of(full, True), "-mean * col_sum dropped")
    blocks = [(f"rows of group {i}", g == i) for i in range(ngroups)]
    return a, w, b, col, table, rpg, rb_mod, full, blocks


TWO_SOURCE_SHAPE = (520, 320, 960)


@cached
def two_source_case(split, device):
    M, N, K = TWO_SOURCE_SHAPE
    a, w, b = rnd(M, K, device=device).half(), rnd(N, K, scale=K ** -0.5, device=device).half(), rnd(N, device=device)
    ref = a.double() @ w.double().t() + b.double()
    need_gap(ref, a[:, :split].double() @ w[:, :split].double().t() + b.double(), tol_of(ref), "second K source zeroed")
    need_gap(ref, a[:, split:].double() @ w[:, split:].double().t() + b.double(), tol_of(ref), "first K source zeroed")
    return a, w, b, ref, [("last row tile", slice(M // BM * BM, M))]


# ------------------------------------------------------------------------------------------- 7. GEGLU and output statistics
GEGLU_SHAPES = [(300, 64, 160), (600, 64, 480)]


@cached
def geglu_case(M, C, NH, device):
    """GEGLU on the [32 value | 32 gate] interleaved projection with the folded LayerNorm in front (tests/test_gemm_w4_gpu.py's case)."""
    from insv2v.unet import fold_layernorm, interleave32
    x = (rnd(M, C, device=device) * 1.3 + 0.2).half()
    w1, b1 = rnd(2 * NH, C, scale=C ** -0.5), rnd(2 * NH, seed=1) * 0.3
    gamma, beta = 1 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    wf, col, bf = (t.to(device) for t in fold_layernorm(w1, gamma, beta, b1))
    xf, mean, rstd = layernorm_terms(x)
    y = F.layer_norm(xf, (C,)) @ wf.double().t() + bf.double()      # == rstd * (x @ wf^T - mean * col) + bf, the operands the kernel gets
    h, g = y.chunk(2, dim=-1)
    ref = h * F.gelu(g)
    need_gap(ref, g * F.gelu(h), tol_of(ref, True), "gate and value halves swapped")
    need_gap(ref, h * F.gelu(h), tol_of(ref, True), "the gate read from the value's accumulator")
    hd, gd = (y + rstd * mean * col.double()).chunk(2, dim=-1)
    need_gap(ref, hd * F.gelu(gd), tol_of(ref, True), "-mean * col_sum dropped")
    args = (x, interleave32(wf).contiguous(), interleave32(bf).contiguous())
    return args, interleave32(col).contiguous(), ref


STATS_SHAPES = [(300, 640, 64, False), (300, 640, 64, True), (258, 320, 128, False)]


def stats_tol(ref):
    return 1e-5 * ref.abs().max().item() + 1e-3


@cached
def stats_case(M, N, K, res, device):
    """Output statistics of gemm_r8: per 160-column part, (sum, sum of squares) of the values BEFORE their fp16 rounding
    (include/insv2v_hip.h).  Returns the operands, the output reference and the [N // 160, M, 2] fp64 sums."""
    a, w, b = (rnd(M, K, device=device) * 1.5 + 0.3).half(), rnd(N, K, scale=K ** -0.5, device=device).half(), rnd(N, device=device) + 0.5
    r = rnd(M, N, seed=3, device=device).half() if res else None
    ref = a.double() @ w.double().t() + b.double() + (r.double() if res else 0)
    parts = ref.reshape(M, N // 160, 160).permute(1, 0, 2)
    sums = torch.stack([parts.sum(2), (parts * parts).sum(2)], 2)
    for p in range(N // 160):
        q = (p + 1) % (N // 160)
        for j, name in enumerate(("sum", "sum of squares")):
            need_gap(sums[p, :, j], sums[q, :, j], stats_tol(sums[p, :, j]), f"{name}: parts {p} and {q} exchanged")
    return a, w, b, r, ref, sums


# ------------------------------------------------------------------------------------------- 8. convolutions at odd grids
# (nb, H, W, stride, upsample): 117 pixels per image - the tile boundaries at rows 256 and 512 fall mid image and mid image row; one image
# row / one image column (top and bottom / left and right taps invalid for every pixel); stride 2 (output 7 x 9); upsample (output 10 x 14)
CONV_GEOMS = [(5, 9, 13, 1, False), (3, 1, 300, 1, False), (3, 300, 1, 1, False), (8, 13, 17, 2, False), (5, 5, 7, 1, True)]
CONV_C1, CONV_COUT = 64, 320


def stream_conv_images(cus):
    """Images of 9 x 13 for CUs + 2 row tiles."""
    nb = (cus + 1) * BM // 117 + 1
    assert (nb * 117 + BM - 1) // BM == cus + 2
    return nb


def conv_ref(x, w, b, stride, ups):
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.conv2d(x, w, b, stride=stride, padding=1)


def conv_ref_tall(x, w, b, stride, ups):
    """The batch convolved as ONE tall image, no padding between the images: the row above an image's first row is the previous image's
    last row, the row below its last row the next image's first.  What a tap-validity mask that ignores the image edge computes."""
    if ups:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    zero = torch.zeros_like(x[:1, :, :1])
    above = torch.cat([zero, x[:-1, :, -1:]], 0)
    below = torch.cat([x[1:, :, :1], zero], 0)
    return F.conv2d(torch.cat([above, x, below], 2), w, b, stride=stride, padding=(0, 1))


def conv_ref_shifted(x, w, b):
    """Stride 2 with the output grid shifted by one input pixel: output (oh, ow) centred on input (2 oh + 1, 2 ow + 1)."""
    return F.conv2d(F.pad(x, (0, 2, 0, 2)), w, b, stride=2, padding=0)


@cached
def conv_case(nb, h, w, stride, ups, c2, device):
    from insv2v.unet import prep_conv3x3
    c1, cout = CONV_C1, CONV_COUT
    x1 = rnd(nb, c1, h, w, device=device).half()
    x2 = rnd(nb, c2, h, w, seed=2, device=device).half() if c2 else None
    xin = (torch.cat([x1, x2], 1) if c2 else x1).double()
    wt = rnd(cout, c1 + c2, 3, 3, scale=(9 * (c1 + c2)) ** -0.5).half()
    b = rnd(cout, seed=4)
    wk, bk = prep_conv3x3({"c.weight": wt.float(), "c.bias": b}, "c", device)
    wt, b = wt.to(device).double(), b.to(device).double()
    conv4 = conv_ref(xin, wt, b, stride, ups)
    oh, ow = conv4.shape[2], conv4.shape[3]
    assert (oh, ow) == ((2 * h, 2 * w) if ups else ((h - 1) // stride + 1, (w - 1) // stride + 1))
    M = nb * oh * ow
    rb = rnd(1, cout, seed=6, device=device) * 0.5           # ONE row-bias group over all rows (117 pixels per image are no multiple of a tile)
    res = rnd(M, cout, seed=7, device=device).half()
    extra = rb.double() + res.double()
    conv = to_cl(conv4)
    ref = conv + extra
    tol = tol_of(ref)
    row = torch.arange(M, device=device) // ow % oh
    edge = (row == 0) | (row == oh - 1)                      # first and last image rows of all images
    need_gap(ref, conv + rb.double(), tol, "residual omitted")
    need_gap(ref, conv + res.double(), tol, "row bias omitted")
    need_gap(ref, to_cl(conv_ref(xin, wt, None, stride, ups)) + extra, tol, "bias omitted")
    # (mirrored left-right; an image one pixel wide only has its centre column of taps: mirrored top-bottom there)
    need_gap(ref, to_cl(conv_ref(xin, wt.flip(3 if w > 1 else 2), b, stride, ups)) + extra, tol, "taps mirrored")
    if c2:
        wz = wt.clone()
        wz[:, c1:] = 0
        need_gap(ref, to_cl(conv_ref(xin, wz, b, stride, ups)) + extra, tol, "second channel source zeroed")
    tall = to_cl(conv_ref_tall(xin, wt, b, stride, ups)) + extra
    assert tall.shape == ref.shape and torch.allclose(tall[~edge], ref[~edge], rtol=0, atol=1e-9)   # interior rows do not see the edge
    need_gap(ref[edge], tall[edge], tol_of(ref[edge]), "the batch convolved as one tall image without padding between images")
    if stride == 2:
        need_gap(ref, to_cl(conv_ref_shifted(xin, wt, b)) + extra, tol, "output grid shifted by one input pixel")
    blocks = [("first and last image rows", edge)]
    if nb <= 8:
        blocks += [(f"image {i}", slice(i * oh * ow, (i + 1) * oh * ow)) for i in range(nb)]
    kw = dict(x2=to_cl(x2) if c2 else None, row_bias=rb, rows_per_group=M, residual=res, stride=stride, upsample=ups)
    return to_cl(x1), wk, bk, kw, (nb, oh, ow), ref, blocks


def stream_conv_blocks(ref, res, nb, cus):
    """The second-pass tiles of the CUs + 2 row tiles of the 9 x 13 stream convolution on one 320-column tile, with their input condition:
    the previous tile's pixels (its convolution under this tile's residual) are far from the true rows."""
    M = ref.shape[0]
    tiles_m = (M + BM - 1) // BM
    grid = min(tiles_m, cus)
    blocks = [("last row tile", slice((tiles_m - 1) * BM, M))]
    for v in range(grid, tiles_m):
        t2, t1 = row_tile_of(v, tiles_m, 1), row_tile_of(v - grid, tiles_m, 1)
        n2 = min(M, (t2 + 1) * BM) - t2 * BM
        rows2, rows1 = slice(t2 * BM, t2 * BM + n2), slice(t1 * BM, t1 * BM + n2)
        blocks.append((f"tile {v} of the stream (row tile {t2})", rows2))
        need_gap(ref[rows2], ref[rows1] - res[rows1].double() + res[rows2].double(), tol_of(ref[rows2]), f"pixels of the workgroup's previous tile ({t1} for {t2})")
    return blocks, tiles_m
