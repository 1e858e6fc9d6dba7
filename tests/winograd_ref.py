"""Float64 restatement of the two Winograd F(2x2, 3x3) transform stages (insv2v_winograd_input / insv2v_winograd_output, csrc/winograd.hip)
for the stage tests (tests/test_winograd_stages_cpu.py, tests/test_winograd_stages_gpu.py), and the inputs of their bit-exact cases.

Written from the algorithm (Lavin & Gray 2016, "Fast Algorithms for Convolutional Neural Networks", F(2x2, 3x3):
Y = A^T [ (G g G^T) . (B^T d B) ] A) and the layout the C header states, with torch on the CPU and no project code:
  * pixels are channels-last rows [NB*H*W, C]; tiles are ordered (image, ty, tx), ceil(H/2) x ceil(W/2) of them per image; a tile's 4x4 patch
    starts one pixel above / left of its 2x2 output pixels; everything outside the image is zero (padding applies AFTER the norm);
  * matrix k = i*4 + j holds (B^T d B)[i][j];
  * upsample form (nearest x2, then the convolution): one tile per INPUT pixel (y, x), the patch is rows 2y-1 .. 2y+2, columns 2x-1 .. 2x+2 of
    the upsampled image; row / column 2 of B^T d B vanish (the patch's two centre rows / columns are equal), the 9 matrices g = ci*3 + cj run
    over patch indices {0, 1, 3}^2.
"""
import functools
import math

import torch

F64 = torch.float64
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=F64)
AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=F64)
UP_IDX = [0, 1, 3]


def tiles_of(NB, H, W, upsample=False):
    return NB * H * W if upsample else NB * ((H + 1) // 2) * ((W + 1) // 2)


def stage_ref(x, NB, H, W, ab=None, ips=1, silu=False):
    """The pixels the input transform works on: x [NB*H*W, C] -> d = x * scale + shift of the image's sample (ab [nsamples, C, 2], sample =
    image // ips), then SiLU, in float64, rounded to fp16 once (the kernel stages fp16).  Returns float64 [NB*H*W, C]."""
    d = x.to(F64)
    assert d.shape[0] == NB * H * W
    if ab is not None:
        sample = torch.arange(NB * H * W) // (ips * H * W)
        t = ab.to(F64)[sample]                       # [pixels, C, 2]
        d = d * t[..., 0] + t[..., 1]
        if silu:
            d = d / (1.0 + torch.exp(-d))
    return d.half().to(F64)


def _patches(d, NB, H, W, upsample):
    """[NB, th, tw, 4, 4, C] zero-padded patches of the staged pixels d [NB*H*W, C]."""
    C = d.shape[1]
    img = d.reshape(NB, H, W, C)
    if upsample:
        img = img.repeat_interleave(2, 1).repeat_interleave(2, 2)
        th, tw = H, W
    else:
        th, tw = (H + 1) // 2, (W + 1) // 2
    pad = torch.zeros((NB, 2 * th + 2, 2 * tw + 2, C), dtype=F64)
    pad[:, 1:1 + img.shape[1], 1:1 + img.shape[2]] = img
    p = torch.empty((NB, th, tw, 4, 4, C), dtype=F64)
    for r in range(4):
        for c in range(4):
            p[:, :, :, r, c] = pad[:, r:r + 2 * th:2, c:c + 2 * tw:2]
    return p


def input_ref(x, NB, H, W, ab=None, ips=1, silu=False, upsample=False):
    """V[k] = (B^T d B)[i][j], k = i*4 + j (upsample: g = ci*3 + cj over {0, 1, 3}^2), d = the staged pixels.  float64 [16 or 9, tiles, C]."""
    d = stage_ref(x, NB, H, W, ab, ips, silu)
    p = _patches(d, NB, H, W, upsample)
    v = torch.einsum("ir,ntxrcC,jc->ijntxC", BT, p, BT)          # [4, 4, NB, th, tw, C]
    if upsample:
        v = v[UP_IDX][:, UP_IDX]
    return v.reshape(v.shape[0] * v.shape[1], -1, d.shape[1]).contiguous()


def weights_ref(w, upsample=False):
    """[Cout, Cin, 3, 3] -> U [16 or 9, Cout, Cin] float64, U[i*4 + j] = (G g G^T)[i][j]."""
    u = torch.einsum("ai,ocij,bj->aboc", G, w.to(F64), G)
    if upsample:
        u = u[UP_IDX][:, UP_IDX]
    return u.reshape(-1, w.shape[0], w.shape[1]).contiguous()


def output_ref(M, NB, H, W, bias=None, row_bias=None, rows_per_group=0, residual=None, upsample=False):
    """M [16 or 9, tiles, Cout] -> y = A^T M A + bias[n] + row_bias[pixel // rows_per_group][n] + residual[pixel][n], float64
    [NB*OH*OW, Cout] (OH, OW = H, W; upsample: 2H, 2W).  An odd H / W: only the pixels that exist."""
    M = M.to(F64)
    Cout = M.shape[2]
    th, tw = (H, W) if upsample else ((H + 1) // 2, (W + 1) // 2)
    OH, OW = (2 * H, 2 * W) if upsample else (H, W)
    assert M.shape[1] == NB * th * tw
    if upsample:
        full = torch.zeros((4, 4, M.shape[1], Cout), dtype=F64)
        for a, i in enumerate(UP_IDX):
            for b, j in enumerate(UP_IDX):
                full[i, j] = M[a * 3 + b]
    else:
        full = M.reshape(4, 4, M.shape[1], Cout)
    full = full.reshape(4, 4, NB, th, tw, Cout)
    y = torch.einsum("ai,ijntxC,bj->ntaxbC", AT, full, AT).reshape(NB, 2 * th, 2 * tw, Cout)[:, :OH, :OW].reshape(NB * OH * OW, Cout)
    if bias is not None:
        y = y + bias.to(F64)
    if row_bias is not None:
        y = y + row_bias.to(F64)[torch.arange(NB * OH * OW) // rows_per_group]
    if residual is not None:
        y = y + residual.to(F64)
    return y


def ulp16(v):
    """The spacing of fp16 numbers at |v| (v a positive float, normal range)."""
    return 2.0 ** (math.floor(math.log2(v)) - 10)


# ---------------------------------------------------------------------------------------------------------------- geometries
# (NB, H, W, images per GroupNorm sample).  The regime of insv2v_winograd_input each one meets (ipb = images per workgroup = 32 // tiles per
# image, clipped by LDS; an image is staged whole up to 512 LDS slots, else in bands of tile rows) is stated behind it; ips is chosen so that
# a sample boundary falls inside one workgroup's images wherever a workgroup has several.
DIRECT = [(7, 4, 6, 2),      # ipb 5, tail of 2
          (3, 2, 2, 2),      # ipb 32, 3 images
          (5, 1, 1, 2),      # one pixel per image
          (3, 1, 7, 2),      # one row
          (3, 7, 1, 2),      # one column
          (3, 5, 7, 1),      # ipb 2, tail, odd slot count
          (2, 16, 32, 1),    # whole image at the 512-slot limit
          (2, 19, 27, 1),    # banded, odd H and W, 2 bands
          (1, 13, 80, 1),    # 4 bands, the last one partial
          (1, 8, 103, 1),    # one tile row per band
          (1, 9, 128, 1)]    # one tile row per band, 64 KiB of LDS
UPSAMPLE = [(7, 2, 3, 2),    # ipb 5, tail
            (3, 1, 1, 2),
            (2, 1, 5, 1),    # ipb 6, both images in one workgroup
            (3, 3, 5, 1),    # ipb 2, tail
            (2, 16, 32, 1),  # whole image at the limit
            (1, 19, 27, 1),  # 2 bands
            (1, 5, 128, 1)]  # 3 bands, 64 KiB of LDS
GEOMS = [(g, False) for g in DIRECT] + [(g, True) for g in UPSAMPLE]
C_IN, C1_IN = 128, 64


def geom_id(p):
    (NB, H, W, ips), up = p
    return f"{'up' if up else 'direct'}-{NB}x{H}x{W}"


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


SCALES = torch.tensor([0.5, 1.0, 1.5, 2.0], dtype=F64)
SHIFTS = torch.tensor([-1.0, -0.75, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0], dtype=F64)


def exact_table(nsamples, C, g):
    """(scale, shift) [nsamples, C, 2]: scales in {0.5, 1, 1.5, 2}, shifts non-zero multiples of 0.25 in [-1, 1]; neighbouring samples differ
    in both, in every channel."""
    s = torch.arange(nsamples)[:, None]
    si = (torch.randint(0, 4, (1, C), generator=g) + s) % 4
    hi = (torch.randint(0, 8, (1, C), generator=g) + 3 * s) % 8
    return torch.stack([SCALES[si], SHIFTS[hi]], -1)


@functools.lru_cache(maxsize=None)
def exact_input_case(NB, H, W, ips, upsample, norm):
    """Inputs on which insv2v_winograd_input is exact.  No norm: x = k * 2^-6, |k| <= 256 - a V element is a signed sum of 4 pixels (upsample:
    up to 2 * 2 * d): |V| <= 16 in steps of 2^-6.  Norm (no SiLU): x = k * 2^-4, |x| <= 2, with exact_table(): staged pixels are multiples
    of 2^-5 with |d| <= 5, |V| <= 20.  Returns (x float64 [pixels, C_IN], ab float64 or None)."""
    g = _gen(NB, H, W, ips, upsample, norm)
    n = NB * H * W
    if norm:
        x = torch.randint(-32, 33, (n, C_IN), generator=g).to(F64) / 16
        ab = exact_table(-(-NB // ips), C_IN, g)
    else:
        x = torch.randint(-256, 257, (n, C_IN), generator=g).to(F64) / 64
        ab = None
    return x, ab


@functools.lru_cache(maxsize=None)
def exact_output_case(NB, H, W, ips, upsample, Cout):
    """Inputs on which insv2v_winograd_output is exact: M, bias, row bias and residual multiples of 2^-3 in [-4, 4] - |y| <= 9 * 4 + 12 = 48
    in steps of 2^-3.  Neighbouring row-bias groups differ in every channel.  Returns (M [16 or 9, tiles, Cout], bias, row_bias
    [groups, Cout], rows_per_group, residual [NB*OH*OW, Cout]), float64."""
    g = _gen(NB, H, W, ips, upsample, Cout, 77)
    ng, tiles = (9 if upsample else 16), tiles_of(NB, H, W, upsample)
    pixels = NB * H * W * (4 if upsample else 1)
    rpg = ips * H * W * (4 if upsample else 1)
    groups = -(-pixels // rpg)

    def eighths(*shape):
        return torch.randint(-32, 33, shape, generator=g).to(F64) / 8
    M, bias, res = eighths(ng, tiles, Cout), eighths(Cout), eighths(pixels, Cout)
    rb = ((torch.randint(0, 65, (1, Cout), generator=g) + 7 * torch.arange(groups)[:, None]) % 65 - 32).to(F64) / 8
    return M, bias, rb, rpg, res


def is_fp16(t):
    return bool(torch.equal(t.half().to(F64), t))


def first_diff(got, ref, names):
    """'' if equal, else the first differing index of two equal-shaped tensors, named."""
    ne = (got != ref).nonzero()
    if ne.numel() == 0:
        return ""
    i = ne[0].tolist()
    where = ", ".join(f"{n} {v}" for n, v in zip(names, i))
    return f"{ne.shape[0]} of {got.numel()} elements differ; first at ({where}): got {got[tuple(i)].item()!r}, reference {ref[tuple(i)].item()!r}"
