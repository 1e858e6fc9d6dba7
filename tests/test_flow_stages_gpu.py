"""Stage-level parity of the optical-flow kernels (csrc/raft.hip: insv2v_im2col, insv2v_instance_norm, insv2v_ew, insv2v_avgpool2x2,
insv2v_corr_lookup, insv2v_raft_flow_rows, insv2v_convex_upsample; csrc/elementwise.hip: insv2v_warp_image, insv2v_resize_flow,
insv2v_flow_correction), each called through the C ABI on its own against the float64 restatement of tests/flow_ref.py - at 1/8 grids
that are odd (17x23: pyramid 17x23 -> 8x11 -> 4x5 -> 2x2; 45x80, the named workload: 45 -> 22 -> 11 -> 5 rows), where the whole-estimator
tests of tests/test_raft_gpu.py would let a swapped offset order, a mis-sized level or a wrong padding rule at a few border pixels pass.

Every operand that has a stride gets one that differs from its width: a column view of a wider buffer, NaN around the inputs, a sentinel
bit pattern around the outputs.  Outputs lie in sentinel buffers with guard rows: what must not be written still holds the sentinel
afterwards, and everything that must be written does not.  Operands without a stride (fp32 planes) lie between guards in one flat buffer.

Bounds.  Exact cases (tests/test_flow_stages_cpu.py shows that the kernels' fp32 arithmetic rounds nowhere on them): bit for bit.
  corr_lookup, random operands: |out - ref| <= ulp16(|ref|) + 1e-6 max|pyramid| elementwise - half a step of final rounding plus fp32 error
    that can move the rounding by one step.
  convex_upsample, random operands: 1e-3 of max|ref|.     instance_norm: 4e-3 of max|ref|, max|ref| over the rows other than row 0 (the
    outlier).     ew: RELU, ADD_RELU, GRU_RH bit for bit on normal-range fp16 inputs (sums and products of two fp16 numbers are exact in
    fp32); GRU_OUT within one fp16 step of |ref| (q and h of one sign, |.| >= 1/8: fp32 error <= 2^-23, far below the half step it is added
    to); TANH 2e-3 of max|ref|.
  warp_image, resize_flow: |out - ref| <= 1e-5 |ref| + 2e-5 elementwise, flow_correction 1e-4 |ref| + 1e-4 elementwise (the worst
    |out - ref| is printed as well); flow_correction is compared where the float64 coverage sum is more than 1e-3 from the 0.5
    threshold (at most 1 % of the pixels are not: tests/test_flow_stages_cpu.py), and is exactly 0 where every reference frame is out of view."""
import math

import pytest
import torch

import flow_ref as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SENT16 = 0x7EAB            # an fp16 NaN bit pattern: no kernel output, no test input
SENT32 = 0x7FC0ABCD        # an fp32 NaN bit pattern
GUARD = 8                  # sentinel rows before and after an output matrix
GUARD32 = 256              # sentinel / NaN elements before and after a flat fp32 operand
EINVAL = -1


def lib():
    from insv2v import _lib
    return _lib.load()


def stream():
    from insv2v import ops
    return ops._stream()


def ok(code, what):
    from insv2v import _lib
    _lib.check(code, what)
    torch.cuda.synchronize()


def sentinel16(rows, cols):
    return torch.full((rows, cols), SENT16, dtype=torch.int16, device=DEV).view(torch.float16)


def is_sent16(t):
    return t.view(torch.int16) == SENT16


def is_sent32(t):
    return t.view(torch.int32) == SENT32


def nan_framed(values, left, right, dtype=torch.float16):
    """`values` [rows, n] as a column view of a NaN-filled [rows, left + n + right] buffer."""
    rows, n = values.shape
    buf = torch.full((rows, left + n + right), float("nan"), dtype=dtype, device=DEV)
    view = buf[:, left:left + n]
    view.copy_(values)
    return view


def out16(rows, cols, left=8, right=16):
    """(whole sentinel buffer, the [rows, cols] view a kernel writes): GUARD rows above and below, `left` / `right` columns beside."""
    buf = sentinel16(GUARD + rows + GUARD, left + cols + right)
    return buf, buf[GUARD:GUARD + rows, left:left + cols]


def check_out16(buf, rows, cols, what, left=8):
    sent = is_sent16(buf)
    assert sent[:GUARD].all() and sent[GUARD + rows:].all(), f"{what}: wrote rows outside its output"
    assert sent[:, :left].all() and sent[:, left + cols:].all(), f"{what}: wrote columns outside its output"
    unwritten = sent[GUARD:GUARD + rows, left:left + cols].cpu()
    assert not unwritten.any(), f"{what}: not written: " + fr.first_diff(unwritten, torch.zeros_like(unwritten), ("row", "column"))


def in32(values):
    """A contiguous fp32 operand between GUARD32 NaNs in one flat buffer."""
    buf = torch.full((GUARD32 + values.numel() + GUARD32,), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[GUARD32:GUARD32 + values.numel()].view(values.shape)
    view.copy_(values)
    return view


def out32(shape):
    n = math.prod(shape)
    buf = torch.full((GUARD32 + n + GUARD32,), SENT32, dtype=torch.int32, device=DEV).view(torch.float32)
    return buf, buf[GUARD32:GUARD32 + n].view(shape)


def check_out32(buf, n, what):
    sent = is_sent32(buf)
    assert sent[:GUARD32].all() and sent[GUARD32 + n:].all(), f"{what}: wrote outside its output"
    assert not sent[GUARD32:GUARD32 + n].any(), f"{what}: {int(sent[GUARD32:GUARD32 + n].sum())} elements not written"


def assert_bit_equal(got, ref64, names, what, dtype=torch.float16):
    got, ref = got.cpu(), ref64.to(dtype)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(got, ref), f"{what}: " + fr.first_diff(got, ref, names)


def report_elementwise(what, err, ref, rel, abs_, extra=""):
    """|out - ref| <= rel |ref| + abs_ for every element (err = |out - ref|, already zeroed where it is not compared)."""
    excess = (err - rel * ref.abs() - abs_).max().item()
    print(f"[parity] {what}: worst |out - ref| {err.max().item():.4g} (max|ref| {ref.abs().max().item():.4g}), worst elementwise excess over "
          f"{rel:g} |ref| + {abs_:g}: {excess:.3g} (<= 0 passes){extra}")
    assert math.isfinite(excess) and excess <= 0, f"{what}: an element exceeds {rel:g} |ref| + {abs_:g} by {excess:.4g}"


def report(what, err, bound, extra=""):
    print(f"[parity] {what}: worst {err:.4g} (bound {bound:.4g}){extra}")
    assert math.isfinite(err) and err <= bound, f"{what}: {err:.4g} > {bound:.4g}"


# ---------------------------------------------------------------------------------------------------------------- im2col
CONV_CASES = [g[:4] + (0,) for g in fr.CONV_GEOMS] + [g[:4] + (g[4] or g[0] // 2,) for g in fr.CONV_GEOMS if g[0] >= 16]


@pytest.mark.parametrize("C,kh,kw,stride,C1", CONV_CASES)
def test_im2col_is_a_copy(C, kh, kw, stride, C1):
    """The six convolution geometries of the estimator onto the 17x23 grid (stride 2 from 34x46), from one source and from two
    (8 channels are one chunk: one source only); ldx, ldx2 and ldo larger than the widths."""
    from insv2v import ops, _lib
    N, (IH, IW) = 2, ((34, 46) if stride == 2 else (17, 23))
    x64, x264 = fr.im2col_case(N, IH, IW, C, C1)
    pad = ((kh - 1) // 2, (kw - 1) // 2)
    ref, (_, OH, OW) = fr.im2col_ref(x64, x264, (N, IH, IW), kh, kw, stride, pad)
    x = nan_framed(x64, 8, 16)
    K, rows = kh * kw * C, N * OH * OW
    buf, out = out16(rows, K)
    d = _lib.Im2colDesc()
    d.x, d.out, d.ldx, d.ldo, d.C1 = x.data_ptr(), out.data_ptr(), x.stride(0), out.stride(0), C
    if x264 is not None:
        x2 = nan_framed(x264, 16, 24)
        d.x2, d.ldx2, d.C1 = x2.data_ptr(), x2.stride(0), C1
        assert d.ldx2 == C - C1 + 40
    d.N, d.IH, d.IW, d.C, d.KH, d.KW = N, IH, IW, C, kh, kw
    d.stride_h = d.stride_w = stride
    d.pad_h, d.pad_w, d.OH, d.OW = pad[0], pad[1], OH, OW
    assert d.ldx == x64.shape[1] + 24 and d.ldo == K + 24 and (OH, OW) == (17, 23)
    ok(lib().insv2v_im2col(ops._byref(d), stream()), "insv2v_im2col")
    check_out16(buf, rows, K, "im2col")
    assert_bit_equal(out, ref, ("row", "column"), f"im2col C={C} {kh}x{kw} stride {stride} C1={C1}")


# ---------------------------------------------------------------------------------------------------------------- avgpool2x2
@pytest.mark.parametrize("n,h,w", [(5, 17, 23), (2, 45, 80)])
def test_avgpool_chain_is_exact(n, h, w):
    """(17, 23) -> (8, 11) -> (4, 5) -> (2, 2) and 45x80 -> 22x40 -> 11x20 -> 5x10, each level from the kernel's previous output: the last
    row / column of an odd level is dropped, rows keep the INPUT's length as their stride."""
    x64 = fr.avgpool_case(n, h, w)
    x = in32(x64.float())
    for _ in range(3):
        ref = fr.avgpool_ref(x64)
        buf, y = out32((n, h // 2, w // 2))
        ok(lib().insv2v_avgpool2x2(x.data_ptr(), y.data_ptr(), n, h, w, stream()), "insv2v_avgpool2x2")
        check_out32(buf, y.numel(), f"avgpool2x2 {h}x{w}")
        assert fr.is_fp32(ref)
        assert_bit_equal(y, ref, ("image", "row", "column"), f"avgpool2x2 {h}x{w}", torch.float32)
        x, x64, h, w = y, ref, h // 2, w // 2
    assert (h, w) in ((2, 2), (5, 10))


# ---------------------------------------------------------------------------------------------------------------- corr_lookup
def run_corr_lookup(pyr64, coords64, radius, ldo):
    from insv2v import ops, _lib
    B, _, h, w = coords64.shape
    npix = B * h * w
    keep = [in32(p.float()) for p in pyr64]
    coords = in32(coords64.float())
    buf = sentinel16(GUARD + npix + GUARD, ldo)
    out = buf[GUARD:GUARD + npix]
    d = _lib.CorrLookupDesc()
    ptrs = [t.data_ptr() for t in keep] + [None] * (4 - len(keep))
    d.pyr0, d.pyr1, d.pyr2, d.pyr3 = ptrs
    d.coords, d.out, d.ldo = coords.data_ptr(), out.data_ptr(), ldo
    d.B, d.h, d.w, d.levels, d.radius = B, h, w, len(keep), radius
    ok(lib().insv2v_corr_lookup(ops._byref(d), stream()), "insv2v_corr_lookup")
    sent = is_sent16(buf)
    assert sent[:GUARD].all() and sent[GUARD + npix:].all(), "corr_lookup wrote rows outside its output"
    assert not sent[GUARD:GUARD + npix].any(), "corr_lookup left part of its rows unwritten"
    return out


@pytest.mark.parametrize("B,h,w,levels,radius,ldo", [(2, 17, 23, 4, 4, 328), (2, 17, 23, 4, 4, 336), (2, 17, 23, 2, 1, 24), (2, 16, 16, 4, 4, 328),
                                                     (1, 45, 80, 4, 4, 328)])
def test_corr_lookup_exact(B, h, w, levels, radius, ldo):
    """Integer pyramids, coordinates in eighths (flow_ref.corr_case): on integers, in (-1, 0) and (w - 1, w), +-10^4 away, on the row and
    column an odd level drops.  The output is the fp16 rounding of the exact value; the padding columns are exactly zero."""
    pyr, coords = fr.corr_case(B, h, w, levels)
    out = run_corr_lookup(pyr, coords, radius, ldo)
    ref = fr.corr_lookup_ref(pyr, coords, radius, ldo)
    nch = levels * (2 * radius + 1) ** 2
    assert ldo > nch and (out[:, nch:].view(torch.int16) == 0).all(), "padding columns must be +0"
    assert_bit_equal(out, ref, ("pixel", "channel"), f"corr_lookup {B}x{h}x{w} levels {levels} radius {radius} ldo {ldo}")


@pytest.mark.parametrize("B,h,w", [(2, 17, 23), (1, 45, 80)])
def test_corr_lookup_random(B, h, w):
    g = fr._gen(B, h, w, 31)
    pyr = [torch.randn((B * h * w, h, w), generator=g).to(F64)]
    for _ in range(3):
        pyr.append(fr.avgpool_ref(pyr[-1]).float().to(F64))
    coords = (fr.grid_xy(B, h, w) + 6 * torch.randn((B, 2, h, w), generator=g)).float().to(F64)
    out = run_corr_lookup(pyr, coords, 4, 328).cpu().to(F64)
    ref = fr.corr_lookup_ref(pyr, coords, 4, 328)
    pmax = pyr[0].abs().max().item()
    excess = ((out - ref).abs() - fr.ulp16(ref) - 1e-6 * pmax).max().item()
    steps = ((out - ref).abs() / fr.ulp16(ref)).max().item()
    share = (out.half() == ref.half()).double().mean().item()
    print(f"[parity] corr_lookup random {B}x{h}x{w}: worst |out - ref| = {steps:.3f} fp16 steps of |ref|, worst excess over the bound {excess:.3g} "
          f"(<= 0 passes), {100 * share:.2f} % bit-equal to fp16(reference)")
    assert torch.isfinite(out).all() and excess <= 0


# ---------------------------------------------------------------------------------------------------------------- raft_flow_rows
def run_flow_rows(coords64, delta64, ncols, with_rows=True):
    """coords1 between guards; delta = columns [1, 3) ... of a NaN-framed fp32 matrix (ldd = width + 4); rows = columns [4, 4 + ncols) of a
    24-wide sentinel matrix.  Returns (coords1 after the call, the rows view or None)."""
    B, _, h, w = coords64.shape
    npix = B * h * w
    cbuf, coords = out32((B, 2, h, w))
    coords.copy_(coords64.float())
    delta = nan_framed(delta64.float(), 1, 3, torch.float32) if delta64 is not None else None
    rbuf = sentinel16(GUARD + npix + GUARD, 24)
    rows = rbuf[GUARD:GUARD + npix, 4:4 + ncols]
    code = lib().insv2v_raft_flow_rows(coords.data_ptr(), delta.data_ptr() if delta is not None else None, delta.stride(0) if delta is not None else 0,
                                       rows.data_ptr() if with_rows else None, rows.stride(0) if with_rows else 0, ncols if with_rows else 0,
                                       B, h, w, stream())
    ok(code, "insv2v_raft_flow_rows")
    check_out32(cbuf, coords.numel(), "raft_flow_rows (coords1)")
    sent = is_sent16(rbuf)
    if with_rows:
        assert sent[:GUARD].all() and sent[GUARD + npix:].all() and sent[:, :4].all() and sent[:, 4 + ncols:].all(), \
            "raft_flow_rows wrote outside columns [0, ncols) of its rows"
        assert not sent[GUARD:GUARD + npix, 4:4 + ncols].any()
    else:
        assert sent.all(), "raft_flow_rows(rows = NULL) wrote flow rows"
    return coords, rows if with_rows else None


@pytest.mark.parametrize("ncols", [8, 2])
def test_flow_rows_update_and_rows(ncols):
    B, h, w = 2, 17, 23
    c64, d64 = fr.flow_rows_case(B, h, w, 6)
    assert d64.shape[1] == 6
    want_c, want_rows = fr.flow_rows_ref(c64, d64, ncols)
    coords, rows = run_flow_rows(c64, d64, ncols)
    assert_bit_equal(coords, want_c, ("image", "channel", "row", "column"), "coords1 += delta", torch.float32)
    assert_bit_equal(rows, want_rows, ("pixel", "column"), f"flow rows, ncols {ncols}")
    assert (rows[:, 2:].view(torch.int16) == 0).all()


def test_flow_rows_without_delta_and_without_rows():
    B, h, w = 2, 17, 23
    c64, d64 = fr.flow_rows_case(B, h, w, 6)
    coords, rows = run_flow_rows(c64, None, 8)                           # delta = NULL: coords1 unchanged, rows written (the estimator's
    assert_bit_equal(coords, c64, ("image", "channel", "row", "column"), "coords1 without delta", torch.float32)   # motion[:, 126:128])
    assert_bit_equal(rows, fr.flow_rows_ref(c64, None, 8)[1], ("pixel", "column"), "flow rows without delta")
    coords, _ = run_flow_rows(c64, d64, 8, with_rows=False)               # rows = NULL: the update alone
    assert_bit_equal(coords, fr.flow_rows_ref(c64, d64, 2)[0], ("image", "channel", "row", "column"), "coords1 += delta, no rows", torch.float32)


# ---------------------------------------------------------------------------------------------------------------- convex_upsample
def run_upsample(coords64, mask64):
    B, _, h, w = coords64.shape
    coords = in32(coords64.float())
    mask = nan_framed(mask64.half(), 8, 16)
    assert mask.stride(0) == 600
    buf, out = out32((B, 2, 8 * h, 8 * w))
    ok(lib().insv2v_convex_upsample(coords.data_ptr(), mask.data_ptr(), mask.stride(0), out.data_ptr(), B, h, w, stream()), "insv2v_convex_upsample")
    check_out32(buf, out.numel(), "convex_upsample")
    return out


@pytest.mark.parametrize("B,h,w", [(2, 17, 23), (1, 45, 80)])
def test_convex_upsample_exact(B, h, w):
    """One-hot softmax (one logit 0, eight -60000): bit for bit 8 x the selected neighbour's flow, exactly 0 where it lies outside the
    grid; every pixel selects each of the 9 neighbours."""
    coords, mask, _ = fr.upsample_case(B, h, w)
    ref = fr.convex_upsample_ref(coords, mask)
    assert_bit_equal(run_upsample(coords, mask), ref, ("image", "channel", "row", "column"), f"convex_upsample {B}x{h}x{w}", torch.float32)


def test_convex_upsample_random():
    B, h, w = 2, 17, 23
    g = fr._gen(B, h, w, 41)
    coords = (fr.grid_xy(B, h, w) + 5 * torch.randn((B, 2, h, w), generator=g)).float().to(F64)
    mask = (3 * torch.randn((B * h * w, 576), generator=g)).half().to(F64)
    out = run_upsample(coords, mask).cpu().to(F64)
    ref = fr.convex_upsample_ref(coords, mask)
    report("convex_upsample random 2x17x23, |out - ref| / max|ref|", ((out - ref).abs().max() / ref.abs().max()).item(), 1e-3)


# ---------------------------------------------------------------------------------------------------------------- instance_norm
@pytest.mark.parametrize("relu", [False, True], ids=["", "relu"])
@pytest.mark.parametrize("C", [8, 24, 96, 256])
@pytest.mark.parametrize("HW", [391, 3600, 64, 7])
def test_instance_norm(HW, C, relu):
    """1 to 56 chunks with a ragged last one (391 rows: 6 chunks of 66 and a tail of 61), idle threads (C = 24, 96), all 256 row lanes
    (C = 8); means up to +-30 around a standard deviation of 0.5, a constant channel, row 0 eight standard deviations off."""
    N = 2
    x64 = fr.instance_norm_case(N, HW, C)
    ref = fr.instance_norm_ref(x64, N, HW, relu, 1e-5)
    x = nan_framed(x64, 8, 16)
    buf, y = out16(N * HW, C, 16, 8)
    nchunks = max(1, min(64, HW // 64))            # ops.instance_norm's choice
    assert nchunks == {391: 6, 3600: 56, 64: 1, 7: 1}[HW]
    pbuf, part = out32((N * nchunks * C * 2,))
    code = lib().insv2v_instance_norm(x.data_ptr(), y.data_ptr(), part.data_ptr(), N, HW, C, x.stride(0), y.stride(0), nchunks, 1e-5, int(relu), stream())
    ok(code, "insv2v_instance_norm")
    assert x.stride(0) == C + 24 and y.stride(0) == C + 24
    check_out16(buf, N * HW, C, "instance_norm", 16)
    check_out32(pbuf, part.numel(), "instance_norm (partials)")
    out = y.cpu().to(F64)
    assert torch.isfinite(out).all()
    assert (out.reshape(N, HW, C)[:, :, 3] == 0).all(), "a constant channel normalises to exactly 0"
    others = ref.reshape(N, HW, C)[:, 1:] if HW > 1 else ref
    scale = others.abs().max().item()
    report(f"instance_norm HW={HW} C={C} relu={relu}, |out - ref| / max|ref, rows > 0|", (out - ref).abs().max().item() / scale, 4e-3)


# ---------------------------------------------------------------------------------------------------------------- ew
def ew_inputs(rows, C):
    """fp16 numbers with 1/8 <= |.| < 8 and random signs (a, b), q / h of one sign with 1/8 <= |.| < 1 (qa, qb), and z in (0, 1)."""
    g = fr._gen(rows, C, 51)

    def mag(lo, hi):
        return torch.exp(torch.rand((rows, C), generator=g, dtype=F64) * (math.log(hi) - math.log(lo)) + math.log(lo))

    def sign():
        return (torch.randint(0, 2, (rows, C), generator=g) * 2 - 1).to(F64)
    a, b = (mag(0.125, 7.9) * sign()).half().to(F64), (mag(0.125, 7.9) * sign()).half().to(F64)
    s = sign()
    qa, qb = (mag(0.126, 0.99) * s).half().to(F64), (mag(0.126, 0.99) * s).half().to(F64)
    z = (torch.rand((rows, C), generator=g, dtype=F64) * 0.998 + 0.001).half().to(F64)
    return a, b, qa, qb, z


def run_ew(op, a64, b64=None, c64=None, inplace_b=False):
    """a, b, c = column slices of NaN-framed buffers with three different strides; out = a slice of a sentinel buffer with a fourth (or b)."""
    from insv2v import ops
    rows, C = a64.shape
    a = nan_framed(a64, 8, 16)
    b = nan_framed(b64, 16, 24) if b64 is not None else None
    c = nan_framed(c64, 24, 8) if c64 is not None else None
    if inplace_b:
        out, before = b, b._base.clone()
    else:
        buf, out = out16(rows, C, 16, 32)
    code = lib().insv2v_ew(op, a.data_ptr(), b.data_ptr() if b is not None else None, c.data_ptr() if c is not None else None, out.data_ptr(), rows, C,
                           a.stride(0), b.stride(0) if b is not None else 0, c.stride(0) if c is not None else 0, out.stride(0), stream())
    ok(code, "insv2v_ew")
    assert len({t.stride(0) for t in (a, b, c, out) if t is not None}) == len([t for t in (a, b, c, out) if t is not None]) - int(inplace_b)
    if inplace_b:
        after = b._base
        assert torch.equal(after[:, :16].view(torch.int16), before[:, :16].view(torch.int16)) and \
            torch.equal(after[:, 16 + C:].view(torch.int16), before[:, 16 + C:].view(torch.int16)), "ew in place wrote outside b's columns"
    else:
        check_out16(buf, rows, C, f"ew op {op}", 16)
    return out.cpu()


def test_ew_ops():
    from insv2v import ops
    assert (ops.EW_RELU, ops.EW_ADD_RELU, ops.EW_TANH, ops.EW_GRU_RH, ops.EW_GRU_OUT) == (1, 2, 3, 4, 5)
    rows, C = 391, 128                      # 6256 chunks of 8 channels: 25 blocks, the last one partial
    a, b, qa, qb, z = ew_inputs(rows, C)
    names = ("row", "channel")
    assert_bit_equal(run_ew(ops.EW_RELU, a), fr.ew_ref("relu", a), names, "ew RELU")
    assert_bit_equal(run_ew(ops.EW_ADD_RELU, a, b), fr.ew_ref("add_relu", a, b), names, "ew ADD_RELU")
    assert_bit_equal(run_ew(ops.EW_GRU_RH, z, b), fr.ew_ref("gru_rh", z, b), names, "ew GRU_RH")
    assert_bit_equal(run_ew(ops.EW_GRU_RH, a, b), fr.ew_ref("gru_rh", a, b), names, "ew GRU_RH, |r| up to 8")
    ref = fr.ew_ref("gru_out", qa, qb, z)
    assert ref.abs().min().item() >= 0.125
    for inplace in (False, True):           # out is b: insv2v/raft.py updates the hidden state where it lies
        out = run_ew(ops.EW_GRU_OUT, qa, qb, z, inplace_b=inplace).to(F64)
        steps = ((out - ref).abs() / fr.ulp16(ref)).max().item()
        report(f"ew GRU_OUT{' in place' if inplace else ''}, |out - ref| in fp16 steps of |ref|", steps, 1.0,
               f", {100 * (out.half() == ref.half()).double().mean().item():.2f} % bit-equal to fp16(reference)")
    ref = fr.ew_ref("tanh", a)
    out = run_ew(ops.EW_TANH, a).to(F64)
    report("ew TANH, |out - ref| / max|ref|", ((out - ref).abs().max() / ref.abs().max()).item(), 2e-3)


# ---------------------------------------------------------------------------------------------------------------- warp / resize / correction
SIZES = [(17, 23), (45, 80), (5, 7), (2, 2)]


@pytest.mark.parametrize("H,W", SIZES)
def test_warp_image(H, W):
    """Samples on column 0 and W - 1, on row 0 and H - 1, half a pixel outside, 10^4 pixels outside (flow_ref.warp_specials)."""
    N, C = 2, 3
    img64, flow64 = fr.warp_case(N, C, H, W)
    ref = fr.warp_ref(img64, flow64)
    img, flow = in32(img64.float()), in32(flow64.float())
    buf, out = out32((N, C, H, W))
    ok(lib().insv2v_warp_image(img.data_ptr(), flow.data_ptr(), out.data_ptr(), N, C, H, W, stream()), "insv2v_warp_image")
    check_out32(buf, out.numel(), "warp_image")
    out = out.cpu().to(F64)
    assert (out[1, :, H - 1, W - 1] == 0).all(), "a sample 10^4 pixels outside is exactly 0"
    report_elementwise(f"warp_image {H}x{W}", (out - ref).abs(), ref, 1e-5, 2e-5)


@pytest.mark.parametrize("src,dst", fr.RESIZE_PAIRS)
def test_resize_flow(src, dst):
    N = 2
    flow64 = fr.resize_case(N, *src)
    ref = fr.resize_flow_ref(flow64, dst)
    flow = in32(flow64.float())
    buf, out = out32((N, 2) + dst)
    ok(lib().insv2v_resize_flow(flow.data_ptr(), out.data_ptr(), N, src[0], src[1], dst[0], dst[1], stream()), "insv2v_resize_flow")
    check_out32(buf, out.numel(), "resize_flow")
    report_elementwise(f"resize_flow {src[0]}x{src[1]} -> {dst[0]}x{dst[1]}", (out.cpu().to(F64) - ref).abs(), ref, 1e-5, 2e-5)


@pytest.mark.parametrize("h,w,R,Q", [s for s in fr.CORRECTION_SETS if s[2] in (1, 3)])
def test_flow_correction(h, w, R, Q):
    eps64, lat64, ref64, flows64 = fr.correction_case(h, w, R, Q)
    want, msum = fr.flow_correction_ref(eps64, lat64, ref64, flows64, fr.SQRT_A, fr.SQRT_1MA)
    eps, lat, ref, flows = (in32(t.float()) for t in (eps64, lat64, ref64, flows64))
    buf, out = out32((Q, 4, h, w))
    code = lib().insv2v_flow_correction(eps.data_ptr(), lat.data_ptr(), ref.data_ptr(), flows.data_ptr(), out.data_ptr(), R + Q, R, h, w,
                                        fr.SQRT_A, fr.SQRT_1MA, stream())
    ok(code, "insv2v_flow_correction")
    check_out32(buf, out.numel(), "flow_correction")
    out = out.cpu().to(F64)
    near = ((msum - 0.5).abs() <= 1e-3)[:, None].expand_as(out)
    masked = (msum <= 0.5 - 1e-3)[:, None].expand_as(out)
    assert near.double().mean().item() <= 0.01 and masked.any() and (msum >= R - 1e-9).any()
    assert (out[masked] == 0).all(), "pixels whose reference frames are all out of view are exactly 0"
    report_elementwise(f"flow_correction {h}x{w} R={R}, away from the threshold", (out - want).abs() * (~near), want, 1e-4, 1e-4,
                       f", {100 * masked.double().mean().item():.1f} % of pixels masked, {int(near[:, 0].sum())} pixels within 1e-3 of the threshold")


# ---------------------------------------------------------------------------------------------------------------- rejections
def entry_points(h16, f32):
    """The ten entry points on two buffers (fp16 [2048, 512], fp32 [2^20]; inputs in the first half, outputs in the second), each with a
    VALID default call that the keyword arguments vary."""
    from insv2v import ops, _lib
    L, st = lib(), stream()
    p16, p32 = h16.data_ptr(), f32.data_ptr()
    o16, o32 = p16 + 1024 * 512 * 2, p32 + (1 << 19) * 4

    def im2col(null_desc=False, **kw):
        d = _lib.Im2colDesc()
        v = dict(x=p16, x2=None, out=o16, ldx=64, ldx2=0, ldo=576, N=1, IH=8, IW=8, C=64, C1=64, KH=3, KW=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1,
                 OH=8, OW=8)
        v.update(kw)
        for k, val in v.items():
            setattr(d, k, val)
        return L.insv2v_im2col(None if null_desc else ops._byref(d), st)

    def inorm(x=p16, y=o16, part=o32, N=2, HW=64, C=64, ldx=64, ldy=64, nchunks=1):
        return L.insv2v_instance_norm(x, y, part, N, HW, C, ldx, ldy, nchunks, 1e-5, 0, st)

    def ew(op=5, a=p16, b=p16 + 4096, c=p16 + 8192, out=o16, rows=16, C=64, lda=64, ldb=64, ldc=64, ldo=64):
        return L.insv2v_ew(op, a, b, c, out, rows, C, lda, ldb, ldc, ldo, st)

    def pool(x=p32, y=o32, n=3, h=5, w=7):
        return L.insv2v_avgpool2x2(x, y, n, h, w, st)

    def lookup(null_desc=False, **kw):
        d = _lib.CorrLookupDesc()
        v = dict(pyr0=p32, pyr1=p32, pyr2=p32, pyr3=p32, coords=p32, out=o16, ldo=328, B=1, h=17, w=23, levels=4, radius=4)
        v.update(kw)
        for k, val in v.items():
            setattr(d, k, val)
        return L.insv2v_corr_lookup(None if null_desc else ops._byref(d), st)

    def frows(c=o32, delta=p32, ldd=2, rows=o16, ldf=8, ncols=8, B=1, h=5, w=7):
        return L.insv2v_raft_flow_rows(c, delta, ldd, rows, ldf, ncols, B, h, w, st)

    def upsample(c=p32, m=p16, ldm=576, out=o32, B=1, h=2, w=3):
        return L.insv2v_convex_upsample(c, m, ldm, out, B, h, w, st)

    def warp(img=p32, flow=p32, out=o32, N=1, C=2, H=2, W=2):
        return L.insv2v_warp_image(img, flow, out, N, C, H, W, st)

    def resize(flow=p32, out=o32, N=1, h=4, w=6, H=2, W=3):
        return L.insv2v_resize_flow(flow, out, N, h, w, H, W, st)

    def correction(eps=p32, lat=p32, ref=p32, flows=p32, out=o32, F=4, R=2, h=2, w=2):
        return L.insv2v_flow_correction(eps, lat, ref, flows, out, F, R, h, w, 0.8, 0.6, st)
    return dict(im2col=im2col, inorm=inorm, ew=ew, pool=pool, lookup=lookup, frows=frows, upsample=upsample, warp=warp, resize=resize,
                correction=correction, p16=p16, o16=o16, p32=p32, o32=o32)


def test_rejections():
    """Each of the ten entry points returns INSV2V_EINVAL for each condition of its guard - plain error returns, nothing is launched - and
    writes nothing: the buffers the refused calls name are sentinels before and after.  The calls the refusals vary are valid: on zeroed
    buffers of the same size each one returns 0 first."""
    e = entry_points(torch.zeros((2048, 512), dtype=torch.float16, device=DEV), torch.zeros((1 << 20,), dtype=torch.float32, device=DEV))
    split = dict(x2=e["p16"] + 64 * 64 * 2, ldx2=32, C1=32)
    for name, kw in (("im2col", {}), ("im2col", split), ("inorm", {}), ("ew", {}), ("ew", dict(op=1, b=None, c=None)), ("pool", {}), ("lookup", {}),
                     ("lookup", dict(h=15, levels=3)), ("frows", {}), ("frows", dict(delta=None, ldd=0)), ("frows", dict(rows=None, ldf=0, ncols=0)),
                     ("upsample", {}), ("warp", {}), ("resize", {}), ("correction", {})):
        assert e[name](**kw) == 0, (name, kw)
    torch.cuda.synchronize()

    h16 = sentinel16(2048, 512)
    f32 = torch.full((1 << 20,), SENT32, dtype=torch.int32, device=DEV).view(torch.float32)
    e = entry_points(h16, f32)
    p16, o16, p32 = e["p16"], e["o16"], e["p32"]
    split = dict(x2=p16 + 64 * 64 * 2, ldx2=32, C1=32)
    refused = {
        "im2col": (dict(null_desc=True), dict(x=None), dict(out=None), dict(x=p16 + 2), dict(out=o16 + 2), dict(split, x2=split["x2"] + 2),
                   dict(split, C=60, ldo=544), dict(C=0), dict(KW=0), dict(stride_h=0), dict(split, C1=36), dict(split, C1=0), dict(split, C1=72), dict(ldx=68), dict(ldo=580), dict(split, ldx2=36),
                   dict(ldo=568), dict(OH=7), dict(OW=9), dict(stride_h=2), dict(stride_w=0), dict(KH=0), dict(N=0)),
        "inorm": (dict(x=None), dict(y=None), dict(part=None), dict(x=p16 + 2), dict(y=o16 + 2), dict(C=60), dict(C=0), dict(ldx=68), dict(ldy=68),
                  dict(nchunks=0), dict(nchunks=65), dict(y=p16), dict(N=0), dict(HW=0), dict(C=2056, ldx=2056, ldy=2056)),                     # y = x: in place
        "ew": (dict(a=None), dict(out=None), dict(op=0), dict(op=6), dict(C=60), dict(rows=0), dict(lda=68), dict(ldo=68), dict(op=2, b=None),
               dict(op=4, b=None), dict(b=None), dict(ldb=68), dict(c=None), dict(ldc=68), dict(a=p16 + 2), dict(b=p16 + 4098), dict(c=p16 + 8194),
               dict(out=o16 + 2)),
        "pool": (dict(x=None), dict(y=None), dict(n=0), dict(h=1), dict(w=1)),
        "lookup": (dict(null_desc=True), dict(coords=None), dict(out=None), dict(levels=5), dict(levels=0), dict(radius=-1), dict(ldo=323),
                   dict(pyr2=None), dict(pyr0=None), dict(h=15), dict(w=15), dict(levels=2, radius=1, ldo=17), dict(B=0), dict(h=0), dict(w=0)),   # 15 >> 3 = 1
        "frows": (dict(c=None), dict(ncols=1), dict(ncols=0), dict(ldf=7), dict(ldd=1), dict(B=0), dict(h=0), dict(w=0)),
        "upsample": (dict(c=None), dict(m=None), dict(out=None), dict(ldm=575), dict(ldm=512), dict(B=0), dict(h=0), dict(w=0)),
        "warp": (dict(img=None), dict(flow=None), dict(out=None), dict(N=0), dict(C=0), dict(H=1), dict(W=1)),
        "resize": (dict(flow=None), dict(out=None), dict(N=0), dict(h=0), dict(w=0), dict(H=0), dict(W=0)),
        "correction": (dict(eps=None), dict(lat=None), dict(ref=None), dict(flows=None), dict(out=None), dict(R=4), dict(R=5), dict(R=0), dict(h=1),
                       dict(w=1)),                                                                                # R = F, R > F
    }
    assert len(refused) == 10
    for name, cases in refused.items():
        for kw in cases:
            assert e[name](**kw) == EINVAL, (name, kw)
    torch.cuda.synchronize()
    assert is_sent16(h16).all() and is_sent32(f32).all(), "a refused call wrote to one of its buffers"
