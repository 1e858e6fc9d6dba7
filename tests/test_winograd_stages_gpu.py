"""Stage-level parity of the two Winograd transform kernels (csrc/winograd.hip: insv2v_winograd_input, insv2v_winograd_output), called
through the C ABI on their own - not through ops.winograd_conv3x3, whose 640 - 2560-channel GEMM and whole-output norm hide a stage that
is slightly off - against the float64 restatement of tests/winograd_ref.py.

Both transforms are short sums with coefficients +-1 and 2.  On the inputs of winograd_ref.exact_input_case / exact_output_case every
intermediate is an fp16 number (tests/test_winograd_stages_cpu.py checks that, and that a kernel taking the neighbouring sample's table,
a normalised padding, x for x2 or the neighbouring row-bias group computes something else), so the assertion is torch.equal.

Every operand that has a stride gets one that differs from its width: x / x2 / residual / y are column views of wider buffers (NaN around
the inputs, a sentinel bit pattern around the outputs), row_bias has ld_rb > Cout; M is NaN beyond its `tiles` rows.  V and y lie in sentinel
buffers with guard rows: what must not be written (rows [tiles, v_group_rows) of every matrix, guard rows, columns outside [0, Cout)) still
holds the sentinel afterwards, and everything that must be written does not.

Geometries (winograd_ref.DIRECT / UPSAMPLE): several images per workgroup with a partial last workgroup and a GroupNorm sample boundary
inside it, one-pixel / one-row / one-column images, the whole-image limit of 512 LDS slots, bands of tile rows with odd W, a partial last
band, one tile row per band, and the 64 KiB dynamic-LDS launch at W = 128 - in the direct and in the upsample form.

Bounds.  Exact cases: bit for bit.  With SiLU the staged pixel is fp16(silu(fma(x, scale, shift))) from fp32 arithmetic with a fast
exponential against the reference's fp16(float64): it may land one fp16 step from the reference's; V sums four of them (upsample: 2 * 2 * one)
- 4 steps - and is rounded once more - half a step of a value up to 4 max|d|, i.e. 2 steps of max|d|: |V - ref| <= 8 * ulp16(max|d|)
elementwise, max|d| over the reference's staged pixels.  Composition (input kernel -> fp16(V_k U_k^T) in torch -> output kernel) against
the float64 convolution of the staged input: the project's stated Winograd tolerance 2e-3 * max|ref| + 1e-3."""
import math

import pytest
import torch
import torch.nn.functional as F

import winograd_ref as wr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
SENT = 0x7EAB        # an fp16 NaN bit pattern: no kernel output, no test input
GUARD = 8            # sentinel rows before and after V / y
EINVAL, EUNSUPPORTED = -1, -2
# v_group_rows / m_group_rows = exactly `tiles` here (the ABI allows >=), tiles rounded up to 256 elsewhere
TIGHT = {((3, 5, 7, 1), False), ((1, 9, 128, 1), False), ((3, 3, 5, 1), True), ((7, 2, 3, 2), True)}


def sentinel(rows, cols):
    return torch.full((rows, cols), SENT, dtype=torch.int16, device=DEV).view(torch.float16)


def is_sent(t):
    return t.view(torch.int16) == SENT


def nan_framed(values, left, right, dtype=torch.float16):
    """`values` [rows, n] as a column view of a NaN-filled [rows, left + n + right] buffer."""
    rows, n = values.shape
    buf = torch.full((rows, left + n + right), float("nan"), dtype=dtype, device=DEV)
    view = buf[:, left:left + n]
    view.copy_(values)
    return view


def group_rows(geom, up):
    NB, H, W, _ = geom
    tiles = wr.tiles_of(NB, H, W, up)
    return tiles if (geom, up) in TIGHT else -(-tiles // 256) * 256


def run_input(x64, geom, up, ab=None, silu=False, vgr=None):
    """insv2v_winograd_input on x64 [pixels, 128] passed as x (64 channels, ldx 88) | x2 (64 channels, ldx2 104) -> V [ng, tiles, 128] fp16 on
    the GPU, after the checks on what was and was not written."""
    from insv2v import ops, _lib
    NB, H, W, ips = geom
    C, C1 = wr.C_IN, wr.C1_IN
    assert ops.winograd_ok((NB, H, W), C, C1, upsample=up)
    x, x2 = nan_framed(x64[:, :C1], 8, 16), nan_framed(x64[:, C1:], 16, 24)
    assert x.stride(0) == 88 and x2.stride(0) == 104 and x.data_ptr() % 16 == 0 and x2.data_ptr() % 16 == 0
    tiles, ng = wr.tiles_of(NB, H, W, up), 9 if up else 16
    vgr = group_rows(geom, up) if vgr is None else vgr
    vb = sentinel(GUARD + ng * vgr + GUARD, C)
    v = vb[GUARD:GUARD + ng * vgr]
    d = _lib.WinogradInDesc()
    d.x, d.x2, d.v, d.ldx, d.ldx2, d.v_group_rows = x.data_ptr(), x2.data_ptr(), v.data_ptr(), x.stride(0), x2.stride(0), vgr
    d.NB, d.H, d.W, d.C, d.C1, d.upsample = NB, H, W, C, C1, int(up)
    if ab is not None:
        abd = ab.to(device=DEV, dtype=torch.float32).contiguous()
        d.gn_ab, d.gn_images_per_sample, d.gn_silu = abd.data_ptr(), ips, int(silu)
    _lib.check(_lib.load().insv2v_winograd_input(ops._byref(d), ops._stream()), "insv2v_winograd_input")
    torch.cuda.synchronize()
    assert is_sent(vb[:GUARD]).all() and is_sent(vb[GUARD + ng * vgr:]).all(), "the input transform wrote outside V"
    V = v.reshape(ng, vgr, C)
    assert is_sent(V[:, tiles:]).all(), "the input transform wrote rows [tiles, v_group_rows) of a matrix"
    unwritten = is_sent(V[:, :tiles]).cpu()
    assert not unwritten.any(), "V not written: " + wr.first_diff(unwritten, torch.zeros_like(unwritten), ("matrix", "tile", "channel"))
    return V[:, :tiles]


def run_output(M, geom, up, bias=None, rb=None, rpg=0, res=None, mgr=None):
    """insv2v_winograd_output on M [ng, tiles, Cout] (float64 or fp16, CPU or GPU) -> y [pixels, Cout] fp16 on the GPU; ldy = Cout + 24,
    ldr = Cout + 16, ld_rb = Cout + 12."""
    from insv2v import ops, _lib
    NB, H, W, _ = geom
    ng, tiles, Cout = M.shape
    assert ng == (9 if up else 16) and tiles == wr.tiles_of(NB, H, W, up)
    pixels = NB * H * W * (4 if up else 1)
    mgr = group_rows(geom, up) if mgr is None else mgr
    m = torch.full((ng, mgr, Cout), float("nan"), dtype=torch.float16, device=DEV)
    m[:, :tiles] = M.to(DEV)
    yb = sentinel(GUARD + pixels + GUARD, Cout + 24)
    y = yb[GUARD:GUARD + pixels, 8:8 + Cout]
    d = _lib.WinogradOutDesc()
    d.m, d.y, d.m_group_rows, d.ldy = m.data_ptr(), y.data_ptr(), mgr, y.stride(0)
    d.NB, d.H, d.W, d.Cout, d.upsample = NB, H, W, Cout, int(up)
    keep = [m]
    if bias is not None:
        keep.append(bias.to(device=DEV, dtype=torch.float32).contiguous())
        d.bias = keep[-1].data_ptr()
    if rb is not None:
        keep.append(nan_framed(rb, 4, 8, torch.float32))
        d.row_bias, d.ld_rb, d.rows_per_group = keep[-1].data_ptr(), keep[-1].stride(0), rpg
        assert d.ld_rb == Cout + 12
    if res is not None:
        keep.append(nan_framed(res, 8, 8))
        d.residual, d.ldr = keep[-1].data_ptr(), keep[-1].stride(0)
        assert d.ldr == Cout + 16
    assert d.ldy == Cout + 24 and y.data_ptr() % 16 == 0
    _lib.check(_lib.load().insv2v_winograd_output(ops._byref(d), ops._stream()), "insv2v_winograd_output")
    torch.cuda.synchronize()
    sent = is_sent(yb)
    assert sent[:GUARD].all() and sent[GUARD + pixels:].all(), "the output transform wrote rows outside y"
    assert sent[:, :8].all() and sent[:, 8 + Cout:].all(), "the output transform wrote columns outside [0, Cout)"
    unwritten = sent[GUARD:GUARD + pixels, 8:8 + Cout].cpu()
    assert not unwritten.any(), "y not written: " + wr.first_diff(unwritten, torch.zeros_like(unwritten), ("pixel", "channel"))
    return y


def assert_bit_equal(got, ref64, names, what):
    assert wr.is_fp16(ref64), f"{what}: the reference is not exact in fp16 (a condition on the test's inputs)"
    got, ref = got.cpu(), ref64.half()
    assert got.shape == ref.shape
    assert torch.equal(got, ref), f"{what}: " + wr.first_diff(got, ref, names)


# ---------------------------------------------------------------------------------------------------------------- input transform
@pytest.mark.parametrize("geom,up", wr.GEOMS, ids=[wr.geom_id(p) for p in wr.GEOMS])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
def test_input_transform_exact(geom, up, norm):
    NB, H, W, ips = geom
    x, ab = wr.exact_input_case(NB, H, W, ips, up, norm)
    V = run_input(x, geom, up, ab)
    ref = wr.input_ref(x, NB, H, W, ab, ips, False, up)
    assert_bit_equal(V, ref, ("matrix", "tile", "channel"), f"input transform {wr.geom_id((geom, up))} norm {norm}")


def silu_case(geom, up):
    NB, H, W, ips = geom
    g = wr._gen(NB, H, W, ips, up, 99)
    x = (torch.rand((NB * H * W, wr.C_IN), generator=g, dtype=F64) * 7.98 - 3.99).half().to(F64)
    ns = -(-NB // ips)
    ab = torch.stack([1 + 0.2 * torch.randn((ns, wr.C_IN), generator=g, dtype=F64), 0.3 * torch.randn((ns, wr.C_IN), generator=g, dtype=F64)], -1).float().to(F64)
    return x, ab


SILU_GEOMS = [((7, 4, 6, 2), False), ((2, 19, 27, 1), False), ((3, 3, 5, 1), True)]


@pytest.mark.parametrize("geom,up", SILU_GEOMS, ids=[wr.geom_id(p) for p in SILU_GEOMS])
def test_input_transform_silu(geom, up):
    NB, H, W, ips = geom
    x, ab = silu_case(geom, up)
    assert x.abs().max().item() < 4
    V = run_input(x, geom, up, ab, silu=True).cpu()
    ref = wr.input_ref(x, NB, H, W, ab, ips, True, up)
    dmax = wr.stage_ref(x, NB, H, W, ab, ips, True).abs().max().item()
    bound = 8 * wr.ulp16(dmax)
    err = (V.to(F64) - ref).abs()
    share = (V == ref.half()).double().mean().item()
    print(f"[winograd stages] input transform with SiLU {wr.geom_id((geom, up))}: {100 * share:.2f} % of V bit-equal to fp16(reference), "
          f"worst |V - ref| {err.max().item():.4g} (bound 8 * ulp16({dmax:.4g}) = {bound:.4g})")
    bad = err > bound
    assert torch.isfinite(V).all() and not bad.any(), wr.first_diff(bad, torch.zeros_like(bad), ("matrix", "tile", "channel"))


# ---------------------------------------------------------------------------------------------------------------- output transform
@pytest.mark.parametrize("geom,up", wr.GEOMS, ids=[wr.geom_id(p) for p in wr.GEOMS])
@pytest.mark.parametrize("use_res", [False, True], ids=["", "res"])
@pytest.mark.parametrize("use_rb", [False, True], ids=["", "rb"])
def test_output_transform_exact(geom, up, use_res, use_rb):
    """The eight RES x RB x UP instantiations at every geometry, Cout = 16."""
    NB, H, W, ips = geom
    M, bias, rb, rpg, res = wr.exact_output_case(NB, H, W, ips, up, 16)
    y = run_output(M, geom, up, bias, rb if use_rb else None, rpg, res if use_res else None)
    ref = wr.output_ref(M, NB, H, W, bias, rb if use_rb else None, rpg, res if use_res else None, up)
    assert_bit_equal(y, ref, ("pixel", "channel"), f"output transform {wr.geom_id((geom, up))} residual {use_res} row bias {use_rb}")


@pytest.mark.parametrize("geom,up,Cout,use_bias", [((3, 5, 7, 1), False, 8, True), ((7, 2, 3, 2), True, 8, True),
                                                   ((7, 4, 6, 2), False, 16, False), ((3, 3, 5, 1), True, 16, False)])
def test_output_transform_exact_cout8_and_no_bias(geom, up, Cout, use_bias):
    """Cout = 8 (one 8-channel chunk per tile: thread index == tile index) and bias = NULL, row bias and residual on."""
    NB, H, W, ips = geom
    M, bias, rb, rpg, res = wr.exact_output_case(NB, H, W, ips, up, Cout)
    bias = bias if use_bias else None
    y = run_output(M, geom, up, bias, rb, rpg, res)
    assert_bit_equal(y, wr.output_ref(M, NB, H, W, bias, rb, rpg, res, up), ("pixel", "channel"), f"output transform {wr.geom_id((geom, up))} Cout {Cout} bias {use_bias}")


# ---------------------------------------------------------------------------------------------------------------- composition
COMPOSE = [((3, 5, 7, 1), False), ((2, 19, 27, 1), False), ((3, 3, 5, 1), True), ((1, 19, 27, 1), True)]


@pytest.mark.parametrize("geom,up", COMPOSE, ids=[wr.geom_id(p) for p in COMPOSE])
def test_stages_compose_to_the_convolution(geom, up):
    """Input kernel -> M_k = fp16(V_k U_k^T) in torch -> output kernel == the float64 convolution of the staged input: the two kernels agree
    on the tile order and the matrix numbering without the GEMM engine in between.  C = 128, Cout = 16, norm + SiLU, row bias, residual."""
    from insv2v import ops
    NB, H, W, ips = geom
    Cout, C = 16, wr.C_IN
    x, ab = silu_case(geom, up)
    g = wr._gen(NB, H, W, ips, up, 123)
    w = (torch.randn((Cout, C, 3, 3), generator=g) * (9 * C) ** -0.5).half().float()
    pixels, scale = NB * H * W * (4 if up else 1), 4 if up else 1
    rpg = ips * H * W * scale
    bias = torch.randn(Cout, generator=g)
    rb = torch.randn((-(-NB // ips), Cout), generator=g) * 0.5
    res = torch.randn((pixels, Cout), generator=g).half()
    V = run_input(x, geom, up, ab, silu=True)
    U = ops.winograd_weights(w, DEV, upsample=up)
    M = torch.bmm(V.float(), U.float().transpose(1, 2)).half()
    y = run_output(M, geom, up, bias, rb, rpg, res).cpu().to(F64)
    img = wr.stage_ref(x, NB, H, W, ab, ips, True).reshape(NB, H, W, C).permute(0, 3, 1, 2)
    if up:
        img = F.interpolate(img, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(img, w.to(F64), bias.to(F64), padding=1).permute(0, 2, 3, 1).reshape(pixels, Cout)
    ref = ref + rb.to(F64)[torch.arange(pixels) // rpg] + res.to(F64)
    err, tol = (y - ref).abs().max().item(), 2e-3 * ref.abs().max().item() + 1e-3
    share = (y.half() == ref.half()).double().mean().item()
    print(f"[winograd stages] composition {wr.geom_id((geom, up))}: worst |y - ref| {err:.4g} (tolerance {tol:.4g}, max|ref| {ref.abs().max().item():.4g}), "
          f"{100 * share:.2f} % of y bit-equal to fp16(reference)")
    assert math.isfinite(err) and err <= tol, f"composition {wr.geom_id((geom, up))}: max err {err:.4g} > tol {tol:.4g}"


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    """Return codes only: every call below is refused before a launch.  (The buffers are large enough for each descriptor as stated.)"""
    from insv2v import ops, _lib
    lib = _lib.load()
    x = torch.zeros((8 * 129, 256), dtype=torch.float16, device=DEV)
    v = torch.zeros((16 * 1024, 128), dtype=torch.float16, device=DEV)

    def in_desc(NB=2, H=4, W=6, C=128, C1=0, ldx=256, vgr=None, up=0):
        d = _lib.WinogradInDesc()
        tiles = wr.tiles_of(NB, H, W, bool(up))
        d.x, d.v, d.ldx, d.v_group_rows = x.data_ptr(), v.data_ptr(), ldx, tiles if vgr is None else vgr
        if C1:
            d.x2, d.ldx2, d.C1 = x.data_ptr(), 256, C1
        d.NB, d.H, d.W, d.C, d.upsample = NB, H, W, C, up
        return d

    def call_in(**kw):
        return lib.insv2v_winograd_input(ops._byref(in_desc(**kw)), ops._stream())
    assert call_in(NB=1, H=8, W=129) == EUNSUPPORTED            # an image row of more than 128 pixels
    assert call_in(C=96) == EUNSUPPORTED
    assert call_in(C1=32) == EUNSUPPORTED
    assert call_in(vgr=2 * 2 * 3 - 1) == EINVAL                 # tiles - 1
    assert call_in(up=1, vgr=2 * 4 * 6 - 1) == EINVAL
    assert call_in(ldx=68) == EINVAL
    assert not ops.winograd_ok((1, 8, 129), 128) and not ops.winograd_ok((1, 8, 129), 128, upsample=True)

    m = torch.zeros((16 * 256, 16), dtype=torch.float16, device=DEV)
    y = torch.zeros((2 * 8 * 12, 16), dtype=torch.float16, device=DEV)
    rb = torch.zeros((4, 16), dtype=torch.float32, device=DEV)

    def call_out(NB=2, H=4, W=6, Cout=16, mgr=None, rpg=0, up=0):
        d = _lib.WinogradOutDesc()
        tiles = wr.tiles_of(NB, H, W, bool(up))
        d.m, d.y, d.m_group_rows, d.ldy = m.data_ptr(), y.data_ptr(), tiles if mgr is None else mgr, 16
        d.NB, d.H, d.W, d.Cout, d.upsample = NB, H, W, Cout, up
        if rpg:
            d.row_bias, d.ld_rb, d.rows_per_group = rb.data_ptr(), 16, rpg
        return lib.insv2v_winograd_output(ops._byref(d), ops._stream())
    assert call_out(Cout=12) == EUNSUPPORTED
    assert call_out(mgr=2 * 2 * 3 - 1) == EINVAL                # tiles - 1
    assert call_out(up=1, mgr=2 * 4 * 6 - 1) == EINVAL
    assert call_out(rpg=4 * 6 + 1) == EINVAL                    # not a multiple of the image
    assert call_out(rpg=36) == EINVAL
    assert call_out(up=1, rpg=2 * 4 * 6) == EINVAL              # upsample: the image is the 2H x 2W one
    torch.cuda.synchronize()
