"""Kernel-level parity of the two kernels of csrc/gemm.hip, forced with tile=: gemm_kernel (the tile kernel, codes = shape 1 - 9 + 10 x ring
depth, with splitk_reduce_kernel behind a split) and conv_halo_kernel (the patch-tiled convolution, codes 100 - 103).  The cases and their
fp64 references come from tests/gemm_tile_ref.py, which asserts a need_gap condition per feature (a kernel that skips the feature cannot
pass; tests/test_gemm_tile_cpu.py asserts the same conditions without a GPU).

Every case
  * asks insv2v_gemm_plan for the descriptor it is about to launch (`planned`) and asserts family, shape, ring, split_k and
    splitk_reduce: no case can silently run on another kernel;
  * runs twice: the two outputs are bit-identical;
  * is compared with the fp64 reference on the SAME fp16-rounded operands, as a whole and on every named block against the block's OWN
    max|ref|: 2e-3 * max|ref| + 2e-3 for a GEMM or a convolution, 4e-3 for both terms where a LayerNorm, GEGLU or GroupNorm is involved,
    R.stats_tol for emitted statistics;
  * is compared element by element with another kernel or another pass over the same arguments (the 128x128 tile 5, or 4 where the case
    IS 5; the single pass for a split): no element beyond |ref| * 2^-9 + 2^-12.
Outputs that go through a window of a wider buffer leave the sentinel (-77) around the window alone.  The exact-rounding case has
tolerance zero.  test_zz_headroom prints the worst err / tol per numbered case of the run.

One-line mutations of csrc/gemm.hip that turn these tests red.  Each was built once into a scratch library (not committed) and the 440
tests of this file were run once against it; all six change values only, their reads stay inside the tests' tensors.  "by" is
err / tol of the first failing comparison of the failing tests; every test not named stayed green.
  * group 1's accumulators not added in the K-group merge of tile_epilogue: 86 tests fail by 89 .. 250 x - every test on a K-group code
    (8, 9 and their deep rings; 101 of the patch-tiled kernel): test_c01_layout 6, c02 15 of 18 (K = 8 passes: group 1's half of the
    only slice is masked zeros), c03 10, c05 1, c06 4, c07 22, c09 16, c10 8, and test_c11_exact_rounding 4 with 40 960 of 81 920
    elements off;
  * the `ktail` masking removed from issue_slice (run without c05's producer / consumer, c07's K = 328 and c08's two-source form, whose
    unmasked reads would leave their tensors): test_c02_k_loop_and_ring fails in the 27 cases with K = 8, 72, 200 and test_c08_batched
    (K = 72) in 2, with errors of 5.7e4 .. inf (the operands hold 64.0 behind column K);
  * activation and residual exchanged in splitk_reduce_kernel: the 20 split_k = 2 cases of test_c04_activations fail by 228 .. 360 x;
  * cur_k.kh / cur_k.kw initialised to 0 at a split's start: all 18 cases of test_c07_split_k_conv fail by 223 .. 287 x;
  * wave_live tested against `wn * NI * 32 + 32` instead of the wave's first column: the 24 cout = 72 cases of test_c10_patch_tiled_conv
    fail by 170 .. 236 x (columns 64 .. 71 stay without their products); cout = 320 is the same predicate and stays green;
  * `hchunk[i] < 0 ? 0 : t` dropped in normalize: all 8 cases of test_c10_patch_tiled_conv_fused_groupnorm fail by 87 .. 119 x.
(test_zz_headroom fails with each of them: it repeats the worst ratio.)
Worked out from the code only (their stores or reads would leave the tensors of the test): `m >= p.M` dropped from the generic store loop
or `ok[it]`'s row term from the fast one (test_c03_store_paths: rows 200 .. 207 of the sentinel buffer, and beyond it on 128-row tiles);
`on + e < oN` dropped from the scalar stores (forms c, d, e, h: the sentinel right of column N).
"""
import ctypes
import math
import re

import pytest
import torch

import gemm_engine_ref as R
import gemm_tile_ref as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TAG = "[gemm_tile]"
SENTINEL = T.SENTINEL
WORST = {}       # numbered case -> (worst err / tol, what)
CASE = [0]


@pytest.fixture(autouse=True)
def _case_number(request):
    m = re.match(r"test_c(\d+)_", request.node.name)
    CASE[0] = int(m.group(1)) if m else 0
    yield


def note(err, tol, what):
    ratio = err / tol if tol > 0 else (0.0 if err == 0 else math.inf)
    if ratio >= WORST.get(CASE[0], (-1.0, ""))[0]:
        WORST[CASE[0]] = (ratio, what)
    return ratio


def close(out, ref, ln=False, what=""):
    err, tol = (out.double() - ref).abs().max().item(), R.tol_of(ref, ln)
    print(f"{TAG} {what}: max err {err:.4g} (tol {tol:.4g}, ratio {note(err, tol, what):.3f})")
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
    print(f"{TAG} {what}: {n} groups, worst group {worst}: max err {err[worst].item():.4g} (tol {tol[worst].item():.4g}, ratio {note((err / tol).max().item(), 1.0, what):.3f})")
    bad = (~(err <= tol)).nonzero().flatten().tolist()
    assert not bad, f"{what}: groups {bad[:16]} beyond their own tolerance (worst {(err - tol).max().item():.4g} over)"


def one_ulp_close(out, ref, what):
    d = (out.float() - ref.float()).abs()
    tol = ref.float().abs() * 2.0 ** -9 + 2.0 ** -12   # two fp16 ulps of slack for values straddling a binade
    bad = int((d > tol).sum())
    print(f"{TAG} {what}: {bad} elements beyond one fp16 rounding step, worst {d.max().item():.4g}")
    assert bad == 0, f"{what}: {bad} elements beyond one fp16 rounding step, worst {d.max().item():.4g}"


def sentinel_intact(big, M, N, what, left=0):
    """big[:M, left:left + N] is the output window of the sentinel-filled 2-D buffer `big`."""
    below, right, lft = int((big[M:] != SENTINEL).sum()), int((big[:M, left + N:] != SENTINEL).sum()), int((big[:M, :left] != SENTINEL).sum())
    print(f"{TAG} {what}: {below} elements written below row {M}, {right} right of column {left + N}, {lft} left of column {left}")
    assert below == 0 and right == 0 and lft == 0, f"{what}: {below} elements below the output, {right} right and {lft} left of it were overwritten"


class planned:
    """Every insv2v_gemm descriptor issued inside is first given to insv2v_gemm_plan (this device's CU count, as the launch plans it): the
    plan is not refused and has the expected fields.  At least one launch is seen."""

    def __init__(self, what, **expect):
        self.what, self.expect, self.seen = what, expect, 0

    def __enter__(self):
        from insv2v import _lib
        lib = self.lib = _lib.load()
        real = self.real = lib.insv2v_gemm

        def spy(ref, stream):
            p = _lib.GemmPlan()
            assert lib.insv2v_gemm_plan(ref, 0, ctypes.byref(p)) == 0
            got = {k: getattr(p, k) for k in self.expect}
            assert p.rc == 0 and got == self.expect, f"{self.what}: planned rc {p.rc} {got}, expected {self.expect}"
            self.seen += 1
            return real(ref, stream)
        lib.insv2v_gemm = spy
        return self

    def __exit__(self, et, ev, tb):
        self.lib.insv2v_gemm = self.real
        if et is None:
            assert self.seen > 0, f"{self.what}: no launch seen"
        return False


def tile_plan(code, split=1, **more):
    return dict(family=T.PLAN_TILE, variant=T.shape_of(code), ring=T.ring_of(code), split_k=split, splitk_reduce=int(split > 1), **more)


def halo_plan(code, oh, ow):
    if code == 103:
        tws = 4 if oh % 16 == 0 and ow % 16 == 0 else 3
    else:
        tws = 4 if oh % 8 == 0 and ow % 16 == 0 else 3
    return dict(family=T.PLAN_HALO, variant=code - 100, tw_shift=tws, split_k=1, splitk_reduce=0)


def versus_of(code):
    return 4 if code == 5 else 5


def run_and_check(run, code, ref, ln, what, blocks=(), expect=None, other="tile"):
    """run(code) -> output.  Planned, forced twice (bit-identical), against fp64 as a whole and on each of `blocks` (name, index) on its
    own; against `other`: a thunk giving the same arguments' output of another kernel / pass and its name, default the 128x128 tile."""
    with planned(what, **(expect or tile_plan(code))):
        out = run(code)
    assert torch.equal(out, run(code)), f"{what}: two calls differ"
    assert out.shape == ref.shape
    close(out, ref, ln, what)
    for name, idx in blocks:
        close(out[idx], ref[idx], ln, f"{what}, {name}")
    if other == "tile":
        v = versus_of(code)
        other = (lambda: run(v)), f"tile {v}"
    if other is not None:
        one_ulp_close(out, other[0](), f"{what} vs {other[1]}")
    return out


def sentinel_buffer(rows, cols, fp32=False):
    return torch.full((rows, cols), SENTINEL, dtype=torch.float32 if fp32 else torch.float16, device=DEV)


# ------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("code,kind", [(46, "unsupported configuration"), (14, "invalid argument"), (55, "invalid argument")])
def test_c00_invalid_codes_are_refused(code, kind):
    """256 x 128 at ring 4 needs a 192 KiB ring; ring 1 and ring 5 do not exist.  LINEAR and CONV3X3."""
    from insv2v import ops, _lib
    a, w, ref = T.layout_case(DEV)
    with pytest.raises(_lib.HipKernelError, match=kind):
        ops.gemm(a, w, tile=code)
    x, wk, bk, kw, geom, cref, blocks = T.splitk_conv_case(DEV)
    with pytest.raises(_lib.HipKernelError, match=kind):
        ops.conv3x3(x, geom, wk, bk, tile=code, **kw)


def test_c00_patch_kernel_refuses_what_it_cannot_do():
    """Code 100 with a ReLU (the patch-tiled kernel never sees the optical-flow activations) and on a 6 x 4 image (no 8 x 16 / 16 x 8
    patches); code 103 on 8 x 32 (no 16 x 16 / 32 x 8 patches)."""
    from insv2v import ops, _lib
    x, wk, bk, kw, geom, ref, blocks = T.halo_case(3, 8, 16, False, False, 72, DEV)
    with pytest.raises(_lib.HipKernelError, match="unsupported configuration"):
        ops.conv3x3(x, (3, 8, 16), wk, bk, tile=100, act=ops.ACT_RELU, **kw)
    x, wk, bk, kw, geom, ref, blocks = T.splitk_conv_case(DEV)
    with pytest.raises(_lib.HipKernelError, match="unsupported configuration"):
        ops.conv3x3(x, geom, wk, bk, tile=100, **kw)
    x, wk, bk, kw, geom, ref, blocks = T.halo_case(2, 8, 32, False, False, 72, DEV)
    with pytest.raises(_lib.HipKernelError, match="unsupported configuration"):
        ops.conv3x3(x, (2, 8, 32), wk, bk, tile=103, **kw)


# ------------------------------------------------------------------------------------------- 1. layout
@pytest.mark.parametrize("code", T.VALID)
def test_c01_layout(code):
    """A = identity, asymmetric W, all 26 valid codes: the staging map, the swizzle, the MFMA C layout, j / wm / wn and the K groups."""
    from insv2v import ops
    a, w, ref = T.layout_case(DEV)
    out = run_and_check(lambda t: ops.gemm(a, w, tile=t), code, ref, False, f"code {code} identity")
    close_groups(out, ref, 1, 8, False, f"code {code} identity, 8-column groups")
    close_groups(out, ref, 0, 16, False, f"code {code} identity, 16-row blocks")


# ------------------------------------------------------------------------------------------- 2. K loop and ring
@pytest.mark.parametrize("code", T.KLOOP_CODES)
@pytest.mark.parametrize("K", T.KLOOP_K)
def test_c02_k_loop_and_ring(K, code):
    """1 partial, 1, 2 with a tail, 2, 4 with a tail and 5 slices through rings of 2, 3 and 4: the prologue's `s < nk`, the counted
    waits, the ring wrap, the K-tail mask.  What lies behind column K of both operands is 64.0."""
    from insv2v import ops
    a, w, b, ref, blocks = T.kloop_case(K, DEV)
    run_and_check(lambda t: ops.gemm(a, w, b, tile=t), code, ref, False, f"code {code} 200x136x{K}", blocks)


# ------------------------------------------------------------------------------------------- 3. store paths
@pytest.mark.parametrize("code", (2, 4, 5, 8))
@pytest.mark.parametrize("form", list(T.STORE_FORMS))
def test_c03_store_paths(form, code):
    """Bias, a three-group row bias, residual and alpha = 0.5 through every store path of tile_epilogue (T.STORE_FORMS); output and residual
    are windows of sentinel-filled buffers."""
    from insv2v import ops
    a, w, b, table, r, g, ref, blocks = T.store_case(form, DEV)
    M, N = ref.shape
    rbig = sentinel_buffer(M + 8, g["ldr"])
    rwin = rbig[:M, g["r_off"]:g["r_off"] + N]
    rwin.copy_(r)
    bigs = {}

    def run(t):
        big = bigs[t] = sentinel_buffer(M + 8, g["ldc"], g["fp32"])
        assert big.data_ptr() % 32 == 0 and rbig.data_ptr() % 16 == 0 and table.data_ptr() % 16 == 0
        out = big[:M, g["c_off"]:g["c_off"] + N]
        got = ops.gemm(a, w, b, residual=rwin, row_bias=table, rows_per_group=T.STORE_RPG, rb_mod=g["rb_mod"], alpha=T.STORE_ALPHA, out=out, tile=t)
        assert got.data_ptr() == out.data_ptr() and got.stride(0) == g["ldc"]
        return got
    what = f"code {code} store form {form}"
    run_and_check(run, code, ref, False, what, blocks)
    sentinel_intact(bigs[code], M, N, what, left=g["c_off"])
    assert torch.equal(rwin, r) and int((rbig != SENTINEL).sum()) == M * N


# ------------------------------------------------------------------------------------------- 4. activations
@pytest.mark.parametrize("code", (4, 5))
@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("name", list(T.ACTS))
def test_c04_activations(name, fp32, split, code):
    """act(a w^T + bias) + residual in tile_epilogue (single pass) and in splitk_reduce_kernel's copy of it (split_k = 2 over K = 128)."""
    from insv2v import ops
    a, w, b, r, ref, blocks = T.act_case(name, DEV)

    def run(t, s=split):
        return ops.gemm(a, w, b, act=T.ACTS[name], residual=r, out_fp32=fp32, tile=t, split_k=s)
    other = "tile" if split == 1 else ((lambda: run(code, 1)), "the single pass")
    run_and_check(run, code, ref, False, f"code {code} {name} fp32 {fp32} split_k {split}", blocks, tile_plan(code, split), other)


# ------------------------------------------------------------------------------------------- 5. folded LayerNorm, emitted statistics
@pytest.mark.parametrize("code", (2, 4, 5, 8))
def test_c05_folded_layernorm_finished_stats(code):
    """585 rows in bias groups of 117 with finished (mean, rstd) pairs (from fp64): sStat of a ragged last tile, groups inside a tile."""
    from insv2v import ops
    a, w, b, col, table, rpg, rb_mod, stats, ref, blocks = T.ln_rows_case(DEV)
    run_and_check(lambda t: ops.gemm(a, w, b, row_bias=table, rows_per_group=rpg, rb_mod=rb_mod, row_stats=stats, col_sum=col, tile=t), code, ref, True,
                  f"code {code} folded LayerNorm, finished statistics", blocks)


@pytest.mark.parametrize("ccode", (4, 5))
@pytest.mark.parametrize("pcode", (4, 5))
@pytest.mark.parametrize("res", [False, True])
def test_c05_producer_statistics_into_consumer(res, pcode, ccode):
    """The producer (258 x 328 x 64) emits per column tile the (sum, sum of squares) of the fp16 values it STORES (last part: 72 columns
    on code 5, 8 on code 4); the consumer (258 x 320 x 328, a K tail) finalises them in its prologue."""
    from insv2v import ops
    a, w, b, r, ref, rows = T.producer_case(res, DEV)
    bn = T.TILE_BN[pcode]
    nparts = (T.PC_NP + bn - 1) // bn
    what = f"producer code {pcode} residual {res}"
    with planned(what, **tile_plan(pcode, stats_width=bn)):
        out, st = ops.gemm(a, w, b, residual=r, emit_stats=True, tile=pcode)
    out2, st2 = ops.gemm(a, w, b, residual=r, emit_stats=True, tile=pcode)
    assert isinstance(st, ops.RowStats) and st.nparts == nparts and st.parts.shape == (nparts, T.PC_M, 2)
    assert torch.equal(out, out2) and torch.equal(st.parts, st2.parts), f"{what}: two calls differ"
    assert torch.equal(out, ops.gemm(a, w, b, residual=r, tile=pcode)), "the output changes when statistics are emitted"
    close(out, ref, False, what)
    one_ulp_close(out, rows, f"{what} vs the reference rounded to fp16")
    want = T.part_sums(out, bn)
    for p in range(nparts):
        for j, name in enumerate(("sum", "sum of squares")):
            err, tol = (st.parts[p, :, j].double() - want[p, :, j]).abs().max().item(), R.stats_tol(want[p, :, j])
            print(f"{TAG} {what}, part {p} {name}: max err {err:.4g} (tol {tol:.4g}, ratio {note(err, tol, what):.3f})")
            assert math.isfinite(err) and err <= tol, f"{what}, part {p} {name}: max err {err:.4g} > tol {tol:.4g}"
    cw, cb, col, cref = T.consumer_case(out)
    what = f"consumer code {ccode} of producer code {pcode} residual {res}"
    finished = T.finished_stats(out)
    run_and_check(lambda t: ops.gemm(out, cw, cb, row_stats=st, col_sum=col, tile=t), ccode, cref, True, what, [("last row tile", slice(256, T.PC_M))],
                  tile_plan(ccode, ln_finalize=0), ((lambda: ops.gemm(out, cw, cb, row_stats=finished, col_sum=col, tile=ccode)), "finished statistics from fp64"))


# ------------------------------------------------------------------------------------------- 6. GEGLU
@pytest.mark.parametrize("code", T.GEGLU_CODES)
@pytest.mark.parametrize("M,C,NH", R.GEGLU_SHAPES)
def test_c06_geglu(M, C, NH, code):
    """GEGLU on the [32 value | 32 gate] interleaved projection with the folded LayerNorm in front, on every NI = 2 shape and two deep
    rings; every 16-output-column group against its own tolerance."""
    from insv2v import ops
    args, col, stats, ref = T.geglu_case(M, C, NH, DEV)
    what = f"code {code} GEGLU {M}x{2 * NH}x{C}"
    bm = T.TILE_BM[T.shape_of(code)]
    assert M % bm
    # (against tile 5; for code 5 against code 4, which plans as shape 2)
    out = run_and_check(lambda t: ops.gemm(*args, act=ops.ACT_GEGLU, row_stats=stats, col_sum=col, tile=t), code, ref, True, what,
                        [("last row tile", slice(M - M % bm, M))])
    assert out.shape == (M, NH)
    close_groups(out, ref, 1, 16, True, f"{what}, 16-output-column groups")


def test_c06_geglu_code_4_plans_as_shape_2():
    """A 64-column tile cannot hold a value block and its gate block: code 4 runs as shape 2, bit-identical to code 2."""
    from insv2v import ops
    M, C, NH = R.GEGLU_SHAPES[0]
    args, col, stats, ref = T.geglu_case(M, C, NH, DEV)
    run = lambda t: ops.gemm(*args, act=ops.ACT_GEGLU, row_stats=stats, col_sum=col, tile=t)
    out = run_and_check(run, 4, ref, True, "code 4 GEGLU", expect=tile_plan(2), other=None)
    assert torch.equal(out, run(2))


@pytest.mark.parametrize("code", T.GEGLU_CODES)
@pytest.mark.parametrize("rb_extra", [0, 1])
def test_c06_geglu_row_bias(rb_extra, code):
    """A two-group row bias over value and gate, interleaved like the bias: 16-byte loads of the aligned table (the gate's quarter from
    the next fragment's), scalar loads where the table's rows are N + 1 apart."""
    from insv2v import ops
    args, col, stats, table, rpg, ref, blocks = T.geglu_rb_case(rb_extra, DEV)
    assert table.stride(0) == 2 * T.GEGLU_RB_SHAPE[2] + rb_extra and table.data_ptr() % 16 == 0

    def run(t):
        return ops.gemm(*args, act=ops.ACT_GEGLU, row_stats=stats, col_sum=col, row_bias=table, rows_per_group=rpg, tile=t)
    what = f"code {code} GEGLU with a row bias, ld_rb = N + {rb_extra}"
    out = run_and_check(run, code, ref, True, what, blocks)
    close_groups(out, ref, 1, 16, True, f"{what}, 16-output-column groups")


# ------------------------------------------------------------------------------------------- 7. split-K
@pytest.mark.parametrize("code", (4, 5, 8))
@pytest.mark.parametrize("ns", T.SPLITS)
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("K", T.SPLIT_K)
def test_c07_split_k_linear(K, fp32, ns, code):
    """5 slices, and 6 with a tail, over 2, 3, 5 and 8 splits (the last two leave splits empty: their slabs must hold zeros); bias, row
    bias, alpha and residual in splitk_reduce_kernel."""
    from insv2v import ops
    a, w, b, table, r, ref, blocks = T.splitk_case(K, DEV)

    def run(t, s=ns):
        return ops.gemm(a, w, b, row_bias=table, rows_per_group=T.STORE_RPG, residual=r, alpha=T.SPLIT_ALPHA, out_fp32=fp32, tile=t, split_k=s)
    run_and_check(run, code, ref, False, f"code {code} 200x136x{K} split_k {ns} fp32 {fp32}", blocks, tile_plan(code, ns), ((lambda: run(code, 1)), "the single pass"))


@pytest.mark.parametrize("code", (4, 5, 8))
@pytest.mark.parametrize("ns", T.SPLITS_CONV)
@pytest.mark.parametrize("two", [False, True])
def test_c07_split_k_conv(two, ns, code):
    """2 images of 6 x 4, 128 (or 64 + 64) -> 72 channels, 18 slices: with 4 splits the later ones start at k0 = 320, 640, 960 - inside
    tap 2's second channel block, at tap 5, inside tap 7 - and the cursor's (kh, kw, ci0) must start there."""
    from insv2v import ops
    x, wk, bk, kw, geom, ref, blocks = T.splitk_conv_case(DEV)
    xs = dict(x=x[:, :64].contiguous(), x2=x[:, 64:].contiguous()) if two else dict(x=x)

    def run(t, s=ns):
        out, g = ops.conv3x3(xs["x"], geom, wk, bk, x2=xs.get("x2"), tile=t, split_k=s, **kw)
        assert g == geom
        return out
    run_and_check(run, code, ref, False, f"code {code} conv 2x6x4 two sources {two} split_k {ns}", blocks, tile_plan(code, ns), ((lambda: run(code, 1)), "the single pass"))


# ------------------------------------------------------------------------------------------- 8. batched
@pytest.mark.parametrize("code", (4, 5))
@pytest.mark.parametrize("two", [False, True])
def test_c08_batched(two, code):
    """batch = 3 with a gap behind every batch of every operand; two: [a | a2] with lda2 != lda, the second source's batches a_bs
    elements apart (include/insv2v_hip.h, 'Batched:')."""
    from insv2v import ops
    av, a2v, wv, b, rv, ref, blocks = T.batched_case(two, DEV)
    B, M, N, K = T.BATCH
    L, S = T.BATCH_LD, T.BATCH_STRIDE
    bufs = {}

    def run(t):
        cbuf = bufs[t] = torch.full((B * S["c_bs"],), SENTINEL, dtype=torch.float16, device=DEV)
        out = T.strided_batches(cbuf, S["c_bs"], M, L["ldc"], N, B)
        got = ops.gemm(av, wv, b, a2=a2v, residual=rv, alpha=T.BATCH_ALPHA, out=out, tile=t, batch=B, **S)
        assert got.data_ptr() == cbuf.data_ptr()
        return got
    what = f"code {code} batched two sources {two}"
    run_and_check(run, code, ref, False, what, blocks)
    for z in range(B):
        sentinel_intact(bufs[code].view(B, S["c_bs"] // L["ldc"], L["ldc"])[z], M, N, f"{what}, batch {z}")


# ------------------------------------------------------------------------------------------- 9. gathered convolution
def check_conv(x, in_geom, wk, bk, kw, geom, ref, blocks, code, what, ln=False, expect=None, other="tile", ldc_extra=None):
    from insv2v import ops
    M, N = ref.shape
    bigs = {}

    def run(t):
        out = None
        if ldc_extra is not None:
            bigs[t] = sentinel_buffer(M + 16, N + ldc_extra)
            out = bigs[t][:M, :N]
        got, g = ops.conv3x3(x, in_geom, wk, bk, tile=t, out=out, **kw)
        assert g == geom
        return got
    out = run_and_check(run, code, ref, ln, what, blocks, expect, other)
    if ldc_extra is not None:
        sentinel_intact(bigs[code], M, N, what)
    return out


@pytest.mark.parametrize("code", T.CONV_CODES)
@pytest.mark.parametrize("c2", [0, 64])
@pytest.mark.parametrize("nb,h,w,stride,ups", R.CONV_GEOMS)
def test_c09_gathered_conv(nb, h, w, stride, ups, c2, code):
    """The tile kernel's CONV3X3 gather on six shapes: tiles straddling images and image rows, one-row and one-column images, stride 2,
    nearest x2 upsample; one and two channel sources."""
    x, wk, bk, kw, geom, ref, blocks = R.conv_case(nb, h, w, stride, ups, c2, DEV)
    check_conv(x, (nb, h, w), wk, bk, kw, geom, ref, blocks, code, f"code {code} conv3x3 {nb}x{h}x{w} stride {stride} upsample {ups} c2 {c2}")


@pytest.mark.parametrize("code", T.CONV_CODES)
@pytest.mark.parametrize("c2", [0, 64])
@pytest.mark.parametrize("idx", range(len(T.CONV_EXTRA)))
def test_c09_gathered_conv_pad0_and_cropped_upsample(idx, c2, code):
    """Stride 2 with pad (0, 0) (the extra row / column at the far edge is zero); the x2 image without its last row and / or column: the
    zero padding sits at the cropped edge."""
    nb, h, w = T.CONV_EXTRA[idx][:3]
    x, wk, bk, kw, geom, ref, blocks = T.conv_extra_case(idx, c2, DEV)
    check_conv(x, (nb, h, w), wk, bk, kw, geom, ref, blocks, code, f"code {code} conv3x3 {T.CONV_EXTRA[idx]} c2 {c2}")


# ------------------------------------------------------------------------------------------- 10. patch-tiled convolution
@pytest.mark.parametrize("cout", T.HALO_COUT)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("code,nb,h,w,ups", T.HALO_CASES)
def test_c10_patch_tiled_conv(code, nb, h, w, ups, two, cout):
    """conv_halo_kernel: the patch map of 8 x 16, 16 x 8, 16 x 16 and 32 x 8 patches, one channel block and three (the source switching at
    the third, the patch double-buffered), the half-empty third column tile of cout = 320; against fp64 and the tile kernel."""
    x, wk, bk, kw, geom, ref, blocks = T.halo_case(nb, h, w, ups, two, cout, DEV)
    check_conv(x, (nb, h, w), wk, bk, kw, geom, ref, blocks, code, f"code {code} conv3x3 {nb}x{h}x{w} upsample {ups} two sources {two} cout {cout}",
               expect=halo_plan(code, geom[1], geom[2]), ldc_extra=8)


@pytest.mark.parametrize("h,w,two,silu", T.HALO_GN)
def test_c10_patch_tiled_conv_fused_groupnorm(h, w, two, silu):
    """The (scale, shift) table of the reference module (fp64) applied to the patch in LDS: padding stays zero, image nb takes sample
    nb / 2's table, SiLU on and off."""
    x, wk, bk, kw, geom, ref, blocks = T.halo_gn_case(h, w, two, silu, DEV)
    check_conv(x, geom, wk, bk, kw, geom, ref, blocks, 100, f"code 100 conv3x3 4x{h}x{w} fused GroupNorm two sources {two} SiLU {silu}", ln=True,
               expect=dict(halo_plan(100, h, w), gn_fuse=1), other=None, ldc_extra=8)


# ------------------------------------------------------------------------------------------- 11. exact rounding
@pytest.mark.parametrize("code,ldc_extra,split", T.EXACT_CASES)
@pytest.mark.parametrize("res", [False, True])
def test_c11_exact_rounding(res, code, ldc_extra, split):
    """One non-zero product per accumulator and exact fp32 sums with bits below the fp16 ulp: the stored value EQUALS the fp32 value
    rounded to nearest even - in the vectorised store, in the scalar stores (ldc = N + 4) and in the reduction's conversion."""
    from insv2v import ops
    a, w, b, r, ref32, share, ties = R.exact_case(res, DEV)
    M, N = ref32.shape

    def run():
        out = sentinel_buffer(M, N + ldc_extra)[:, :N] if ldc_extra else None
        return ops.gemm(a, w, b, residual=r, out=out, tile=code, split_k=split or 1)
    what = f"exact rounding, code {code}, ldc = N + {ldc_extra}, split_k {split}, residual {res}"
    with planned(what, **tile_plan(code, split or 1)):
        out = run()
    want = ref32.half()
    bad = out != want
    nbad, toward_zero = int(bad.sum()), int((out == R.round_toward_zero_f16(ref32))[bad].sum())
    print(f"{TAG} {what}: {nbad} of {want.numel()} elements differ from nearest-even ({toward_zero} of them equal toward-zero)")
    note(nbad, 0.0, what)
    assert nbad == 0, f"{what}: {nbad} elements are not the fp32 value rounded to nearest even ({toward_zero} of them are it rounded toward zero)"
    assert torch.equal(out, run())


# ------------------------------------------------------------------------------------------- headroom
def test_zz_headroom():
    """Prints the worst err / tol of every numbered case that ran in this session (case 11: 0 = exact)."""
    for case in sorted(WORST):
        ratio, what = WORST[case]
        print(f"{TAG} headroom: case {case}: worst err / tol {ratio:.3f} ({what})")
        assert ratio <= 1.0
