"""Kernel-level parity of the register-resident row kernels of csrc/rows_ffn.hip - insv2v_rowlin in every form (LN x FRAME x RES, the
GroupNorm-on-load form), on every tile schedule (one round, a persistent workgroup's second round, two token blocks per wave) and
insv2v_ffn_fused - against the fp64 references of tests/rows_ref.py, judged per block.  Every test asks the planner (ops.rowlin_plan,
cus = 0: this device) which kernel its shape runs and asserts that it is the kernel the case claims; the shapes are derived from this
device's CU count.  tests/test_rowlin_forms_cpu.py pins the same plans without a GPU."""
import ctypes

import pytest
import torch

import rows_ref as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def on_this_device(c, M, N, K, form=0, frames=R.FRAMES, gn_rows=0):
    """The planner's answer for THIS device (cus = 0) is the kernel, the tiling and the rounds the case was built for."""
    p0, p = R.plan(M, N, K, form, frames=frames, gn_rows=gn_rows, cus=0), c["plan"]
    fields = [n for n, _ in p._fields_]
    assert [getattr(p0, n) for n in fields] == [getattr(p, n) for n in fields], f"{c['what']}: built for {R.show(p)}, this device runs {R.show(p0)}"
    return p0


def report(what, p, worst):
    print(f"[parity] {what}: {R.show(p)}; worst block '{worst[1]}' at {worst[0]:.3f} of its tolerance")


def launch_rowlin(x, stream, out, N, *, layernorm=False, residual=None, frames=0, rows_per_frame=0, stats=None, gn_ab=None, gn_rows=0):
    """insv2v_rowlin through a descriptor of our own (a caller-owned statistics buffer); returns the rc."""
    from insv2v import _lib
    d = _lib.RowLinDesc()
    d.x, d.out, d.wstream, d.ldx, d.ldo = x.data_ptr(), out.data_ptr(), stream.data_ptr(), x.stride(0), out.stride(0)
    if residual is not None:
        d.residual, d.ldr = residual.data_ptr(), residual.stride(0)
    d.M, d.N, d.K, d.layernorm, d.eps = x.shape[0], N, x.shape[1], int(layernorm), R.EPS
    d.frame_bias, d.rows_per_frame, d.frames = int(frames > 0), rows_per_frame, frames
    if stats is not None:
        d.stats_out, d.stats_eps = stats.data_ptr(), R.EPS
    if gn_ab is not None:
        d.gn_ab, d.gn_rows = gn_ab.data_ptr(), gn_rows
    return _lib.load().insv2v_rowlin(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)


def one_ulp_close(out, ref, what):
    """The bound of test_wide_store_kernels_under_co_residency: one fp16 rounding step per element."""
    d = (out.float() - ref.float()).abs()
    tol = ref.float().abs() * 2.0 ** -9 + 2.0 ** -12
    bad = int((d > tol).sum())
    assert bad == 0, f"{what}: {bad} elements beyond one fp16 rounding step, worst {d.max().item():.4g}"


# ------------------------------------------------------------------------------------------- 1. forms x schedules
@pytest.mark.parametrize("K,N,sched,form,frames", R.form_cases())
def test_forms(K, N, sched, form, frames):
    from insv2v import ops
    c = R.form_case(K, N, sched, form, cus(), dev(), frames)
    p = on_this_device(c, c["M"], N, K, form, frames)
    out = ops.rowlin(c["x"], c["stream"], N, **c["kw"])
    worst = R.judge(out, c["ref"], c["blocks"], c["ln"], c["what"])
    report(c["what"], p, worst)
    assert torch.equal(out, ops.rowlin(c["x"], c["stream"], N, **c["kw"])), f"{c['what']}: not deterministic"


# ------------------------------------------------------------------------------------------- 2. exact layout and rounding
@pytest.mark.parametrize("K,res,tb", R.EXACT_CASES)
def test_exact_layout_and_rounding(K, res, tb):
    """One-hot rows: every stored value must EQUAL the exact fp32 sum rounded to nearest even - a misplaced fragment, a swapped lane half,
    a k-step out of order or a lost lo part of the bias changes it (the builder's input conditions)."""
    from insv2v import ops
    c = R.exact_case(K, res, tb, cus(), dev())
    p = on_this_device(c, c["M"], c["N"], K, int(res))
    out = ops.rowlin(c["x"], c["stream"], c["N"], residual=c["residual"])
    ref32 = c["ref32"]
    rne = ref32.half()
    bad = int((out != rne).sum())
    rtz = int((out != R.round_toward_zero_f16(ref32)).sum())
    print(f"[parity] {c['what']}: {R.show(p)}; {bad} of {out.numel()} elements differ from round-to-nearest-even ({rtz} from round-toward-zero); "
          f"conditions {c['shares']}")
    assert bad == 0, f"{c['what']}: {bad} elements are not the fp32 value rounded to nearest even, worst {(out.float() - ref32).abs().max().item():.4g}"


# ------------------------------------------------------------------------------------------- 3. strides and guards
def guarded_out(M, N, ld):
    return R.window(M, N, ld, 8, dev(), guard=R.GUARD_ROWS)


@pytest.mark.parametrize("K", [320, 640])
@pytest.mark.parametrize("form", R.STRIDED_FORMS)
def test_strided_and_guarded(K, form):
    """x, out and residual as column windows of wider buffers (ldx = K + 8, ldo = N + 16, ldr = N + 24); out between sentinel rows and
    columns; the padding of the inputs is NaN."""
    from insv2v import ops
    N = R.N_MAIN
    c = R.form_case(K, N, "one_round", form, cus(), dev())
    p = on_this_device(c, c["M"], N, K, form)
    kw = dict(c["kw"])
    if kw["residual"] is not None:
        kw["residual"] = R.strided(kw["residual"], N + 24, 16)
    x = R.strided(c["x"], K + 8, 8)
    buf, out = guarded_out(c["M"], N, N + 16)
    assert (x.stride(0), out.stride(0)) == (K + 8, N + 16) and x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    ops.rowlin(x, c["stream"], N, out=out, **kw)
    worst = R.judge(out, c["ref"], c["blocks"], c["ln"], c["what"] + " strided")
    assert R.sentinels_intact(buf, c["M"], N, 8), f"{c['what']}: a sentinel beside the output window was overwritten"
    report(c["what"] + " strided", p, worst)
    assert torch.equal(out, ops.rowlin(c["x"], c["stream"], N, **c["kw"])), "the strided result differs from the contiguous one"


@pytest.mark.parametrize("K", [320, 640])
def test_strided_and_guarded_groupnorm(K):
    """The same for the GroupNorm-on-load form; its last sample is partial and every sample's last wave block has 8 real rows: the overhang
    rows of a block are never stored (they would land in the next sample's rows, or in the sentinel rows behind the last one)."""
    from insv2v import ops
    c = R.gn_case(K, "one_round", cus(), dev())
    N, M = c["N"], c["M"]
    p = on_this_device(c, M, N, K, gn_rows=R.GN_ROWS)
    x = R.strided(c["x"], K + 8, 8)
    buf, out = guarded_out(M, N, N + 16)
    ops.rowlin(x, c["stream"], N, out=out, gn_ab=c["ab"], gn_rows=R.GN_ROWS)
    worst = R.judge(out, c["ref"], c["blocks"], True, c["what"] + " strided")
    assert R.sentinels_intact(buf, M, N, 8), f"{c['what']}: a sentinel beside the output window was overwritten"
    report(c["what"] + " strided", p, worst)


# ------------------------------------------------------------------------------------------- 4. output statistics
@pytest.mark.parametrize("K,sched,form", R.STATS_CASES)
def test_output_statistics(K, sched, form):
    """stats_out: (mean, rsqrt(var + eps)) of the STORED fp16 rows against fp64; rows at or beyond M of the buffer stay untouched."""
    N = R.N_MAIN
    c = R.form_case(K, N, sched, form, cus(), dev())
    M = c["M"]
    p = on_this_device(c, M, N, K, form)
    out = torch.empty(M, N, dtype=torch.float16, device=dev())
    stats = torch.full((M + 64, 2), R.SENTINEL, dtype=torch.float32, device=dev())
    kw = {k: v for k, v in c["kw"].items()}
    assert launch_rowlin(c["x"], c["stream"], out, N, stats=stats, **kw) == 0
    worst = R.judge(out, c["ref"], c["blocks"], c["ln"], c["what"] + " with stats_out")
    R.stats_conditions(c["ref"], c["what"])
    want = R.stats_ref(out)
    ratio = 0.0
    for name, rs, _ in [("whole output", slice(0, M), None)] + c["blocks"][:-1]:
        for j, col in enumerate(("mean", "rstd")):
            err, tol = (stats[:M][rs, j].double() - want[rs, j]).abs().max().item(), R.stats_tol(want[rs, j])
            assert err == err and err <= tol, f"{c['what']}, {col} of {name}: max err {err:.4g} > tol {tol:.4g}"
            ratio = max(ratio, err / tol)
    assert bool((stats[M:] == R.SENTINEL).all()), f"{c['what']}: statistics rows at or beyond M were written"
    report(c["what"] + " with stats_out", p, worst)
    print(f"[parity] {c['what']}: output-row statistics at {ratio:.2e} of their tolerance")


# ------------------------------------------------------------------------------------------- 5. TB = 1 against TB = 2
@pytest.mark.parametrize("form", R.TB12_FORMS)
def test_two_token_blocks_against_one(form):
    """The last 512 rows of the tb2 case as a problem of their own run ONE token block per wave (the plan says so): the two kernels
    differ in schedule only, so the results agree within one fp16 rounding step per element (bit-identical is expected, and printed)."""
    from insv2v import ops
    K, N = 640, R.N_MAIN
    c = R.form_case(K, N, "tb2", form, cus(), dev())
    M = c["M"]
    p2 = on_this_device(c, M, N, K, form)
    p1 = R.plan(R.TB12_ROWS, N, K, form, cus=0)
    assert p2.token_blocks == 2 and p1.rc == 0 and p1.token_blocks == 1 and p1.rounds == 1, f"{R.show(p2)} / {R.show(p1)}"
    two = ops.rowlin(c["x"], c["stream"], N, **c["kw"])[M - R.TB12_ROWS:]
    kw = dict(c["kw"])
    if kw["residual"] is not None:
        kw["residual"] = kw["residual"][M - R.TB12_ROWS:].contiguous()
    one = ops.rowlin(c["x"][M - R.TB12_ROWS:].contiguous(), c["stream"], N, **kw)
    R.judge(one, c["ref"][M - R.TB12_ROWS:], [], c["ln"], c["what"] + " tail at TB = 1")
    one_ulp_close(two, one, c["what"] + ": TB = 2 against TB = 1")
    ndiff = int((two != one).sum())
    print(f"[parity] {c['what']}: {R.show(p2)} against {R.show(p1)} on the last {R.TB12_ROWS} rows: "
          + ("bit-identical" if ndiff == 0 else f"{ndiff} elements differ, all within one fp16 rounding step"))


# ------------------------------------------------------------------------------------------- 6. GroupNorm on load
@pytest.mark.parametrize("K,sched", R.GN_CASES)
def test_groupnorm_on_load(K, sched):
    from insv2v import ops
    c = R.gn_case(K, sched, cus(), dev())
    p = on_this_device(c, c["M"], c["N"], K, gn_rows=R.GN_ROWS)
    out = ops.rowlin(c["x"], c["stream"], c["N"], gn_ab=c["ab"], gn_rows=R.GN_ROWS)
    worst = R.judge(out, c["ref"], c["blocks"], True, c["what"])
    report(c["what"], p, worst)
    assert torch.equal(out, ops.rowlin(c["x"], c["stream"], c["N"], gn_ab=c["ab"], gn_rows=R.GN_ROWS)), f"{c['what']}: not deterministic"


# ------------------------------------------------------------------------------------------- 7. insv2v_ffn_fused
@pytest.mark.parametrize("post", [False, True])
def test_ffn_fused(post):
    """Strided (ldx, ldo, ld_post = C + 8) and guarded operands, judged on the ragged last tile and the first and last 32 channels."""
    from insv2v import ops
    c = R.ffn_case(post, dev())
    M, C = c["M"], c["C"]
    x = R.strided(c["x"], C + 8, 8)
    r2 = R.strided(c["post_residual"], C + 8, 0) if post else None
    buf, out = R.window(M, C, C + 8, 0, dev(), guard=R.GUARD_ROWS)
    ops.ffn_fused(x, c["stream"], c["NH"], eps=R.EPS, out=out, post_residual=r2)
    worst = R.judge(out, c["ref"], c["blocks"], True, c["what"])
    assert R.sentinels_intact(buf, M, C, 0), f"{c['what']}: a sentinel beside the output window was overwritten"
    print(f"[parity] {c['what']}: ffn_fused_kernel<POST={int(post)}>; worst block '{worst[1]}' at {worst[0]:.3f} of its tolerance")
    assert torch.equal(out, ops.ffn_fused(c["x"], c["stream"], c["NH"], eps=R.EPS, post_residual=c["post_residual"])), "strided / contiguous or two runs differ"


# ------------------------------------------------------------------------------------------- 8. refusals against the real entry
@pytest.mark.parametrize("name,rc,kw", R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_refusals(name, rc, kw):
    """insv2v_rowlin returns exactly the plan's rc (the documented one) and writes nothing."""
    from insv2v import _lib
    lib = _lib.load()
    d, out, keep = R.refusal_desc(kw, dev())
    p = _lib.RowLinPlan()
    assert lib.insv2v_rowlin_plan(ctypes.byref(d), 0, ctypes.byref(p)) == 0
    got = lib.insv2v_rowlin(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert got == p.rc == rc, f"{name}: insv2v_rowlin returned {got}, the plan says {p.rc}, documented {rc}"
    assert bool((out == R.SENTINEL).all()), f"{name}: a refused call wrote to its output"
    del keep


def test_refusal_base_is_accepted():
    """The problem every refusal varies runs (so that each refusal is due to its one argument)."""
    from insv2v import _lib
    for kw in ({}, dict(form=7), dict(gn_rows=R.GN_ROWS)):
        d, out, keep = R.refusal_desc(kw, dev())
        assert _lib.load().insv2v_rowlin(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0, kw
        torch.cuda.synchronize()
        M, N, _ = R.REFUSAL_SHAPE
        assert bool((out.reshape(-1)[:M * N] != R.SENTINEL).all()), kw
