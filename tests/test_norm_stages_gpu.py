"""Stage-level parity of csrc/norm.hip: gn_partial / gn_finalize / gn_apply, gn_small<8|4>, gn_frame<256|512|1024>, layernorm<1..4>,
ln_stats<1..4> and softmax_rows<PAD>, each called through the C ABI on its own against the float64 restatements of tests/norm_ref.py.

Which kernel a case runs is not assumed: every GroupNorm descriptor is planned with insv2v_groupnorm_plan first and the plan must be the one
norm_ref's case table pins (tests/test_norm_stages_cpu.py pins the same table without a GPU, so a case that drifts to another kernel fails
there first).  The table holds, for every dispatch threshold, a case on either side of it.

Every strided operand is a column view of a wider NaN-framed buffer (ldx, ldx2 and ldy all differ from the widths and from each other);
y, `partials`, `ab` and `stats` lie in sentinel buffers with guard rows and columns: what must be written is written, nothing else is.

Bounds (norm_ref's docstring has the expressions).  The constants are 8 x the worst ratio of a plain fp32 evaluation to the expression
with K = 1 over all the cases below, rounded up to a power of two (test_norm_stages_cpu.py::test_headroom_of_the_bounds):
    y        worst ratio 2.109 (three-pass cpg-80, constant group, sequential sums)       K = 32
    softmax  worst ratio 0.5   (the final rounding alone)                                 K = 4
    mean     worst ratio 3.621 (three-pass lds-48k, offset inputs, sequential sums)       K = 32
    rstd     worst ratio 1.155 (three-pass empty-chunks, offset inputs, sequential sums)  K = 16
Every line printed below is the worst |out - ref| / bound of its outputs: <= 1 passes.  Nothing is compared with another kernel."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch

import norm_ref as R
from test_flow_stages_gpu import DEV, F64, check_out16, check_out32, in32, is_sent16, is_sent32, lib, nan_framed, ok, out16, out32, sentinel16, stream

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def report(what, ratios, extra=""):
    print(f"[parity] {what}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()) + f" of the bound (<= 1 passes){extra}")
    bad = {k: v for k, v in ratios.items() if not (math.isfinite(v) and v <= 1)}
    assert not bad, f"{what}: beyond the bound: {bad}"


def worse(into, ratios):
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)


# ---------------------------------------------------------------------------------------------------------------- GroupNorm
def run_gn(case, data, eps, silu_on, stats_only=False, ns=None, expect=None):
    """One insv2v_groupnorm call on the case's tensor (its first `ns` samples).  Returns dict(y16 = the fp16 output on the GPU, y, mean, rstd,
    ab = float64 on the CPU or None where the planned kernel writes none, plan)."""
    from insv2v import _lib
    x64, x264, gamma64, beta64 = data
    ns, rows, C, G = ns or case["ns"], case["rows"], case["C"], case["G"]
    n = ns * rows
    x = nan_framed(x64[:n], 8, 16)
    gamma, beta = in32(gamma64.float()), in32(beta64.float())
    d = _lib.GroupNormDesc()
    d.x, d.gamma, d.beta, d.ldx = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), x.stride(0)
    if x264 is not None:
        x2 = nan_framed(x264[:n], 16, 32)
        d.x2, d.ldx2, d.C1 = x2.data_ptr(), x2.stride(0), case["C1"]
    d.nsamples, d.rows_per_sample, d.C, d.G, d.nchunks, d.silu, d.eps, d.stats_only = ns, rows, C, G, case["nchunks"], int(silu_on), eps, int(stats_only)
    if not stats_only:
        ybuf, y = out16(n, C, 16, 24)
        d.y, d.ldy = y.data_ptr(), y.stride(0)
        assert len({d.ldx, d.ldy, d.ldx2 or -1}) == 3 and d.ldx != x64.shape[1] and d.ldy != C
    if case["ab"] or stats_only:
        abbuf, ab = out32((ns, C, 2))
        d.ab = ab.data_ptr()
    part = torch.zeros(1, device=DEV)
    d.partials = part.data_ptr()                   # (the planner reads its null bit only)
    want = expect or (case["plan"][:7] + (0,) if stats_only else case["plan"])
    if ns == case["ns"] and expect is None and not stats_only:
        p = R.check_case_plan(case, d)
    else:
        p = R.plan(d)
        assert p.rc == 0 and R.plan_tuple(p) == want, f"{case['name']}: planned {R.describe(R.plan_tuple(p))}; expected {R.describe(want)}"
    pbuf, part = out32((ns * G * (2 + 3 * p.nchunks),))
    d.partials = part.data_ptr()
    ok(lib().insv2v_groupnorm(ctypes.byref(d), stream()), "insv2v_groupnorm")
    what = f"groupnorm {case['name']}"
    out = dict(plan=p, y16=None, y=None, mean=None, rstd=None, ab=None)
    if not stats_only:
        check_out16(ybuf, n, C, what, 16)
        out["y16"], out["y"] = y, y.cpu().to(F64)
    if p.family == R.THREE_PASS:
        check_out32(pbuf, part.numel(), what + " (partials)")
        head = part[:ns * G * 2].view(ns, G, 2).cpu().to(F64)
        out["mean"], out["rstd"] = head[..., 0], head[..., 1]
        if case["ab"] or stats_only:
            check_out32(abbuf, ab.numel(), what + " (ab)")
            out["ab"] = ab.cpu().to(F64)
    else:
        assert is_sent32(pbuf).all(), what + ": the single-launch kernels write no partials"
    return out


def gn_check(case, gens=R.GN_GENERATORS, expect=None, label=None):
    """The case's tensor from every generator, every (eps, silu) of the case, y and whatever statistics its kernel writes against float64;
    a three-pass case with stats_only as well.  One [parity] line per generator."""
    ns, rows, C, G = case["ns"], case["rows"], case["C"], case["G"]
    for gen in gens:
        data = R.gn_case_data(ns, rows, C, G, gen, case["C1"])
        X = R.gn_join(data[0], data[1]).reshape(ns, rows, C)
        moments = R.gn_moments_fast(X, G)
        worst, plan = {}, None
        for eps, silu_on in R.gn_combos(case):
            ref = R.groupnorm_ref(data[0], data[1], ns, rows, G, data[2], data[3], eps, silu_on, moments=moments)
            got = run_gn(case, data, eps, silu_on, expect=expect)
            plan = got["plan"]
            bounds = R.gn_bounds(X, G, data[2], data[3], eps, silu_on, ref, R.gn_centre(plan.family))
            assert torch.isfinite(got["y"]).all()
            worse(worst, R.gn_ratios((got["y"], got["mean"], got["rstd"], got["ab"]), ref, bounds))
            if plan.family == R.THREE_PASS and case["ab"] and silu_on:          # (the statistics do not depend on silu: once per eps)
                st = run_gn(case, data, eps, 0, stats_only=True)
                worse(worst, {k + " (stats_only)": v for k, v in R.gn_ratios((None, st["mean"], st["rstd"], st["ab"]), ref, bounds).items()})
        report(f"groupnorm {label or case['name']} {ns} x {rows} x {C} G {G} [{R.describe(R.plan_tuple(plan))}] {gen}", worst)


def by_name(cases):
    return pytest.mark.parametrize("case", cases, ids=[c["name"] for c in cases])


@by_name(R.GN_THREE_PASS)
def test_groupnorm_three_pass(case):
    """gn_partial / gn_finalize / gn_apply: y, the (mean, rstd) header and ab, and header and ab again with stats_only."""
    gn_check(case)


@by_name(R.GN_SMALL)
def test_groupnorm_small_slab(case):
    """gn_small<8> and <4> at their limits, with the neighbours that just miss them (planned THREE_PASS: y and header)."""
    gn_check(case)


def other_samples(data, rows):
    """The same tensor with every sample but the first replaced by other data."""
    x = data[0].clone()
    x[rows:] = (0.5 - x[rows:]).flip(0).half().to(F64)
    return (x,) + tuple(data[1:])


@by_name(R.GN_FRAME)
def test_groupnorm_frame(case):
    """gn_frame<256> with 1, 2 and 4 channel parts, and the cases that just miss it."""
    gn_check(case)


@by_name(R.GN_FRAME)
def test_groupnorm_frame_samples_are_independent(case):
    """Sample 0's rows stay bit-identical when every other sample holds other data."""
    eps, silu_on = R.gn_combos(case)[0]
    data = R.gn_case_data(case["ns"], case["rows"], case["C"], case["G"], "benign")
    a = run_gn(case, data, eps, silu_on)["y16"][:case["rows"]].clone()
    b = run_gn(case, other_samples(data, case["rows"]), eps, silu_on)["y16"][:case["rows"]]
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"groupnorm {case['name']}: sample 0 changed with the other samples"


def test_groupnorm_one_sample_short_of_the_frame_kernel():
    """The first 127 samples of the cs1 tensor run gn_small, and every one of them still meets ITS rows of the 128-sample float64 reference
    (a sample's result does not depend on how many samples there are; no kernel is compared with another)."""
    case = R.GN_FRAME[0]
    ns, rows, C, G = case["ns"], case["rows"], case["C"], case["G"]
    data = R.gn_case_data(ns, rows, C, G, "benign")
    eps, silu_on = R.gn_combos(case)[0]
    ref = R.groupnorm_ref(data[0], None, ns, rows, G, data[2], data[3], eps, silu_on)
    X = data[0].reshape(ns, rows, C)
    by = R.gn_bounds(X, G, data[2], data[3], eps, silu_on, ref, "mean")["y"]
    short = next(c for c in R.GN_FRAME if c["name"] == "127-samples")
    got = run_gn(short, data, eps, silu_on)
    assert got["plan"].family == R.SMALL
    report("groupnorm 127 of the 128 samples of cs1 [SMALL] against rows 0..126 of the 128-sample reference", {"y": R.ratio(got["y"], ref[0][:127 * rows], by[:127 * rows])})


def forced_child(switch, value):
    """Runs in a child process whose environment sets `switch`: the listed tensors through the forced form, plan asserted."""
    assert os.environ.get(switch) == value
    for case in R.GN_FORCED[(switch, value)]:
        gn_check(case, label=f"{switch}={value} {case['name']}")
    print("forced child done")


@pytest.mark.parametrize("switch,value", list(R.GN_FORCED), ids=["=".join(k) for k in R.GN_FORCED])
def test_groupnorm_forced_forms(switch, value):
    """gn_frame<512> and <1024> (INSV2V_GN_FRAME_SPLIT=1: one workgroup per sample) and the fallback without the whole-sample kernel
    (INSV2V_GN_FRAME=0): one child process each with the switch in ITS environment, its own time limit, one after the other; a child that
    does not end with status 0 fails the test with its stderr."""
    env = dict(os.environ, **{switch: value})
    code = f"import conftest, test_norm_stages_gpu as t; t.forced_child({switch!r}, {value!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=HERE, env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout, end="")
    assert r.returncode == 0 and "forced child done" in r.stdout, f"{switch}={value}: exit status {r.returncode}\n{r.stderr[-4000:]}"


def test_groupnorm_refusals():
    """Every refusal returns its code, the plan agrees (rc, family NONE) and nothing is written."""
    from insv2v import _lib
    x = torch.zeros((32, 8192 + 24), dtype=torch.float16, device=DEV)
    gb = torch.ones((8192,), dtype=torch.float32, device=DEV)

    def call(y, part, ab, **over):
        v = dict(C=64, G=32, ldx=x.stride(0), ldx2=x.stride(0), ldy=y.stride(0), nchunks=1, stats_only=0, C1=0)
        v.update(over)
        d = _lib.GroupNormDesc()
        d.x, d.y, d.gamma, d.beta, d.partials = x.data_ptr(), y.data_ptr(), gb.data_ptr(), gb.data_ptr(), part.data_ptr()
        if v["C1"]:
            d.x2 = x.data_ptr()
        if not v["stats_only"]:
            d.ab = ab.data_ptr()
        d.nsamples, d.rows_per_sample, d.eps = 2, 16, 1e-5
        for k, val in v.items():
            setattr(d, k, val)
        return lib().insv2v_groupnorm(ctypes.byref(d), stream()), R.plan(d)

    zero = (torch.zeros((32, 8192 + 40), dtype=torch.float16, device=DEV), torch.zeros((2 * 32 * 5,), device=DEV), torch.zeros((2 * 8192 * 2,), device=DEV))
    rc, p = call(*zero)
    assert rc == 0 and p.rc == 0 and p.family == R.THREE_PASS          # the call the refusals vary is valid
    sent = (sentinel16(32, 8192 + 40), out32((2 * 32 * 5,))[0], out32((2 * 8192 * 2,))[0])
    for what, over, want in R.GN_REFUSALS:
        rc, p = call(*sent, **over)
        assert rc == want and (p.rc, p.family) == (want, R.NONE), (what, rc, p.rc, p.family)
    torch.cuda.synchronize()
    assert is_sent16(sent[0]).all() and is_sent32(sent[1]).all() and is_sent32(sent[2]).all(), "a refused call wrote to one of its buffers"


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def run_ln(x64, gamma64, beta64, pe64=None, kw=None):
    """insv2v_layernorm and insv2v_layernorm_stats on one tensor -> (y fp16 on the CPU, mean, rstd float64)."""
    from insv2v import _lib
    rows, C = x64.shape
    x = nan_framed(x64, 8, 16)
    ybuf, y = out16(rows, C, 16, 24)
    gamma, beta = in32(gamma64.float()), in32(beta64.float())
    d = _lib.LayerNormDesc()
    d.x, d.y, d.gamma, d.beta, d.ldx, d.ldy, d.rows, d.C, d.eps = x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), x.stride(0), y.stride(0), rows, C, R.LN_EPS
    if pe64 is not None:
        pe = in32(pe64.float())                   # NaN outside rows [pe_start, pe_start + frames) and around the table
        d.pe, d.rows_per_frame, d.frames, d.pe_start = pe.data_ptr(), kw["rows_per_frame"], kw["frames"], kw["pe_start"]
    assert d.ldx == C + 24 and d.ldy == C + 40
    ok(lib().insv2v_layernorm(ctypes.byref(d), stream()), "insv2v_layernorm")
    check_out16(ybuf, rows, C, f"layernorm {rows} x {C}", 16)
    sbuf, st = out32((rows, 2))
    ok(lib().insv2v_layernorm_stats(x.data_ptr(), st.data_ptr(), x.stride(0), rows, C, R.LN_EPS, stream()), "insv2v_layernorm_stats")
    check_out32(sbuf, 2 * rows, f"layernorm_stats {rows} x {C}")       # rows at and beyond `rows` keep the sentinel
    st = st.cpu().to(F64)
    return y.cpu(), st[:, 0], st[:, 1]


@pytest.mark.parametrize("C", R.LN_CS)
def test_layernorm_and_stats(C):
    """layernorm<NCH> and ln_stats<NCH> on either side of every NCH boundary, rows that fill and do not fill the 4-row waves and the
    16-row workgroups; constant rows give fp16(beta) bit for bit."""
    worst = {}
    for rows in R.LN_ROWS:
        for gen in R.LN_GENERATORS:
            x, gamma, beta = R.ln_case_data(rows, C, gen)
            ref = R.layernorm_ref(x, gamma, beta, R.LN_EPS)
            y, mean, rstd = run_ln(x, gamma, beta)
            assert torch.isfinite(y).all()
            if gen == "constant":
                want = beta.float().half()[None].expand(rows, C)
                assert torch.equal(y, want), f"layernorm {rows} x {C}, constant rows: " + R.first_diff(y, want, ("row", "channel"))
            r = R.ln_ratios((y.to(F64), mean, rstd), ref, R.ln_bounds(x, gamma, ref, R.LN_EPS))
            worse(worst, r)
            assert all(v <= 1 for v in r.values()), (rows, C, gen, r)
    report(f"layernorm + layernorm_stats C {C} (NCH {(C // 8 + 63) // 64}), rows {R.LN_ROWS}, {R.LN_GENERATORS}", worst)


@pytest.mark.parametrize("C", R.LN_PE_CS)
def test_layernorm_positional_encoding(C):
    """y += pe[(row / rows_per_frame) % frames + pe_start]: every other row of the table, and what lies around it, is NaN."""
    worst = {}
    for rpf, frames, samples in R.LN_PE_CASES:
        for pe_start in (0, R.PE_MAX_LEN - frames):
            rows = rpf * frames * samples
            kw = dict(rows_per_frame=rpf, frames=frames, pe_start=pe_start)
            x, gamma, beta = R.ln_case_data(rows, C, "offset")
            pe = R.pe_table(C, frames, pe_start)
            ref = R.layernorm_ref(x, gamma, beta, R.LN_EPS, pe, **kw)
            y, mean, rstd = run_ln(x, gamma, beta, pe, kw)
            assert torch.isfinite(y).all(), f"rows_per_frame {rpf} frames {frames} pe_start {pe_start}: a row of pe outside the window was read"
            r = R.ln_ratios((y.to(F64), mean, rstd), ref, R.ln_bounds(x, gamma, ref, R.LN_EPS, R.pe_rows(pe, rows, **kw)))
            worse(worst, r)
            assert all(v <= 1 for v in r.values()), (kw, C, r)
    report(f"layernorm + pe C {C}, (rows_per_frame, frames, samples) {R.LN_PE_CASES}, pe_start 0 and max_len - frames", worst)


def test_layernorm_refusals():
    from insv2v import _lib
    x = torch.zeros((16, 2056 + 24), dtype=torch.float16, device=DEV)
    gb = torch.ones((2056,), dtype=torch.float32, device=DEV)
    y, st = sentinel16(16, 2056 + 40), out32((16, 2))[0]

    def call(yy, ss, C=64, ldx=x.stride(0)):
        d = _lib.LayerNormDesc()
        d.x, d.y, d.gamma, d.beta, d.ldx, d.ldy, d.rows, d.C, d.eps = x.data_ptr(), yy.data_ptr(), gb.data_ptr(), gb.data_ptr(), ldx, yy.stride(0), 16, C, 1e-5
        return lib().insv2v_layernorm(ctypes.byref(d), stream()), lib().insv2v_layernorm_stats(x.data_ptr(), ss.data_ptr(), ldx, 16, C, 1e-5, stream())
    assert call(torch.zeros_like(y), torch.zeros_like(st)) == (0, 0) and call(torch.zeros_like(y), torch.zeros_like(st), C=2048) == (0, 0)
    for kw in (dict(C=2056), dict(C=60), dict(ldx=2084)):
        assert call(y, st, **kw) == (R.EINVAL, R.EINVAL), kw
    torch.cuda.synchronize()
    assert is_sent16(y).all() and is_sent32(st).all(), "a refused call wrote to one of its buffers"


# ---------------------------------------------------------------------------------------------------------------- row softmax
def run_softmax(x64, scale, valid, inplace):
    """valid None: insv2v_softmax_rows; else insv2v_softmax_rows_padded.  Returns the fp16 output on the CPU."""
    rows, cols = x64.shape
    x = nan_framed(x64, 8, 16)
    if inplace:
        y, before = x, x._base.clone()
    else:
        buf, y = out16(rows, cols, 16, 24)
        assert x.stride(0) != y.stride(0)
    if valid is None:
        code = lib().insv2v_softmax_rows(x.data_ptr(), y.data_ptr(), x.stride(0), y.stride(0), rows, cols, scale, stream())
    else:
        code = lib().insv2v_softmax_rows_padded(x.data_ptr(), y.data_ptr(), x.stride(0), y.stride(0), rows, cols, valid, scale, stream())
    ok(code, "insv2v_softmax_rows" + ("_padded" if valid is not None else ""))
    if inplace:
        after = x._base
        assert torch.equal(after[:, :8].view(torch.int16), before[:, :8].view(torch.int16)) and \
            torch.equal(after[:, 8 + cols:].view(torch.int16), before[:, 8 + cols:].view(torch.int16)), "softmax in place wrote outside its columns"
    else:
        check_out16(buf, rows, cols, f"softmax {rows} x {cols}", 16)
    return y.cpu()


@pytest.mark.parametrize("cols", R.SM_COLS)
def test_softmax_rows(cols):
    """Both entries, in place and out of place; the padded entry with NaN and +-Inf in its pad columns."""
    worst, n = {}, 0
    for rows in R.SM_ROWS:
        for scale in R.SM_SCALES:
            for valid in [None] + R.sm_valids(cols):
                v = cols if valid is None else valid
                x = R.sm_case_data(rows, cols, v)
                ref = R.softmax_ref(x, scale, v)
                for inplace in (False, True):
                    y = run_softmax(x, scale, valid, inplace)
                    what = f"softmax {rows} x {cols} valid {valid} scale {scale:g} in place {inplace}"
                    assert torch.isfinite(y).all(), what
                    assert (y[:, v:].view(torch.int16) == 0).all(), what + ": pad columns must be +0"
                    out = y.to(F64)
                    r = R.ratio(out, ref, R.sm_bound(ref, cols))
                    s = (out[:, :v].sum(1) - 1).abs().max().item()
                    worse(worst, {"y": r, "|row sum - 1| / (cols 2^-11)": s / (cols * 2.0 ** -11)})
                    assert r <= 1 and s <= cols * 2.0 ** -11, (what, r, s)
                    for row in range(rows):
                        if R.SM_GENERATORS[row % 5] == "dominant" and scale > 0:
                            want = torch.zeros(cols, dtype=torch.float16)
                            want[(7 * row + 3) % v] = 1
                            assert torch.equal(y[row], want), what + ": a dominant element gives exactly 1, the others exactly 0"
                    n += 1
    report(f"softmax_rows and softmax_rows_padded, {cols} columns, rows {R.SM_ROWS}, scales 0 / 0.7 / 512^-0.5, valid {R.sm_valids(cols)}: {n} calls", worst)


def test_softmax_refusals():
    x = torch.zeros((4, 96 + 24), dtype=torch.float16, device=DEV)
    y = sentinel16(4, 96 + 40)
    st = stream()

    def plain(yy, cols=96, scale=1.0, ldx=x.stride(0)):
        return lib().insv2v_softmax_rows(x.data_ptr(), yy.data_ptr(), ldx, yy.stride(0), 4, cols, scale, st)

    def padded(yy, cols=96, valid=90, scale=1.0, ldx=x.stride(0), ldy=None):
        return lib().insv2v_softmax_rows_padded(x.data_ptr(), yy.data_ptr(), ldx, ldy or yy.stride(0), 4, cols, valid, scale, st)
    assert plain(torch.zeros_like(y)) == 0 and padded(torch.zeros_like(y)) == 0
    assert plain(y, scale=-1.0) == R.EINVAL and plain(y, cols=92) == R.EINVAL and plain(y, ldx=100) == R.EINVAL
    for kw in (dict(scale=-1.0), dict(valid=0), dict(valid=97), dict(ldx=88), dict(ldy=88), dict(cols=92, valid=90)):
        assert padded(y, **kw) == R.EINVAL, kw
    torch.cuda.synchronize()
    assert is_sent16(y).all(), "a refused call wrote to its output"
