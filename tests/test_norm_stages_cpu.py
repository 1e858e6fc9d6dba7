"""What tests/test_norm_stages_gpu.py rests on, checked without a GPU.

  * The dispatch of insv2v_groupnorm through insv2v_groupnorm_plan (csrc/norm_plan.h): the plan of every GroupNorm case of the GPU file is
    pinned (a case that drifts to another kernel fails HERE, with a message that says so), and a sweep checks the planner's invariants -
    under the INSV2V_GN_FRAME_SPLIT overrides 1, 2, 4, 8 too, one CPU-only child process per value because the switch is read once.
  * The power of the case lists: every mutation of tests/norm_ref.py violates the GPU file's bounds on at least one listed case.
  * The headroom of the bounds: a plain fp32 evaluation of the same formulas, rounded to fp16 where the kernels round, in sequential and
    in pairwise order, satisfies every bound on every case; the constants K of norm_ref.py are 8 x its worst K = 1 ratio, rounded up to a
    power of two."""
import math
import os
import subprocess
import sys

import pytest
import torch

import norm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------------------------------------------- planner corpus
def test_plan_of_every_case():
    for case in R.GN_CASES:
        p = R.check_case_plan(case)
        if p.family == R.THREE_PASS:        # the same tensor with stats_only: passes 1 and 2 of the same plan, no apply launch
            q = R.plan(R.case_desc(case, stats_only=1, ab=True))
            assert q.rc == 0 and R.plan_tuple(q) == case["plan"][:7] + (0,), (case["name"], R.describe(R.plan_tuple(q)))
        assert p.threads == {R.THREE_PASS: case["C"] // 8 * p.p, R.SMALL: 256, R.FRAME: p.nt}[p.family]
    for key, cases in R.GN_FORCED.items():  # without the switch the forced tensors run the product's kernel: gn_frame<256>
        for case in cases:
            p = R.plan(R.case_desc(case))
            assert (p.rc, p.family, p.nt) == (0, R.FRAME, 256), (key, case["name"])
    seen = {R.plan_tuple(R.plan(R.case_desc(c)))[:5] for c in R.GN_CASES}
    assert {(R.SMALL, 0, 0, 8, 0), (R.SMALL, 0, 0, 4, 0), (R.FRAME, 256, 1, 0, 0), (R.FRAME, 256, 2, 0, 0), (R.FRAME, 256, 4, 0, 0)} <= seen
    assert {t[4] for t in seen if t[0] == R.THREE_PASS} >= {1, 2, 3, 6, 10, 16}


def test_plan_of_every_refusal():
    for what, over, rc in R.GN_REFUSALS:
        p = R.plan(R.gn_desc(**{**dict(ns=2, rows=16, C=64, G=32, nchunks=1), **over}))
        assert (p.rc, p.family) == (rc, R.NONE), (what, p.rc, p.family)
        assert R.plan_tuple(p)[1:] == (0,) * 7 and p.threads == 0 and p.lds_bytes == 0, what
    assert R.plan(R.gn_desc(2, 16, 64, 32, 1)).rc == 0                      # the call the refusals vary is valid
    import ctypes
    from insv2v import _lib
    lib = _lib.load()
    assert lib.insv2v_groupnorm_plan(None, ctypes.byref(_lib.GroupNormPlan())) == R.EINVAL
    assert lib.insv2v_groupnorm_plan(ctypes.byref(R.gn_desc(2, 16, 64, 32, 1)), None) == R.EINVAL


# ---------------------------------------------------------------------------------------------------------------- planner sweep
SWEEP_NS = (1, 127, 128, 4096, 4097)
SWEEP_C = (8, 64, 320, 384, 640, 1280, 2048, 2560, 4096, 5464, 8192)
SWEEP_G = (1, 8, 16, 32)


def check_invariants(d, p, split):
    ns, rows, C, G = d.nsamples, d.rows_per_sample, d.C, d.G
    what = f"ns {ns} rows {rows} C {C} G {G} x2 {bool(d.x2)} stats_only {d.stats_only} split {split}: {R.describe(R.plan_tuple(p))}"
    assert (p.rc == 0) == (p.family != R.NONE), what
    assert p.rc in (0, R.EINVAL, R.EUNSUPPORTED), what
    if p.rc:
        return
    cpg = C // G
    assert 0 < p.threads <= 1024, what
    assert p.nchunks >= 1 and p.nchunks * p.rows_per_chunk >= rows, what
    if p.family == R.FRAME:
        nchunk = rows * (C // 8)
        assert not d.stats_only and not d.x2 and ns >= 128 and 2048 <= nchunk <= 15360, what
        assert p.cs >= 1 and G % p.cs == 0 and p.nt in (256, 512, 1024) and p.threads == p.nt, what
        gw = G // p.cs
        tpg = p.nt // gw
        assert p.nt % gw == 0 and tpg <= 64 and tpg & (tpg - 1) == 0, what          # the kernel's reduction contract
        assert nchunk % p.cs == 0 and nchunk // p.cs <= p.nt * 15, what
        assert p.lds_bytes == 4 * (nchunk // p.cs + 2 * gw + 2 * (C // p.cs)) <= 96 * 1024, what
        assert p.apply_grid_x == ns, what
    elif p.family == R.SMALL:
        assert not d.stats_only and p.vw in (4, 8) and cpg % p.vw == 0 and 16 <= cpg <= 256, what
        assert rows * cpg // p.vw <= 4096 and p.threads == 256 and p.lds_bytes == 2080 and p.apply_grid_x == G, what
        assert not d.x2 or d.C1 % p.vw == 0, what
    else:
        assert p.family == R.THREE_PASS and p.p == max(1, min(16, 256 // (C // 8))) and p.threads == C // 8 * p.p, what
        assert p.lds_bytes == 12 * p.p * C <= 64 * 1024, what
        assert p.nchunks == min(d.nchunks, rows) and p.rows_per_chunk == -(-rows // p.nchunks), what
        want = 0 if d.stats_only else min(-(-rows // (4 * p.p)), max(1, 4096 // ns))
        assert p.apply_grid_x == want and (d.stats_only or p.apply_grid_x * ns <= max(4096, ns)), what


def sweep(split=0):
    """The planner's invariants over the sweep; with split > 0 (a child process with INSV2V_GN_FRAME_SPLIT set) what the override must and
    must not do as well.  Returns the number of plans per family."""
    assert int(os.environ.get("INSV2V_GN_FRAME_SPLIT", "0")) == split
    count = {f: 0 for f in R.FAMILY_NAMES}
    for C in SWEEP_C:
        for G in SWEEP_G:
            if C % G:
                continue
            C1 = C // 2 // 8 * 8
            for ns in SWEEP_NS:
                for rows in range(1, 201):
                    for x2 in ((False, True) if C1 else (False,)):
                        for stats_only in (0, 1):
                            d = R.gn_desc(ns, rows, C, G, R.default_nchunks(ns, rows), C1 if x2 else 0, stats_only, ab=bool(stats_only))
                            p = R.plan(d)
                            check_invariants(d, p, split)
                            count[p.family] += 1
                            if C in (5464, 8192):
                                assert p.rc == (R.EUNSUPPORTED if p.family == R.NONE else 0)
    assert all(count.values()), count
    if split:
        for G, want in ((32, min(split, 8)), (16, min(split, 4))):      # 128 x 96 x 1280: 15360 chunks.  G = 16 in 8 parts would be 128 threads per group
            p = R.plan(R.gn_desc(128, 96, 1280, G, 1))
            assert (p.family, p.cs) == (R.FRAME, want), (G, split, R.describe(R.plan_tuple(p)))
        p = R.plan(R.gn_desc(128, 52, 640, 16, 1))                      # 4160 chunks: at least 1024 per part
        assert (p.family, p.cs, p.nt) == (R.FRAME, min(split, 4), 512 if split == 1 else 256)
    return count


def test_plan_sweep_invariants():
    count = sweep(0)
    print("[plan] sweep: " + ", ".join(f"{R.FAMILY_NAMES[f]} {n}" for f, n in count.items()))


@pytest.mark.parametrize("split", [1, 2, 4, 8])
def test_plan_sweep_invariants_under_split_override(split):
    env = dict(os.environ, INSV2V_GN_FRAME_SPLIT=str(split))
    r = subprocess.run([sys.executable, "-c", f"import conftest, test_norm_stages_cpu as t; print(t.sweep({split}))"], cwd=HERE, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------- case lists and bounds
def gn_eval(case, gen, eps, silu_on, got_fn, ks=None):
    """{output: ratio} of got_fn(data) against the float64 reference of one GroupNorm case, under the bounds of the kernel that runs it
    (ks: one such dict per set of constants K)."""
    x, x2, gamma, beta = data = R.gn_case_data(case["ns"], case["rows"], case["C"], case["G"], gen, case["C1"])
    ns, rows, G = case["ns"], case["rows"], case["G"]
    ref = R.groupnorm_ref(x, x2, ns, rows, G, gamma, beta, eps, silu_on)
    X = R.gn_join(x, x2).reshape(ns, rows, -1)
    family = case["plan"][0]
    outputs = ("y", "mean", "rstd", "ab") if family == R.THREE_PASS else ("y",)     # what the kernel writes
    got = got_fn(data)
    out = [R.gn_ratios(got, ref, R.gn_bounds(X, G, gamma, beta, eps, silu_on, ref, R.gn_centre(family), k), outputs) for k in (ks or [None])]
    return out if ks else out[0]


def ln_items():
    for C in R.LN_CS:
        for rows in R.LN_ROWS:
            for gen in R.LN_GENERATORS:
                yield C, rows, gen, None
    for C in R.LN_PE_CS:
        for rpf, frames, samples in R.LN_PE_CASES:
            for pe_start in (0, R.PE_MAX_LEN - frames):
                yield C, rpf * frames * samples, "offset", (rpf, frames, pe_start)


def ln_eval(C, rows, gen, pe_case, got_fn, ks=None):
    x, gamma, beta = R.ln_case_data(rows, C, gen)
    pe, kw = None, {}
    if pe_case:
        rpf, frames, pe_start = pe_case
        pe, kw = R.pe_table(C, frames, pe_start), dict(rows_per_frame=rpf, frames=frames, pe_start=pe_start)
    ref = R.layernorm_ref(x, gamma, beta, R.LN_EPS, pe, **kw)
    pe_r = R.pe_rows(pe, rows, **kw) if pe_case else None
    got = got_fn(x, gamma, beta, pe, kw, pe_r)
    out = [R.ln_ratios(got, ref, R.ln_bounds(x, gamma, ref, R.LN_EPS, pe_r, k)) for k in (ks or [None])]
    return out if ks else out[0]


def sm_items():
    for cols in R.SM_COLS:
        for rows in R.SM_ROWS:
            for scale in R.SM_SCALES:
                for valid in R.sm_valids(cols):
                    yield rows, cols, scale, valid


@pytest.mark.parametrize("mutate", R.MUTATIONS_GN)
def test_groupnorm_mutations_are_caught(mutate):
    caught = []
    for case in R.GN_CASES:
        if case["ns"] * case["rows"] * case["C"] > 3_000_000 or case["ns"] > 200:        # (the slow per-slab loop of the mutated reference)
            continue
        if mutate == "x2_column" and not case["C1"]:
            continue
        for gen in R.GN_GENERATORS:
            eps, silu_on = R.gn_combos(case)[0]
            r = gn_eval(case, gen, eps, silu_on, lambda d: R.groupnorm_ref(d[0], d[1], case["ns"], case["rows"], case["G"], d[2], d[3], eps, silu_on, mutate))
            caught += [(case["name"], gen, k, v) for k, v in r.items() if not v <= 1]
    by_family = {f: sorted({c[0] for c in caught if c[0] in {x["name"] for x in R.GN_CASES if x["plan"][0] == f}}) for f in (R.THREE_PASS, R.SMALL, R.FRAME)}
    print(f"[power] GroupNorm {mutate}: caught on " + "; ".join(f"{R.FAMILY_NAMES[f]}: {', '.join(v) or '-'}" for f, v in by_family.items()))
    assert caught, f"no listed GroupNorm case notices `{mutate}`"
    if mutate != "eps_outside":       # (eps outside the root moves y by less than fp16 resolves unless var ~ eps: only the statistics outputs can see it)
        assert any(c[2] == "y" for c in caught) and (by_family[R.SMALL] or by_family[R.FRAME]), f"`{mutate}` is not seen through y alone"


@pytest.mark.parametrize("mutate", R.MUTATIONS_LN)
def test_layernorm_mutations_are_caught(mutate):
    caught = []
    for C, rows, gen, pe_case in ln_items():
        r = ln_eval(C, rows, gen, pe_case, lambda x, g, b, pe, kw, pe_r: R.layernorm_ref(x, g, b, R.LN_EPS, pe, mutate=mutate, **kw))
        caught += [(C, rows, gen, pe_case, k) for k, v in r.items() if not v <= 1]
    print(f"[power] LayerNorm {mutate}: caught on {len(caught)} (case, output) pairs, first {caught[:1]}")
    assert caught, f"no listed LayerNorm case notices `{mutate}`"


@pytest.mark.parametrize("mutate", R.MUTATIONS_SM)
def test_softmax_mutations_are_caught(mutate):
    caught = []
    for rows, cols, scale, valid in sm_items():
        x = R.sm_case_data(rows, cols, valid)
        ref = R.softmax_ref(x, scale, valid)
        if not R.ratio(R.softmax_ref(x, scale, valid, mutate), ref, R.sm_bound(ref, cols)) <= 1:
            caught.append((rows, cols, scale, valid))
    print(f"[power] softmax {mutate}: caught on {len(caught)} cases, first {caught[:1]}")
    assert caught, f"no listed softmax case notices `{mutate}`"


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


def test_headroom_of_the_bounds():
    """The fp32 restatement against every bound with K = 1 (the ratios that define K) and with K (every ratio <= 1)."""
    one = dict.fromkeys(R.K, 1.0)
    worst1, worstk, where = {}, {}, {}

    def note(family, r1, rk, what):
        for expr in r1:
            key = (family, expr)
            if r1[expr] > worst1.get(key, -1):
                worst1[key], where[key] = r1[expr], what
            worstk[key] = max(worstk.get(key, 0), rk[expr])

    for order in ("sequential", "pairwise"):
        for case in R.GN_CASES:
            family = case["plan"][0]
            for gen in R.GN_GENERATORS:
                for eps, silu_on in R.gn_combos(case):
                    fn = lambda d: R.groupnorm_fp32(d[0], d[1], case["ns"], case["rows"], case["G"], d[2], d[3], eps, silu_on, R.gn_centre(family), order)
                    r1, rk = gn_eval(case, gen, eps, silu_on, fn, [one, R.K])
                    note("GroupNorm " + R.FAMILY_NAMES[family], r1, rk, f"{case['name']} {gen} eps {eps} silu {silu_on} {order}")
        for C, rows, gen, pe_case in ln_items():
            fn = lambda x, g, b, pe, kw, pe_r: R.layernorm_fp32(x, g, b, R.LN_EPS, pe_r, order)
            r1, rk = ln_eval(C, rows, gen, pe_case, fn, [one, R.K])
            note("LayerNorm", r1, rk, f"C {C} rows {rows} {gen} pe {pe_case} {order}")
        for rows, cols, scale, valid in sm_items():
            x = R.sm_case_data(rows, cols, valid)
            ref, got = R.softmax_ref(x, scale, valid), R.softmax_fp32(x, scale, valid, order)
            note("softmax", {"softmax": R.ratio(got, ref, R.sm_bound(ref, cols, one))}, {"softmax": R.ratio(got, ref, R.sm_bound(ref, cols, R.K))},
                 f"{rows} x {cols} valid {valid} scale {scale:g} {order}")
    for key in sorted(worst1):
        kk = f"with K = {R.K[key[1]]:g}" if key[1] in R.K else "with those K"
        print(f"[headroom] {key[0]:22s} {key[1]:8s} worst ratio at K = 1: {worst1[key]:9.4g}   {kk}: {worstk[key]:.4g}   ({where[key]})")
    for expr in R.K:      # (ab has no constant of its own: its bound is the mean's and the rstd's, propagated)
        w = max(v for (f, e), v in worst1.items() if e == expr)
        print(f"[headroom] {expr}: worst ratio {w:.4g} -> K = {pow2_ceil(8 * w):g} (norm_ref.K: {R.K[expr]:g})")
    for expr in R.K:
        w = max(v for (f, e), v in worst1.items() if e == expr)
        assert R.K[expr] == pow2_ceil(8 * w), f"norm_ref.K['{expr}'] = {R.K[expr]:g} is not 8 x {w:.4g} rounded up to a power of two"
        assert abs(R.K_MEASURED[expr] / w - 1) < 0.25, f"norm_ref.K_MEASURED['{expr}'] = {R.K_MEASURED[expr]} but the worst ratio is {w:.4g}"
    assert all(v <= 1 for v in worstk.values()), {k: v for k, v in worstk.items() if not v <= 1}
