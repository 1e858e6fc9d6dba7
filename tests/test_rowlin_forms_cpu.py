"""The part of the row-Linear parity tests (tests/test_rowlin_forms_gpu.py) that needs no GPU:
  * the dispatch of insv2v_rowlin through insv2v_rowlin_plan (csrc/rows_plan.h): the plan of every launch of the GPU file is pinned at a
    fixed CU count (a case that drifts to another kernel fails here, naming both kernels), the case list reaches all 26 rowlin_kernel
    instantiations and a second round on every schedule, the planner's invariants hold over a sweep, every refusal gets the rc that
    insv2v_rowlin documents, and INSV2V_ROWLIN_TB2=0 (read once per process: a child process) turns every plan to one token block;
  * the conditions the builders of tests/rows_ref.py put on their own inputs (need_gap and the exact case's shares), on the CPU at a small
    CU count so that the large cases stay small."""
import os
import subprocess
import sys

import pytest
import torch

import rows_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
CPU = torch.device("cpu")
SMALL_CUS = 4


# ------------------------------------------------------------------------------------------- pinned plans and coverage
@pytest.mark.parametrize("cus", [R.PLAN_CUS, 64])
def test_plan_of_every_case(cus):
    for c in R.case_list(cus):
        p = R.case_plan(c, cus)
        assert p.tile_rows * p.ntiles >= c["M"] or p.gn, c["name"]
        assert p.wgs_per_cu == (2 if c["K"] == 320 else 1) and p.grid == min(p.ntiles, cus * p.wgs_per_cu), c["name"]


def test_pinned_shapes_at_256_cus():
    """The shapes the derivation gives on an MI355X (256 CUs), spelled out once."""
    rows = {(K, s): R.schedule_rows(K, s, 256) for K in (320, 640) for s in R.SCHEDULES[K]}
    assert rows == {(320, "one_round"): 421, (320, "two_rounds"): 513 * 128 + 37, (640, "one_round"): 421, (640, "two_rounds"): 257 * 128 + 37,
                    (640, "tb2"): 131109}
    assert R.gn_samples(320, "gn_two_rounds", 256) == 683 and R.gn_samples(640, "gn_two_rounds", 256) == 342


def test_coverage_table():
    """All 26 instantiations of rowlin_kernel (KS x form x TB, plus the two GroupNorm forms), and a second round on each schedule."""
    cases = R.case_list(R.PLAN_CUS)
    seen = {R.kernel_of(R.case_plan(c, R.PLAN_CUS)) for c in cases}
    want = {(ks, f, 0, 1) for ks in (20, 40) for f in R.FORMS} | {(40, f, 0, 2) for f in R.FORMS} | {(20, 0, 1, 1), (40, 0, 1, 1)}
    assert len(want) == 26 and seen == want, f"missing {sorted(want - seen)}, unexpected {sorted(seen - want)}"
    second = {(c["claim"][0], c["claim"][2], c["claim"][3]) for c in cases if R.case_plan(c, R.PLAN_CUS).rounds >= 2}
    assert second == {(20, 0, 1), (40, 0, 1), (40, 0, 2), (20, 1, 1), (40, 1, 1)}, second
    # every form reaches its second round at TB = 1 (both K) and at TB = 2
    for ks, tb in ((20, 1), (40, 1), (40, 2)):
        forms = {c["form"] for c in cases if c["claim"] == (ks, c["form"], 0, tb) and c["rounds"] >= 2}
        assert forms == set(R.FORMS), (ks, tb, forms)


# ------------------------------------------------------------------------------------------- invariants
def tb2_mask():
    return int(os.environ.get("INSV2V_ROWLIN_TB2", 0xff))


def sweep():
    mask, count = tb2_mask(), {1: 0, 2: 0}
    for cus in (1, 4, 64, 256, 304):
        thr = (2 * cus - 1) * 256 + 1                      # the smallest M with ceil(M / 256) >= 2 cus
        for K in (320, 640):
            for N in (64, 128, 1920):
                for M in (1, 31, 128, 129, 421, 128 * cus, 128 * cus + 1, 256 * cus + 5, thr - 1, thr, thr + 255, 3 * thr + 77, 1474560 + 37):
                    for form in R.FORMS:
                        p = R.plan(M, N, K, form, cus=cus)
                        what = f"M={M} N={N} K={K} form={form} cus={cus}: {R.show(p)}"
                        assert p.rc == 0 and p.ks == K // 16 and p.form == form and not p.gn, what
                        assert p.grid <= cus * p.wgs_per_cu and p.grid * p.rounds >= p.ntiles > p.grid * (p.rounds - 1), what
                        assert p.tile_rows == 128 * p.token_blocks and p.tile_rows * p.ntiles >= M > p.tile_rows * (p.ntiles - 1), what
                        two = K == 640 and bool(mask >> form & 1) and -(-M // 256) >= 2 * cus
                        assert p.token_blocks == (2 if two else 1), what
                        assert p.lds_bytes == (4 if K == 320 else 9) * 16384 and p.lds_bytes * p.wgs_per_cu <= 160 * 1024, what
                        count[p.token_blocks] += 1
                for gn_rows in (1, 32, 72, 96, 1536):
                    for S in (1, 3, 5 * cus + 1):
                        M = S * gn_rows - gn_rows // 3
                        p = R.plan(M, N, K, gn_rows=gn_rows, cus=cus)
                        what = f"GN M={M} gn_rows={gn_rows} K={K} cus={cus}: {R.show(p)}"
                        assert p.rc == 0 and p.gn and p.token_blocks == 1 and p.tile_rows == 128 and p.gn_units == -(-gn_rows // 32), what
                        assert p.ntiles == -(-S * p.gn_units // 4) and p.grid <= cus * p.wgs_per_cu and p.grid * p.rounds >= p.ntiles > p.grid * (p.rounds - 1), what
                        assert p.lds_bytes == ((4 if K == 320 else 8) * 16384 + 4 * K * 8) and p.lds_bytes * p.wgs_per_cu <= 160 * 1024, what
    return count


def test_plan_sweep_invariants():
    count = sweep()
    assert count[1] > 0 and (count[2] > 0) == bool(tb2_mask())
    print(f"[plan] sweep: TB = 1 {count[1]}, TB = 2 {count[2]}")


def test_tb2_threshold():
    """M just below and just at ceil(M / 256) = 2 cus."""
    for cus in (4, 64, R.PLAN_CUS):
        thr = (2 * cus - 1) * 256 + 1
        for form in R.FORMS:
            below, at = R.plan(thr - 1, 128, 640, form, cus=cus), R.plan(thr, 128, 640, form, cus=cus)
            assert (below.token_blocks, at.token_blocks) == (1, 2), (cus, form, R.show(below), R.show(at))
            assert at.ntiles == 2 * cus and at.rounds == 2 and below.ntiles == 2 * (2 * cus - 1)
            assert R.plan(10 * thr, 128, 320, form, cus=cus).token_blocks == 1          # K = 320 has no two-block kernels
        assert R.plan(10 * thr, 128, 640, gn_rows=96, cus=cus).token_blocks == 1       # nor has the GroupNorm form


def test_plan_with_switch_off():
    """INSV2V_ROWLIN_TB2=0 in a CPU-only child process (the switch is read once): every plan says one token block per wave."""
    env = dict(os.environ, INSV2V_ROWLIN_TB2="0")
    r = subprocess.run([sys.executable, "-c", "import conftest, test_rowlin_forms_cpu as t; c = t.sweep(); assert c[2] == 0 and c[1] > 0, c; print(c)"],
                       cwd=HERE, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]


# ------------------------------------------------------------------------------------------- refusals
def test_plan_of_every_refusal():
    M, N, K = R.REFUSAL_SHAPE
    assert R.refusal_plan({}).rc == 0 and R.refusal_plan(dict(form=7)).rc == 0 and R.refusal_plan(dict(gn_rows=R.GN_ROWS)).rc == 0   # what the refusals vary is valid
    for name, rc, kw in R.REFUSALS:
        p = R.refusal_plan(kw)
        assert p.rc == rc, f"{name}: rc {p.rc}, documented {rc}"
    # every aligned-pointer and stride bit on its own
    for kw in (dict(x=4096 + 8), dict(wstream=12288 + 8), dict(ldo=132), dict(form=1, ldr=132), dict(form=1, residual=16384 + 8)):
        assert R.refusal_plan(kw).rc == R.EINVAL, kw
    for kw in (dict(x=0), dict(out=0), dict(wstream=0), dict(M=0), dict(N=0)):
        assert R.refusal_plan(kw).rc == R.EINVAL, kw
    assert R.refusal_plan(dict(gn_rows=R.GN_ROWS, gn_ab=20480 + 8)).rc == R.EUNSUPPORTED
    assert R.refusal_plan(dict(ldx=1 << 22)).rc == R.EUNSUPPORTED and R.refusal_plan(dict(form=1, ldr=1 << 22)).rc == R.EUNSUPPORTED
    assert R.refusal_plan(dict(ldx=(1 << 22) - 8, ldo=(1 << 22) - 8)).rc == 0


def test_plan_entry_arguments():
    import ctypes
    from insv2v import _lib
    lib = _lib.load()
    assert lib.insv2v_rowlin_plan(None, 0, ctypes.byref(_lib.RowLinPlan())) == R.EINVAL
    assert lib.insv2v_rowlin_plan(ctypes.byref(_lib.RowLinDesc()), 0, None) == R.EINVAL


# ------------------------------------------------------------------------------------------- builder conditions
@pytest.mark.parametrize("K,N,sched,form,frames", R.form_cases())
def test_form_case_conditions(K, N, sched, form, frames):
    c = R.form_case(K, N, sched, form, SMALL_CUS, CPU, frames)
    assert c["ref"].shape == (c["M"], N) and c["stream"].numel() == (N // 64) * (48 if K == 320 else 96) * 512
    # a reference passes its own judgement, and an error of 1.5 tolerances inside ONE block only is caught
    R.judge(c["ref"], c["ref"], c["blocks"], c["ln"], c["what"])
    for name, rs, cs in c["blocks"]:
        bad = c["ref"].clone()
        blk = bad[rs, cs]
        blk[-1, -1] += 1.5 * R.tol_of(c["ref"][rs, cs], c["ln"])
        with pytest.raises(AssertionError):
            R.judge(bad, c["ref"], c["blocks"], c["ln"], c["what"])


@pytest.mark.parametrize("K,sched,form", R.STATS_CASES)
def test_stats_case_conditions(K, sched, form):
    c = R.form_case(K, R.N_MAIN, sched, form, SMALL_CUS, CPU)
    R.stats_conditions(c["ref"], c["what"])


@pytest.mark.parametrize("K,res,tb", R.EXACT_CASES)
def test_exact_case_conditions(K, res, tb):
    c = R.exact_case(K, res, tb, SMALL_CUS, CPU)
    s = c["shares"]
    print(f"[conditions] {c['what']}: nearest-even != toward-zero {s['rtz']:.3f}, ties {s['ties']}, lo part {s['lo']:.3f}, k-steps {s['kstep']:.3f}, lane halves {s['halves']:.3f}")
    assert c["plan"].token_blocks == tb and int((c["x"] != 0).sum()) == c["M"]


@pytest.mark.parametrize("K,sched", R.GN_CASES)
def test_gn_case_conditions(K, sched):
    c = R.gn_case(K, sched, SMALL_CUS, CPU)
    assert c["plan"].gn and all(c["ref"][rs, cs].numel() > 0 for _, rs, cs in c["blocks"])


@pytest.mark.parametrize("post", [False, True])
def test_ffn_case_conditions(post):
    c = R.ffn_case(post, CPU)
    assert c["ref"].shape == (R.FFN_M, R.FFN_C)


def test_guard_helpers():
    buf, win = R.window(5, 64, 80, 8, CPU, guard=R.GUARD_ROWS)
    assert R.sentinels_intact(buf, 5, 64, 8)
    win.zero_()
    assert R.sentinels_intact(buf, 5, 64, 8)
    for r, c in ((R.GUARD_ROWS - 1, 8), (R.GUARD_ROWS + 5, 70), (R.GUARD_ROWS, 7), (R.GUARD_ROWS + 4, 72)):
        b2 = buf.clone()
        b2[r, c] = 0
        assert not R.sentinels_intact(b2, 5, 64, 8), (r, c)
    x = R.strided(torch.ones(4, 64, dtype=torch.float16), 72, 8)
    assert x.stride(0) == 72 and x.data_ptr() % 16 == 0 and bool((x == 1).all())
