"""What tests/test_attention_variants_gpu.py rests on, checked without a GPU.

  * The dispatch of insv2v_attention through insv2v_attention_plan (csrc/attn_plan.h): the plan of every case of the GPU file is pinned (a
    case that drifts to another form fails HERE, with a message that says so), a coverage table says which forms the case lists must reach,
    the refusals are listed (the 2 GiB rule just inside and just outside per family, by descriptor alone), and a sweep checks the planner's
    invariants - with each of the five switches set to 0 too, one CPU-only child process per switch because they are read once.
  * The power of the case lists: every mutation of attention_ref.emulate violates the GPU file's assertions on at least one listed case.
  * The headroom of the bounds: the unmutated emulation satisfies every assertion on every case; the constants K of attention_ref are
    8 x its worst K = 1 ratio, rounded up to a power of two; the per-case conditions hold (one admitted gap key violates the bound 100
    times over; the late_spike and very_negative inputs move the running maximum of at least a third of the rows after the first tile)."""
import ctypes
import math
import os
import subprocess
import sys

import pytest

import attention_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = ("INSV2V_ATTN_SHORT", "INSV2V_ATTN_FOLD", "INSV2V_ATTN_SINGLE", "INSV2V_ATTN_REP", "INSV2V_ATTN_SHORT_WGS")
WINDOW = 0x7FFFFFFF


# ---------------------------------------------------------------------------------------------------------------- planner corpus
def test_plan_of_every_case():
    for c in R.CASES:
        p = R.check_case_plan(c)
        assert p.threads == p.nw * 64 and p.ntiles == -(-c["sk"] // p.kvt) and p.ragged == int(c["sk"] % p.kvt != 0), c["name"]


def test_coverage_table():
    """The case lists reach every form the product dispatches."""
    seen = {c["plan"] for c in R.CASES}
    want = set()
    for hd in R.HEAD_DIMS:
        want |= {(R.SHORT, hd), (R.SHORT_BIAS, hd)}
        for nw, qb in ((1, 1), (2, 1), (4, 1), (4, 2), (8, 2)):
            if qb == 2 and hd > 96:
                continue                            # the two-query-block forms admit head_dim <= 96
            want.add((R.GENERIC, hd, nw, qb, 64 if nw >= 4 else 32, int(hd in (40, 80) and nw >= 4)))
    short_seen = {(t[0], t[1]) for t in seen if t[0] in (R.SHORT, R.SHORT_BIAS)}
    missing = {w for w in want if (w not in seen if len(w) > 2 else w not in short_seen)}
    assert not missing, "no listed case runs " + "; ".join(R.describe(w + (0,) * (6 - len(w))) for w in sorted(missing))
    assert (R.SINGLE, 160, 6, 1, 96, 0) in seen and (R.SINGLE_REP, 160, 6, 1, 96, 0) in seen
    for hd in (40, 80):                             # FOLD with <4,1>, <4,2>, <8,2>
        assert {(R.GENERIC, hd, nw, qb, 64, 1) for nw, qb in ((4, 1), (4, 2), (8, 2))} <= seen
    # the fall-backs: short -> generic by LDS, SINGLE -> <4,1> by output alignment (the rows' stride, and the base alone)
    c = R.BY_NAME["g11-d160-q16-k16-h16"]
    assert c["sq"] <= 16 and c["sk"] <= 16 and not c["causal"] and c["heads"] * 10 * 16 * 20 * 2 > 64 * 1024 and c["plan"] == (R.GENERIC, 160, 1, 1, 32, 0)
    for name in ("single-q80-k77-fallback", "rep-q80-k77-fallback", "g41-d160-q65-k65"):
        c = R.BY_NAME[name]
        assert 64 < c["sq"] <= 96 and c["sk"] <= 96 and c["plan"] == (R.GENERIC, 160, 4, 1, 64, 0), name
    for fam_names, forms in ((R.EXTREMES, {"generic", "fold", "short"}),):      # the extreme inputs reach every form, not only FOLD
        for fam in fam_names:
            assert {R.form_of(c) for c in R.CASES if c["fam"] == fam} == forms, fam
    kinds = {(c["plan"][0], c["kind"]) for c in R.CASES}
    assert {(R.GENERIC, "cross"), (R.GENERIC, "temporal"), (R.SHORT, "cross"), (R.SHORT, "temporal"), (R.SINGLE, "cross"), (R.SINGLE_REP, "cross")} <= kinds
    per_form = {}
    for c in R.CASES:
        per_form.setdefault((R.GENERIC,) + c["plan"][2:4] if c["plan"][0] == R.GENERIC else c["plan"][:1], set()).add("cols" if c["heads"] == 1 else c["name"].rsplit("-", 1)[-1])
    for form, tags in per_form.items():
        assert {"cols", "place", "scale"} <= tags or form[0] in (R.SHORT_BIAS, R.SINGLE_REP) and {"cols"} <= tags, (form, sorted(tags)[:8])


def window_rs(sk, hd):
    """The largest row stride (a multiple of 8) whose sk rows + hd columns end inside the descriptor's window."""
    rs = (WINDOW // 2 - hd) // sk // 8 * 8
    assert (sk * rs + hd) * 2 <= WINDOW < (sk * (rs + 8) + hd) * 2
    return rs


WINDOW_CASES = [  # (family, descriptor keywords): one per family, every K / V row stride at the limit
    (R.GENERIC, dict(heads=2, hd=64, sq=64, sk=100)),
    (R.GENERIC, dict(heads=8, hd=40, sq=1536, sk=1536)),
    (R.GENERIC, dict(heads=8, hd=40, sq=24, sk=24)),                 # temporal attention over 24 frames: the row stride is the frame
    (R.SINGLE, dict(heads=8, hd=160, sq=96, sk=96)),
    (R.SINGLE_REP, dict(heads=8, hd=160, sq=96, sk=77, batch=4, kv_inner=2, kv_step=0)),
    (R.D512, dict(heads=1, hd=512, sq=1000, sk=1000)),
    (R.SHORT, dict(heads=8, hd=40, sq=16, sk=16)),
    (R.SHORT_BIAS, dict(heads=8, hd=160, sq=16, sk=16)),
]


@pytest.mark.parametrize("family,kw", WINDOW_CASES, ids=[f"{R.FAMILY_NAMES[f]}-d{kw['hd']}-k{kw['sk']}" for f, kw in WINDOW_CASES])
def test_two_gib_rule(family, kw):
    """K / V rows beyond the 2 GiB a buffer descriptor spans from the (problem, head) base would read as zeros: refused, by descriptor alone."""
    rs = window_rs(kw["sk"], kw["hd"])
    mk = (lambda **o: R.with_bias(R.plain_desc(**{**kw, **o}))) if family == R.SHORT_BIAS else (lambda **o: R.plain_desc(**{**kw, **o}))
    base = mk(q_rs=rs + 8, o_rs=kw["heads"] * kw["hd"])                            # (q and o are addressed with 64-bit offsets: no rule on them)
    inside, outside_v, outside_k = mk(k_rs=rs, v_rs=rs, q_rs=rs + 8), mk(k_rs=rs, v_rs=rs + 8), mk(k_rs=rs + 8, v_rs=rs)
    assert R.plan(base).family == family
    p = R.plan(inside)
    assert (p.rc, p.family) == (0, family), (p.rc, R.describe(R.plan_tuple(p)))
    p = R.plan(outside_v)
    assert (p.rc, p.family) == (R.EUNSUPPORTED, R.NONE)
    p = R.plan(outside_k)
    if family in (R.SHORT, R.SHORT_BIAS):           # the short kernel reads K with plain 64-bit loads: its rule is on v_rs alone
        assert (p.rc, p.family) == (0, family)
    else:
        assert (p.rc, p.family) == (R.EUNSUPPORTED, R.NONE)


REFUSALS = [
    ("q NULL", dict(q=None), R.EINVAL), ("o NULL", dict(o=None), R.EINVAL), ("head_dim 20", dict(head_dim=20, q_rs=40, k_rs=40, v_rs=40, o_rs=40), R.EINVAL),
    ("head_dim 168", dict(head_dim=168, q_rs=168, k_rs=168, v_rs=168, o_rs=168), R.EINVAL), ("head_dim 0", dict(head_dim=0), R.EINVAL),
    ("head_dim 24", dict(head_dim=24, q_rs=24, k_rs=24, v_rs=24, o_rs=24), R.EUNSUPPORTED), ("seq_q 0", dict(seq_q=0), R.EINVAL),
    ("seq_k 0", dict(seq_k=0), R.EINVAL), ("batch 0", dict(batch=0), R.EINVAL), ("heads 0", dict(heads=0), R.EINVAL),
    ("q_rs 4 mod 8", dict(q_rs=68), R.EINVAL), ("k_rs 4 mod 8", dict(k_rs=68), R.EINVAL), ("v_rs 4 mod 8", dict(v_rs=68), R.EINVAL),
    ("o_rs 2 mod 4", dict(o_rs=66), R.EINVAL),
    ("d = 512 causal", dict(head_dim=512, q_rs=512, k_rs=512, v_rs=512, o_rs=512, causal=1), R.EUNSUPPORTED),
]
BIAS_REFUSALS = [
    ("only q_bias", dict(k_bias=None, v_bias=None), R.EINVAL), ("bias_rs 4 mod 8", dict(bias_rs=3 * 64 + 4), R.EINVAL),
    ("q_bias 8 mod 16", dict(q_bias=32768 + 8), R.EINVAL), ("v_bias 8 mod 16", dict(v_bias=32768 + 8), R.EINVAL),
    ("bias with 24 rows", dict(seq_q=24, seq_k=24), R.EUNSUPPORTED), ("bias with 17 keys", dict(seq_k=17), R.EUNSUPPORTED),
    ("bias, causal", dict(causal=1), R.EUNSUPPORTED), ("bias, head_dim 24", dict(head_dim=24, q_rs=24, k_rs=24, v_rs=24, o_rs=24), R.EUNSUPPORTED),
]


def _blank(p):
    return all(getattr(p, n) == 0 for n, _ in p._fields_ if n != "rc")


def test_plan_of_every_refusal():
    assert R.plan(R.plain_desc()).rc == 0 and R.plan(R.with_bias(R.plain_desc(sq=16, sk=16))).family == R.SHORT_BIAS     # the calls the refusals vary are valid
    for what, over, rc in REFUSALS:
        p = R.plan(R.plain_desc(**over))
        assert p.rc == rc and _blank(p), (what, p.rc, R.describe(R.plan_tuple(p)))
    for what, over, rc in BIAS_REFUSALS:
        d = R.with_bias(R.plain_desc(sq=16, sk=16))
        for key, val in over.items():
            setattr(d, key, val)
        p = R.plan(d)
        assert p.rc == rc and _blank(p), (what, p.rc, R.describe(R.plan_tuple(p)))
    for heads in range(1, 17):                      # the biased short kernel is compiled for <= 8 heads; unbiased for 16
        for hd in R.HEAD_DIMS:
            fits = heads * -(-hd // 16) * 16 * 20 * 2 <= 64 * 1024
            p, pb = R.plan(R.plain_desc(heads=heads, hd=hd, sq=16, sk=16)), R.plan(R.with_bias(R.plain_desc(heads=heads, hd=hd, sq=16, sk=16)))
            assert (p.rc, p.family) == ((0, R.SHORT) if fits else (0, R.GENERIC)), (heads, hd)
            assert (pb.rc, pb.family) == ((0, R.SHORT_BIAS) if fits and heads <= 8 else (R.EUNSUPPORTED, R.NONE)), (heads, hd)
    p = R.plan(R.plain_desc(heads=17, hd=16, sq=16, sk=16))
    assert (p.family, p.nw) == (R.GENERIC, 1)
    from insv2v import _lib
    lib = _lib.load()
    assert lib.insv2v_attention_plan(None, 0, ctypes.byref(_lib.AttentionPlan())) == R.EINVAL
    assert lib.insv2v_attention_plan(ctypes.byref(R.plain_desc()), 0, None) == R.EINVAL
    # cus <= 0 on a machine without a GPU: the persistent short grid falls back to one workgroup per problem; a CU count caps it
    d = R.with_bias(R.plain_desc(batch=5000, heads=8, hd=40, sq=16, sk=16))
    assert R.plan(d, 256).grid == 512 and R.plan(d, 4000).grid == 5000 and R.plan(d, 256).rows_per_wg == 16 * 8 * 10


# ---------------------------------------------------------------------------------------------------------------- planner sweep
SWEEP_SEQ = tuple(n + e for n in (16, 32, 64, 96, 128, 256, 512) for e in (-1, 0, 1))


def switches():
    dflt = dict(zip(SWITCHES, (1, 1, 1, 1, 2)))
    return {k: int(os.environ.get(k, v)) for k, v in dflt.items()}


def check_invariants(d, p, sw, biased):
    what = (f"batch {d.batch} heads {d.heads} d {d.head_dim} seq {d.seq_q}/{d.seq_k} causal {d.causal} biased {biased} kv_inner {d.kv_inner} o {d.o % 16} "
            f"{sw}: rc {p.rc} {R.describe(R.plan_tuple(p))}")
    assert p.rc in (0, R.EINVAL, R.EUNSUPPORTED) and (p.rc == 0) == (p.family != R.NONE), what
    if p.rc:
        assert _blank(p), what
        return
    hd, sq, sk = d.head_dim, d.seq_q, d.seq_k
    assert 0 < p.threads <= 1024 and p.threads == p.nw * 64 and p.d == hd, what
    assert p.grid >= 1 and p.rows_per_wg * p.grid >= sq * d.heads * d.batch, what
    assert p.ntiles == -(-sk // p.kvt) and p.ragged == int(sk % p.kvt != 0), what
    assert biased == (p.family == R.SHORT_BIAS), what
    rs = d.v_rs if p.family in (R.SHORT, R.SHORT_BIAS) else max(d.k_rs, d.v_rs)
    assert (sk * rs + hd) * 2 <= WINDOW, what
    if p.family in (R.SHORT, R.SHORT_BIAS):
        assert sq <= 16 and sk <= 16 and not d.causal and d.heads <= 16 and p.nw == d.heads and (p.qb, p.kvt, p.fold) == (1, 16, 0), what
        assert p.lds_bytes == d.heads * -(-hd // 16) * 16 * 20 * 2 <= 64 * 1024, what
        assert sw["INSV2V_ATTN_SHORT"] or biased, what
        if biased:
            assert d.heads * 64 <= 512, what
            assert p.grid == (min(d.batch, R.PLAN_CUS * sw["INSV2V_ATTN_SHORT_WGS"]) if sw["INSV2V_ATTN_SHORT_WGS"] > 0 else d.batch), what
        else:
            assert p.grid == d.batch and p.rows_per_wg == 16 * d.heads, what
        return
    dp = (hd + 31) // 32 * 32
    single = p.family in (R.SINGLE, R.SINGLE_REP)
    assert p.lds_bytes == (1 if single else 2) * (p.kvt * (dp + 8) + dp * (p.kvt + 4)) * 2 <= 160 * 1024, what
    assert p.fold == int(bool(sw["INSV2V_ATTN_FOLD"]) and hd in (40, 80) and p.nw >= 4 and not single), what
    if single:
        assert sw["INSV2V_ATTN_SINGLE"] and sk <= 96 and 64 < sq <= 96 and hd == 160 and not d.causal and (p.nw, p.qb, p.kvt, p.ntiles) == (6, 1, 96, 1), what
        assert d.o % 16 == 0 and d.o_rs % 8 == 0 and d.o_outer % 8 == 0 and d.o_step % 8 == 0, what
        rep = p.family == R.SINGLE_REP
        assert rep == bool(sw["INSV2V_ATTN_REP"] and d.kv_inner > 1 and d.kv_step == 0 and d.batch % d.kv_inner == 0), what
        assert p.rows_per_wg == 96 * (d.kv_inner if rep else 1) and p.grid == d.heads * (d.batch // d.kv_inner if rep else d.batch), what
        return
    assert p.family == R.GENERIC and (p.nw, p.qb) in ((1, 1), (2, 1), (4, 1), (4, 2), (8, 2)) and p.kvt == (64 if p.nw >= 4 else 32), what
    assert p.rows_per_wg == 16 * p.nw * p.qb and p.grid == -(-sq // p.rows_per_wg) * d.heads * d.batch, what
    assert p.qb == 1 or hd <= 96, what
    assert sq > (p.nw // 2) * 16 or p.nw == 4, what              # no workgroup wider than the sequence needs (4 waves: the widest one-block form)


def sweep(switch=None):
    """The planner's invariants over heads 1..16, every head dim and sequence lengths around the thresholds; with `switch` (a child process
    with that variable set to 0) what the switch must and must not do as well.  Returns the number of plans per family."""
    sw = switches()
    assert all(v == (0 if k == switch else d) for (k, v), d in zip(sw.items(), (1, 1, 1, 1, 2))), (switch, sw)
    from insv2v import ops
    count = {f: 0 for f in R.FAMILY_NAMES}
    for heads in range(1, 17):
        for hd in R.HEAD_DIMS:
            rs = heads * hd
            for sq in SWEEP_SEQ:
                for sk in SWEEP_SEQ:
                    variants = [({}, False)]
                    if heads in (1, 8):
                        variants.append((dict(causal=1), False))
                    if sq <= 17 and sk <= 17:
                        variants.append((dict(batch=700), True))
                    if hd == 160 and sq <= 97 and sk <= 97:
                        variants += [(dict(batch=4, kv_inner=2, kv_step=0), False), (dict(batch=5, kv_inner=2, kv_step=0), False),
                                     (dict(batch=4, kv_inner=2, kv_step=8), False), (dict(o=16384 + 8), False), (dict(o_rs=rs + 4), False), (dict(o_step=4), False)]
                    for over, biased in variants:
                        d = R.plain_desc(heads=heads, hd=hd, sq=sq, sk=sk, **over)
                        if biased:
                            R.with_bias(d)
                        p = R.plan(d)
                        check_invariants(d, p, sw, biased and p.rc == 0)
                        count[p.family] += 1
                        if sq == sk and not over:          # the planner against Python: attention_short_supported has no rule of its own
                            assert ops.attention_short_supported(heads, hd, sq) == (p.family == R.SHORT), (heads, hd, sq)
                        if sq == sk and biased:
                            assert ops.attention_short_supported(heads, hd, sq, biased=True) == (p.family == R.SHORT_BIAS), (heads, hd, sq)
    off = {"INSV2V_ATTN_SHORT": R.SHORT, "INSV2V_ATTN_SINGLE": R.SINGLE, "INSV2V_ATTN_REP": R.SINGLE_REP}
    for key in off:
        assert bool(count[off[key]]) == (switch != key) or (key == "INSV2V_ATTN_REP" and switch == "INSV2V_ATTN_SINGLE"), (switch, count)
    assert count[R.SHORT_BIAS] and count[R.GENERIC] and count[R.NONE], count
    if switch == "INSV2V_ATTN_FOLD":            # the unfolded d = 40 / 80 forms: A/B forms, covered here by plan only
        for hd in (40, 80):
            for sq, nw, qb in ((64, 4, 1), (128, 4, 2), (512, 8, 2)):
                assert R.plan_tuple(R.plan(R.plain_desc(heads=8, hd=hd, sq=sq, sk=sq))) == (R.GENERIC, hd, nw, qb, 64, 0)
    p = R.plan(R.plain_desc(heads=1, hd=512, sq=100, sk=100))
    assert R.plan_tuple(p) == (R.D512, 512, 4, 1, 32, 0) and p.lds_bytes == 2 * (32 * 520 + 512 * 36) * 2 and p.rows_per_wg == 64
    return count


def test_plan_sweep_invariants():
    count = sweep()
    print("[plan] sweep: " + ", ".join(f"{R.FAMILY_NAMES[f]} {n}" for f, n in count.items()))


@pytest.mark.parametrize("switch", SWITCHES)
def test_plan_sweep_invariants_with_switch_off(switch):
    env = dict(os.environ, **{switch: "0"})
    r = subprocess.run([sys.executable, "-c", f"import conftest, test_attention_variants_cpu as t; print(t.sweep('{switch}'))"], cwd=HERE, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------- power and headroom
def applies(mutate, c):
    """Whether a mutation changes anything on a case at all (the others are skipped to save time, not to pass)."""
    kvt = c["plan"][4]
    return {"ragged_extra_key": c["sk"] % kvt != 0, "ragged_zero_key": c["sk"] % kvt != 0, "causal_strict": c["causal"], "kv_of_z": c["kind"] == "cross",
            "bias_next_row": c["bias"], "store_next_block_row": c["sq"] % 16 != 0, "next_head_columns": c["hd"] % 32 != 0,
            "no_rescale": c["sk"] > kvt, "unrounded_sum": R.form_of(c) != "short"}.get(mutate, True)


@pytest.mark.parametrize("mutate", R.MUTATIONS)
def test_mutations_are_caught(mutate):
    caught = []
    for c in R.CASES:
        if not applies(mutate, c):
            continue
        _, data, r = R.prepared(c["name"])
        v = R.verdict(c, r, R.emulate(c, data, mutate))
        if not R.passes(v):
            caught.append((c["name"], R.form_of(c), [k for k in ("ratio", "gaps", "ones") if (v[k] > 1 if k == "ratio" else v[k])]))
    forms = sorted({f for _, f, _ in caught})
    by = sorted({k for _, _, ks in caught for k in ks})
    print(f"[power] {mutate}: caught on {len(caught)} cases, forms {forms}, through {by}, first {caught[:2]}")
    assert caught, f"no listed case notices `{mutate}`"
    want = {"generic", "fold", "short"}
    if mutate in ("no_rescale", "unrounded_sum"):
        want = {"generic", "fold"}                  # one tile, and a row sum that is the unrounded one by design, in the short kernel
    if mutate == "causal_strict":
        want = {"generic", "fold"}                  # the short kernel refuses causal
    if mutate == "bias_next_row":
        want = {"short"}
    if mutate == "kv_of_z":
        want = {"generic", "fold", "short"}
    assert want <= set(forms), f"`{mutate}` is not noticed in {sorted(want - set(forms))}"


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


def test_headroom_of_the_bounds():
    """The fp32 emulation against every assertion with K = 1 (the ratios that define K) and with K (every case passes); the per-case conditions."""
    one = dict.fromkeys(R.K, 1.0)
    worst, where = {}, {}
    for c in R.CASES:
        _, data, r = R.prepared(c["name"])
        out = R.emulate(c, data)
        v1, vk = R.verdict(c, r, out, one), R.verdict(c, r, out)
        assert R.passes(vk), (c["name"], vk)
        f = R.form_of(c)
        if v1["ratio"] > worst.get(f, -1):
            worst[f], where[f] = v1["ratio"], c["name"]
        # conditions on the case itself, by the reference alone
        leak = R.verdict(c, r, R.emulate(c, data, "gap_key"))["ratio"]
        assert leak >= 100, f"{c['name']}: one admitted gap key violates the bound only {leak:.3g} times over"
        if c["fam"] in ("late_spike", "very_negative"):
            mf = R.moved_fraction(c, r)
            assert mf is None or mf >= 1 / 3, f"{c['name']}: only {mf:.2f} of the rows move their maximum after the first tile"
    for f in sorted(worst):
        print(f"[headroom] {f:8s} worst ratio at K = 1: {worst[f]:.4g} ({where[f]}) -> K = {pow2_ceil(8 * worst[f]):g} (attention_ref.K: {R.K[f]:g})")
    for f in R.K:
        assert R.K[f] == pow2_ceil(8 * worst[f]), f"attention_ref.K['{f}'] = {R.K[f]:g} is not 8 x {worst[f]:.4g} rounded up to a power of two"
        assert abs(R.K_MEASURED[f] / worst[f] - 1) < 0.25, f"attention_ref.K_MEASURED['{f}'] = {R.K_MEASURED[f]} but the worst ratio is {worst[f]:.4g}"
