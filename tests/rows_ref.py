"""Case builders and fp64 references for the kernel-level parity tests of the register-resident row kernels of csrc/rows_ffn.hip:
insv2v_rowlin (rowlin_kernel<KS, LN, FRAME, RES, GN, TB>: 2 x 8 forms with one token block per wave, 8 forms at K = 640 with two, the
GroupNorm-on-load form at both K) and insv2v_ffn_fused (ffn_fused_kernel<POST>).  Device-agnostic, in the style of gemm_engine_ref.py
(whose helpers are reused): every builder takes `device`, draws its operands with a CPU generator, and returns the fp16 operands, the
packed stream of insv2v.fused and the fp64 reference on the SAME fp16-rounded operands, with the blocks of the output to be judged on
their own - a wrong tile must not be averaged away by the global max|ref|.  Every builder asserts with need_gap that a reference computed
WITHOUT a feature it exercises is more than 10 x the tolerance away from the true one; tests/test_rowlin_forms_cpu.py asserts these
conditions without a GPU (at a small CU count), tests/test_rowlin_forms_gpu.py again at the device's own.

Which kernel a shape runs depends on the CU count: no shape is hard-coded to one part.  Every builder takes `cus`, derives its rows from
the planner (ops.rowlin_plan -> insv2v_rowlin_plan, csrc/rows_plan.h) and asserts that the plan is what the case claims.

What the kernel dictates to the reference: the per-frame bias table is carried as fp16 (the reference uses the table rounded to fp16);
the plain bias is carried as hi + lo fp16 parts (the reference uses the fp32 bias unrounded)."""
import torch
import torch.nn.functional as F

from gemm_engine_ref import rnd, randint, tol_of, need_gap, cached, stats_tol, round_toward_zero_f16, round_half_away_f16  # noqa: F401

PLAN_CUS = 256          # the CU count the CPU file pins every plan at (an MI355X)
N_MAIN = 128            # two column pairs: the pr > 0 path of the pair loop runs
RPF, FRAMES = 40, 5     # rows per frame (no multiple of 32: a wave's 32 tokens straddle two frames), frames (wraps several times)
PERIOD = 4099           # prime: rows of the random block that large operands repeat - no tile or wave block repeats another's rows
EPS = 1e-5
GN_ROWS = 72            # rows per sample of the GroupNorm-on-load cases: 3 wave blocks, the last with 8 real rows
FORMS = tuple(range(8))
SCHEDULES = {320: ("one_round", "two_rounds"), 640: ("one_round", "two_rounds", "tb2")}
EXPECT = {"one_round": (1, 1), "two_rounds": (1, 2), "tb2": (2, 3)}   # schedule -> (token blocks per wave, rounds)


def form_bits(form):
    """form = LN << 2 | FRAME << 1 | RES"""
    return bool(form & 4), bool(form & 2), bool(form & 1)


def plan(M, N, K, form=0, frames=FRAMES, gn_rows=0, cus=PLAN_CUS, rows_per_frame=RPF, **over):
    from insv2v import ops
    ln, fr, res = form_bits(form)
    return ops.rowlin_plan(M, N, K, layernorm=ln, residual=over.pop("residual", res), frames=frames if fr else 0, rows_per_frame=rows_per_frame if fr else 0, gn_rows=gn_rows,
                           cus=cus, **over)


def kernel_of(p):
    return (p.ks, p.form, p.gn, p.token_blocks)


def describe(t):
    return f"rowlin_kernel<KS={t[0]}, LN={t[1] >> 2 & 1}, FRAME={t[1] >> 1 & 1}, RES={t[1] & 1}, GN={t[2]}, TB={t[3]}>"


def show(p):
    return f"{describe(kernel_of(p))} tiles={p.ntiles}x{p.tile_rows} grid={p.grid} rounds={p.rounds}"


def schedule_rows(K, sched, cus):
    """Rows of a schedule, from G = cus * wgs_per_cu workgroup slots:
    one_round  3 x 128 + 37: the last tile is ragged - wave 0 full, wave 1 has 5 rows, waves 2 and 3 none;
    two_rounds (G + 1) x 128 + 37: G + 2 tiles, the prefetch of tile blockIdx.x + gridDim.x runs and mostly requests rows at or beyond M;
    tb2        2 cus x 256 + 37: ceil(M / 256) = 2 cus + 1, the smallest M that runs two token blocks per wave with a ragged third round -
               its last 256-row tile holds wave 0's first block in full, 5 rows of its second and nothing else."""
    G = cus * plan(128, 64, K, cus=cus).wgs_per_cu
    return {"one_round": 3 * 128 + 37, "two_rounds": (G + 1) * 128 + 37, "tb2": 2 * cus * 256 + 37}[sched]


def check_schedule(p, sched, M, what):
    assert p.rc == 0, f"{what}: refused, rc {p.rc}"
    assert (p.token_blocks, p.rounds) == EXPECT[sched] and not p.gn, f"{what}: claims {sched} = (TB, rounds) {EXPECT[sched]}, the plan says {show(p)}"
    assert p.tile_rows == 128 * p.token_blocks and p.tile_rows * p.ntiles >= M > p.tile_rows * (p.ntiles - 1) and p.grid * p.rounds >= p.ntiles


def gn_samples(K, sched, cus):
    """one_round: 5 samples (the last one partial, see gn_case); gn_two_rounds: the smallest sample count whose plan has rounds >= 2."""
    if sched == "one_round":
        return 5
    G = cus * plan(128, 64, K, cus=cus).wgs_per_cu
    units = (GN_ROWS + 31) // 32
    s = (4 * G) // units + 1                     # smallest s with ceil(units s / 4) > G
    assert plan(s * GN_ROWS, 64, K, gn_rows=GN_ROWS, cus=cus).rounds >= 2 and plan((s - 1) * GN_ROWS, 64, K, gn_rows=GN_ROWS, cus=cus).rounds == 1
    return s


def rows(M, cols, seed, device, scale=1.0, shift=0.0):
    """[M, cols] fp16 random rows; beyond PERIOD rows a PERIOD-row block repeated down the rows (the large cases stay cheap to draw)."""
    blk = (rnd(min(M, PERIOD), cols, seed=seed) * scale + shift).half().to(device)
    return blk if M <= PERIOD else blk.repeat((M + PERIOD - 1) // PERIOD, 1)[:M].contiguous()


def chunked(fn, x, chunk=16384):
    """fn over row chunks of x in fp64 (the reference of the large cases is computed on the device, 16 384 rows at a time)."""
    return torch.cat([fn(x[i:i + chunk].double()) for i in range(0, x.shape[0], chunk)], 0)


def blocks_of(p, M, N):
    """(name, rows, columns) judged on their own: first tile, last (ragged) tile, first tile of the second round, last column pair."""
    T = p.tile_rows
    out = [("first tile", slice(0, min(T, M)), slice(0, N)), ("last tile", slice((p.ntiles - 1) * T, M), slice(0, N))]
    if p.rounds >= 2:
        out.append(("first tile of round 2", slice(p.grid * T, min((p.grid + 1) * T, M)), slice(0, N)))
    out.append(("last column pair", slice(0, M), slice(N - 64, N)))
    return out


def judge(out, ref, blocks, ln, what):
    """Every block against ITS max|ref|: asserts, and returns (worst error / tolerance, its block)."""
    worst = (0.0, "")
    for name, rs, cs in [("whole output", slice(None), slice(None))] + list(blocks):
        o, r = out[rs, cs].double(), ref[rs, cs]
        assert r.numel() > 0, f"{what}: block '{name}' is empty"
        err, tol = (o - r).abs().max().item(), tol_of(r, ln)
        assert err == err and err <= tol, f"{what}, {name}: max err {err:.4g} > tol {tol:.4g} (block max|ref| {r.abs().max().item():.4g})"
        worst = max(worst, (err / tol, name))
    return worst


def swap_token_blocks(ref):
    """The two 32-token blocks of a wave exchanged: m ^ 32 within each whole 64 rows."""
    M = ref.shape[0]
    m = torch.arange(M, device=ref.device)
    return ref[torch.where(m < M // 64 * 64, m ^ 32, m)]


# ------------------------------------------------------------------------------------------- 1. forms x schedules
@cached
def base_case(K, N, sched, cus, device):
    """Operands shared by the eight forms of one (K, N, schedule): x (non-zero row means, for the LayerNorm), W, the plain bias, the
    per-frame tables, the residual, and the two fp64 products x W^T and LayerNorm(x) W^T."""
    M = schedule_rows(K, sched, cus)
    x, r = rows(M, K, 0, device, 1.4, 0.3), rows(M, N, 3, device)
    w, b = rnd(N, K, scale=K ** -0.5).half(), rnd(N, seed=1) * 0.5
    tables = {f: rnd(f, N, seed=5) * 0.5 for f in (FRAMES, 16)}
    wd = w.to(device).double()
    lin = chunked(lambda xs: xs @ wd.t(), x)
    lnlin = chunked(lambda xs: F.layer_norm(xs, (K,), eps=EPS) @ wd.t(), x)
    return dict(M=M, x=x, r=r, w=w, b=b, tables=tables, lin=lin, lnlin=lnlin)


def form_case(K, N, sched, form, cus, device, frames=FRAMES):
    """One form at one schedule: dict(x, stream, residual, kw (of ops.rowlin), ref, ln, blocks, plan, what)."""
    from insv2v.fused import pack_linear_stream
    base = base_case(K, N, sched, cus, device)
    ln, fr, res = form_bits(form)
    M = base["M"]
    what = f"rowlin K={K} N={N} {sched} form={form} M={M} frames={frames if fr else 0}"
    p = plan(M, N, K, form, frames=frames, cus=cus)
    check_schedule(p, sched, M, what)
    m = torch.arange(M, device=device)
    core, rr = base["lnlin"] if ln else base["lin"], base["r"].double() if res else 0
    if fr:
        t16 = base["tables"][frames].half().double().to(device)     # the table as the stream carries it
        bias = t16[(m // RPF) % frames]
    else:
        bias = base["b"].double().to(device)
    ref = core + bias + rr
    tol = tol_of(ref, ln)
    if ln:
        need_gap(ref, base["lin"] + bias + rr, tol, f"{what}: LayerNorm omitted")
    if res:
        need_gap(ref, core + bias, tol, f"{what}: residual omitted")
    need_gap(ref, core + rr, tol, f"{what}: bias omitted")
    if fr:
        f = m // RPF
        if M > RPF * frames:        # (the one-hot of a frame index beyond the table selects nothing)
            nowrap = torch.where((f < frames)[:, None], t16[f.clamp(max=frames - 1)], torch.zeros((), dtype=torch.float64, device=device))
            need_gap(ref, core + nowrap + rr, tol, f"{what}: frame index m // rows_per_frame without the % frames wrap")
        need_gap(ref, core + t16[((m + 32) // RPF) % frames] + rr, tol, f"{what}: frame index shifted by one row block of 32")
    need_gap(ref, ref.reshape(M, N // 64, 2, 32).flip(2).reshape(M, N), tol, f"{what}: 32-column tiles 2p and 2p + 1 exchanged")
    if p.token_blocks == 2:
        need_gap(ref, swap_token_blocks(ref), tol, f"{what}: the two 32-token blocks of a wave exchanged")
    table = base["tables"][frames] if fr else None
    stream = pack_linear_stream(base["w"].float(), None if fr else base["b"], table).to(device)
    kw = dict(layernorm=ln, residual=base["r"] if res else None, frames=frames if fr else 0, rows_per_frame=RPF if fr else 0)
    return dict(M=M, N=N, K=K, x=base["x"], stream=stream, kw=kw, ref=ref, ln=ln, blocks=blocks_of(p, M, N), plan=p, what=what)


def form_cases():
    """(K, N, schedule, form, frames) of every case of the forms test, the operands of one (K, N, schedule) adjacent."""
    out = []
    for K in (320, 640):
        for sched in SCHEDULES[K]:
            for N in ((64, N_MAIN, 192) if sched == "one_round" else (N_MAIN,)):
                out += [(K, N, sched, form, FRAMES) for form in FORMS]
    out.append((320, N_MAIN, "two_rounds", 2, 16))      # frames = 16: both lane halves of the one-hot, wraps (M > 16 x 40)
    return out


# ------------------------------------------------------------------------------------------- 2. exact layout and rounding
EXACT_BIAS_BASE = {False: 1.0, True: -4.0}


@cached
def exact_case(K, res, tb, cus, device):
    """x one-hot (row m: a single 1 at column (37 m) % K), so every accumulator holds ONE product plus the bias; W = s (1 + i / 1024),
    residual 1 + r / 1024 (gemm_engine_ref.exact_case).  bias = base + (n % 8) / 8192 with base = 1 (plain) / -4 (residual): its fp16
    rounding - the hi part - is a multiple of 2^-10, and ONLY the lo part of the bias fragment can carry the rest of (n % 8) / 8192.  ((n % 8) / 8192 alone is
    an fp16 value: its lo part would be zero and the lo condition below could not hold.  The base is chosen per form so that the sums
    fall where that condition and exact_case's own hold.)  Every fp32 sum is exact and carries bits below the fp16 ulp: the stored value
    must EQUAL the fp32 value rounded to nearest even.  Returns dict(x, stream, residual, ref32, plan, shares)."""
    from insv2v.fused import pack_linear_stream
    N = N_MAIN
    sched = "tb2" if tb == 2 else "one_round"
    M = schedule_rows(K, sched, cus)
    what = f"exact K={K} res={res} TB={tb} M={M}"
    p = plan(M, N, K, int(res), cus=cus)
    check_schedule(p, sched, M, what)
    m = torch.arange(M, device=device)
    hot = (37 * m) % K
    x = torch.zeros(M, K, device=device, dtype=torch.float16)
    x[m, hot] = 1
    i = randint(1024, N, K, seed=1, device=device)
    s = 1.0 - 2.0 * (randint(4, N, K, seed=2, device=device) == 0).float()
    w = (s * (1.0 + i.float() / 1024.0)).half()
    assert torch.equal(w.double(), s.double() * (1.0 + i.double() / 1024.0))
    b = EXACT_BIAS_BASE[res] + (torch.arange(N, device=device) % 8).float() / 8192.0
    hi = b.half().float()
    lo = (b - hi).half().float()
    assert torch.equal(hi.double() + lo.double(), b.double()) and torch.equal(hi * 1024, (hi * 1024).round()), "the hi + lo parts do not carry the bias exactly"
    assert bool((lo != 0)[torch.arange(N, device=device) % 8 != 0].all()), "a bias whose lo part is zero"
    rblk = (1.0 + randint(1024, min(M, PERIOD), N, seed=3, device=device).float() / 1024.0).half()
    r = (rblk if M <= PERIOD else rblk.repeat((M + PERIOD - 1) // PERIOD, 1)[:M].contiguous()) if res else None

    def value(wt, bias):      # (fp32, fp64) sums with weights wt and bias
        c = wt.float()[:, hot].t()
        v32, v64 = c + bias, c.double() + bias.double()
        return (v32 + r.float(), v64 + r.double()) if res else (v32, v64)

    ref32, ref64 = value(w, b)
    assert torch.equal(ref32.double(), ref64), "the fp32 sums of the exact case are not exact"
    rne, rtz = ref32.half(), round_toward_zero_f16(ref32)
    share = (rne != rtz).float().mean().item()
    assert share > 1 / 3, f"input condition, {what}: only {share:.3f} of the elements tell nearest-even from toward-zero"
    rha, _ = round_half_away_f16(ref32)
    ties = int((rha != rne).sum())
    assert ties > 0, f"input condition, {what}: no exact tie whose nearest-even result differs from round-half-away"
    lo_share = (value(w, hi)[0].half() != rne).float().mean().item()
    assert lo_share >= 0.25, f"input condition, {what}: dropping the lo bias part changes only {lo_share:.3f} of the fp16 results"
    cols = torch.arange(K, device=device)
    kswap = torch.where(cols < 32, cols ^ 16, cols)                   # k-steps 0 and 1 exchanged
    ks_share = (value(w[:, kswap], b)[0].half() != rne).float().mean().item()
    assert ks_share > 0.02, f"input condition, {what}: two k-steps exchanged changes only {ks_share:.3f} of the results"
    hs_share = (value(w[:, cols ^ 8], b)[0].half() != rne).float().mean().item()
    assert hs_share > 0.5, f"input condition, {what}: the lane halves of a fragment exchanged changes only {hs_share:.3f} of the results"
    stream = pack_linear_stream(w.float().cpu(), b.cpu()).to(device)
    return dict(M=M, N=N, x=x, stream=stream, residual=r, ref32=ref32.contiguous(), plan=p, what=what,
                shares=dict(rtz=share, ties=ties, lo=lo_share, kstep=ks_share, halves=hs_share))


EXACT_CASES = [(320, False, 1), (320, True, 1), (640, False, 1), (640, True, 1), (640, False, 2), (640, True, 2)]


# ------------------------------------------------------------------------------------------- 3. strides and guards
GUARD_ROWS, SENTINEL = 3, 777.0


def window(M, cols, ld, off, device, fill=None, guard=0):
    """(buffer, window): a [M, cols] column window at column `off` of a [guard + M + guard, ld] buffer (16-byte aligned base)."""
    assert ld % 8 == 0 and off % 8 == 0 and off + cols <= ld
    buf = torch.full((M + 2 * guard, ld), SENTINEL if fill is None else fill, dtype=torch.float16, device=device)
    return buf, buf[guard:guard + M, off:off + cols]


def sentinels_intact(buf, M, cols, off, guard=GUARD_ROWS):
    """Every element of the buffer outside the window still holds the sentinel."""
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[guard:guard + M, off:off + cols] = False
    return bool((buf[mask] == SENTINEL).all())


def strided(t, ld, off):
    """A copy of t as a column window of a buffer of row stride ld whose padding is NaN (an input: the padding must never be read)."""
    buf, win = window(t.shape[0], t.shape[1], ld, off, t.device, fill=float("nan"))
    win.copy_(t)
    return win


STRIDED_FORMS = (0, 1, 5)


# ------------------------------------------------------------------------------------------- 4. GroupNorm on load
@cached
def gn_case(K, sched, cus, device):
    """The (scale, shift) table is drawn directly as [samples][K][2] fp32; ref = (x scale + shift) W^T + b in fp64.  one_round: 5 samples,
    the last one PARTIAL (19 rows short); gn_two_rounds: whole samples.  72 rows per sample = 3 wave blocks, the last with 8 real rows."""
    from insv2v.fused import pack_linear_stream
    N = N_MAIN
    S = gn_samples(K, sched, cus)
    M = S * GN_ROWS - (19 if sched == "one_round" else 0)
    what = f"rowlin GroupNorm-on-load K={K} {sched} samples={S} M={M}"
    p = plan(M, N, K, gn_rows=GN_ROWS, cus=cus)
    assert p.rc == 0 and p.gn and p.token_blocks == 1 and p.gn_units == 3 and p.rounds == (1 if sched == "one_round" else 2), f"{what}: {show(p)}"
    assert p.ntiles * 4 >= S * p.gn_units > (p.ntiles - 1) * 4
    x = rows(M, K, 0, device, 1.4, 0.3)
    w, b = rnd(N, K, scale=K ** -0.5).half(), rnd(N, seed=1) * 0.5
    ab = torch.stack([1 + 0.3 * rnd(S, K, seed=7), 0.5 * rnd(S, K, seed=8)], 2).contiguous().to(device)     # [S][K][2]
    wd, bd = w.to(device).double(), b.to(device).double()
    smp = torch.arange(M, device=device) // GN_ROWS

    xd = x.double()

    def value(sample, shift=1.0):
        a = ab.double()[sample]
        return (xd * a[:, :, 0] + shift * a[:, :, 1]) @ wd.t() + bd

    ref = value(smp)
    tol = tol_of(ref, True)
    need_gap(ref, value((smp + 1) % S), tol, f"{what}: table of the neighbouring sample")
    need_gap(ref, value(smp, 0.0), tol, f"{what}: shift omitted")
    # blocks: the first tile's rows, every sample's last wave block (8 real rows) and the last sample
    tail = (torch.arange(M, device=device) % GN_ROWS) >= 64
    blocks = [("first tile", slice(0, 128), slice(0, N)), ("last wave blocks of the samples", tail, slice(0, N)),
              ("last sample", slice((S - 1) * GN_ROWS, M), slice(0, N)), ("last column pair", slice(0, M), slice(N - 64, N))]
    stream = pack_linear_stream(w.float(), b).to(device)
    return dict(M=M, N=N, K=K, x=x, stream=stream, ab=ab, ref=ref, blocks=blocks, plan=p, what=what)


GN_CASES = [(K, s) for K in (320, 640) for s in ("one_round", "gn_two_rounds")]


# ------------------------------------------------------------------------------------------- 5. output statistics
def stats_ref(out):
    """fp64 (mean, rsqrt(var + eps)) of the STORED fp16 rows."""
    o = out.double()
    return torch.stack([o.mean(1), (o.var(1, unbiased=False) + EPS).rsqrt()], 1)


def stats_conditions(ref, what):
    """Input condition of the statistics comparison: the statistics of the neighbouring row are far from a row's own (references only)."""
    want = stats_ref(ref.half())
    for j, name in enumerate(("mean", "rstd")):
        need_gap(want[:, j], want.roll(1, 0)[:, j], stats_tol(want[:, j]), f"{what}: {name} of the neighbouring row")


STATS_CASES = [(K, s, f) for K in (320, 640) for s in SCHEDULES[K] for f in (1, 5)]


# ------------------------------------------------------------------------------------------- 6. insv2v_ffn_fused
FFN_M, FFN_C, FFN_NH = 2 * 128 + 37, 320, 1280


@cached
def ffn_case(post, device):
    """C = 320 feed-forward (LayerNorm -> Linear(320, 2560) -> h gelu(g) -> Linear(1280, 320) -> + x [-> Wp . + bp + post_residual]) at
    M = 2 x 128 + 37.  fp64 reference on the operands the kernel gets, the hidden activations (and, POST, the feed-forward result that
    feeds the trailing projection) rounded to fp16 once, as in test_ffn_fused_vs_fp32."""
    from insv2v.fused import pack_ffn_stream
    from insv2v.unet import fold_layernorm
    M, C, NH = FFN_M, FFN_C, FFN_NH
    what = f"ffn_fused post={post} M={M}"
    x = (rnd(M, C) * 1.3 + 0.2).half().to(device)
    w1, b1 = rnd(2 * NH, C, scale=C ** -0.5), rnd(2 * NH, seed=1) * 0.3
    w2, b2 = rnd(C, NH, scale=NH ** -0.5, seed=2).half(), rnd(C, seed=3) * 0.3
    gamma, beta = 1 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    wf, _, bf = fold_layernorm(w1, gamma, beta, b1)
    wp, bp = rnd(C, C, scale=C ** -0.5, seed=6).half(), rnd(C, seed=7) * 0.3
    r2 = rnd(M, C, seed=8).half().to(device)
    stream = pack_ffn_stream(wf.float(), bf, w2.float(), b2, post=(wp.float(), bp) if post else None).to(device)
    xd = x.double()
    wfd, bfd, w2d, b2d, wpd, bpd = (t.to(device).double() for t in (wf, bf, w2, b2, wp, bp))

    def value(ln=True, swap=False, resx=True, res2=True):
        y = (F.layer_norm(xd, (C,), eps=EPS) if ln else xd) @ wfd.t() + bfd
        h, g = y.chunk(2, dim=-1)
        if swap:
            h, g = g, h
        ff = (h * F.gelu(g)).half().double() @ w2d.t() + b2d + (xd if resx else 0)
        if not post:
            return ff
        return ff.half().double() @ wpd.t() + bpd + (r2.double() if res2 else 0)

    ref = value()
    tol = tol_of(ref, True)
    need_gap(ref, value(ln=False), tol, f"{what}: LayerNorm omitted")
    need_gap(ref, value(swap=True), tol, f"{what}: h and gate halves exchanged")
    need_gap(ref, value(resx=False), tol, f"{what}: the residual x omitted")
    if post:
        need_gap(ref, value(res2=False), tol, f"{what}: post_residual omitted")
    blocks = [("ragged last tile", slice(256, M), slice(0, C)), ("first 32 channels", slice(0, M), slice(0, 32)), ("last 32 channels", slice(0, M), slice(C - 32, C))]
    return dict(M=M, C=C, NH=NH, x=x, stream=stream, post_residual=r2 if post else None, ref=ref, blocks=blocks, what=what)


# ------------------------------------------------------------------------------------------- every launch of the GPU file
TB12_FORMS = (0, 1, 4, 5)      # TB = 1 against TB = 2: the forms whose rows do not depend on their position (no per-frame bias)
TB12_ROWS = 512


def gn_rows_of(K, sched, cus):
    return gn_samples(K, sched, cus) * GN_ROWS - (19 if sched == "one_round" else 0)


def case_list(cus):
    """Every insv2v_rowlin problem the GPU file launches, with the kernel it CLAIMS (from its name alone) and its shape derived for `cus`:
    dict(name, M, N, K, form, frames, gn_rows, claim = (KS, form, GN, TB), rounds)."""
    out = []

    def add(family, M, N, K, form, sched, frames=FRAMES, gn=False):
        tb, rounds = (1, 2 if sched == "gn_two_rounds" else 1) if gn else EXPECT[sched]
        out.append(dict(name=f"{family} K={K} N={N} {sched} form={form}" + (" GN" if gn else "") + (f" frames={frames}" if frames != FRAMES else ""),
                        M=M, N=N, K=K, form=form, frames=frames, gn_rows=GN_ROWS if gn else 0, claim=(K // 16, form, int(gn), tb), rounds=rounds, sched=sched))

    for K, N, sched, form, frames in form_cases():
        add("forms", schedule_rows(K, sched, cus), N, K, form, sched, frames)
    for K, res, tb in EXACT_CASES:
        add("exact", schedule_rows(K, "tb2" if tb == 2 else "one_round", cus), N_MAIN, K, int(res), "tb2" if tb == 2 else "one_round")
    for K in (320, 640):
        for form in STRIDED_FORMS:
            add("strided", schedule_rows(K, "one_round", cus), N_MAIN, K, form, "one_round")
        add("strided", gn_rows_of(K, "one_round", cus), N_MAIN, K, 0, "one_round", gn=True)
    for K, sched, form in STATS_CASES:
        add("stats", schedule_rows(K, sched, cus), N_MAIN, K, form, sched)
    for form in TB12_FORMS:
        add("tb1 of the tb2 tail", TB12_ROWS, N_MAIN, 640, form, "one_round")
    for K, sched in GN_CASES:
        add("gn", gn_rows_of(K, sched, cus), N_MAIN, K, 0, sched, gn=True)
    return out


def case_plan(c, cus):
    """The plan of a case of case_list at `cus`, asserted to be the kernel and the rounds the case claims."""
    p = plan(c["M"], c["N"], c["K"], c["form"], frames=c["frames"], gn_rows=c["gn_rows"], cus=cus)
    assert p.rc == 0, f"{c['name']}: refused, rc {p.rc}"
    assert kernel_of(p) == c["claim"], f"{c['name']} (M={c['M']}, {cus} CUs) claims {describe(c['claim'])} but the plan says {describe(kernel_of(p))}"
    assert p.rounds == c["rounds"], f"{c['name']} (M={c['M']}, {cus} CUs) claims {c['rounds']} round(s) but the plan says {show(p)}"
    return p


# ------------------------------------------------------------------------------------------- the planner's refusals
EINVAL, EUNSUPPORTED = -1, -2
# (name, the rc insv2v_rowlin documents, arguments of plan()).  Pointers: x = 4096, out = 8192, wstream = 12288, residual = 16384, gn_ab = 20480
REFUSALS = [
    ("K = 512", EUNSUPPORTED, dict(K=512)),
    ("N = 96", EUNSUPPORTED, dict(N=96)),
    ("frames = 17", EUNSUPPORTED, dict(form=2, frames=17)),
    ("frame_bias with rows_per_frame = 0", EUNSUPPORTED, dict(form=2, rows_per_frame=0)),
    ("ldx % 8 != 0", EINVAL, dict(ldx=324)),
    ("a pointer off by 8 bytes", EINVAL, dict(out_off=8)),
    ("gn_ab together with layernorm", EUNSUPPORTED, dict(gn_rows=GN_ROWS, form=4)),
    ("gn_ab together with residual", EUNSUPPORTED, dict(gn_rows=GN_ROWS, form=1)),
    ("gn_rows = 0", EUNSUPPORTED, dict(gn_ab=20480)),
    ("256 * ld * 2 >= 2^31", EUNSUPPORTED, dict(ldo=1 << 22)),
]


REFUSAL_SHAPE = (300, 128, 320)     # M, N, K of the problem every refusal starts from (accepted as it stands)


def refusal_plan(kw, cus=PLAN_CUS):
    """The plan of a refusal: the base problem with the arguments of REFUSALS applied."""
    kw = dict(kw)
    M, N, K = REFUSAL_SHAPE
    if "out_off" in kw:
        kw["out"] = 8192 + kw.pop("out_off")
    return plan(kw.pop("M", M), kw.pop("N", N), kw.pop("K", K), kw.pop("form", 0), cus=cus, **kw)


def refusal_desc(kw, device):
    """The same refusal as a REAL descriptor of insv2v_rowlin: (descriptor, sentinel-filled output buffer, tensors to keep alive)."""
    from insv2v import _lib
    kw = dict(kw)
    M, N, K = REFUSAL_SHAPE
    N, K, form = kw.pop("N", N), kw.pop("K", K), kw.pop("form", 0)
    ln, fr, res = form_bits(form)
    x = rows(M, K, 0, device)
    out = torch.full((M + 1, N + 8), SENTINEL, dtype=torch.float16, device=device)
    wst = torch.zeros(max(int(_lib.load().insv2v_rowlin_stream_elems(N, K)), 4096), dtype=torch.float16, device=device)
    r = rows(M, N, 3, device)
    ab = torch.ones(8, K, 2, dtype=torch.float32, device=device)
    d = _lib.RowLinDesc()
    d.x, d.out, d.wstream, d.ldx, d.ldo = x.data_ptr(), out.data_ptr() + kw.pop("out_off", 0), wst.data_ptr(), K, N
    d.M, d.N, d.K, d.layernorm, d.eps = M, N, K, int(ln), EPS
    if res:
        d.residual, d.ldr = r.data_ptr(), N
    if fr:
        d.frame_bias, d.rows_per_frame, d.frames = 1, kw.pop("rows_per_frame", RPF), kw.pop("frames", FRAMES)
    if "gn_rows" in kw or "gn_ab" in kw:
        kw.pop("gn_ab", None)
        d.gn_ab, d.gn_rows = ab.data_ptr(), kw.pop("gn_rows", 0)
    for key, val in kw.items():
        setattr(d, key, val)
    return d, out, (x, wst, r, ab)
