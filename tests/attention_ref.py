"""Cases, float64 reference, bounds and an fp32 emulation of csrc/attention.hip, shared by tests/test_attention_variants_cpu.py and
tests/test_attention_variants_gpu.py.  Plain torch on the CPU, importable without a GPU.

A case names one call of insv2v_attention and PINS the kernel form it runs (family, D, NW, QB, KVT, FOLD of insv2v_attention_plan).
Its operands are laid out with gaps, so that a read or a store outside the problem shows:
  * every row stride is wider than heads * head_dim (gap columns behind the last head; with heads = 1 directly behind head_dim, where
    the zero-padded contraction columns D .. DP-1 of the kernels lie), every problem has GAP_ROWS gap rows behind its last row;
  * K gaps hold a copy of the problem's own key 0 (a leaked key gets an ordinary logit), V gaps hold +-60000 (finite: an exact zero
    weight on a loaded gap row stays harmless), Q gaps hold ordinary values;
  * the output buffer is prefilled with the bit pattern of an fp16 NaN, gaps included, and every gap element has to keep it.

Reference: float64 softmax attention on the fp16 operands (bias cases: on the fp16 sums q + table[row], which is what the kernel forms).

Bound, per element.  With p_j the float64 weights, A = sum_j p_j |v_j| and S = max_j c2 sum_d |q_d k_jd| (the largest score magnitude in
log2 units, c2 = scale log2(e)):
    |out - ref| <= K_form (2^-10 A + [FOLD] 2^-11 ln2 S A) + 2^-11 |ref| + 2^-24
for the roundings the kernels' comments name: P rounded to fp16 (toward zero in attn_kernel, to nearest in attn_short_kernel), in FOLD
Q scale log2(e) rounded to fp16 before the MFMAs, the output rounded to fp16.  K_form = 8 x the worst K = 1 ratio of emulate() - a plain
fp32 evaluation that rounds where the kernel rounds, in key-tile order and in one pass - against the reference over every listed case,
rounded up to a power of two (test_attention_variants_cpu.py::test_headroom_of_the_bounds measures the ratios and pins K to them).  The
constants come from the emulation, never from the kernels.

Weights that sum to one.  In the `normal` family the last column of every head of V holds the constant CONST_V = 2 - 2^-9.  attn_kernel
normalises by the sum of the ROUNDED probabilities it fed the P.V MFMAs, so that column comes out as CONST_V (1 + e) with |e| <=
(2 seq_k + 8) 2^-24 < 2^-12 from the fp32 sums - less than half an fp16 step at CONST_V (2^-11 relative): it has to be bit-exact.  A row
sum over other probabilities than the MFMAs saw (unrounded ones: -0.7 steps on average; one key more or fewer) moves it by a step or more.
attn_short_kernel rounds P to nearest and normalises by the unrounded sum: up to 2^-11 relative, one step allowed.

emulate(mutate=...) plants one mistake (MUTATIONS); the CPU file shows that each is caught by verdict() on at least one listed case."""
import functools
import math
import zlib

import torch

F64, F32, F16 = torch.float64, torch.float32, torch.float16
EINVAL, EUNSUPPORTED = -1, -2
NONE, SHORT, SHORT_BIAS, GENERIC, SINGLE, SINGLE_REP, D512 = range(7)
FAMILY_NAMES = {NONE: "NONE", SHORT: "SHORT", SHORT_BIAS: "SHORT_BIAS", GENERIC: "GENERIC", SINGLE: "SINGLE", SINGLE_REP: "SINGLE_REP", D512: "D512"}
HEAD_DIMS = (16, 32, 40, 64, 80, 128, 160)
LOG2E = 1.4426950408889634
GAP_ROWS = 3
GAP_COLS = 32                 # q / k / v: >= DP - D of every head dim, a multiple of 8
V_POISON = 60000.0
O_PREFILL = 0x7E5A            # an fp16 NaN: no result equals it
CONST_V = 2.0 - 2.0 ** -9
BIAS_ROWS = 17
PLAN_CUS = 256                # the CU count the pinned plans are asked with (it sizes the persistent short grid only)

# 8 x the worst K = 1 ratio of emulate() over CASES, rounded up to a power of two; the measured ratios: K_MEASURED
# (test_attention_variants_cpu.py::test_headroom_of_the_bounds prints and pins them).
K_MEASURED = {"generic": 0.7111, "fold": 0.2425, "short": 0.6227}
K = {"generic": 8.0, "fold": 2.0, "short": 8.0}

INPUT_FAMILIES = ("normal", "rising", "late_spike", "small_steps", "very_negative", "wide")
EXTREMES = INPUT_FAMILIES[1:]
MUTATIONS = ("ragged_extra_key", "ragged_zero_key", "tile_first_key_dropped", "causal_strict", "no_rescale", "unrounded_sum", "next_head_columns",
             "kv_of_z", "bias_next_row", "store_next_block_row", "scale_without_log2e")


def f32(v):
    return torch.tensor(v, dtype=F32).item()


# ================================================================================================================== cases
def case(name, kind, batch, heads, hd, sq, sk, plan, fam="normal", scale=None, causal=False, bias=False, inner=1, o_off=0, o_gap=4):
    """kind: `spatial` (problem z = rows of sample z), `cross` (K / V of sample z // inner, kv_step = 0) or `temporal` (problem z = pixel
    z % inner of sample z // inner, row stride inner * ld).  plan = (family, D, NW, QB, KVT, FOLD).  o_off: halfs the output base is moved
    by; o_gap: gap columns of the output rows."""
    assert kind in ("spatial", "cross", "temporal") and batch % inner == 0 and fam in INPUT_FAMILIES
    return dict(name=name, kind=kind, batch=batch, heads=heads, hd=hd, sq=sq, sk=sk, plan=tuple(plan), fam=fam, scale=hd ** -0.5 if scale is None else scale,
                causal=causal, bias=bias, inner=inner, o_off=o_off, o_gap=o_gap)


def form_of(c):
    return "short" if c["plan"][0] in (SHORT, SHORT_BIAS) else "fold" if c["plan"][5] else "generic"


def specs(c):
    """{operand: (O, R, I, C)}: the buffer of an operand is [O][R][I][C] halfs - O outer blocks, R rows (the last GAP_ROWS are gap rows), I problems
    interleaved per row (temporal), C columns (the last ones are gap columns).  (cross: K / V get one block per PROBLEM - a kernel that reads
    the K / V of problem z instead of sample z // inner stays inside the buffer and finds poison.)"""
    H, hd, I = c["heads"], c["hd"], c["inner"] if c["kind"] == "temporal" else 1
    Okv = c["batch"] if c["kind"] == "cross" else c["batch"] // c["inner"]
    return dict(q=(c["batch"] // I, c["sq"] + GAP_ROWS, I, H * hd + GAP_COLS), kv=(Okv, c["sk"] + GAP_ROWS, I, H * hd + GAP_COLS),
                o=(c["batch"] // I, c["sq"] + GAP_ROWS, I, H * hd + c["o_gap"]))


def addr(c, which):
    """(inner, outer stride, step, row stride) of insv2v_attention's addressing rule, in halfs."""
    O, R, I, C = specs(c)[which]
    if which == "kv" and c["kind"] == "cross":
        return c["inner"], R * C, 0, C
    return I, R * I * C, C if I > 1 else 0, I * C


def problem_index(c, which, mutate=None):
    """(outer block, interleave slot) of every problem z."""
    O, R, I, C = specs(c)[which]
    z = torch.arange(c["batch"])
    if which == "kv" and c["kind"] == "cross":
        if mutate == "kv_of_z":
            return z, torch.zeros_like(z)
        return z // c["inner"], torch.zeros_like(z)
    return z // I, z % I


def _seed(c):
    """(A `-fallback` case is the same problem as the case it is named after.)"""
    return zlib.crc32(c["name"].replace("-fallback", "").encode()) & 0x7FFFFFFF


def logical_inputs(c):
    """q [Z, H, sq, hd], k, v [Zkv, H, sk, hd] float32 of the case's input family (Zkv = distinct K / V problems)."""
    g = torch.Generator().manual_seed(_seed(c))
    Z, H, hd, sq, sk = c["batch"], c["heads"], c["hd"], c["sq"], c["sk"]
    Zkv = Z // c["inner"] if c["kind"] == "cross" else Z
    rep = Z // Zkv
    q = torch.randn(Z, H, sq, hd, generator=g)
    k = torch.randn(Zkv, H, sk, hd, generator=g)
    v = torch.randn(Zkv, H, sk, hd, generator=g)
    sg = torch.sign(torch.randn(Zkv, H, 1, hd, generator=g))          # one sign pattern per K / V problem
    sgq = sg.repeat_interleave(rep, 0)
    idx = torch.arange(sk).view(1, 1, sk, 1).float()
    nat = 1.0 / (abs(c["scale"]) * 0.8 * hd)                            # |k| that gives a logit of one nat against q = |q| sg
    fam = c["fam"]
    if fam == "rising":          # key norms grow with the key index: the maximum moves in almost every tile
        k = k * (0.5 + 3.0 * idx / sk)
        q = q * 2
    elif fam == "late_spike":    # one key near the end matches every query ~9 nats above the rest: one big move in the last tile
        q = q.abs() * sgq
        k[:, :, max(sk - 3, 0)] = (9.0 * nat * sg)[:, :, 0]
    elif fam == "small_steps":   # the maximum creeps up a little per tile (FOLD: the lazy path keeps probabilities > 1)
        q = q.abs() * sgq
        k = k * 0.2 + sg * (idx / sk) * 6.0 * nat
    elif fam == "very_negative":  # every score far below zero, the least negative ones last: the maximum climbs through negative values
        q = q.abs() * sgq
        k = k * 0.1 - sg * (12.0 - 8.0 * idx / sk) * nat
    elif fam == "wide":          # logits spread over +-40 (log2 units) at random
        q, k = q * 3.5, k * 3.5
    else:
        v[..., hd - 1] = CONST_V
    return q, k, v


def _scatter(x, O, R, I, C, s, Hhd, base):
    """Logical [Z, H, s, hd] (Z = O I) into the real region of a buffer image [O, R, I, C] that starts as `base`."""
    Z, H, _, hd = x.shape
    base[:, :s, :, :Hhd] = x.reshape(O, I, H, s, hd).permute(0, 3, 1, 2, 4).reshape(O, s, I, Hhd)
    return base


def make(c):
    """The operands of a case: fp16 buffers q, k, v (flat), the bias table or None, all on the CPU."""
    g = torch.Generator().manual_seed(_seed(c) ^ 0x5A5A)
    H, hd, sq, sk = c["heads"], c["hd"], c["sq"], c["sk"]
    Hhd = H * hd
    q, k, v = logical_inputs(c)
    sp = specs(c)
    Oq, Rq, Iq, Cq = sp["q"]
    Ok, Rk, Ik, Ck = sp["kv"]
    qb = _scatter(q, Oq, Rq, Iq, Cq, sq, Hhd, torch.randn(Oq, Rq, Iq, Cq, generator=g))
    Zb = k.shape[0] // Ik                                       # blocks that hold problems (cross: the others are gap blocks)
    kb = torch.zeros(Ok, Rk, Ik, Ck)
    _scatter(k, Zb, Rk, Ik, Ck, sk, Hhd, kb[:Zb])
    kb[:, :, :, Hhd:] = kb[:, :1, :, :Ck - Hhd]              # gap columns: the first columns of key 0
    kb[:, sk:] = kb[:, :1]                                      # gap rows: key 0
    kb[Zb:] = kb[:1, :1]                                        # gap blocks: key 0 of the first sample
    r, col = torch.arange(Rk).view(1, Rk, 1, 1), torch.arange(Ck).view(1, 1, 1, Ck)
    poison = V_POISON * (1.0 - 2.0 * ((r + col) % 2)).expand(Ok, Rk, Ik, Ck)
    vb = poison.clone()
    _scatter(v, Zb, Rk, Ik, Ck, sk, Hhd, vb[:Zb])
    table = None
    if c["bias"]:
        table = 0.5 * torch.randn(BIAS_ROWS, 3 * Hhd, generator=g)
        if c["fam"] == "normal":
            table[:, 2 * Hhd + hd - 1::hd] = 0.0               # the constant column of V stays constant
        table = table.half()
    return dict(q=qb.half().reshape(-1), k=kb.half().reshape(-1), v=vb.half().reshape(-1), table=table)


def o_numel(c):
    O, R, I, C = specs(c)["o"]
    return c["o_off"] + O * R * I * C


def o_prefill(c):
    return torch.full((o_numel(c),), O_PREFILL, dtype=torch.int16).view(F16)


def gather(c, buf, which, width, mutate=None):
    """[Z, H, R, width] of a flat buffer: columns head * hd .. + width of every row (gap rows included) of every problem."""
    O, R, I, C = specs(c)[which]
    zo, zi = problem_index(c, which, mutate)
    rows = buf.view(O, R, I, C)[zo, :, zi, :]
    cols = torch.arange(c["heads"]).view(-1, 1) * c["hd"] + torch.arange(width).view(1, -1)
    return rows[:, :, cols].permute(0, 2, 1, 3)


def operands(c, data, width=None, mutate=None):
    """fp16 q [Z, H, Rq, width], k [Z, H, Rk, width], v [Z, H, Rk, hd] as the kernel sees them (the bias tables added in fp16), gap rows included."""
    hd = c["hd"]
    width = width or hd
    q, k, v = gather(c, data["q"], "q", width), gather(c, data["k"], "kv", width, mutate), gather(c, data["v"], "kv", hd, mutate)
    if c["bias"]:
        Hhd = c["heads"] * hd
        t = data["table"].float()

        def rows_of(n, part):                                               # [1, H, n, hd]: the table rows of sequence positions 0 .. n-1
            i = (torch.arange(n) + (1 if mutate == "bias_next_row" else 0)).clamp(max=BIAS_ROWS - 1)
            cols = part * Hhd + torch.arange(c["heads"]).view(-1, 1) * hd + torch.arange(hd).view(1, -1)
            return t[i][:, cols].permute(1, 0, 2)[None]
        q, k, v = (_pad_add(x, rows_of(x.shape[2], part)).half() for part, x in enumerate((q, k, v)))    # one fp16 rounding = the kernel's fp16 add
    return q, k, v


def _pad_add(x, t):
    """x [.., width] + t [.., hd] on the first hd columns (float32)."""
    y = x.float().clone()
    y[..., :t.shape[-1]] += t
    return y


def visible(c, nq, nk, nvis=None, strict=False):
    """[nq, nk] bool: key j visible to query i."""
    i, j = torch.arange(nq).view(-1, 1), torch.arange(nk).view(1, -1)
    m = (j < (c["sk"] if nvis is None else nvis)).expand(nq, nk)
    if c["causal"]:
        m = m & ((j < i) if strict else (j <= i))
    return m


def reference(c, data):
    """dict(ref, A [Z, H, sq, hd], S [Z, H, sq]) in float64 on the fp16 operands."""
    q, k, v = operands(c, data)
    sq, sk = c["sq"], c["sk"]
    q, k, v = q[:, :, :sq].double(), k[:, :, :sk].double(), v[:, :, :sk].double()
    vis = visible(c, sq, sk)
    s = (q @ k.transpose(-1, -2)) * f32(c["scale"])
    p = torch.softmax(s.masked_fill(~vis, float("-inf")), -1)
    c2 = f32(c["scale"]) * LOG2E
    S = ((q.abs() @ k.abs().transpose(-1, -2)) * abs(c2)).masked_fill(~vis, 0.0).amax(-1)
    return dict(ref=p @ v, A=p @ v.abs(), S=S, logits=s.masked_fill(~vis, float("-inf")))


def bound(c, r, k=None):
    kf = (k or K)[form_of(c)]
    fold = 2.0 ** -11 * math.log(2.0) * r["S"][..., None] * r["A"] if c["plan"][5] else 0.0
    return kf * (2.0 ** -10 * r["A"] + fold) + 2.0 ** -11 * r["ref"].abs() + 2.0 ** -24


def moved_fraction(c, r):
    """Share of the query rows whose running maximum moves in a key tile after the first (kvt of the pinned plan)."""
    kvt = c["plan"][4]
    if c["sk"] <= kvt:
        return None
    lg = r["logits"]
    return (lg[..., kvt:].amax(-1) > lg[..., :kvt].amax(-1)).double().mean().item()


# ================================================================================================================== fp32 emulation
def rtz16(x):
    """fp32 >= 0 -> the fp16 toward zero, as fp32 (v_cvt_pkrtz_f16_f32)."""
    h = x.half()
    up = h.float() > x
    return torch.where(up, (h.view(torch.int16) - up.to(torch.int16)).view(F16), h).float()


def _emu_tiles(c, q, k, v, mutate):
    """attn_kernel in fp32: key tiles of KVT in order, online softmax, P rounded toward zero, normalised by the sum of the rounded P."""
    _, D, NW, QB, kvt, fold = c["plan"]
    sk = c["sk"]
    Z, H, Rq, _ = q.shape
    Rk = k.shape[2]
    c2 = (torch.tensor(c["scale"], dtype=F32) * torch.tensor(LOG2E, dtype=F32)) if mutate != "scale_without_log2e" else torch.tensor(c["scale"], dtype=F32)
    qf, kf, vf = q.float(), k.float(), v.float()
    if fold:
        qf = (qf * c2).half().float()
    nvis = sk
    if mutate in ("ragged_extra_key", "ragged_zero_key") and sk % kvt:
        nvis = sk + 1
        if mutate == "ragged_zero_key":       # the mask alone admits it: the tile load has zeroed the row
            kf, vf = kf.clone(), vf.clone()
            kf[:, :, sk], vf[:, :, sk] = 0.0, 0.0
    vis_all = visible(c, Rq, Rk, nvis, strict=mutate == "causal_strict")
    ntiles = (sk + kvt - 1) // kvt
    if mutate == "gap_key":                   # (not a planted mistake: the condition every poisoned case has to meet) the first gap row, whatever the masks say
        vis_all = vis_all.clone()
        vis_all[:, sk] = True
        ntiles = (sk + kvt) // kvt
    m = torch.zeros(Z, H, Rq, 1) if fold else torch.full((Z, H, Rq, 1), -1.0e30)
    l = torch.zeros(Z, H, Rq, 1)
    acc = torch.zeros(Z, H, Rq, v.shape[-1])
    for t in range(ntiles):
        j0, j1 = t * kvt, min((t + 1) * kvt, Rk)
        vis = vis_all[:, j0:j1].clone()
        if mutate == "tile_first_key_dropped" and (t >= 1 or ntiles == 1):
            vis[:, 0] = False
        s = qf @ kf[:, :, j0:j1].transpose(-1, -2)
        if fold:
            s = (s - m).masked_fill(~vis, -1.0e30)
            rowtrig = (s > 8.0).any(-1)
            rowtrig[:, :, c["sq"]:] = False                                  # (rows behind seq_q are zero queries in the kernel)
            nb = (Rq + 15) // 16
            pad = torch.zeros(Z, H, nb * 16, dtype=torch.bool)
            pad[:, :, :Rq] = rowtrig
            trig = pad.view(Z, H, nb, 16).any(-1, keepdim=True).expand(Z, H, nb, 16).reshape(Z, H, nb * 16)[:, :, :Rq, None]
            if t == 0:
                trig = torch.ones_like(trig)
            mx = s.amax(-1, keepdim=True)
            want = m + (mx if t == 0 else mx.clamp(min=0.0))
            mnew = torch.where(trig, want.half().float(), m)
            shift = mnew - m
            if t > 0 and mutate != "no_rescale":
                alpha = torch.exp2(-shift)
                l, acc = l * alpha, acc * alpha
            s, m = s - shift, mnew
            e = torch.exp2(s)
        else:
            s = s.masked_fill(~vis, -1.0e30)
            mx = torch.maximum(m, s.amax(-1, keepdim=True))
            if mutate != "no_rescale":
                alpha = torch.exp2((m - mx) * c2)
                l, acc = l * alpha, acc * alpha
            m = mx
            e = torch.exp2(s * c2 - mx * c2)
        p = rtz16(e)
        l = l + (e if mutate == "unrounded_sum" else p).sum(-1, keepdim=True)
        acc = acc + p @ vf[:, :, j0:j1]
    return (acc * (1.0 / l)).half()


def _emu_short(c, q, k, v, mutate):
    """attn_short_kernel in fp32: one block of <= 16 keys, P rounded to nearest, normalised by the unrounded sum."""
    sk = c["sk"]
    c2 = (torch.tensor(c["scale"], dtype=F32) * torch.tensor(LOG2E, dtype=F32)) if mutate != "scale_without_log2e" else torch.tensor(c["scale"], dtype=F32)
    qf, kf, vf = q.float(), k.float(), v.float()
    nvis = sk
    if mutate in ("ragged_extra_key", "ragged_zero_key") and sk < 16:
        nvis = sk + 1
        if mutate == "ragged_zero_key":
            kf, vf = kf.clone(), vf.clone()
            kf[:, :, sk], vf[:, :, sk] = 0.0, 0.0
    vis = visible(c, q.shape[2], k.shape[2], nvis).clone()
    if mutate == "gap_key":
        vis[:, sk] = True
    if mutate == "tile_first_key_dropped":
        vis[:, 0] = False
    s = (qf @ kf.transpose(-1, -2)).masked_fill(~vis, -1.0e30)
    mx = s.amax(-1, keepdim=True)
    e = torch.exp2(s * c2 - mx * c2)
    l = e.sum(-1, keepdim=True)
    return ((e.half().float() @ vf) * (1.0 / l)).half()


def emulate(c, data, mutate=None):
    """The output buffer (flat fp16, prefilled) of an fp32 evaluation that rounds where the kernel of the pinned plan rounds."""
    hd = c["hd"]
    width = (hd + 31) // 32 * 32 if mutate == "next_head_columns" else hd
    q, k, v = operands(c, data, width, mutate)
    rows = (_emu_short if form_of(c) == "short" else _emu_tiles)(c, q, k, v, mutate)        # [Z, H, Rq, hd], gap rows included
    nstore = c["sq"] + (1 if mutate == "store_next_block_row" and c["sq"] % 16 else 0)
    return store(c, rows, nstore)


def store(c, rows, nstore=None):
    """Rows [Z, H, >= nstore, hd] fp16 into a prefilled output buffer."""
    O, R, I, C = specs(c)["o"]
    nstore = c["sq"] if nstore is None else nstore
    Z, H, _, hd = rows.shape
    out = o_prefill(c)
    o4 = out[c["o_off"]:].view(O, R, I, C)
    o4[:, :nstore, :, :H * hd] = rows[:, :, :nstore].reshape(O, I, H, nstore, hd).permute(0, 3, 1, 2, 4).reshape(O, nstore, I, H * hd)
    return out


def real_rows(c, out):
    """[Z, H, sq, hd] of a flat output buffer."""
    O, R, I, C = specs(c)["o"]
    H, hd, sq = c["heads"], c["hd"], c["sq"]
    o4 = out[c["o_off"]:].view(O, R, I, C)[:, :sq, :, :H * hd]
    return o4.reshape(O, sq, I, H, hd).permute(0, 2, 3, 1, 4).reshape(O * I, H, sq, hd)


def gap_mask(c):
    O, R, I, C = specs(c)["o"]
    m = torch.ones(o_numel(c), dtype=torch.bool)
    m[c["o_off"]:].view(O, R, I, C)[:, :c["sq"], :, :c["heads"] * c["hd"]] = False
    return m


def verdict(c, r, out, k=None):
    """What the GPU file asserts of an output buffer: dict(ratio = max |out - ref| / bound, gaps = gap elements that lost the prefill,
    ones = elements of the constant column off by more than allowed)."""
    out = out.cpu()
    got = real_rows(c, out).double()
    ratio = ((got - r["ref"]).abs() / bound(c, r, k))
    ratio = float("inf") if not torch.isfinite(got).all() else ratio.max().item()
    gaps = int((out.view(torch.int16)[gap_mask(c)] != O_PREFILL).sum())
    ones = 0
    if c["fam"] == "normal":
        tol = 2.0 ** -10 if form_of(c) == "short" else 0.0
        ones = int(((got[..., c["hd"] - 1] - CONST_V).abs() > tol).sum())
    return dict(ratio=ratio, gaps=gaps, ones=ones)


def passes(v):
    return v["ratio"] <= 1 and v["gaps"] == 0 and v["ones"] == 0


@functools.lru_cache(maxsize=None)
def prepared(name):
    """(case, data, reference) of a listed case, computed once and shared (do not modify)."""
    c = BY_NAME[name]
    data = make(c)
    return c, data, reference(c, data)


# ================================================================================================================== planner
def desc(c=None, **over):
    """insv2v_attention_desc of a case (pointers: only their null and alignment bits matter to the planner), or of keyword fields alone."""
    from insv2v import _lib
    d = _lib.AttentionDesc()
    if c is not None:
        d.q, d.k, d.v, d.o = 4096, 8192, 12288, 16384 + 2 * c["o_off"]
        d.q_inner, d.q_outer, d.q_step, d.q_rs = addr(c, "q")
        d.kv_inner, d.kv_outer, d.kv_step, d.k_rs = addr(c, "kv")
        d.v_rs = d.k_rs
        d.o_inner, d.o_outer, d.o_step, d.o_rs = addr(c, "o")
        d.batch, d.heads, d.head_dim, d.seq_q, d.seq_k, d.scale, d.causal = c["batch"], c["heads"], c["hd"], c["sq"], c["sk"], c["scale"], int(c["causal"])
        if c["bias"]:
            Hhd = c["heads"] * c["hd"]
            d.q_bias, d.k_bias, d.v_bias, d.bias_rs = 32768, 32768 + 2 * Hhd, 32768 + 4 * Hhd, 3 * Hhd
    for key, val in over.items():
        setattr(d, key, val)
    return d


def plain_desc(batch=1, heads=1, hd=64, sq=64, sk=64, rs=None, **over):
    """A valid contiguous self-attention descriptor, for the planner's refusals and sweeps."""
    rs = rs or heads * hd
    kw = dict(q=4096, k=8192, v=12288, o=16384, q_rs=rs, k_rs=rs, v_rs=rs, o_rs=rs, q_inner=1, kv_inner=1, o_inner=1, q_outer=sq * rs, kv_outer=sk * rs,
              o_outer=sq * rs, batch=batch, heads=heads, head_dim=hd, seq_q=sq, seq_k=sk, scale=1.0)
    kw.update(over)
    return desc(None, **kw)


def with_bias(d):
    Hhd = d.heads * d.head_dim
    d.q_bias, d.k_bias, d.v_bias, d.bias_rs = 32768, 32768 + 2 * Hhd, 32768 + 4 * Hhd, 3 * Hhd
    return d


def plan(d, cus=PLAN_CUS):
    import ctypes
    from insv2v import _lib
    p = _lib.AttentionPlan()
    assert _lib.load().insv2v_attention_plan(ctypes.byref(d), cus, ctypes.byref(p)) == 0
    return p


def plan_tuple(p):
    return (p.family, p.d, p.nw, p.qb, p.kvt, p.fold)


def describe(t):
    return f"{FAMILY_NAMES.get(t[0], t[0])} D={t[1]} NW={t[2]} QB={t[3]} KVT={t[4]} FOLD={t[5]}"


def check_case_plan(c):
    p = plan(desc(c))
    assert p.rc == 0, f"{c['name']}: refused with rc {p.rc}"
    assert plan_tuple(p) == c["plan"], f"case {c['name']} has drifted to another form: it runs {describe(plan_tuple(p))}, pinned {describe(c['plan'])}"
    return p


# ================================================================================================================== case lists
def _gen(hd, nw, qb, fold=0):
    return (GENERIC, hd, nw, qb, 64 if nw >= 4 else 32, fold)


FOLD_DIMS = (40, 80)            # the head dims with a spare contraction column; folded in the workgroups of 4 and 8 waves
SMALL_DIMS = (16, 32, 40, 64, 80)   # the head dims of the two-query-block forms (head_dim <= 96)


def _build():
    L = []

    def add(*a, **kw):
        L.append(case(*a, **kw))

    def families(prefix, kind, batch, heads, hd, sq, sk, plan, **kw):
        for fam in EXTREMES:
            add(f"{prefix}-{fam}", kind, batch, heads, hd, sq, sk, plan, fam=fam, **kw)

    # ---- <1,1>: seq_q <= 16 with more than 16 keys (or causal); 32-key tiles
    for hd in HEAD_DIMS:
        add(f"g11-d{hd}-q5-k33", "spatial", 2, 2, hd, 5, 33, _gen(hd, 1, 1))
        add(f"g11-d{hd}-q16-k65", "spatial", 1, 3, hd, 16, 65, _gen(hd, 1, 1))
    for sq in (5, 16):
        for sk in (31, 32, 33, 65):
            add(f"g11-d40-q{sq}-k{sk}-grid", "spatial", 2, 2, 40, sq, sk, _gen(40, 1, 1))
    families("g11-d64-q16-k65", "spatial", 2, 2, 64, 16, 65, _gen(64, 1, 1))
    add("g11-d64-q16-k65-scale", "spatial", 2, 2, 64, 16, 65, _gen(64, 1, 1), scale=0.23)
    add("g11-d40-q16-k33-cols", "spatial", 3, 1, 40, 16, 33, _gen(40, 1, 1))
    add("g11-d32-q16-k33-cross", "cross", 4, 2, 32, 16, 33, _gen(32, 1, 1), inner=2)
    add("g11-d80-q12-k20-temporal", "temporal", 6, 2, 80, 12, 20, _gen(80, 1, 1), inner=3)
    add("g11-d64-q16-k16-causal", "spatial", 2, 2, 64, 16, 16, _gen(64, 1, 1), causal=True)
    add("g11-d40-q13-k13-causal", "spatial", 2, 3, 40, 13, 13, _gen(40, 1, 1), causal=True)
    add("g11-d32-q16-k33-place", "spatial", 7, 3, 32, 16, 33, _gen(32, 1, 1))
    add("g11-d160-q16-k16-h16", "temporal", 4, 16, 160, 16, 16, _gen(160, 1, 1), inner=2)     # the short kernel's LDS would be 100 KiB
    # ---- <2,1>: 17 .. 32 queries
    for hd in HEAD_DIMS:
        add(f"g21-d{hd}-q17-k33", "spatial", 2, 2, hd, 17, 33, _gen(hd, 2, 1))
        add(f"g21-d{hd}-q32-k65", "spatial", 1, 3, hd, 32, 65, _gen(hd, 2, 1))
    for sq in (17, 32):
        for sk in (31, 32, 33, 65):
            add(f"g21-d80-q{sq}-k{sk}-grid", "spatial", 2, 2, 80, sq, sk, _gen(80, 2, 1))
    families("g21-d16-q32-k65", "spatial", 2, 2, 16, 32, 65, _gen(16, 2, 1))
    add("g21-d16-q32-k65-scale", "spatial", 2, 2, 16, 32, 65, _gen(16, 2, 1), scale=0.23)
    add("g21-d80-q17-k33-cols", "spatial", 3, 1, 80, 17, 33, _gen(80, 2, 1))
    add("g21-d64-q32-k33-cross", "cross", 4, 2, 64, 32, 33, _gen(64, 2, 1), inner=2)
    add("g21-d40-q24-k24-temporal", "temporal", 6, 2, 40, 24, 24, _gen(40, 2, 1), inner=3)
    add("g21-d128-q17-k31-place", "spatial", 7, 3, 128, 17, 31, _gen(128, 2, 1))
    # ---- <4,1>: 33 .. 127 queries, or head_dim > 96; 64-key tiles; folded at d = 40 / 80
    for hd in HEAD_DIMS:
        f = int(hd in FOLD_DIMS)
        add(f"g41-d{hd}-q33-k63", "spatial", 2, 2, hd, 33, 63, _gen(hd, 4, 1, f))
        add(f"g41-d{hd}-q65-k65", "spatial", 1, 3, hd, 65, 65, _gen(hd, 4, 1, f))           # (d = 160: SINGLE's shape, but the output rows are 8-byte aligned)
        add(f"g41-d{hd}-q127-k129", "spatial", 1, 2, hd, 127, 129, _gen(hd, 4, 1, f))
    for sq in (33, 64, 65, 127):
        for sk in (63, 64, 65, 129):
            add(f"g41-d40-q{sq}-k{sk}-grid", "spatial", 1, 2, 40, sq, sk, _gen(40, 4, 1, 1))
    add("g41-d160-q257-k136", "spatial", 1, 2, 160, 257, 136, _gen(160, 4, 1))
    families("g41-d40-q64-k129", "spatial", 2, 2, 40, 64, 129, _gen(40, 4, 1, 1))
    families("g41-d64-q64-k129", "spatial", 2, 2, 64, 64, 129, _gen(64, 4, 1))
    families("g41-d160-q33-k129", "spatial", 1, 2, 160, 33, 129, _gen(160, 4, 1))
    add("g41-d40-q64-k129-scale", "spatial", 2, 2, 40, 64, 129, _gen(40, 4, 1, 1), scale=0.23)
    add("g41-d64-q64-k129-scale", "spatial", 2, 2, 64, 64, 129, _gen(64, 4, 1), scale=0.23)
    add("g41-d40-q65-k65-cols", "spatial", 3, 1, 40, 65, 65, _gen(40, 4, 1, 1))
    add("g41-d80-q65-k65-cols", "spatial", 3, 1, 80, 65, 65, _gen(80, 4, 1, 1))
    add("g41-d16-q65-k65-cols", "spatial", 3, 1, 16, 65, 65, _gen(16, 4, 1))
    add("g41-d40-q96-k77-cross", "cross", 6, 2, 40, 96, 77, _gen(40, 4, 1, 1), inner=3)
    add("g41-d32-q40-k40-temporal", "temporal", 4, 2, 32, 40, 40, _gen(32, 4, 1), inner=2)
    add("g41-d64-q77-k77-causal", "spatial", 2, 2, 64, 77, 77, _gen(64, 4, 1), causal=True)     # the CLIP text tower
    add("g41-d40-q65-k65-causal", "spatial", 2, 2, 40, 65, 65, _gen(40, 4, 1, 1), causal=True)
    add("g41-d80-q64-k65-place", "spatial", 6, 3, 80, 64, 65, _gen(80, 4, 1, 1))
    add("g41-d128-q64-k65-place", "spatial", 6, 3, 128, 64, 65, _gen(128, 4, 1))
    # ---- <4,2>: >= 128 queries at head_dim <= 96
    for hd in SMALL_DIMS:
        f = int(hd in FOLD_DIMS)
        add(f"g42-d{hd}-q128-k77", "spatial", 2, 2, hd, 128, 77, _gen(hd, 4, 2, f))
        add(f"g42-d{hd}-q136-k136", "spatial", 1, 3, hd, 136, 136, _gen(hd, 4, 2, f))
        add(f"g42-d{hd}-q257-k128", "spatial", 1, 2, hd, 257, 128, _gen(hd, 4, 2, f))
    for hd in (40, 64, 80):
        families(f"g42-d{hd}-q128-k136", "spatial", 1, 2, hd, 128, 136, _gen(hd, 4, 2, int(hd in FOLD_DIMS)))
    add("g42-d80-q128-k136-scale", "spatial", 1, 2, 80, 128, 136, _gen(80, 4, 2, 1), scale=0.23)
    add("g42-d40-q136-k77-cols", "spatial", 2, 1, 40, 136, 77, _gen(40, 4, 2, 1))
    add("g42-d64-q136-k77-cols", "spatial", 2, 1, 64, 136, 77, _gen(64, 4, 2))
    add("g42-d80-q128-k77-cross", "cross", 4, 2, 80, 128, 77, _gen(80, 4, 2, 1), inner=2)
    add("g42-d16-q130-k130-temporal", "temporal", 2, 2, 16, 130, 130, _gen(16, 4, 2), inner=2)
    add("g42-d40-q136-k77-place", "spatial", 3, 3, 40, 136, 77, _gen(40, 4, 2, 1))
    add("g42-d32-q136-k77-place", "spatial", 3, 3, 32, 136, 77, _gen(32, 4, 2))
    # ---- <8,2>: seq_q a multiple of 256 from 512 on, head_dim <= 96
    for hd in SMALL_DIMS:
        add(f"g82-d{hd}-q512-k200", "spatial", 1, 2, hd, 512, 200, _gen(hd, 8, 2, int(hd in FOLD_DIMS)))
    for sk in (77, 512):
        add(f"g82-d40-q512-k{sk}", "spatial", 1, 2, 40, 512, sk, _gen(40, 8, 2, 1))
        add(f"g82-d64-q512-k{sk}", "spatial", 1, 1, 64, 512, sk, _gen(64, 8, 2))
    families("g82-d80-q512-k200", "spatial", 1, 1, 80, 512, 200, _gen(80, 8, 2, 1))
    families("g82-d32-q512-k200", "spatial", 1, 1, 32, 512, 200, _gen(32, 8, 2))
    add("g82-d40-q512-k200-scale", "spatial", 1, 2, 40, 512, 200, _gen(40, 8, 2, 1), scale=0.23)
    add("g82-d40-q512-k77-cols", "spatial", 1, 1, 40, 512, 77, _gen(40, 8, 2, 1))
    add("g82-d16-q512-k77-cols", "spatial", 1, 1, 16, 512, 77, _gen(16, 8, 2))
    add("g82-d40-q512-k77-cross", "cross", 2, 2, 40, 512, 77, _gen(40, 8, 2, 1), inner=2)
    add("g82-d32-q512-k512-temporal", "temporal", 2, 1, 32, 512, 512, _gen(32, 8, 2), inner=2)
    add("g82-d80-q512-k77-place", "spatial", 3, 3, 80, 512, 77, _gen(80, 8, 2, 1))
    add("g82-d64-q512-k77-place", "spatial", 3, 3, 64, 512, 77, _gen(64, 8, 2))
    # ---- SINGLE / SINGLE_REP: d = 160, 65 .. 96 queries, <= 96 keys in one tile, 16-byte aligned output rows
    single, rep = (SINGLE, 160, 6, 1, 96, 0), (SINGLE_REP, 160, 6, 1, 96, 0)
    for sq in (65, 80, 96):
        for sk in (20, 77, 96):
            add(f"single-q{sq}-k{sk}", "spatial", 2, 2, 160, sq, sk, single, o_gap=8)
    for sq in (65, 96):
        for sk in (20, 77, 96):
            add(f"rep-q{sq}-k{sk}", "cross", 4, 2, 160, sq, sk, rep, inner=2, o_gap=8)
    add("rep-q80-k77", "cross", 4, 2, 160, 80, 77, rep, inner=2, o_gap=8)
    add("single-q80-k77-inner1-cross", "cross", 3, 2, 160, 80, 77, single, inner=1, o_gap=8)
    add("single-q80-k80-temporal", "temporal", 4, 2, 160, 80, 80, single, inner=2, o_gap=8)
    families("single-q80-k77", "spatial", 2, 2, 160, 80, 77, single, o_gap=8)
    families("rep-q80-k77", "cross", 4, 2, 160, 80, 77, rep, inner=2, o_gap=8)
    add("single-q80-k77-scale", "spatial", 2, 2, 160, 80, 77, single, o_gap=8, scale=0.23)
    add("single-q80-k77-cols", "spatial", 3, 1, 160, 80, 77, single, o_gap=8)
    add("rep-q80-k77-cols", "cross", 4, 1, 160, 80, 77, rep, inner=2, o_gap=8)
    add("single-q96-k96-place", "spatial", 6, 3, 160, 96, 96, single, o_gap=8)
    add("rep-q96-k77-place", "cross", 12, 3, 160, 96, 77, rep, inner=2, o_gap=8)
    add("single-q80-k77-fallback", "spatial", 2, 2, 160, 80, 77, _gen(160, 4, 1), o_gap=8, o_off=4)     # the same problem, output moved by 8 bytes
    add("rep-q80-k77-fallback", "cross", 4, 2, 160, 80, 77, _gen(160, 4, 1), inner=2, o_gap=8, o_off=4)
    # ---- the short kernel: <= 16 queries and keys, one wave per head; with and without the bias tables
    for hd in HEAD_DIMS:
        for n in (1, 7, 13, 16):
            add(f"short-d{hd}-n{n}", "temporal", 4, 2 if hd > 64 else 3, hd, n, n, (SHORT, hd, 2 if hd > 64 else 3, 1, 16, 0), inner=2)
            add(f"shortb-d{hd}-n{n}", "temporal", 4, 2 if hd > 64 else 3, hd, n, n, (SHORT_BIAS, hd, 2 if hd > 64 else 3, 1, 16, 0), inner=2, bias=True)
    for sq, sk in ((7, 13), (16, 5), (1, 16)):
        add(f"short-d40-q{sq}-k{sk}", "spatial", 3, 2, 40, sq, sk, (SHORT, 40, 2, 1, 16, 0))
        add(f"shortb-d80-q{sq}-k{sk}", "spatial", 3, 2, 80, sq, sk, (SHORT_BIAS, 80, 2, 1, 16, 0), bias=True)
    families("short-d40-n13", "temporal", 4, 2, 40, 13, 13, (SHORT, 40, 2, 1, 16, 0), inner=2)
    families("shortb-d160-n16", "temporal", 4, 2, 160, 16, 16, (SHORT_BIAS, 160, 2, 1, 16, 0), inner=2, bias=True)
    add("short-d64-n13-scale", "temporal", 4, 2, 64, 13, 13, (SHORT, 64, 2, 1, 16, 0), inner=2, scale=0.23)
    add("short-d40-n13-cols", "temporal", 4, 1, 40, 13, 13, (SHORT, 40, 1, 1, 16, 0), inner=2)
    add("shortb-d16-n13-cols", "temporal", 4, 1, 16, 13, 13, (SHORT_BIAS, 16, 1, 1, 16, 0), inner=2, bias=True)
    add("short-d32-n7-k13-cross", "cross", 4, 2, 32, 7, 13, (SHORT, 32, 2, 1, 16, 0), inner=2)
    add("short-d40-n16-h12", "temporal", 4, 12, 40, 16, 16, (SHORT, 40, 12, 1, 16, 0), inner=2)
    add("short-d16-n16-h16", "temporal", 4, 16, 16, 16, 16, (SHORT, 16, 16, 1, 16, 0), inner=2)
    add("shortb-d160-n16-h8", "temporal", 4, 8, 160, 16, 16, (SHORT_BIAS, 160, 8, 1, 16, 0), inner=2, bias=True)
    add("short-d80-n13-place", "temporal", 18, 3, 80, 13, 13, (SHORT, 80, 3, 1, 16, 0), inner=3)
    add("shortb-d16-n16-persistent", "temporal", 600, 2, 16, 16, 16, (SHORT_BIAS, 16, 2, 1, 16, 0), inner=300, bias=True)   # more problems than workgroups
    return L


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
PLACEMENT = [c["name"] for c in CASES if c["name"].endswith("-place")]
CAUSAL = [c["name"] for c in CASES if c["causal"]]
