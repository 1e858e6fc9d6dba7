"""Float64 restatements of csrc/norm.hip (GroupNorm, LayerNorm with the temporal PE add, row softmax), the case lists that
tests/test_norm_stages_cpu.py and tests/test_norm_stages_gpu.py share, and the bounds both apply.  Plain torch on the CPU, no kernel tricks.

Every reference takes `mutate=`: one realistic error planted into it (MUTATIONS).  tests/test_norm_stages_cpu.py shows that each of them
violates the bounds below on at least one listed case - a case list or a bound too weak to notice a planted error fails there - and that a
plain fp32 evaluation of the same formulas satisfies every bound (that is where the constants K come from).

Bounds (all references float64 on the same fp16 inputs; ulp16(ref) = one fp16 step at |ref|, floored at 2^-24):
  y        |y - ref| <= ulp16(ref) + K_Y 2^-23 (|x| + |mean| [+ |pe|]) rstd |gamma| L          L = 1.1 with SiLU, else 1
  softmax  |y - ref| <= ulp16(ref) + K_SOFTMAX 2^-23 cols^(1/2) ref
  mean     |mean - ref| <= K_MEAN 2^-23 (|mean_ref| + sigma_ref)
  rstd     |rstd / rstd_ref - 1| <= K_RSTD 2^-23 n^(1/2) (1 + shift^2 / (var + eps))
           n = elements reduced; shift = distance of the reduction's centre from the true mean: the three-pass form centres every channel
           on the sample's first token (the largest such distance over the group's channels is taken), the two-pass kernels on the mean
  ab       a = rstd gamma, b = beta - mean a: the two expressions above propagated, plus one fp32 rounding of each product and sum
K = 8 x the worst ratio of the fp32 restatement's error to the expression with K = 1, rounded up to a power of two
(test_norm_stages_cpu.py::test_headroom_of_the_bounds measures the ratios and pins K to them)."""
import math

import torch

from flow_ref import _gen, ulp16, first_diff, is_fp16  # noqa: F401

F64 = torch.float64
F32 = torch.float32
U = 2.0 ** -23

# 8 x the worst K = 1 ratio of the fp32 restatement (sequential and pairwise order) over the case lists, rounded up to a power of two.
# Measured ratios (tests/test_norm_stages_cpu.py::test_headroom_of_the_bounds prints them): see K_MEASURED.
K_MEASURED = {"y": 2.109, "softmax": 0.5, "mean": 3.621, "rstd": 1.155}
K = {"y": 32.0, "softmax": 4.0, "mean": 32.0, "rstd": 16.0}

MUTATIONS_GN = ("group_boundary", "last_row_out", "next_sample_row", "var_n1", "eps_outside", "x2_column")
MUTATIONS_LN = ("var_n1", "eps_outside", "pe_no_mod", "pe_no_start")
MUTATIONS_SM = ("pad_in_max", "pad_in_sum", "pad_softmax")

EINVAL, EUNSUPPORTED = -1, -2
NONE, THREE_PASS, SMALL, FRAME = 0, 1, 2, 3
FAMILY_NAMES = {NONE: "NONE", THREE_PASS: "THREE_PASS", SMALL: "SMALL", FRAME: "FRAME"}


def f32(v):
    """The float32 nearest to the Python float v, as a Python float (what a kernel sees of an `eps` or `scale` argument)."""
    return torch.tensor(v, dtype=F32).item()


def silu(t):
    return t * torch.sigmoid(t)


# ================================================================================================================== GroupNorm
def gn_moments(X, G, mutate=None):
    """X [ns, rows, C] float64 -> (mean, var) [ns, G] of every (sample, group), population variance."""
    ns, rows, C = X.shape
    cpg = C // G
    if mutate == "group_boundary":      # group g = channels [g cpg + 1, (g + 1) cpg + 1): the last one is a channel short
        parts = [X[:, :, g * cpg + 1:min((g + 1) * cpg + 1, C)] for g in range(G)]
    else:
        parts = [X[:, :, g * cpg:(g + 1) * cpg] for g in range(G)]
    mean, var = [], []
    for g, part in enumerate(parts):
        per_sample = []
        for s in range(ns):
            v = part[s]
            if mutate == "last_row_out" and rows > 1:
                v = v[:-1]
            if mutate == "next_sample_row" and s + 1 < ns:
                v = torch.cat([v, part[s + 1][:1]], 0)
            v = v.reshape(-1)
            m = v.mean()
            d = ((v - m) ** 2).sum()
            per_sample.append((m, d / (v.numel() - 1 if mutate == "var_n1" else v.numel())))
        mean.append(torch.stack([m for m, _ in per_sample]))
        var.append(torch.stack([q for _, q in per_sample]))
    return torch.stack(mean, 1), torch.stack(var, 1)


def gn_moments_fast(X, G):
    """The unmutated gn_moments, vectorised."""
    ns, rows, C = X.shape
    v = X.reshape(ns, rows, G, C // G).permute(0, 2, 1, 3).reshape(ns, G, -1)
    mean = v.mean(-1)
    return mean, ((v - mean[..., None]) ** 2).mean(-1)


def gn_join(x, x2, mutate=None):
    if x2 is None:
        return x
    if mutate == "x2_column":           # x2 read at column c instead of c - C1: beyond x2's width lies the NaN frame
        C1, C2 = x.shape[1], x2.shape[1]
        moved = torch.full_like(x2, float("nan"))
        if C1 < C2:
            moved[:, :C2 - C1] = x2[:, C1:]
        x2 = moved
    return torch.cat([x, x2], 1)


def groupnorm_ref(x, x2, nsamples, rows, G, gamma, beta, eps, silu_on, mutate=None, moments=None):
    """x [nsamples rows, C1], x2 [nsamples rows, C - C1] or None, gamma / beta [C], all float64.
    Returns y [nsamples rows, C], mean [nsamples, G], rstd [nsamples, G], ab [nsamples, C, 2] = (rstd gamma, beta - mean rstd gamma).
    moments: (mean, var) of an earlier unmutated call on the same tensor (they do not depend on eps or silu)."""
    full = gn_join(x, x2, mutate)
    C = full.shape[1]
    X = full.reshape(nsamples, rows, C)
    if moments is None:
        moments = gn_moments_fast(X, G) if mutate in (None, "eps_outside", "x2_column") else gn_moments(X, G, mutate)
    mean, var = moments
    eps = f32(eps)
    rstd = 1.0 / (var.sqrt() + eps) if mutate == "eps_outside" else 1.0 / (var + eps).sqrt()
    cpg = C // G
    a = rstd.repeat_interleave(cpg, 1) * gamma[None]
    b = beta[None] - mean.repeat_interleave(cpg, 1) * a
    y = X * a[:, None] + b[:, None]
    if silu_on:
        y = silu(y)
    return y.reshape(nsamples * rows, C), mean, rstd, torch.stack([a, b], 2)


def gn_shift2(X, G, centre):
    """Squared distance of the reduction's centre from the true mean, [ns, G]: "first_token" = every channel is centred on the sample's
    first token (the largest distance of a channel's first token from that channel's mean over the group), "mean" = 0."""
    ns, rows, C = X.shape
    if centre == "mean":
        return torch.zeros((ns, G), dtype=F64)
    d = (X[:, 0] - X.mean(1)) ** 2
    return d.reshape(ns, G, C // G).max(-1).values


def gn_bounds(X, G, gamma, beta, eps, silu_on, ref, centre, k=None):
    """The bound tensors of one GroupNorm case: dict(y, mean, rstd [relative], ab)."""
    k = k or K
    y, mean, rstd, ab = ref
    ns, rows, C = X.shape
    cpg = C // G
    n = rows * cpg
    var = 1.0 / rstd ** 2 - f32(eps)
    sigma = var.clamp_min(0).sqrt()
    mc, rc = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    L = 1.1 if silu_on else 1.0
    by = ulp16(y).reshape(ns, rows, C) + k["y"] * U * (X.abs() + mc[:, None].abs()) * (rc * gamma.abs()[None])[:, None] * L
    bmean = k["mean"] * U * (mean.abs() + sigma)
    brstd = k["rstd"] * U * math.sqrt(n) * (1 + gn_shift2(X, G, centre) / (var.clamp_min(0) + f32(eps)))
    a, b = ab[..., 0], ab[..., 1]
    ba = a.abs() * (brstd.repeat_interleave(cpg, 1) + U)
    bb = bmean.repeat_interleave(cpg, 1) * a.abs() + mc.abs() * ba + U * (beta.abs()[None] + (mc * a).abs())
    return dict(y=by.reshape(ns * rows, C), mean=bmean, rstd=brstd, ab=torch.stack([ba, bb], 2))


def ratio(got, ref, bound, relative=False):
    """The worst |got - ref| / bound (inf where got is not finite or a zero bound is missed): <= 1 passes."""
    err = (got / ref - 1).abs() if relative else (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(got) & torch.isfinite(r), r, torch.full_like(r, float("inf")))
    return r.max().item() if r.numel() else 0.0


def gn_ratios(got, ref, bounds, outputs=("y", "mean", "rstd", "ab")):
    """got / ref = (y, mean, rstd, ab) (entries of got may be None) -> {output: worst ratio to its bound}."""
    out = {}
    for i, name in enumerate(("y", "mean", "rstd", "ab")):
        if name in outputs and got[i] is not None:
            out[name] = ratio(got[i], ref[i], bounds[name], relative=(name == "rstd"))
    return out


# ---- inputs: three generators per tensor, all values exact in fp16 -------------------------------------------------------------------
GN_GENERATORS = ("benign", "offset", "constant-group")
CONST_V = 1.5          # v rows cpg is an integer multiple of 1/2 below 2^24 for every listed case: exact in fp32


def constant_group_of(sample, G):
    return (5 * sample + 3) % G


def gn_case_data(ns, rows, C, G, gen, C1=0):
    """(x [ns rows, C1 or C], x2 or None, gamma [C], beta [C]) float64; x exact in fp16, gamma / beta exact in fp32."""
    g = _gen(ns, rows, C, G, GN_GENERATORS.index(gen))
    if gen == "offset":
        x = 40 + 0.25 * torch.randn((ns * rows, C), generator=g)
    else:
        x = torch.randn((ns * rows, C), generator=g) + 3 * torch.randn((1, C), generator=g)
    x = x.half()
    if gen == "constant-group":
        cpg = C // G
        xv = x.view(ns, rows, C)
        for s in range(ns):
            c0 = constant_group_of(s, G) * cpg
            xv[s, :, c0:c0 + cpg] = CONST_V
    gamma = (1 + 0.5 * torch.randn((C,), generator=g)).float().to(F64)
    beta = (0.5 * torch.randn((C,), generator=g)).float().to(F64)
    x = x.to(F64)
    if C1:
        return x[:, :C1].contiguous(), x[:, C1:].contiguous(), gamma, beta
    return x, None, gamma, beta


# ---- case lists ----------------------------------------------------------------------------------------------------------------------
def gn_case(name, ns, rows, C, G, nchunks=0, C1=0, plan=None, combos="all", note="", ab=False):
    """nchunks 0 = ops.groupnorm's choice.  plan = (family, nt, cs, vw, p, nchunks, rows_per_chunk, apply_grid_x) the planner must give for
    the descriptor with y (not stats_only), no switch set.  ab: the descriptor names an `ab` table as well as y - all three passes run and
    write y, the header and ab, whatever the slab size (the small-slab and whole-sample kernels write no table)."""
    return dict(name=name, ns=ns, rows=rows, C=C, G=G, nchunks=nchunks or default_nchunks(ns, rows), C1=C1, plan=plan, combos=combos, note=note, ab=ab)


def default_nchunks(ns, rows):
    """insv2v.ops._gn_chunks, restated (the SMALL and FRAME forms ignore it)."""
    return max(1, min(rows // 32, max(1, 1024 // ns), 128))


ALL_COMBOS = [(1e-5, 1), (1e-5, 0), (1e-6, 1), (1e-6, 0)]       # (eps, silu)
TWO_COMBOS = [(1e-5, 1), (1e-6, 0)]

# (family, nt, cs, vw, p, nchunks, rows_per_chunk, apply_grid_x): pinned by test_norm_stages_cpu.py::test_plan_of_every_case
GN_THREE_PASS = [
    gn_case("ragged-chunks", 2, 100, 320, 32, 3, plan=(THREE_PASS, 0, 0, 0, 6, 3, 34, 5), ab=True, note="cpg 10, P 6, chunks of 34 / 34 / 32 rows"),
    gn_case("empty-chunks", 3, 10, 320, 32, 8, plan=(THREE_PASS, 0, 0, 0, 6, 8, 2, 1), ab=True, note="rows_per_chunk 2: chunks 5-7 are empty"),
    gn_case("130-chunks", 2, 130, 64, 32, 200, plan=(THREE_PASS, 0, 0, 0, 16, 130, 1, 3), ab=True, note="nchunks clamped to 130: two trips of gn_finalize's lane loop; P capped at 16, cpg 2"),
    gn_case("one-row", 1, 1, 8, 8, 1, plan=(THREE_PASS, 0, 0, 0, 16, 1, 1, 1), ab=True, note="cpg 1, one row: variance 0"),
    gn_case("cpg-80", 2, 37, 2560, 32, 2, plan=(THREE_PASS, 0, 0, 0, 1, 2, 19, 10), ab=True, note="P 1, 320 threads, cpg 80 > 64: the ab loop"),
    gn_case("lds-48k", 1, 9, 4096, 32, 1, plan=(THREE_PASS, 0, 0, 0, 1, 1, 9, 3), ab=True, note="48 KiB of LDS"),
    gn_case("apply-cap-1", 4100, 1, 64, 32, 1, plan=(THREE_PASS, 0, 0, 0, 16, 1, 1, 1), ab=True, note="4100 samples: apply grid cap 1"),
    gn_case("apply-unrolled", 2, 1000, 640, 32, 5, plan=(THREE_PASS, 0, 0, 0, 3, 5, 200, 84), ab=True, note="both trip counts of the 4-row unrolled apply loop"),
    gn_case("concat-in-group", 2, 192, 192, 32, 3, C1=128, plan=(THREE_PASS, 0, 0, 0, 10, 3, 64, 5), ab=True, note="cpg 6, C1 = 128 inside group 21"),
    gn_case("concat-640-320", 3, 50, 960, 32, 2, C1=640, plan=(THREE_PASS, 0, 0, 0, 2, 2, 25, 7), ab=True, note="cpg 30"),
]
GN_SMALL = [
    gn_case("4096-chunks", 2, 2048, 512, 32, plan=(SMALL, 0, 0, 8, 0, 1, 2048, 32), combos="two", note="cpg 16, vw 8, exactly 256 x 16 chunks"),
    gn_case("4098-chunks", 2, 2049, 512, 32, plan=(THREE_PASS, 0, 0, 0, 4, 64, 33, 129), combos="two", note="one row more: THREE_PASS"),
    gn_case("2-chunks", 3, 1, 512, 32, plan=(SMALL, 0, 0, 8, 0, 1, 1, 32), combos="two", note="254 idle threads"),
    gn_case("vw4", 2, 77, 640, 32, plan=(SMALL, 0, 0, 4, 0, 1, 77, 32), combos="two", note="cpg 20, vw 4"),
    gn_case("vw4-concat", 2, 77, 640, 32, C1=328, plan=(SMALL, 0, 0, 4, 0, 1, 77, 32), combos="two", note="C1 = 328 inside group 16"),
    gn_case("cpg-40", 3, 96, 1280, 32, plan=(SMALL, 0, 0, 8, 0, 1, 96, 32), combos="two", note="cpr 5: 256 % cpr != 0"),
    gn_case("cpg-256", 2, 24, 2048, 8, plan=(SMALL, 0, 0, 8, 0, 1, 24, 8), combos="two", note="the widest group gn_small takes"),
    gn_case("cpg-264", 1, 24, 2112, 8, plan=(THREE_PASS, 0, 0, 0, 1, 1, 24, 6), combos="two", note="one chunk wider: THREE_PASS"),
]
GN_FRAME = [
    gn_case("cs1", 128, 17, 1280, 32, plan=(FRAME, 256, 1, 0, 0, 1, 17, 128), combos="two", note="2720 chunks"),
    gn_case("cs2", 128, 25, 1280, 32, plan=(FRAME, 256, 2, 0, 0, 1, 25, 128), combos="two", note="4000 chunks in 2 parts"),
    gn_case("cs4", 128, 49, 1280, 32, plan=(FRAME, 256, 4, 0, 0, 1, 49, 128), combos="two", note="7840 chunks in 4 parts"),
    gn_case("g16-cpr5", 128, 52, 640, 16, plan=(FRAME, 256, 2, 0, 0, 1, 52, 128), combos="two", note="cpr 5, 4160 chunks in 2 parts"),
    gn_case("product-96", 128, 96, 1280, 32, plan=(FRAME, 256, 4, 0, 0, 1, 96, 128), combos="two", note="the product's 8x12 frames"),
    gn_case("130-samples", 130, 7, 2560, 32, plan=(FRAME, 256, 1, 0, 0, 1, 7, 130), combos="two", note="2240 chunks, C = 2560"),
    gn_case("1920-chunks", 130, 6, 2560, 32, plan=(SMALL, 0, 0, 8, 0, 1, 6, 32), combos="two", note="1920 < 2048 chunks: one row short of FRAME, SMALL"),
    gn_case("127-samples", 127, 17, 1280, 32, plan=(SMALL, 0, 0, 8, 0, 1, 17, 32), combos="two", note="one sample short of FRAME: SMALL"),
]
# the frame tensors under the two switches, one child process each: {switch value: [(case name, plan)]}
GN_FORCED = {
    ("INSV2V_GN_FRAME_SPLIT", "1"): [gn_case("split1-512", 128, 40, 1280, 32, plan=(FRAME, 512, 1, 0, 0, 1, 40, 128), combos="one", note="6400 chunks: gn_frame<512>"),
                                    gn_case("split1-1024", 128, 96, 1280, 32, plan=(FRAME, 1024, 1, 0, 0, 1, 96, 128), combos="one", note="15360 chunks: gn_frame<1024>")],
    ("INSV2V_GN_FRAME", "0"): [gn_case("noframe-17", 128, 17, 1280, 32, plan=(SMALL, 0, 0, 8, 0, 1, 17, 32), combos="one"),
                               gn_case("noframe-25", 128, 25, 1280, 32, plan=(SMALL, 0, 0, 8, 0, 1, 25, 32), combos="one"),
                               gn_case("noframe-49", 128, 49, 1280, 32, plan=(SMALL, 0, 0, 8, 0, 1, 49, 32), combos="one")],
}
GN_CASES = GN_THREE_PASS + GN_SMALL + GN_FRAME


def gn_combos(case):
    return {"all": ALL_COMBOS, "two": TWO_COMBOS, "one": TWO_COMBOS[:1]}[case["combos"]]


def gn_centre(family):
    return "first_token" if family == THREE_PASS else "mean"


# refusals: (what, descriptor overrides on top of a valid 2 x 16 x 64 / G 32 three-pass call, return code)
GN_REFUSALS = [
    ("C = 5464: 65568 B of LDS", dict(C=5464, G=8), EUNSUPPORTED), ("C = 8192", dict(C=8192, G=8), EUNSUPPORTED),
    ("C % 8", dict(C=60, G=4), EINVAL), ("C % G", dict(C=64, G=5), EINVAL), ("C1 % 8", dict(C1=20, ldx=88, ldx2=96), EINVAL),
    ("ldx % 8", dict(ldx=68), EINVAL), ("nchunks = 0", dict(nchunks=0), EINVAL), ("stats_only without ab", dict(stats_only=1), EINVAL),
]


# ---- the fp32 restatement ------------------------------------------------------------------------------------------------------------
def sum32(t, dim, order):
    """fp32 sum along dim: "sequential" (one running sum) or "pairwise" (torch.sum)."""
    return t.cumsum(dim)[(slice(None),) * (dim % t.dim()) + (-1,)] if order == "sequential" else t.sum(dim)


def groupnorm_fp32(x, x2, nsamples, rows, G, gamma, beta, eps, silu_on, centre, order):
    """The same formulas in fp32, y rounded to fp16: centre "first_token" = per-channel sums shifted by the sample's first token, merged over
    a group's channels with Chan's formula; "mean" = two passes over the group."""
    X = gn_join(x, x2).float().reshape(nsamples, rows, -1)
    C = X.shape[2]
    cpg = C // G
    eps = torch.tensor(eps, dtype=F32)
    if centre == "first_token":
        k = X[:, :1]
        d = X - k
        s, q = sum32(d, 1, order), sum32(d * d, 1, order)
        n = torch.tensor(float(rows), dtype=F32)
        cm = (k[:, 0] + s / n).reshape(nsamples, G, cpg)
        m2 = (q - s * s / n).clamp_min(0).reshape(nsamples, G, cpg)
        mean, M2, cnt = cm[..., 0], m2[..., 0], n.clone()
        for j in range(1, cpg):
            tot = cnt + n
            dlt = cm[..., j] - mean
            mean = mean + dlt * (n / tot)
            M2 = M2 + m2[..., j] + dlt * dlt * (cnt * n / tot)
            cnt = tot
        var = M2 / cnt
    else:
        v = X.reshape(nsamples, rows, G, cpg).permute(0, 2, 1, 3).reshape(nsamples, G, -1)
        n = torch.tensor(float(rows * cpg), dtype=F32)
        mean = sum32(v, 2, order) / n
        dv = v - mean[..., None]
        var = sum32(dv * dv, 2, order) / n
    rstd = 1 / (var + eps).sqrt()
    a = rstd.repeat_interleave(cpg, 1) * gamma.float()[None]
    b = beta.float()[None] - mean.repeat_interleave(cpg, 1) * a
    y = X * a[:, None] + b[:, None]
    if silu_on:
        y = y / (1 + torch.exp(-y))
    return y.half().to(F64).reshape(nsamples * rows, C), mean.to(F64), rstd.to(F64), torch.stack([a, b], 2).to(F64)


# ================================================================================================================== LayerNorm
LN_CS = (8, 512, 520, 1024, 1032, 1536, 1544, 2048)       # NCH 1 | 1, 2 | 2, 3 | 3, 4 | 4
LN_ROWS = (1, 3, 4, 5, 16, 17, 21)
LN_GENERATORS = ("offset", "constant", "huge")
LN_EPS = 1e-5
PE_MAX_LEN = 24
# (rows_per_frame, frames, samples): rows = samples frames rows_per_frame, so (row / rows_per_frame) % frames wraps samples - 1 = 2 times
LN_PE_CASES = [(1, 5, 3), (7, 4, 3)]
LN_PE_CS = (8, 520, 1032, 2048)


def ln_case_data(rows, C, gen):
    g = _gen(rows, C, 7 + LN_GENERATORS.index(gen))
    if gen == "offset":
        x = 30 + 0.05 * torch.randn((rows, C), generator=g)
    elif gen == "constant":
        x = (0.25 * (1 + torch.arange(rows, dtype=F64) % 37))[:, None].expand(rows, C)          # v C exact in fp32
    else:
        x = 60000.0 * (torch.randint(0, 2, (rows, C), generator=g) * 2 - 1)
    gamma = (1 + 0.5 * torch.randn((C,), generator=g)).float().to(F64)
    beta = (0.5 * torch.randn((C,), generator=g)).float().to(F64)
    return x.half().to(F64), gamma, beta


def pe_table(C, frames, pe_start):
    """fp32 [PE_MAX_LEN, C] as float64: random inside rows [pe_start, pe_start + frames), NaN in every other row."""
    g = _gen(C, frames, pe_start, 3)
    pe = torch.full((PE_MAX_LEN, C), float("nan"), dtype=F64)
    pe[pe_start:pe_start + frames] = torch.randn((frames, C), generator=g).float().to(F64)
    return pe


def layernorm_ref(x, gamma, beta, eps, pe=None, rows_per_frame=1, frames=1, pe_start=0, mutate=None):
    """x [rows, C] float64 -> (y [rows, C], mean [rows], rstd [rows]); pe [max_len, C]: y += pe[(row / rows_per_frame) % frames + pe_start]."""
    rows, C = x.shape
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).sum(1) / (C - 1 if mutate == "var_n1" else C)
    eps = f32(eps)
    rstd = 1 / (var.sqrt() + eps) if mutate == "eps_outside" else 1 / (var + eps).sqrt()
    y = (x - mean[:, None]) * rstd[:, None] * gamma[None] + beta[None]
    if pe is not None:
        y = y + pe_rows(pe, rows, rows_per_frame, frames, pe_start, mutate)
    return y, mean, rstd


def pe_rows(pe, rows, rows_per_frame, frames, pe_start, mutate=None):
    f = torch.arange(rows) // rows_per_frame
    if mutate != "pe_no_mod":
        f = f % frames
    if mutate != "pe_no_start":
        f = f + pe_start
    padded = torch.cat([pe, torch.full((rows + PE_MAX_LEN, pe.shape[1]), float("nan"), dtype=F64)], 0)     # beyond the table: not a number either
    return padded[f]


def ln_bounds(x, gamma, ref, eps, pe_r=None, k=None):
    k = k or K
    y, mean, rstd = ref
    C = x.shape[1]
    var = (1 / rstd ** 2 - f32(eps)).clamp_min(0)
    bracket = x.abs() + mean[:, None].abs() + (pe_r.abs() if pe_r is not None else 0)
    by = ulp16(y) + k["y"] * U * bracket * rstd[:, None] * gamma.abs()[None]
    return dict(y=by, mean=k["mean"] * U * (mean.abs() + var.sqrt()), rstd=k["rstd"] * U * math.sqrt(C) * torch.ones_like(rstd))


def ln_ratios(got, ref, bounds):
    out = {}
    for i, name in enumerate(("y", "mean", "rstd")):
        if got[i] is not None:
            out[name] = ratio(got[i], ref[i], bounds[name], relative=(name == "rstd"))
    return out


def layernorm_fp32(x, gamma, beta, eps, pe_r, order):
    X = x.float()
    C = torch.tensor(float(X.shape[1]), dtype=F32)
    mean = sum32(X, 1, order) / C
    d = X - mean[:, None]
    rstd = 1 / (sum32(d * d, 1, order) / C + torch.tensor(eps, dtype=F32)).sqrt()
    y = d * rstd[:, None] * gamma.float()[None] + beta.float()[None]
    if pe_r is not None:
        y = y + pe_r.float()
    return y.half().to(F64), mean.to(F64), rstd.to(F64)


# ================================================================================================================== row softmax
SM_COLS = (8, 96, 2048, 2056, 4104)                        # 2056, 4104: a second trip of the 256-thread loop
SM_ROWS = (1, 5)
SM_SCALES = (0.0, 0.7, 512 ** -0.5)
SM_GENERATORS = ("random", "all-lowest", "dominant", "max-last-valid", "max-first-pad")
PAD_VALUES = (float("nan"), float("inf"), float("-inf"))


def sm_valids(cols):
    return sorted({1, max(1, cols - 7), cols - 1, cols})


def sm_case_data(rows, cols, valid):
    """x [rows, cols] float64, exact in fp16 where finite; row r follows generator r % 5.  Columns [valid, cols) hold NaN, +Inf, -Inf in
    turn; in a "max-first-pad" row column `valid` holds 65504, the largest fp16 number."""
    g = _gen(rows, cols, valid, 11)
    x = (3 * torch.randn((rows, cols), generator=g)).half().to(F64)
    for r in range(rows):
        gen = SM_GENERATORS[r % 5]
        if gen == "all-lowest":
            x[r] = -65504.0
        elif gen == "dominant":
            x[r, (7 * r + 3) % valid] = 60000.0
        elif gen == "max-last-valid":
            x[r, valid - 1] = 24.0
    if valid < cols:
        x[:, valid:] = torch.tensor([PAD_VALUES[j % 3] for j in range(cols - valid)], dtype=F64)[None]
        for r in range(rows):
            if SM_GENERATORS[r % 5] == "max-first-pad":
                x[r, valid] = 65504.0
    return x


def softmax_ref(x, scale, valid=None, mutate=None):
    """softmax(scale x) over the first `valid` columns of every row, exactly 0 in the others."""
    rows, cols = x.shape
    valid = cols if valid is None else valid
    scale = f32(scale)
    v = x[:, :valid]
    seen = x[:, :min(valid + 1, cols)]          # what a kernel that is one column off sees: the first pad column as well
    mx = (seen if mutate == "pad_in_max" else v).max(1, keepdim=True).values
    e = torch.exp((x - mx) * scale)
    total = (e[:, :min(valid + 1, cols)] if mutate == "pad_in_sum" else e[:, :valid]).sum(1, keepdim=True)
    y = e / total
    if mutate != "pad_softmax":
        y[:, valid:] = 0
    return y


def sm_bound(ref, cols, k=None):
    k = k or K
    return ulp16(ref) + k["softmax"] * U * math.sqrt(cols) * ref


def softmax_fp32(x, scale, valid, order):
    X = x.float()[:, :valid]
    mx = X.max(1, keepdim=True).values
    e = torch.exp2((X - mx) * (torch.tensor(scale, dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32)))
    y = e * (1 / sum32(e, 1, order))[:, None]
    out = torch.zeros(x.shape, dtype=F64)
    out[:, :valid] = y.half().to(F64)
    return out


# ================================================================================================================== the planner
PLAN_FIELDS = ("family", "nt", "cs", "vw", "p", "nchunks", "rows_per_chunk", "apply_grid_x")
FAKE = 4096        # a non-null pointer for descriptors that are planned, never run


def gn_desc(ns, rows, C, G, nchunks, C1=0, stats_only=0, ab=False, **over):
    """A descriptor with placeholder pointers (the planner reads their null bits only); `over` sets fields last (x2=True: a pointer)."""
    from insv2v import _lib
    d = _lib.GroupNormDesc()
    d.x = d.gamma = d.beta = d.partials = FAKE
    if not stats_only:
        d.y = FAKE
    if ab:
        d.ab = FAKE
    d.nsamples, d.rows_per_sample, d.C, d.G, d.nchunks, d.stats_only, d.eps = ns, rows, C, G, nchunks, stats_only, 1e-5
    d.ldx, d.ldy = (C1 or C) + 24, C + 40
    if C1:
        d.x2, d.ldx2, d.C1 = FAKE, C - C1 + 48, C1
    for name, v in over.items():
        setattr(d, name, FAKE if v is True else v)
    return d


def case_desc(case, **kw):
    kw.setdefault("ab", case["ab"])
    return gn_desc(case["ns"], case["rows"], case["C"], case["G"], case["nchunks"], case["C1"], **kw)


def plan(d):
    import ctypes
    from insv2v import _lib
    p = _lib.GroupNormPlan()
    assert _lib.load().insv2v_groupnorm_plan(ctypes.byref(d), ctypes.byref(p)) == 0
    return p


def plan_tuple(p):
    return tuple(getattr(p, f) for f in PLAN_FIELDS)


def describe(t):
    return ", ".join(f"{f} {FAMILY_NAMES[v] if f == 'family' else v}" for f, v in zip(PLAN_FIELDS, t))


def check_case_plan(case, d=None):
    """The plan of the case's descriptor is the one the table pins (d: the real descriptor of a GPU test)."""
    p = plan(d if d is not None else case_desc(case))
    assert p.rc == 0, f"GroupNorm case {case['name']}: refused with {p.rc}"
    assert plan_tuple(p) == case["plan"], (f"GroupNorm case {case['name']} ({case['ns']} x {case['rows']} x {case['C']}, G {case['G']}) no longer runs what it is "
                                           f"listed for ({case['note']}): planned {describe(plan_tuple(p))}; listed {describe(case['plan'])}")
    return p
