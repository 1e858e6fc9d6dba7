"""Case builders and fp64 references for the kernel-level parity tests of the two kernels of csrc/gemm.hip: gemm_kernel (the tile kernel:
tile codes = shape 1 - 9 + 10 x ring depth 2 - 4, LINEAR and CONV3X3, K groups, split-K with splitk_reduce_kernel, batching) and
conv_halo_kernel (the patch-tiled convolution: codes 100 - 103, GroupNorm fused in).  In the style of tests/gemm_engine_ref.py, whose
builders are reused wherever they have the arguments: every builder takes `device`, draws its operands with a CPU generator and returns
the fp16 operands, the fp64 reference on the SAME fp16-rounded operands and the named blocks (name, index) to be judged on their own.

Every builder asserts need_gap per feature: a reference computed WITHOUT the feature is more than 10 x the tolerance of the comparison
away from the true one, so a kernel that skips the feature cannot pass.  The conditions involve references only;
tests/test_gemm_tile_cpu.py asserts them without a GPU.

Tile shapes (csrc/gemm_plan.h): 1 = 128x128, 2 = 64x128, 3 = 128x64, 4 = 64x64 (4 waves); 5 = 128x128, 6 = 256x128, 7 = 128x64 (8 waves);
8 = 128x128, 9 = 128x64 (8 waves as 2 K groups of 4).  K slices are 64 wide.
"""
import torch
import torch.nn.functional as F

import gemm_engine_ref as R
from gemm_engine_ref import rnd, tol_of, need_gap, cached, to_cl

BK = 64
TILE_BM = {1: 128, 2: 64, 3: 128, 4: 64, 5: 128, 6: 256, 7: 128, 8: 128, 9: 128}
TILE_BN = {1: 128, 2: 128, 3: 64, 4: 64, 5: 128, 6: 128, 7: 64, 8: 128, 9: 64}
TILE_LDS_MAX = 160 * 1024
PLAN_TILE, PLAN_HALO = 1, 2                    # INSV2V_PLAN_TILE, INSV2V_PLAN_HALO
EINVAL, EUNSUPPORTED = -1, -2                  # INSV2V_EINVAL, INSV2V_EUNSUPPORTED
ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_QUICK_GELU, ACT_RELU, ACT_SIGMOID, ACT_TANH = range(7)   # include/insv2v_hip.h


def tile_lds_bytes(bm, bn, stages):
    """csrc/gemm_plan.h: the ring or the fp32 staging tile, whichever is larger, plus bias, column sums and (mean, rstd)."""
    ring, stage = stages * (bm + bn) * BK * 2, bm * (bn + 4) * 4
    return max(ring, stage) + (2 * bn + 2 * bm) * 4


def shape_of(code):
    return code % 10


def ring_of(code):
    return code // 10 or 2


VALID = [r * 10 + s for r in (2, 3, 4) for s in range(1, 10) if tile_lds_bytes(TILE_BM[s], TILE_BN[s], r) <= TILE_LDS_MAX]
PRODUCT = (2, 4, 5)                            # what pick_tile and split-K choose
KG = (8, 9)
DEEP = (34, 35, 38, 44, 45, 48)
SENTINEL = -77.0
FILL = 64.0                                    # what lies behind column K of the K-loop case's operands


def group_of(M, rpg, rb_mod, device):
    g = torch.arange(M, device=device) // rpg
    return g % rb_mod if rb_mod > 0 else g


# ------------------------------------------------------------------------------------------- 1. layout
@cached
def layout_case(device):
    """R.layout_case (A = identity: the output IS W^T) with the tile kernel's own two exchanges: the 32-row fragments j / the wave rows wm,
    and the wave columns wn of a 128-column tile."""
    a, w, ref = R.layout_case(device)
    M, N = ref.shape
    tol = tol_of(ref)
    need_gap(ref, ref[torch.arange(M, device=ref.device) ^ 32], tol, "32-row blocks exchanged (the j fragment, wm)")
    alt = ref.clone()
    alt[:, :256] = ref[:, :256].reshape(M, 2, 2, 64).flip(2).reshape(M, 256)
    need_gap(ref, alt, tol, "the two 64-column halves of each 128-column tile exchanged (wn at BN = 128)")
    return a, w, ref


# ------------------------------------------------------------------------------------------- 2. K loop and ring
KLOOP_M, KLOOP_N = 200, 136
KLOOP_K = (8, 64, 72, 128, 200, 320)           # slices: 1 partial, 1, 2 with a tail, 2, 4 with a tail, 5 - below, at and above every ring depth
KLOOP_CODES = [r * 10 + s for s in (4, 5, 8) for r in (2, 3, 4)]


@cached
def kloop_case(K, device):
    """A and W are the column slices [:, :K] of buffers whose rows are (K rounded up to 64) + 8 long and hold FILL from column K on: a
    K tail that is not masked reads FILL, and stays inside the buffers."""
    M, N = KLOOP_M, KLOOP_N
    Kc = (K + BK - 1) // BK * BK
    abuf = torch.full((M, Kc + 8), FILL, dtype=torch.float16, device=device)
    wbuf = torch.full((N, Kc + 8), FILL, dtype=torch.float16, device=device)
    abuf[:, :K], wbuf[:, :K] = rnd(M, K, device=device).half(), rnd(N, K, scale=K ** -0.5, seed=1, device=device).half()
    b = rnd(N, seed=3, device=device)

    def prod(k0, k1):
        return abuf[:, k0:k1].double() @ wbuf[:, k0:k1].double().t()
    ref = prod(0, K) + b.double()
    tol, nk = tol_of(ref), Kc // BK
    if K % BK:
        need_gap(ref, prod(0, Kc) + b.double(), tol, "the K tail not masked")
    need_gap(ref, prod(0, (nk - 1) * BK) + b.double(), tol, "the last K slice dropped")
    need_gap(ref, ref + prod(0, min(BK, K)), tol, "the first K slice counted twice")
    blocks = [("last row tile", slice(192, M)), ("last 8 columns", (slice(None), slice(128, N)))]
    return abuf[:, :K], wbuf[:, :K], b, ref, blocks


# ------------------------------------------------------------------------------------------- 3. store paths
STORE_M, STORE_K, STORE_RPG = 200, 64, 80
# form: (N, fp32 output, ldc, first column of the output window, ldr, first column of the residual window, ld_rb - N, rb_mod)
STORE_FORMS = {
    "a": (136, False, 144, 0, 144, 0, 0, 0),        # fast path, partial column tile
    "a_mod2": (136, False, 144, 0, 144, 0, 0, 2),   # ... the third row-bias group wraps to table row 0
    "b": (136, False, 144, 4, 144, 4, 0, 0),        # misaligned pointers: scalar stores
    "c": (136, False, 140, 0, 144, 0, 0, 0),        # ldc % 8 != 0: scalar stores
    "d": (132, False, 144, 0, 144, 0, 0, 0),        # N % 8 != 0: the last chunk partial
    "e": (134, False, 144, 0, 144, 0, 0, 0),        # N % 4 != 0: the scalar row-bias path
    "f": (136, False, 144, 0, 144, 4, 0, 0),        # misaligned residual only
    "g": (136, True, 144, 0, 144, 0, 0, 0),         # fp32 output, 32-byte aligned: 16-byte stores
    "h": (136, True, 144, 4, 144, 0, 0, 0),         # fp32 output at a 16-byte offset: scalar stores
    "i": (136, False, 144, 0, 144, 0, 1, 0),        # row-bias table rows N + 1 apart: scalar row-bias loads
}
STORE_ALPHA = 0.5


@cached
def store_case(form, device):
    N, fp32, ldc, c_off, ldr, r_off, rb_extra, rb_mod = STORE_FORMS[form]
    M, K, rpg = STORE_M, STORE_K, STORE_RPG
    a, w, b = rnd(M, K, device=device).half(), rnd(N, K, scale=K ** -0.5, seed=1, device=device).half(), rnd(N, seed=3, device=device)
    tbuf = torch.zeros(3, N + rb_extra, device=device)
    tbuf[:, :N] = rnd(3, N, seed=9, device=device) * 0.5 + torch.tensor([[0.0], [1.0], [-1.0]], device=device)
    table = tbuf[:, :N]
    r = rnd(M, N, seed=5, device=device).half()
    g, ng = group_of(M, rpg, rb_mod, device), (rb_mod or 3)
    prod = a.double() @ w.double().t()
    ref = STORE_ALPHA * prod + b.double() + table.double()[g] + r.double()
    tol = tol_of(ref)
    need_gap(ref, ref - table.double()[g] + table.double()[(g + 1) % ng], tol, "row bias of the neighbouring group")
    need_gap(ref, ref - table.double()[g], tol, "row bias omitted")
    need_gap(ref, ref - r.double(), tol, "residual omitted")
    need_gap(ref, ref + (1 - STORE_ALPHA) * prod, tol, "alpha omitted")
    need_gap(ref, ref - b.double(), tol, "bias omitted")
    blocks = [(f"rows from {i * rpg} (one bias group)", slice(i * rpg, min(M, (i + 1) * rpg))) for i in range(3)]
    blocks.append(("columns of the last column tile", (slice(None), slice(128, N))))
    if rb_mod:
        wrapped = slice(2 * rpg, M)
        need_gap(ref[wrapped], (ref - table.double()[g] + table.double()[2])[wrapped], tol_of(ref[wrapped]), "rb_mod ignored: the third group takes table row 2")
    geom = dict(N=N, fp32=fp32, ldc=ldc, c_off=c_off, ldr=ldr, r_off=r_off, rb_mod=rb_mod)
    return a, w, b, table, r, geom, ref, blocks


# ------------------------------------------------------------------------------------------- 4. activations
ACTS = {"silu": ACT_SILU, "quick_gelu": ACT_QUICK_GELU, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "tanh": ACT_TANH}
ACT_FN = {"silu": F.silu, "quick_gelu": lambda x: x * torch.sigmoid(1.702 * x), "relu": F.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}
ACT_SHAPE = (200, 136, 128)


@cached
def act_case(name, device):
    """ref = act(a w^T + bias) + residual; the pre-activation has a standard deviation of ~1.6 and the residual of 1, so that also the
    bounded sigmoid and tanh are far from both 'no activation' and 'activation after the residual'."""
    M, N, K = ACT_SHAPE
    a, w = rnd(M, K, device=device).half(), rnd(N, K, scale=1.5 * K ** -0.5, seed=1, device=device).half()
    b, r = rnd(N, seed=3, device=device) * 0.5, rnd(M, N, seed=5, device=device).half()
    pre, f = a.double() @ w.double().t() + b.double(), ACT_FN[name]
    ref = f(pre) + r.double()
    tol = tol_of(ref)
    need_gap(ref, pre + r.double(), tol, f"{name} omitted")
    need_gap(ref, f(pre + r.double()), tol, f"{name} applied after the residual")
    need_gap(ref, f(pre), tol, "residual omitted")
    return a, w, b, r, ref, [("last row tile", slice(192, M)), ("last 8 columns", (slice(None), slice(128, N)))]


# ------------------------------------------------------------------------------------------- 5. folded LayerNorm, emitted statistics
def finished_stats(a):
    """[M, 2] fp32 (mean, rstd) of the rows a, from fp64."""
    _, mean, rstd = R.layernorm_terms(a)
    return torch.cat([mean, rstd], 1).float().contiguous()


@cached
def ln_rows_case(device):
    """R.row_bias_case('odd', ln=True): 585 rows in bias groups of 117, folded LayerNorm in the finished (mean, rstd) form."""
    a, w, b, col, table, rpg, rb_mod, ref, blocks = R.row_bias_case("odd", True, device)
    return a, w, b, col, table, rpg, rb_mod, finished_stats(a), ref, blocks


PC_M, PC_NP, PC_NC = 258, 328, 320             # producer: N = 328 (last part 72 columns on BN = 128, 8 on BN = 64); consumer: K = 328, N = 320


def part_sums(rows, bn):
    """[ceil(N / bn), M, 2] fp64: (sum, sum of squares) of every bn-column part of the fp16 rows."""
    x = rows.double()
    return torch.stack([torch.stack([p.sum(1), (p * p).sum(1)], 1) for p in x.split(bn, 1)], 0)


@cached
def producer_case(res, device):
    """The GEMM whose rows (and their emitted partial sums) feed the consumer's folded LayerNorm.  Returns its operands, its fp64
    reference and `rows`, the CPU twin of what it stores (the reference rounded to fp16)."""
    a, w, b = R.producer_operands(PC_M, PC_NP, device)
    r = rnd(PC_M, PC_NP, seed=31, device=device).half() if res else None
    ref = a.double() @ w.double().t() + b.double() + (r.double() if res else 0)
    if res:
        need_gap(ref, ref - r.double(), tol_of(ref), "residual omitted")
    rows = ref.half()
    for bn in (64, 128):
        sums = part_sums(rows, bn)
        assert sums.shape[0] == (PC_NP + bn - 1) // bn
        for p in range(sums.shape[0]):
            q = (p + 1) % sums.shape[0]
            for j, name in enumerate(("sum", "sum of squares")):
                need_gap(sums[p, :, j], sums[q, :, j], R.stats_tol(sums[p, :, j]), f"{name}: parts {p} and {q} of {bn} columns exchanged")
        # (the tile kernel sums AFTER the fp16 rounding: the sums of the unrounded values are a different, if close, quantity)
    return a, w, b, r, ref, rows


def consumer_case(rows):
    """The consumer on the rows the producer stored: R.layernorm_case asserts '-mean * col_sum dropped' and 'LayerNorm not applied'."""
    w, b, col, ref = R.layernorm_case(rows, PC_NC, seed=2)
    return w, b, col, ref


# ------------------------------------------------------------------------------------------- 6. GEGLU
GEGLU_CODES = (2, 5, 6, 8, 32, 35)
GEGLU_RB_SHAPE = (300, 64, 160)


@cached
def geglu_case(M, C, NH, device):
    """R.geglu_case with the (mean, rstd) pairs from fp64."""
    args, col, ref = R.geglu_case(M, C, NH, device)
    return args, col, finished_stats(args[0]), ref


@cached
def geglu_rb_case(rb_extra, device):
    """R.geglu_case's operands at 300 x 320 x 64 plus a two-group row bias over value and gate, interleaved like the bias; the table's
    rows are 2 NH + rb_extra apart (rb_extra = 1: unaligned, the scalar row-bias path for value and gate)."""
    from insv2v.unet import fold_layernorm, interleave32
    M, C, NH = GEGLU_RB_SHAPE
    rpg = M // 2
    x = (rnd(M, C, device=device) * 1.3 + 0.2).half()
    w1, b1 = rnd(2 * NH, C, scale=C ** -0.5), rnd(2 * NH, seed=1) * 0.3
    gamma, beta = 1 + 0.1 * rnd(C, seed=4), 0.1 * rnd(C, seed=5)
    wf, col, bf = (t.to(device) for t in fold_layernorm(w1, gamma, beta, b1))
    tb = (rnd(2, 2 * NH, seed=9) * 0.5 + torch.tensor([[0.6], [-0.6]])).to(device)       # [h | g] order
    g = group_of(M, rpg, 0, device)
    xf, mean, rstd = R.layernorm_terms(x)
    y0 = F.layer_norm(xf, (C,)) @ wf.double().t() + bf.double()
    y = y0 + tb.double()[g]

    def glu(t):
        h, gt = t.chunk(2, dim=-1)
        return h * F.gelu(gt)
    ref = glu(y)
    tol = tol_of(ref, True)
    h, gt = y.chunk(2, dim=-1)
    need_gap(ref, gt * F.gelu(h), tol, "gate and value halves swapped")
    need_gap(ref, h * F.gelu(h), tol, "the gate read from the value's accumulator")
    need_gap(ref, glu(y + rstd * mean * col.double()), tol, "-mean * col_sum dropped")
    need_gap(ref, glu(y0), tol, "row bias omitted")
    need_gap(ref, glu(y0 + tb.double()[1 - g]), tol, "row bias of the neighbouring group")
    need_gap(ref, h * F.gelu(y0.chunk(2, dim=-1)[1]), tol, "the gate's row bias omitted")
    need_gap(ref, y0.chunk(2, dim=-1)[0] * F.gelu(gt), tol, "the value's row bias omitted")
    tbuf = torch.zeros(2, 2 * NH + rb_extra, device=device)
    tbuf[:, :2 * NH] = interleave32(tb.t().contiguous()).t()
    args = (x, interleave32(wf).contiguous(), interleave32(bf).contiguous())
    blocks = [(f"rows of bias group {i}", slice(i * rpg, (i + 1) * rpg)) for i in range(2)]
    return args, interleave32(col).contiguous(), finished_stats(x), tbuf[:, :2 * NH], rpg, ref, blocks


# ------------------------------------------------------------------------------------------- 7. split-K
SPLIT_M, SPLIT_N = 200, 136
SPLIT_K = (320, 328)                           # 5 slices; 6 slices with a tail
SPLITS = (2, 3, 5, 8)                          # 5 and 8 leave splits empty
SPLIT_ALPHA = 0.5
SPLIT_CONV = (2, 6, 4, 128, 72)                # nb, h, w, Cin, cout: 18 K slices
SPLITS_CONV = (2, 4, 5)                        # 4: every later split starts at k0 = 320 s - tap 2, second channel block


def split_ranges(nk, ns):
    """Slices [k0, k1) of every non-empty split (gemm_kernel: nk_per = ceil(nk / ns), split s starts at s * nk_per)."""
    per = (nk + ns - 1) // ns
    return [(s * per, min(nk, (s + 1) * per)) for s in range(ns) if s * per < nk]


def split_conditions(ref, slices, alpha, splits, what):
    tol, nk = tol_of(ref), len(slices)
    for ns in splits:
        rngs = split_ranges(nk, ns)
        assert sum(k1 - k0 for k0, k1 in rngs) == nk
        k0, k1 = rngs[-1]
        need_gap(ref, ref - alpha * sum(slices[k0:k1]), tol, f"{what}, {ns} splits: the last non-empty split dropped")
        for s, (k0, k1) in enumerate(rngs):
            need_gap(ref, ref + alpha * sum(slices[k0:k1]), tol, f"{what}, {ns} splits: split {s} counted twice")


@cached
def splitk_case(K, device):
    M, N = SPLIT_M, SPLIT_N
    a, w, b = rnd(M, K, device=device).half(), rnd(N, K, scale=K ** -0.5, seed=1, device=device).half(), rnd(N, seed=3, device=device)
    table = rnd(3, N, seed=9, device=device) * 0.5 + torch.tensor([[0.0], [1.0], [-1.0]], device=device)
    r = rnd(M, N, seed=5, device=device).half()
    g = group_of(M, STORE_RPG, 0, device)
    slices = [a[:, k:k + BK].double() @ w[:, k:k + BK].double().t() for k in range(0, K, BK)]
    extra = b.double() + table.double()[g] + r.double()
    ref = SPLIT_ALPHA * sum(slices) + extra
    tol = tol_of(ref)
    split_conditions(ref, slices, SPLIT_ALPHA, SPLITS, f"K = {K}")
    need_gap(ref, ref - table.double()[g], tol, "row bias omitted")
    need_gap(ref, ref - table.double()[g] + table.double()[(g + 1) % 3], tol, "row bias of the neighbouring group")
    need_gap(ref, ref - r.double(), tol, "residual omitted")
    need_gap(ref, ref + (1 - SPLIT_ALPHA) * sum(slices), tol, "alpha omitted")
    blocks = [("last row tile", slice(192, M)), ("last 8 columns", (slice(None), slice(128, N)))]
    return a, w, b, table, r, ref, blocks


def im2col(x):
    """[nb, C, h, w] -> [nb h w, 9 C] for stride 1 / pad 1, tap-major (kh, kw, c): the K order of prep_conv3x3's weights."""
    nb, c, h, w = x.shape
    return F.unfold(x, 3, padding=1).reshape(nb, c, 9, h * w).permute(0, 3, 2, 1).reshape(nb * h * w, 9 * c)


@cached
def splitk_conv_case(device):
    """2 images of 6 x 4, 128 -> 72 channels.  Returns the one-source operands (the test splits x into 64 + 64 itself)."""
    from insv2v.unet import prep_conv3x3
    nb, h, w_, cin, cout = SPLIT_CONV
    M = nb * h * w_
    x = rnd(nb, cin, h, w_, device=device).half()
    wt, b = rnd(cout, cin, 3, 3, scale=(9 * cin) ** -0.5).half(), rnd(cout, seed=4)
    wk, bk = prep_conv3x3({"c.weight": wt.float(), "c.bias": b}, "c", device)
    wt, b = wt.to(device).double(), b.to(device).double()
    col, wd = im2col(x.double()), wk.double()
    conv = to_cl(R.conv_ref(x.double(), wt, b, 1, False))
    assert torch.allclose(col @ wd.t() + b, conv, rtol=0, atol=1e-9)
    table, r = rnd(nb, cout, seed=6, device=device) * 0.5, rnd(M, cout, seed=7, device=device).half()
    g = group_of(M, h * w_, 0, device)
    extra = b + table.double()[g] + r.double()
    slices = [col[:, k:k + BK] @ wd[:, k:k + BK].t() for k in range(0, 9 * cin, BK)]
    ref = sum(slices) + extra
    tol = tol_of(ref)
    split_conditions(ref, slices, 1.0, SPLITS_CONV, "conv")
    for ns in SPLITS_CONV:   # every later split gathers from tap 0 on (its channel block and its weights are the right ones)
        alt = extra.clone()
        for k0, k1 in split_ranges(len(slices), ns):
            for t, kt in enumerate(range(k0, k1)):
                vk = kt * BK if k0 == 0 else (k0 * BK) % cin + t * BK
                alt = alt + col[:, vk:vk + BK] @ wd[:, kt * BK:(kt + 1) * BK].t()
        need_gap(ref, alt, tol, f"conv, {ns} splits: every later split started at tap 0")
    need_gap(ref, ref - r.double(), tol, "residual omitted")
    need_gap(ref, ref - table.double()[g], tol, "row bias omitted")
    kw = dict(row_bias=table, rows_per_group=h * w_, residual=r)
    return to_cl(x), wk, bk, kw, (nb, h, w_), ref, [(f"image {i}", slice(i * h * w_, (i + 1) * h * w_)) for i in range(nb)]


# ------------------------------------------------------------------------------------------- 8. batched
BATCH = (3, 96, 80, 72)                        # batch, M, N, K
BATCH_ALPHA = 0.25
BATCH_LD = dict(lda=80, ldw=80, ldc=88, ldr=96, lda2=16)
BATCH_STRIDE = dict(a_bs=80 * (96 + 3), w_bs=80 * (80 + 2), c_bs=88 * (96 + 4), r_bs=96 * (96 + 1))   # each leaves a gap; multiples of 8


def strided_batches(flat, bs, rows, ld, cols, batch):
    return torch.as_strided(flat, (batch, rows, cols), (bs, ld, 1))


@cached
def batched_case(two, device):
    """batch = 3 with a gap behind every batch of a, w, residual (FILL / the sentinel) and output.  two: K = 64 + 8 from two sources,
    lda2 = 16 != lda, the second source's batches a_bs ELEMENTS apart like the first's (insv2v_gemm has one stride for both)."""
    B, M, N, K = BATCH
    L, S = BATCH_LD, BATCH_STRIDE
    k1 = 64 if two else K
    a, w = rnd(B, M, K, device=device).half(), rnd(B, N, K, scale=K ** -0.5, seed=1, device=device).half()
    b, r = rnd(N, seed=3, device=device), rnd(B, M, N, seed=5, device=device).half()
    abuf = torch.full((B * S["a_bs"],), FILL, dtype=torch.float16, device=device)
    wbuf = torch.full((B * S["w_bs"],), FILL, dtype=torch.float16, device=device)
    rbuf = torch.full((B * S["r_bs"],), SENTINEL, dtype=torch.float16, device=device)
    strided_batches(abuf, S["a_bs"], M, L["lda"], k1, B).copy_(a[:, :, :k1])
    strided_batches(wbuf, S["w_bs"], N, L["ldw"], K, B).copy_(w)
    strided_batches(rbuf, S["r_bs"], M, L["ldr"], N, B).copy_(r)
    ref = BATCH_ALPHA * a.double() @ w.double().transpose(1, 2) + b.double() + r.double()
    tol = tol_of(ref[1:])
    need_gap(ref[1:], (BATCH_ALPHA * a.double() @ w[:1].double().transpose(1, 2) + b.double() + r.double())[1:], tol, "every batch multiplied by batch 0's W")
    need_gap(ref[1:], (ref - r.double() + r[:1].double())[1:], tol, "the residual of batch 0 used everywhere")
    need_gap(ref[1:], (BATCH_ALPHA * a[:1].double() @ w.double().transpose(1, 2) + b.double() + r.double())[1:], tol, "batch 0's A used everywhere")
    need_gap(ref, ref - r.double(), tol_of(ref), "residual omitted")
    need_gap(ref, ref + (1 - BATCH_ALPHA) * (a.double() @ w.double().transpose(1, 2)), tol_of(ref), "alpha omitted")
    a2v = None
    if two:
        a2buf = torch.full(((B - 1) * S["a_bs"] + M * L["lda2"],), FILL, dtype=torch.float16, device=device)
        strided_batches(a2buf, S["a_bs"], M, L["lda2"], K - k1, B).copy_(a[:, :, k1:])
        natural = strided_batches(a2buf, M * L["lda2"], M, L["lda2"], K - k1, B)      # what a stride of its own (M * lda2) would read
        alt = BATCH_ALPHA * torch.cat([a[:, :, :k1], natural], 2).double() @ w.double().transpose(1, 2) + b.double() + r.double()
        need_gap(ref[1:], alt[1:], tol, "the second source's batches taken M * lda2 elements apart")
        need_gap(ref, BATCH_ALPHA * a[:, :, :k1].double() @ w[:, :, :k1].double().transpose(1, 2) + b.double() + r.double(), tol_of(ref), "second K source zeroed")
        a2v = strided_batches(a2buf, S["a_bs"], M, L["lda2"], K - k1, B)[0]
    av = strided_batches(abuf, S["a_bs"], M, L["lda"], k1, B)[0]               # batch 0's 2-D views: what ops.gemm reads pointers and row strides from
    wv = strided_batches(wbuf, S["w_bs"], N, L["ldw"], K, B)[0]
    rv = strided_batches(rbuf, S["r_bs"], M, L["ldr"], N, B)
    return av, a2v, wv, b, rv, ref, [(f"batch {z}", z) for z in range(B)]


# ------------------------------------------------------------------------------------------- 9. gathered convolution
CONV_CODES = (2, 4, 5, 7, 9, 35)
# (nb, h, w, stride, pad, upsample, out_size): the VAE downsample's asymmetric pad (pad 0, one extra row / column at the far edge); the
# nearest-x2 image without its last row and column, and without its last column only
CONV_EXTRA = [(4, 10, 6, 2, (0, 0), False, None), (3, 5, 7, 1, (1, 1), True, (9, 13)), (3, 5, 7, 1, (1, 1), True, (10, 13))]


def conv_general(xu, w, b, stride, pt, pl, oh, ow, tall=False):
    """3x3 convolution of the (already upsampled / cropped) images xu to oh x ow outputs with pt / pl zero rows / columns in front and as
    many behind as the output extent needs.  tall: the padding rows above / below an image hold the previous image's last / the next
    image's first row - what a tap-validity test that ignores the image edge between images gathers."""
    H, W = xu.shape[2:]
    pb, pr = (oh - 1) * stride + 3 - pt - H, (ow - 1) * stride + 3 - pl - W
    xp = F.pad(xu, (pl, pr, pt, pb))
    if tall and pt > 0:
        xp[1:, :, pt - 1, pl:pl + W] = xu[:-1, :, -1]
    if tall and pb > 0:
        xp[:-1, :, pt + H, pl:pl + W] = xu[1:, :, 0]
    return F.conv2d(xp, w, b, stride=stride)


def edge_rows(M, oh, ow, device):
    row = torch.arange(M, device=device) // ow % oh
    return (row == 0) | (row == oh - 1)


@cached
def conv_extra_case(idx, c2, device):
    from insv2v.unet import prep_conv3x3
    nb, h, w_, stride, (pt, pl), ups, out_size = CONV_EXTRA[idx]
    c1, cout = R.CONV_C1, R.CONV_COUT
    x1 = rnd(nb, c1, h, w_, device=device).half()
    x2 = rnd(nb, c2, h, w_, seed=2, device=device).half() if c2 else None
    xin = (torch.cat([x1, x2], 1) if c2 else x1).double()
    wt, b = rnd(cout, c1 + c2, 3, 3, scale=(9 * (c1 + c2)) ** -0.5).half(), rnd(cout, seed=4)
    wk, bk = prep_conv3x3({"c.weight": wt.float(), "c.bias": b}, "c", device)
    wt, b = wt.to(device).double(), b.to(device).double()
    full = F.interpolate(xin, scale_factor=2.0, mode="nearest") if ups else xin
    oh, ow = out_size if ups else ((h + 1 - 3) // 2 + 1, (w_ + 1 - 3) // 2 + 1)
    xu = full[:, :, :oh, :ow] if ups else full
    if ups:   # F.interpolate(size=...) is the x2 image without its last row / column
        assert torch.equal(xu, F.interpolate(xin, size=(oh, ow), mode="nearest"))
    conv4 = conv_general(xu, wt, b, stride, pt, pl, oh, ow)
    assert conv4.shape[2:] == (oh, ow)
    M = nb * oh * ow
    rb, res = rnd(1, cout, seed=6, device=device) * 0.5, rnd(M, cout, seed=7, device=device).half()
    extra = rb.double() + res.double()
    conv = to_cl(conv4)
    ref = conv + extra
    tol = tol_of(ref)

    def other(xx=xu, ww=wt, bb=b, **kw):
        args = dict(stride=stride, pt=pt, pl=pl, oh=oh, ow=ow)
        args.update(kw)
        return to_cl(conv_general(xx, ww, bb, **args)) + extra
    need_gap(ref, conv + rb.double(), tol, "residual omitted")
    need_gap(ref, conv + res.double(), tol, "row bias omitted")
    need_gap(ref, other(bb=None), tol, "bias omitted")
    need_gap(ref, other(ww=wt.flip(3)), tol, "taps mirrored")
    if c2:
        for name, sl in (("second", slice(c1, None)), ("first", slice(0, c1))):
            wz = wt.clone()
            wz[:, sl] = 0
            need_gap(ref, other(ww=wz), tol, f"{name} channel source zeroed")
    edge = edge_rows(M, oh, ow, device)
    tall = other(tall=True)
    assert torch.allclose(tall[~edge], ref[~edge], rtol=0, atol=1e-9)
    need_gap(ref[edge], tall[edge], tol_of(ref[edge]), "the batch convolved as one tall image without padding between images")
    blocks = [("first and last image rows", edge)] + [(f"image {i}", slice(i * oh * ow, (i + 1) * oh * ow)) for i in range(nb)]
    if stride == 2:
        need_gap(ref, other(pt=1, pl=1), tol, "output grid shifted by one input pixel")
    if ups:   # the uncropped x2 image: its last row / column is a tap of the last output row / column where the crop must give zero
        seen = to_cl(conv_general(full, wt, b, 1, 1, 1, full.shape[2], full.shape[3])[:, :, :oh, :ow]) + extra
        pix = torch.arange(M, device=device)
        crop = ((pix // ow % oh == oh - 1) if oh < full.shape[2] else torch.zeros_like(edge)) | ((pix % ow == ow - 1) if ow < full.shape[3] else torch.zeros_like(edge))
        assert torch.allclose(seen[~crop], ref[~crop], rtol=0, atol=1e-9)
        need_gap(ref[crop], seen[crop], tol_of(ref[crop]), "the uncropped image's last row / column seen as a tap")
        blocks.append(("output rows / columns at the cropped edge", crop))
    kw = dict(x2=to_cl(x2) if c2 else None, row_bias=rb, rows_per_group=M, residual=res, stride=stride, pad=(pt, pl), upsample=ups, out_size=out_size)
    return to_cl(x1), wk, bk, kw, (nb, oh, ow), ref, blocks


# ------------------------------------------------------------------------------------------- 10. patch-tiled convolution
# (nb, h, w, upsample): 8 x 16 and 16 x 8 patches, one and several per image; nearest-x2 upsample to one patch per image
HALO_GEOMS = [(3, 8, 16, False), (3, 16, 8, False), (2, 16, 16, False), (2, 8, 32, False), (3, 4, 8, True), (2, 8, 4, True)]
HALO_GEOMS_256 = [(2, 16, 16, False), (2, 32, 8, False)]          # code 103: 16 x 16 and 32 x 8 patches
HALO_COUT = (320, 72)                                              # 320: the third 128-column tile is half empty (two waves skip their MFMAs)
HALO_CASES = ([(100,) + g for g in HALO_GEOMS] + [(t,) + g for t in (101, 102) for g in HALO_GEOMS[:2]] + [(103,) + g for g in HALO_GEOMS_256])


@cached
def halo_case(nb, h, w_, ups, two, cout, device):
    """Stride 1 / pad 1 (after the optional exact x2 upsample).  two: Cin = 128 + 64 from two sources - three channel blocks, the source
    switching at the third; else Cin = 64, one block and no double buffer.  Row bias per image, residual."""
    from insv2v.unet import prep_conv3x3
    c1, c2 = (128, 64) if two else (64, 0)
    x1 = rnd(nb, c1, h, w_, device=device).half()
    x2 = rnd(nb, c2, h, w_, seed=2, device=device).half() if two else None
    xin = (torch.cat([x1, x2], 1) if two else x1).double()
    wt, b = rnd(cout, c1 + c2, 3, 3, scale=(9 * (c1 + c2)) ** -0.5).half(), rnd(cout, seed=4)
    wk, bk = prep_conv3x3({"c.weight": wt.float(), "c.bias": b}, "c", device)
    wt, b = wt.to(device).double(), b.to(device).double()
    xu = F.interpolate(xin, scale_factor=2.0, mode="nearest") if ups else xin
    oh, ow = xu.shape[2:]
    M = nb * oh * ow
    table, res = rnd(nb, cout, seed=6, device=device) * 0.5 + 0.3 * torch.arange(nb, device=device)[:, None], rnd(M, cout, seed=7, device=device).half()
    g = group_of(M, oh * ow, 0, device)
    extra = table.double()[g] + res.double()
    conv = to_cl(conv_general(xu, wt, b, 1, 1, 1, oh, ow))
    assert torch.allclose(conv, to_cl(R.conv_ref(xin, wt, b, 1, ups)), rtol=0, atol=1e-9)
    ref = conv + extra
    tol = tol_of(ref)

    def other(xx=xu, ww=wt, bb=b, tall=False):
        return to_cl(conv_general(xx, ww, bb, 1, 1, 1, oh, ow, tall)) + extra
    need_gap(ref, ref - res.double(), tol, "residual omitted")
    need_gap(ref, ref - table.double()[g], tol, "row bias omitted")
    need_gap(ref, ref - table.double()[g] + table.double()[(g + 1) % nb], tol, "row bias of the neighbouring image")
    need_gap(ref, other(bb=None), tol, "bias omitted")
    need_gap(ref, other(ww=wt.flip(3)), tol, "taps mirrored")
    need_gap(ref, other(ww=wt.flip(2)), tol, "taps mirrored top to bottom")
    if two:
        for name, sl in (("second", slice(c1, None)), ("first", slice(0, c1))):
            wz = wt.clone()
            wz[:, sl] = 0
            need_gap(ref, other(ww=wz), tol, f"{name} channel source zeroed")
        xs = xu.clone()
        xs[:, :c2] = xu[:, c1:]
        need_gap(ref, other(xx=xs), tol, "the second source read where the first's first channel block belongs")
    edge = edge_rows(M, oh, ow, device)
    tall = other(tall=True)
    assert torch.allclose(tall[~edge], ref[~edge], rtol=0, atol=1e-9)
    need_gap(ref[edge], tall[edge], tol_of(ref[edge]), "the batch convolved as one tall image without padding between images")
    blocks = [("first and last image rows", edge)] + [(f"image {i}", slice(i * oh * ow, (i + 1) * oh * ow)) for i in range(nb)]
    if cout > 256:
        blocks.append(("columns of the half-empty third column tile", (slice(None), slice(256, cout))))
    kw = dict(x2=to_cl(x2) if two else None, row_bias=table, rows_per_group=oh * ow, residual=res, upsample=ups)
    return to_cl(x1), wk, bk, kw, (nb, oh, ow), ref, blocks


HALO_GN = [(h, w_, two, silu) for (h, w_) in ((8, 16), (16, 8)) for two in (False, True) for silu in (True, False)]
GN_COUT, GN_GROUPS, GN_EPS = 192, 32, 1e-5


@cached
def halo_gn_case(h, w_, two, silu, device):
    """GroupNorm (+ SiLU) of the input applied inside the convolution: 2 samples x 2 frames, the statistics over (C / G, frames, h, w) per
    sample; the (scale, shift) table comes from the fp64 moments of the fp16 input, every shift is at least 0.5 in magnitude (so padding
    that is normalised too shows)."""
    from insv2v.unet import prep_conv3x3
    B, frames, G, cout = 2, 2, GN_GROUPS, GN_COUT
    nb, c1, c2 = B * frames, 128, 64 if two else 0
    C = c1 + c2
    x1 = (rnd(nb, c1, h, w_, device=device) * 1.5 + rnd(1, c1, 1, 1, seed=2, device=device) * 0.5).half()
    x2 = (rnd(nb, c2, h, w_, seed=1, device=device) - 0.3).half() if two else None
    x1[:frames] = (x1[:frames].float() * 0.6 + 0.8).half()                     # the two samples' moments differ
    xin = (torch.cat([x1, x2], 1) if two else x1).double()
    gamma = (1 + 0.1 * rnd(C, seed=3, device=device)).double()
    bsign = torch.where(torch.arange(C, device=device) % 3 == 0, -1.0, 1.0).double()
    beta = bsign * (2.0 + 0.5 * rnd(C, seed=4, device=device).abs().double())
    wt, b = rnd(cout, C, 3, 3, scale=(9 * C) ** -0.5).half(), rnd(cout, seed=5)
    wk, bk = prep_conv3x3({"c.weight": wt.float(), "c.bias": b}, "c", device)
    wt, b = wt.to(device).double(), b.to(device).double()
    x5 = xin.reshape(B, frames, C, h, w_).permute(0, 2, 1, 3, 4)
    grp = x5.reshape(B, G, -1)
    mean, rstd = grp.mean(2), (grp.var(2, unbiased=False) + GN_EPS).rsqrt()
    scale = rstd.repeat_interleave(C // G, 1) * gamma[None]
    shift = beta[None] - mean.repeat_interleave(C // G, 1) * scale
    assert shift.abs().min().item() >= 0.5, f"input condition: a channel's shift is only {shift.abs().min().item():.3g}"
    act = F.silu if silu else (lambda t: t)
    assert torch.allclose((x5 * scale[:, :, None, None, None] + shift[:, :, None, None, None]), F.group_norm(x5, G, gamma, beta, GN_EPS), rtol=0, atol=1e-9)

    def normed(x, sc, sh, act=act):
        s = torch.arange(nb, device=device) // frames
        return act(x * sc[s][:, :, None, None] + sh[s][:, :, None, None])
    M = nb * h * w_
    table, res = rnd(B, cout, seed=6, device=device) * 0.5, rnd(M, cout, seed=7, device=device).half()
    g = group_of(M, frames * h * w_, 0, device)
    extra = table.double()[g] + res.double()
    ref = to_cl(F.conv2d(normed(xin, scale, shift), wt, b, padding=1)) + extra
    tol = tol_of(ref, True)
    pix = torch.arange(M, device=device)
    rim = edge_rows(M, h, w_, device) | (pix % w_ == 0) | (pix % w_ == w_ - 1)         # every pixel with a tap in the padding
    padded = to_cl(F.conv2d(normed(F.pad(xin, (1, 1, 1, 1)), scale, shift), wt, b)) + extra
    assert torch.allclose(padded[~rim], ref[~rim], rtol=0, atol=1e-9)
    need_gap(ref[rim], padded[rim], tol_of(ref[rim], True), "the zero padding normalised too")
    need_gap(ref, to_cl(F.conv2d(normed(xin, scale.flip(0), shift.flip(0)), wt, b, padding=1)) + extra, tol, "the other sample's (scale, shift) table")
    need_gap(ref, to_cl(F.conv2d(xin, wt, b, padding=1)) + extra, tol, "GroupNorm not applied")
    if silu:
        need_gap(ref, to_cl(F.conv2d(normed(xin, scale, shift, lambda t: t), wt, b, padding=1)) + extra, tol, "SiLU omitted")
    need_gap(ref, ref - res.double(), tol, "residual omitted")
    need_gap(ref, ref - table.double()[g], tol, "row bias omitted")
    ab = torch.stack([scale, shift], 2).float().contiguous()                     # [samples, C, 2]
    kw = dict(x2=to_cl(x2) if two else None, row_bias=table, rows_per_group=frames * h * w_, residual=res, gn_ab=ab, gn_images_per_sample=frames, gn_silu=silu)
    blocks = [("pixels at the image edge", rim)] + [(f"sample {i}", slice(i * frames * h * w_, (i + 1) * frames * h * w_)) for i in range(B)]
    return to_cl(x1), wk, bk, kw, (nb, h, w_), ref, blocks


# ------------------------------------------------------------------------------------------- 11. exact rounding
# (tile code, ldc - N, split_k): the vectorised store of five shapes, the scalar stores (ldc % 8 != 0) and the reduction's conversion
EXACT_CASES = [(2, 0, 0), (4, 0, 0), (8, 0, 0), (9, 0, 0), (35, 0, 0), (4, 4, 0), (5, 4, 0), (5, 0, 2)]
