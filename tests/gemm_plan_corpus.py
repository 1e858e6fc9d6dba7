"""Descriptor corpus of the GEMM dispatch (csrc/gemm_plan.h): a seeded sweep over shapes, epilogue options, alignments and forced
tile codes.  One descriptor is a dict of the integer fields of insv2v_gemm_desc (pointers as dummy addresses; alpha / ln_eps do not
take part in the dispatch).  tests/test_gemm_plan_cpu.py rebuilds the sweep from SEED; tools/gemm_plan_trace/check.py writes it as text
for a dispatch-trace harness (profiles/gemm_plan_parity.txt)."""

FIELDS = ["a", "a2", "w", "c", "bias", "row_bias", "residual", "row_stats", "col_sum", "lda", "lda2", "ldw", "ldc", "ldr", "ld_rb",
          "a_bs", "w_bs", "c_bs", "r_bs", "workspace", "workspace_bytes", "M", "N", "K", "k_split", "rows_per_group", "rb_mod", "act",
          "c_fp32", "mode", "NB", "IH", "IW", "OH", "OW", "Cin", "stride", "pad_t", "pad_l", "upsample", "batch", "tile", "split_k",
          "gn_ab", "gn_images_per_sample", "gn_silu", "stats_out", "stats_scratch", "stats_parts", "w_group_stride", "w_group_rows"]
POINTERS = ["a", "a2", "w", "c", "bias", "row_bias", "residual", "row_stats", "col_sum", "workspace", "gn_ab", "stats_out", "stats_scratch"]
ADDR = {p: 0x10000000 * (i + 1) for i, p in enumerate(POINTERS)}   # dummy, 16-byte aligned, never dereferenced
SEED = 20261019

MS = [1, 255, 256, 1152, 4096, 4608, 5760, 8192, 10240, 11520, 12288, 23040, 46080, 92160, 1 << 24]
NS = [8, 64, 128, 256, 320, 512, 640, 960, 1280, 1920, 2560, 3840, 5120, 10240]
KS = [64, 128, 256, 320, 640, 1152, 1280, 2880, 5760, 11520]
# output images of the convolutions: with and without an 8 x 16 / 16 x 8 patch, odd, tiny
IMAGES = [(1, 1), (15, 17), (16, 16), (16, 8), (24, 48), (48, 24), (24, 24), (8, 12), (6, 4), (32, 48), (64, 64), (45, 80), (12, 8), (32, 8)]
TILES = (list(range(1, 10)) + [20 + s for s in range(1, 10)] + [30 + s for s in range(1, 10)] + [40 + s for s in range(1, 10)] + [77, 200] +
         list(range(100, 104)) + list(range(201, 207)) + list(range(210, 222)) + list(range(230, 250)))


class Rng:
    """64-bit LCG (Knuth's MMIX constants): the sweep must not depend on the Python version's random module."""

    def __init__(self, seed):
        self.x = seed

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & ((1 << 64) - 1)
        return (self.x >> 33) % n

    def pick(self, seq):
        return seq[self.below(len(seq))]


def linear(M, N, K):
    d = dict.fromkeys(FIELDS, 0)
    d.update(a=ADDR["a"], w=ADDR["w"], c=ADDR["c"], M=M, N=N, K=K, lda=K, ldw=K, ldc=N, mode=0)
    return d


def conv(NB, OH, OW, Cin, N, geom="same"):
    """geom: same (stride 1, pad 1), s2 (stride 2, pad 0: the VAE's), s2p (stride 2, pad 1), up (exact x2), upodd (x2 less one row and column)."""
    d = linear(NB * OH * OW, N, 9 * Cin)
    d.update(mode=1, NB=NB, OH=OH, OW=OW, IH=OH, IW=OW, Cin=Cin, lda=Cin, stride=1, pad_t=1, pad_l=1)
    if geom in ("s2", "s2p"):
        d.update(stride=2, IH=2 * OH, IW=2 * OW, pad_t=int(geom == "s2p"), pad_l=int(geom == "s2p"))
    elif geom in ("up", "upodd"):
        d.update(upsample=1, IH=(OH + 1) // 2, IW=(OW + 1) // 2)
    return d


def _k_split(d):
    if d["mode"] == 1:
        c1 = d["Cin"] // 128 * 64
        d.update(k_split=c1, a2=ADDR["a2"], lda=max(c1, 8), lda2=max(d["Cin"] - c1, 8))
    else:
        k1 = d["K"] // 128 * 64
        d.update(k_split=k1, a2=ADDR["a2"], lda=max(k1, 8), lda2=max(d["K"] - k1, 8))


def _row_bias(rows, mod=0, ld_pad=0):
    def f(d):
        d.update(row_bias=ADDR["row_bias"], rows_per_group=d["M"] if rows == "M" else rows, ld_rb=d["N"] + ld_pad, rb_mod=mod)
    return f


def _row_stats(parts):
    def f(d):
        d.update(row_stats=ADDR["row_stats"], col_sum=ADDR["col_sum"], stats_parts=parts, stats_scratch=ADDR["stats_scratch"] if parts else 0)
    return f


def _set(**kw):
    return lambda d: d.update(kw)


def _bump(name, by):
    return lambda d: d.update({name: d[name] + by}) if d[name] else None


def _residual(d):
    d.update(residual=ADDR["residual"], ldr=d["N"])


def _batch2(d):
    d.update(batch=2, a_bs=d["M"] * d["lda"], w_bs=d["N"] * d["ldw"], c_bs=d["M"] * d["ldc"], r_bs=d["M"] * d["ldc"], workspace=0, workspace_bytes=0)


def _wgroup(rows):
    return lambda d: d.update(w_group_rows=rows, w_group_stride=d["N"] * d["K"])


WS = 64 << 20
OPTIONS = {
    "silu": _set(act=1), "geglu": _set(act=2), "quick_gelu": _set(act=3), "relu": _set(act=4), "sigmoid": _set(act=5), "tanh": _set(act=6),
    "act7": _set(act=7), "act_neg": _set(act=-1),
    "bias": _set(bias=ADDR["bias"]), "residual": _residual, "k_split": _k_split, "k_split_32": _set(k_split=32, a2=ADDR["a2"], lda2=64),
    "rb_256": _row_bias(1024), "rb_odd": _row_bias(576), "rb_one": _row_bias("M"), "rb_mod": _row_bias(1024, 16), "rb_odd_mod": _row_bias(576, 16),
    "rb_ld": _row_bias(1024, 0, 2), "rb_zero": _row_bias(0),
    "row_stats": _row_stats(0), "row_stats_parts": _row_stats(3), "stats_out": _set(stats_out=ADDR["stats_out"]),
    "gn_ab": _set(gn_ab=ADDR["gn_ab"], gn_images_per_sample=1), "gn_ab16": _set(gn_ab=ADDR["gn_ab"], gn_images_per_sample=16, gn_silu=1),
    "batch2": _batch2, "c_fp32": _set(c_fp32=1),
    "ws": _set(workspace=ADDR["workspace"], workspace_bytes=WS), "ws_small": _set(workspace=ADDR["workspace"], workspace_bytes=4096),
    "split0": _set(split_k=0), "split1": _set(split_k=1), "split2": _set(split_k=2),
    "wgroup256": _wgroup(256), "wgroup1024": _wgroup(1024), "wgroup100": _wgroup(100),
    "c_mis": _bump("c", 4), "residual_mis": _bump("residual", 8), "bias_mis": _bump("bias", 4), "col_sum_mis": _bump("col_sum", 4),
    "row_bias_mis": _bump("row_bias", 4), "ldc_pad8": _bump("ldc", 8), "ldc_pad4": _bump("ldc", 4), "ldr_pad4": _bump("ldr", 4),
}
# (the alignment options act on what earlier options set: they come last)
ORDER = list(OPTIONS)


def with_options(d, names):
    d = dict(d)
    for n in sorted(set(names), key=ORDER.index):
        OPTIONS[n](d)
    return d


def _conv_shapes(M, K):
    """(NB, OH, OW, Cin) of every IMAGES entry that divides M; K = 9 Cin."""
    if K % 576:
        return []
    return [(M // (oh * ow), oh, ow, K // 9) for oh, ow in IMAGES if M % (oh * ow) == 0]


def sweep(seed=SEED):
    """[(name, descriptor)]: the product M x N x K x mode plain and with random option sets, every option alone and every forced tile
    code over a few shapes of each mode.  Deterministic in seed."""
    rng, rows = Rng(seed), []
    names = ORDER

    def draw(d, tag, n):
        for _ in range(n):
            opts = [rng.pick(names) for _ in range(1 + rng.below(4))]
            if rng.below(2):
                opts.append("ws")
            rows.append((tag + "+" + "+".join(opts), with_options(d, opts)))

    geoms = ["same", "same", "same", "s2", "s2p", "up", "upodd"]
    for M in MS:
        for N in NS:
            for K in KS:
                d = linear(M, N, K)
                rows.append((f"lin{M}x{N}x{K}", d))
                rows.append((f"lin{M}x{N}x{K}+ws", with_options(d, ["ws"])))
                draw(d, f"lin{M}x{N}x{K}", 3)
                shapes = _conv_shapes(M, K)
                for NB, oh, ow, cin in shapes[:2] + ([rng.pick(shapes)] if len(shapes) > 2 else []):
                    g = rng.pick(geoms)
                    d = conv(NB, oh, ow, cin, N, g)
                    tag = f"conv{NB}x{oh}x{ow}x{cin}->{N}{g}"
                    rows.append((tag, d))
                    rows.append((tag + "+ws", with_options(d, ["ws"])))
                    draw(d, tag, 3)
    base = [linear(8192, 640, 256), linear(8192, 5120, 640), linear(4096, 1024, 640), linear(8192, 2560, 320), linear(1152, 1280, 1280),
            linear(128, 128, 4096), linear(23040, 1280, 5120), linear(92160, 320, 320), linear(255, 8, 64), linear(12288, 960, 640),
            conv(2, 16, 16, 64, 128), conv(16, 64, 64, 320, 320), conv(48, 32, 48, 320, 320), conv(240, 8, 12, 1280, 1280), conv(16, 32, 48, 640, 640, "up"),
            conv(16, 32, 48, 320, 640, "s2"), conv(4, 45, 80, 128, 256), conv(9, 15, 17, 64, 64, "upodd"), conv(64, 32, 8, 256, 512)]
    for d in base:
        tag = ("conv" if d["mode"] else "lin") + f"{d['M']}x{d['N']}x{d['K']}"
        for o in names:
            rows.append((f"{tag}+{o}", with_options(d, [o, "ws"])))
        for t in TILES:
            rows.append((f"{tag}@{t}", with_options(dict(d, tile=t), ["ws"])))
            for o in ("geglu", "residual", "row_stats_parts", "stats_out", "gn_ab", "split2", "k_split", "relu", "c_mis", "rb_odd"):
                if rng.below(3) == 0:
                    rows.append((f"{tag}@{t}+{o}", with_options(dict(d, tile=t), [o, "ws"])))
    return rows


def text_line(d):
    return " ".join(str(d[f]) for f in FIELDS)


PLAN_FIELDS = ["rc", "family", "variant", "ring", "tw_shift", "cim", "split_k", "ln_finalize", "splitk_reduce", "stats_width", "gn_fuse", "parts",
               "units_per_part", "forced_tile"]


def c_desc(d):
    from insv2v._lib import GemmDesc
    c = GemmDesc()
    for f in FIELDS:
        if d[f]:
            setattr(c, f, d[f])
    c.ln_eps = 1e-5
    return c


def plan_of(lib, d, cus=256):
    """The plan of descriptor d (a dict, or a GemmDesc) as a dict; cus = 0: this device's CU count, as insv2v_gemm itself plans."""
    import ctypes
    from insv2v._lib import GemmPlan
    p = GemmPlan()
    assert lib.insv2v_gemm_plan(ctypes.byref(d if not isinstance(d, dict) else c_desc(d)), cus, ctypes.byref(p)) == 0
    return {f: getattr(p, f) for f in PLAN_FIELDS}


def plan_text(p):
    """Canonical text of a plan.  A refused problem is its return code and the two query answers; nothing else of it is a promise."""
    keep = PLAN_FIELDS if p["rc"] == 0 else ["rc", "stats_width", "gn_fuse"]
    return " ".join(f"{f}={p[f]}" for f in keep)
