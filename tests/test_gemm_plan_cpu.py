"""The dispatch of insv2v_gemm, pinned without a GPU through insv2v_gemm_plan (csrc/gemm_plan.h).

Where the expected values come from: profiles/gemm_plan_parity.txt.  The commit before the planner existed was traced launch by launch
(a build whose launches print instead of running) over the corpus below; the planner's answers were compared with that trace field
by field, and only then were the product rows' fields and the sweep's hash recorded here.  256 CUs (MI355X) unless a test says otherwise."""
import ctypes
import hashlib
import json
import os

import pytest

import gemm_plan_corpus as G
from gemm_plan_corpus import conv, linear, with_options as opt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_dispatch_product.json")
SWEEP_SHA256 = "9c98b8e3569e4ea934d9ec17aede83f20193553e7f5f9909a598811e9f9194e6"
TILE, HALO, Q8, R8, W4 = 1, 2, 3, 4, 5
EINVAL, EUNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    from insv2v import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def product():
    rows = json.load(open(GOLDEN))["rows"]
    return [(f"{r['src']}#{i}", dict(zip(G.FIELDS, r["d"])), r) for i, r in enumerate(rows)]


@pytest.fixture(scope="module")
def sweep():
    return G.sweep()


# One row per rule of plan_gemm, in its order, and one per refusal reason.
W = ["ws"]
NAMED = [
    # refused before any rule
    ("null operand", dict(linear(256, 256, 256), a=0), dict(rc=EINVAL)),
    ("K not a multiple of 8", linear(256, 256, 100), dict(rc=EINVAL)),
    ("second source not a multiple of 64", opt(linear(256, 256, 256), ["k_split_32"]), dict(rc=EINVAL)),
    ("row bias without rows_per_group", opt(linear(256, 256, 256), ["rb_zero"]), dict(rc=EINVAL)),
    ("row statistics with batch 2", opt(linear(256, 256, 256), ["row_stats", "batch2"]), dict(rc=EINVAL)),
    ("stats_out on a convolution", opt(conv(2, 16, 16, 64, 128), ["stats_out"]), dict(rc=EUNSUPPORTED, stats_width=0)),
    ("GEGLU with N % 64", opt(linear(256, 8, 256), ["geglu"]), dict(rc=EINVAL)),
    ("unknown activation", opt(linear(256, 256, 256), ["act7"]), dict(rc=EINVAL)),
    ("weight groups of 100 rows", opt(linear(8192, 640, 256), ["wgroup100"]), dict(rc=EINVAL)),
    ("weight groups with a residual", opt(linear(8192, 640, 256), ["wgroup256", "residual"]), dict(rc=EUNSUPPORTED)),
    ("gn_ab on a linear problem", opt(linear(256, 256, 256), ["gn_ab"]), dict(rc=EINVAL)),
    ("conv with K != 9 Cin", dict(conv(2, 16, 16, 64, 128), K=640), dict(rc=EINVAL)),
    ("upsample to another size", dict(conv(2, 16, 16, 64, 128, "up"), IH=7), dict(rc=EINVAL)),
    ("unknown mode", dict(linear(256, 256, 256), mode=2), dict(rc=EUNSUPPORTED)),
    # beyond the operand window
    ("2^24 rows run as 21 parts", linear(1 << 24, 1280, 64), dict(rc=0, parts=21, units_per_part=798976, family=W4, variant=0, stats_width=0)),
    ("beyond the window with batch 2", opt(linear(1 << 24, 1280, 64), ["batch2"]), dict(rc=EUNSUPPORTED)),
    ("beyond the window with stats_out", opt(linear(1 << 24, 640, 256), ["stats_out"]), dict(rc=EUNSUPPORTED, stats_width=0)),
    ("beyond the window, bias groups across images", opt(conv(4096, 64, 64, 64, 320), ["rb_odd"]), dict(rc=EUNSUPPORTED)),
    ("beyond the window, finalize once for all parts", opt(linear(1 << 24, 640, 256), ["row_stats_parts"]), dict(rc=0, ln_finalize=1, family=R8, parts=11)),
    # grouped weights
    ("weight groups, N % 320: gemm_r8", opt(linear(8192, 640, 256), ["wgroup256"]), dict(rc=0, family=R8, variant=0, forced_tile=240)),
    ("weight groups, N % 256 only: gemm_q8", opt(linear(8192, 512, 256), ["wgroup256"]), dict(rc=0, family=Q8, variant=0, forced_tile=230)),
    ("weight groups forced to gemm_q8 at N = 640", dict(opt(linear(8192, 640, 256), ["wgroup256"]), tile=230), dict(rc=EUNSUPPORTED)),
    # forced tile codes
    ("tile 200: the retired 256x256 kernel", dict(linear(8192, 640, 256), tile=200), dict(rc=EUNSUPPORTED)),
    ("tile 232 with a residual", dict(opt(linear(8192, 640, 256), ["residual"]), tile=232), dict(rc=EUNSUPPORTED)),
    ("tile 233", dict(linear(8192, 640, 256), tile=233), dict(rc=0, family=Q8, variant=3, forced_tile=233)),
    ("tile 236: no such gemm_q8 variant", dict(linear(8192, 640, 256), tile=236), dict(rc=EINVAL)),
    ("tile 240 with stats_out", dict(opt(linear(8192, 640, 256), ["stats_out"]), tile=240), dict(rc=0, family=R8, stats_width=160)),
    ("tile 240 with a misaligned bias", dict(opt(linear(8192, 640, 256), ["bias", "bias_mis"]), tile=240), dict(rc=EUNSUPPORTED)),
    ("tile 244 on a stride-1 convolution: CIM", dict(conv(16, 64, 64, 320, 320), tile=244), dict(rc=0, family=R8, variant=4, cim=1)),
    ("tile 242 on the same: tap-major", dict(conv(16, 64, 64, 320, 320), tile=242), dict(rc=0, family=R8, variant=2, cim=0)),
    ("tile 211 with bias groups of 576 rows", dict(opt(linear(8192, 640, 256), ["rb_odd"]), tile=211), dict(rc=EUNSUPPORTED)),
    ("tile 220 on a convolution", dict(conv(16, 64, 64, 320, 320), tile=220), dict(rc=EUNSUPPORTED)),
    ("tile 213", dict(linear(8192, 640, 256), tile=213), dict(rc=0, family=W4, variant=3, forced_tile=213)),
    ("tile 230 with partial row statistics", dict(opt(linear(8192, 640, 256), ["row_stats_parts"]), tile=230), dict(rc=0, family=Q8, ln_finalize=1)),
    ("tile 46: a 4-deep ring of 256x128 tiles exceeds the LDS", dict(linear(8192, 640, 256), tile=46), dict(rc=EUNSUPPORTED)),
    ("tile 36", dict(linear(8192, 640, 256), tile=36), dict(rc=0, family=TILE, variant=6, ring=3, forced_tile=36)),
    ("tile 77: no ring depth 7", dict(linear(8192, 640, 256), tile=77), dict(rc=EINVAL)),
    ("tile 3 with GEGLU becomes 64x128", dict(opt(linear(1152, 1280, 1280), ["geglu"]), tile=3), dict(rc=0, family=TILE, variant=2)),
    ("tile 100 where no patch fits", dict(conv(9, 15, 17, 64, 64), tile=100), dict(rc=EUNSUPPORTED)),
    ("tile 100 with ReLU", dict(opt(conv(2, 16, 16, 64, 128), ["relu"]), tile=100), dict(rc=EUNSUPPORTED)),
    ("tile 100 on a small convolution", dict(conv(2, 16, 16, 64, 128), tile=100), dict(rc=0, family=HALO, variant=0, tw_shift=4, gn_fuse=1)),
    ("tile 101", dict(conv(2, 16, 16, 64, 128), tile=101), dict(rc=0, family=HALO, variant=1, tw_shift=4, gn_fuse=0)),
    ("tile 103 on 32 x 8 images", dict(conv(64, 32, 8, 256, 512), tile=103), dict(rc=0, family=HALO, variant=3, tw_shift=3)),
    ("tile 103 on 24 x 48 images", dict(conv(4, 24, 48, 128, 256), tile=103), dict(rc=EUNSUPPORTED)),
    # the rules, in order
    ("forced split-K", opt(linear(128, 128, 4096), W + ["split2"]), dict(rc=0, family=TILE, variant=5, split_k=2, splitk_reduce=1)),
    ("automatic split-K", opt(linear(128, 128, 4096), W), dict(rc=0, family=TILE, variant=5, split_k=4, splitk_reduce=1)),
    ("no split-K without a workspace", linear(128, 128, 4096), dict(rc=0, family=TILE, variant=4, split_k=1, splitk_reduce=0)),
    ("one round of 256x320 tiles costs more than 128x128 tiles", opt(linear(8192, 640, 256), W), dict(rc=0, family=TILE, variant=5, stats_width=128)),
    ("gemm_r8 linear", opt(linear(16384, 1280, 256), W), dict(rc=0, family=R8, variant=0, cim=0, forced_tile=240, stats_width=160)),
    ("gemm_r8 with stats_out", opt(linear(16384, 1280, 256), W + ["stats_out"]), dict(rc=0, family=R8, stats_width=160)),
    ("gemm_r8 refuses a misaligned bias under stats_out", opt(linear(16384, 1280, 256), W + ["stats_out", "bias", "bias_mis"]), dict(rc=EUNSUPPORTED, stats_width=160)),
    ("a misaligned bias without stats_out goes on to the next rule", opt(linear(16384, 1280, 256), W + ["bias", "bias_mis"]), dict(rc=0, family=W4, variant=0)),
    ("gemm_r8 CIM convolution", opt(conv(16, 64, 64, 320, 320), W), dict(rc=0, family=R8, cim=1)),
    ("gemm_q8 by rounds of tiles", opt(linear(16384, 1024, 1152), W), dict(rc=0, family=Q8, variant=0, forced_tile=230)),
    ("gemm_r8 GEGLU", opt(linear(8192, 5120, 640), W + ["geglu"]), dict(rc=0, family=R8, variant=0)),
    ("gemm_q8 GEGLU", opt(linear(4096, 1024, 640), W + ["geglu"]), dict(rc=0, family=Q8, variant=0)),
    ("gemm_w4 GEGLU at K = 320", opt(linear(8192, 2560, 320), W + ["geglu"]), dict(rc=0, family=W4, variant=0, forced_tile=210)),
    ("gemm_w4 wide linear", opt(linear(4096, 960, 320), W), dict(rc=0, family=W4, variant=0)),
    ("gemm_q8 wide linear at K = 640", opt(linear(4096, 960, 640), W), dict(rc=0, family=Q8, variant=0)),
    ("partial row statistics ahead of an engine", opt(linear(16384, 1280, 256), W + ["row_stats_parts"]), dict(rc=0, family=R8, ln_finalize=1)),
    ("... but not ahead of the tile kernel", opt(linear(1152, 1280, 1280), W + ["row_stats_parts"]), dict(rc=0, family=TILE, ln_finalize=0)),
    ("patch-tiled convolution", opt(conv(48, 32, 48, 128, 128), W), dict(rc=0, family=HALO, variant=0, tw_shift=4, gn_fuse=1, forced_tile=100)),
    ("... normalising its input", opt(conv(48, 32, 48, 128, 128), W + ["gn_ab"]), dict(rc=0, family=HALO, variant=0, gn_fuse=1)),
    ("16 x 8 patches", opt(conv(1024, 16, 8, 128, 128), W), dict(rc=0, family=HALO, tw_shift=3)),
    ("gn_ab where the patch kernel does not run", opt(conv(2, 16, 16, 64, 128), W + ["gn_ab"]), dict(rc=EUNSUPPORTED, gn_fuse=0)),
    ("big convolution without a patch: gemm_q8", opt(conv(240, 8, 12, 1280, 1280), W), dict(rc=0, family=Q8, variant=0, ln_finalize=0)),
    ("small convolution: 64x64 tiles", opt(conv(2, 16, 16, 64, 128), W), dict(rc=0, family=TILE, variant=4, ring=2, forced_tile=24)),
    ("tile kernel, 128x128", opt(linear(1152, 1280, 1280), W + ["split1"]), dict(rc=0, family=TILE, variant=4, stats_width=64)),
    ("ReLU stays on the tile kernel", opt(linear(8192, 640, 256), W + ["relu"]), dict(rc=0, family=TILE, variant=5, stats_width=128)),
]


@pytest.mark.parametrize("name,d,want", NAMED, ids=[n for n, _, _ in NAMED])
def test_named_rows(lib, name, d, want):
    p = G.plan_of(lib, d)
    assert {k: p[k] for k in want} == want, (name, p)


def test_product_rows_field_by_field(lib, product):
    """Every distinct descriptor the product issues (eager UNet forward alone and as a stack of 5 clips, VAE encode and decode, RAFT; the
    bench geometry and a ragged one): the fields the traced launches of the earlier dispatch show, and its two query answers."""
    assert len(product) > 100
    for name, d, r in product:
        p = G.plan_of(lib, d, 256)
        assert {k: p[k] for k in r["want"]} == r["want"], (name, d, p)
        assert (-(-d["N"] // p["stats_width"]) if p["stats_width"] else 0) == r["parts"] and p["gn_fuse"] == r["fuses"], (name, d, p)
    assert {r["want"].get("family") for _, _, r in product} >= {TILE, HALO, Q8, R8, W4}


def test_sweep_hash(lib, sweep):
    sha = hashlib.sha256()
    for _, d in sweep:
        sha.update((G.plan_text(G.plan_of(lib, d)) + "\n").encode())
    assert len(sweep) == 29711 and sha.hexdigest() == SWEEP_SHA256


def test_queries_read_the_plan_and_no_planned_engine_refuses(lib, sweep, product):
    """For every corpus row, with the CU count insv2v_gemm itself plans by (0 on a machine without a GPU): the two query functions are
    readers of the plan; and an engine the planner names accepts the problem - forcing the plan's own tile code, which asks nothing but
    the engine's predicate, gives the same plan."""
    engines = 0
    for name, d in sweep + [(n, d) for n, d, _ in product] + [(n, d) for n, d, _ in NAMED]:
        c = G.c_desc(d)
        p = G.plan_of(lib, c, 0)
        parts, fuses = lib.insv2v_gemm_stats_parts(ctypes.byref(c)), lib.insv2v_conv3x3_fuses_groupnorm(ctypes.byref(c))
        assert parts == (-(-d["N"] // p["stats_width"]) if p["stats_width"] else 0) and fuses == p["gn_fuse"], (name, p, parts, fuses)
        for cus in (0, 256):
            p = G.plan_of(lib, c, cus)
            if p["rc"] == 0 and p["parts"] == 1 and p["family"] in (Q8, R8, W4):
                engines += 1
                f = G.plan_of(lib, dict(d, tile=p["forced_tile"], split_k=1), cus)
                assert (f["rc"], f["family"], f["variant"], f["cim"]) == (0, p["family"], p["variant"], p["cim"]), (name, p, f)
    assert engines > 5000
