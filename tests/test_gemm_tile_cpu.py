"""The inputs of tests/test_gemm_tile_gpu.py judged without a GPU: every case of tests/gemm_tile_ref.py is built on the CPU, which asserts
every input condition (need_gap: a reference computed without the feature under test is more than 10 x the tolerance away from the true
one); the references are finite and every named block is non-empty; the Python restatement of tile_lds_bytes and the set of valid tile
codes agree with the planner (insv2v_gemm_plan touches no GPU), which also answers the refusals the GPU file asserts on a launch."""
import ctypes

import pytest
import torch

import gemm_engine_ref as R
import gemm_tile_ref as T

CPU = torch.device("cpu")


def finite(*refs):
    for r in refs:
        assert torch.isfinite(r).all()


def nonempty(ref, blocks):
    assert blocks
    for name, idx in blocks:
        assert ref[idx].numel() > 0, name


# ------------------------------------------------------------------------------------------- codes
def test_tile_lds_bytes_and_valid_codes():
    """64 x 64 at ring 2 is bound by its ring, 128 x 128 at ring 2 by the fp32 staging tile, 256 x 128 at ring 4 by a 192 KiB ring: the
    only shape x ring beyond 160 KiB."""
    assert T.tile_lds_bytes(64, 64, 2) == 2 * 128 * 128 + 1024 and T.tile_lds_bytes(128, 128, 2) == 128 * 132 * 4 + 2048
    assert T.tile_lds_bytes(128, 128, 4) == 4 * 256 * 128 + 2048 and T.tile_lds_bytes(256, 128, 4) == 4 * 384 * 128 + 3072 > T.TILE_LDS_MAX
    assert len(T.VALID) == 26 and 46 not in T.VALID and sorted(T.VALID + [46]) == [r * 10 + s for r in (2, 3, 4) for s in range(1, 10)]
    assert set(T.PRODUCT) | set(T.KG) | set(T.DEEP) | set(T.KLOOP_CODES) | set(T.GEGLU_CODES) | set(T.CONV_CODES) <= set(T.VALID) | set(range(1, 10))
    assert all(T.ring_of(c) == 2 and T.shape_of(c) == c for c in range(1, 10)) and T.ring_of(35) == 3 and T.shape_of(48) == 8


def plan(tile, conv=None, act=0, split_k=1):
    """The plan of a small forced problem on 256 CUs (dummy aligned pointers: the planner reads their null / alignment bits only)."""
    from insv2v import _lib
    lib, d, p = _lib.load(), _lib.GemmDesc(), _lib.GemmPlan()
    d.a = d.w = d.c = d.workspace = 256
    d.workspace_bytes, d.tile, d.act, d.split_k, d.batch = 64 << 20, tile, act, split_k, 1
    if conv:
        nb, h, w = conv
        d.M, d.N, d.K, d.mode, d.lda, d.ldw, d.ldc = nb * h * w, 128, 576, 1, 64, 576, 128
        d.NB, d.IH, d.IW, d.OH, d.OW, d.Cin, d.stride, d.pad_t, d.pad_l = nb, h, w, h, w, 64, 1, 1, 1
    else:
        d.M, d.N, d.K, d.lda, d.ldw, d.ldc = 200, 136, 128, 128, 128, 136
    assert lib.insv2v_gemm_plan(ctypes.byref(d), 256, ctypes.byref(p)) == 0
    return p


@pytest.mark.parametrize("conv", [None, (2, 6, 4)])
def test_planner_agrees_with_the_restatement(conv):
    """Every two-digit code 1x .. 5x and every bare shape: planned on the tile kernel with its shape and ring iff the restated LDS size
    fits; ring 1 and ring 5 are invalid arguments, 256 x 128 at ring 4 is unsupported."""
    for code in list(range(1, 10)) + list(range(11, 60)):
        shape, ring = code % 10, (code // 10 or 2)
        p = plan(code, conv)
        if shape == 0:
            continue          # ring forced, shape by rule
        if ring not in (2, 3, 4):
            assert p.rc == T.EINVAL, code
        elif code in T.VALID or code < 10:
            assert (p.rc, p.family, p.variant, p.ring, p.split_k, p.splitk_reduce) == (0, T.PLAN_TILE, shape, ring, 1, 0), code
            assert T.tile_lds_bytes(T.TILE_BM[shape], T.TILE_BN[shape], ring) <= T.TILE_LDS_MAX
        else:
            assert code == 46 and p.rc == T.EUNSUPPORTED
    assert plan(14, conv).rc == T.EINVAL and plan(55, conv).rc == T.EINVAL and plan(46, conv).rc == T.EUNSUPPORTED


def test_planner_refusals_of_the_patch_kernel():
    assert (plan(100, (2, 8, 16)).rc, plan(100, (2, 8, 16)).family, plan(100, (2, 8, 16)).tw_shift) == (0, T.PLAN_HALO, 4)
    assert plan(100, (2, 16, 8)).tw_shift == 3
    assert plan(100, (2, 8, 16), act=T.ACT_RELU).rc == T.EUNSUPPORTED
    assert plan(100, (2, 6, 4)).rc == T.EUNSUPPORTED and plan(100, (2, 12, 20)).rc == T.EUNSUPPORTED
    assert plan(103, (2, 8, 32)).rc == T.EUNSUPPORTED and plan(103, (2, 32, 8)).variant == 3 and plan(103, (2, 16, 16)).tw_shift == 4
    # a forced split runs on the tile kernel's shape, with the reduction behind it
    p = plan(5, None, split_k=2)
    assert (p.rc, p.family, p.variant, p.ring, p.split_k, p.splitk_reduce) == (0, T.PLAN_TILE, 5, 2, 2, 1)
    assert plan(4, None, act=T.ACT_GEGLU).rc == T.EINVAL      # N = 136 is no multiple of 64


# ------------------------------------------------------------------------------------------- cases
def test_layout_inputs():
    a, w, ref = T.layout_case(CPU)
    finite(ref)
    assert torch.equal(a.float(), torch.eye(320)) and ref.shape == (320, 320)


@pytest.mark.parametrize("K", T.KLOOP_K)
def test_kloop_inputs(K):
    a, w, b, ref, blocks = T.kloop_case(K, CPU)
    finite(ref)
    nonempty(ref, blocks)
    Kc = (K + 63) // 64 * 64
    assert a.shape == (T.KLOOP_M, K) and w.shape == (T.KLOOP_N, K) and a.stride(0) == w.stride(0) == Kc + 8
    # what lies behind column K, up to the end of the slice and 8 columns beyond: the fill, inside the buffer
    for t in (a, w):
        behind = torch.as_strided(t, (t.shape[0], Kc + 8 - K), (t.stride(0), 1), K)
        assert (behind == T.FILL).all()


@pytest.mark.parametrize("form", list(T.STORE_FORMS))
def test_store_inputs(form):
    a, w, b, table, r, geom, ref, blocks = T.store_case(form, CPU)
    finite(ref)
    nonempty(ref, blocks)
    N = geom["N"]
    assert ref.shape == (T.STORE_M, N) and geom["c_off"] + N <= geom["ldc"] and geom["r_off"] + N <= geom["ldr"]
    fast = not geom["fp32"] and geom["ldc"] % 8 == 0 and geom["c_off"] % 8 == 0 and geom["ldr"] % 8 == 0 and geom["r_off"] % 8 == 0 and N % 8 == 0
    assert fast == (form in ("a", "a_mod2", "i"))                                   # fast_output_ok of gemm.hip
    assert (N % 4 == 0 and table.stride(0) % 4 == 0) == (form not in ("e", "i"))    # rb_vec


@pytest.mark.parametrize("name", list(T.ACTS))
def test_activation_inputs(name):
    a, w, b, r, ref, blocks = T.act_case(name, CPU)
    finite(ref)
    nonempty(ref, blocks)
    assert ref.shape == T.ACT_SHAPE[:2] and T.ACT_SHAPE[2] == 128


def test_layernorm_inputs():
    a, w, b, col, table, rpg, rb_mod, stats, ref, blocks = T.ln_rows_case(CPU)
    finite(ref, stats)
    nonempty(ref, blocks)
    assert stats.shape == (585, 2) and stats.dtype == torch.float32 and rpg == 117


@pytest.mark.parametrize("res", [False, True])
def test_producer_consumer_inputs(res):
    a, w, b, r, ref, rows = T.producer_case(res, CPU)
    finite(ref)
    assert rows.shape == (T.PC_M, T.PC_NP) and rows.dtype == torch.float16
    for bn, last in ((64, 8), (128, 72)):
        sums = T.part_sums(rows, bn)
        finite(sums)
        assert sums.shape == ((T.PC_NP + bn - 1) // bn, T.PC_M, 2) and T.PC_NP - (sums.shape[0] - 1) * bn == last
        assert torch.allclose(sums[:, :, 0].sum(0), rows.double().sum(1))
    cw, cb, col, cref = T.consumer_case(rows)
    finite(cref)
    assert cref.shape == (T.PC_M, T.PC_NC) and cw.shape == (T.PC_NC, T.PC_NP)


@pytest.mark.parametrize("M,C,NH", R.GEGLU_SHAPES)
def test_geglu_inputs(M, C, NH):
    args, col, stats, ref = T.geglu_case(M, C, NH, CPU)
    finite(ref, stats)
    assert ref.shape == (M, NH) and stats.shape == (M, 2)


@pytest.mark.parametrize("rb_extra", [0, 1])
def test_geglu_row_bias_inputs(rb_extra):
    args, col, stats, table, rpg, ref, blocks = T.geglu_rb_case(rb_extra, CPU)
    finite(ref)
    nonempty(ref, blocks)
    M, C, NH = T.GEGLU_RB_SHAPE
    assert ref.shape == (M, NH) and table.shape == (2, 2 * NH) and table.stride(0) == 2 * NH + rb_extra and 2 * rpg == M


@pytest.mark.parametrize("K", T.SPLIT_K)
def test_splitk_inputs(K):
    a, w, b, table, r, ref, blocks = T.splitk_case(K, CPU)
    finite(ref)
    nonempty(ref, blocks)
    nk = (K + 63) // 64
    assert [len(T.split_ranges(nk, ns)) for ns in T.SPLITS] == ([2, 3, 5, 5] if nk == 5 else [2, 3, 3, 6])      # 5 and 8 leave splits empty


def test_splitk_conv_inputs():
    x, wk, bk, kw, geom, ref, blocks = T.splitk_conv_case(CPU)
    finite(ref)
    nonempty(ref, blocks)
    nb, h, w, cin, cout = T.SPLIT_CONV
    assert ref.shape == (nb * h * w, cout) and wk.shape == (cout, 9 * cin)
    assert [k0 * 64 for k0, _ in T.split_ranges(18, 4)] == [0, 320, 640, 960]          # tap 2 second block, tap 5 first block, tap 7 second block


@pytest.mark.parametrize("two", [False, True])
def test_batched_inputs(two):
    av, a2v, wv, b, rv, ref, blocks = T.batched_case(two, CPU)
    finite(ref)
    nonempty(ref, blocks)
    B, M, N, K = T.BATCH
    assert ref.shape == (B, M, N) and av.shape == (M, 64 if two else K) and av.stride(0) == T.BATCH_LD["lda"]
    assert all(v % 8 == 0 for v in T.BATCH_STRIDE.values())
    assert T.BATCH_STRIDE["a_bs"] > M * T.BATCH_LD["lda"] and T.BATCH_STRIDE["w_bs"] > N * T.BATCH_LD["ldw"]
    assert T.BATCH_STRIDE["c_bs"] > M * T.BATCH_LD["ldc"] and T.BATCH_STRIDE["r_bs"] > M * T.BATCH_LD["ldr"]
    if two:
        assert a2v.shape == (M, 8) and a2v.stride(0) == T.BATCH_LD["lda2"] != T.BATCH_LD["lda"]


@pytest.mark.parametrize("c2", [0, 64])
@pytest.mark.parametrize("idx", range(len(T.CONV_EXTRA)))
def test_conv_extra_inputs(idx, c2):
    x, wk, bk, kw, geom, ref, blocks = T.conv_extra_case(idx, c2, CPU)
    finite(ref)
    nonempty(ref, blocks)
    assert geom == [(4, 5, 3), (3, 9, 13), (3, 10, 13)][idx] and ref.shape == (geom[0] * geom[1] * geom[2], R.CONV_COUT)


def test_conv_general_is_conv_ref():
    x, w, b = R.rnd(2, 8, 7, 5).double(), R.rnd(4, 8, 3, 3).double(), R.rnd(4).double()
    for stride in (1, 2):
        want = R.conv_ref(x, w, b, stride, False)
        assert torch.allclose(T.conv_general(x, w, b, stride, 1, 1, want.shape[2], want.shape[3]), want, rtol=0, atol=1e-12)
    assert torch.allclose(T.conv_general(x, w, b, 1, 1, 1, 7, 5, tall=True), R.conv_ref_tall(x, w, b, 1, False), rtol=0, atol=1e-12)
    assert torch.allclose(T.im2col(x) @ w.permute(0, 2, 3, 1).reshape(4, 72).t() + b, R.to_cl(R.conv_ref(x, w, b, 1, False)), rtol=0, atol=1e-12)


@pytest.mark.parametrize("cout", T.HALO_COUT)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("nb,h,w,ups", sorted(set(T.HALO_GEOMS + T.HALO_GEOMS_256)))
def test_halo_inputs(nb, h, w, ups, two, cout):
    x, wk, bk, kw, geom, ref, blocks = T.halo_case(nb, h, w, ups, two, cout, CPU)
    finite(ref)
    nonempty(ref, blocks)
    oh, ow = geom[1:]
    assert (oh, ow) == ((2 * h, 2 * w) if ups else (h, w)) and ((oh % 8 == 0 and ow % 16 == 0) or (oh % 16 == 0 and ow % 8 == 0))
    assert wk.shape == (cout, 9 * (192 if two else 64))


@pytest.mark.parametrize("h,w,two,silu", T.HALO_GN)
def test_halo_groupnorm_inputs(h, w, two, silu):
    x, wk, bk, kw, geom, ref, blocks = T.halo_gn_case(h, w, two, silu, CPU)
    finite(ref, kw["gn_ab"])
    nonempty(ref, blocks)
    assert kw["gn_ab"].shape == (2, 192 if two else 128, 2) and kw["gn_ab"][..., 1].abs().min() >= 0.5 and geom == (4, h, w)


@pytest.mark.parametrize("res", [False, True])
def test_exact_inputs(res):
    a, w, b, r, ref32, share, ties = R.exact_case(res, CPU)
    finite(ref32)
    assert share > 1 / 3 and ties > 0
    assert all(t in T.VALID or t < 10 for t, _, _ in T.EXACT_CASES) and {(t, e, s) for t, e, s in T.EXACT_CASES if e or s} == {(4, 4, 0), (5, 4, 0), (5, 0, 2)}
