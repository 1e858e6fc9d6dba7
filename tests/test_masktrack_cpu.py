"""A key-frame mask tracked with optical flow, on the host: the float64 restatement (tests/masktrack_ref.py)
against cases worked out by hand, planted misreadings of the definition that the GPU file's inputs must tell apart, the conditions the
GPU file's comparison relies on (share of excluded pixels, the measured K), the interfaces the feature adds (C header, ctypes mirror,
every refusal of the entry, of ``propagate_mask``, ``check_edit_args`` and ``check_args``), the chunking of ``pair_flows``, and the
keywords of a call that uses none of this."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import masktrack_ref as mr
from conftest import ROOT


# ------------------------------------------------------------------------------------------------------------------ the restatement
def test_one_step_by_hand():
    """3 x 4 frame, b = (0.5, 0) everywhere, F_prev_x = column index, F_prev_y = 10 row, M = column index / 4, V_prev with one hole."""
    H, W = 3, 4
    col, row = np.tile(np.arange(W, dtype=np.float64), (H, 1)), np.tile(np.arange(H, dtype=np.float64)[:, None], (1, W))
    b = np.stack([np.full((H, W), 0.5), np.zeros((H, W))])
    Fp = np.stack([col, 10 * row])
    V = np.ones((H, W))
    V[1, 2] = 0.0
    M = col / 4
    r = mr.step(Fp, V, b, None, M, fill=0.125)
    # p = (x + 0.5, y): column 3 leaves the frame (3.5 > 3); inside, S(F_prev_x) = x + 0.5, so F_x = x + 1 and F_y = 10 y
    assert np.array_equal(r["F"][0][:, :3], col[:, :3] + 1.0) and np.array_equal(r["F"][1], 10 * row)
    assert np.array_equal(r["F"][0][:, 3], np.full(H, 3.5))          # clamped to pc = 3: b + F_prev[3] = 0.5 + 3
    want_V = np.ones((H, W))
    want_V[:, 3] = 0.0                                                # out of the frame
    want_V[1, 1] = want_V[1, 2] = 0.0                                 # both touch the hole at (1, 2) with weight 1/2
    assert np.array_equal(r["V"], want_V)
    # mask: M at clamp((x, y) + F) = column min(2 x + 1, 3), row min(11 y, 2) -> min(2 x + 1, 3) / 4; fill where invalid
    want_m = np.minimum(2 * col + 1, 3) / 4
    assert np.array_equal(r["mask"], np.where(want_V == 1, want_m, 0.125))
    # a weight of exactly zero does not count: b = (1, 0) puts column 1 ON the hole's left neighbour column ... and column 2's p = 3
    r = mr.step(Fp, V, np.stack([np.ones((H, W)), np.zeros((H, W))]), None, M)
    assert r["V"][1].tolist() == [1.0, 0.0, 1.0, 0.0] and r["V"][0].tolist() == [1.0, 1.0, 1.0, 0.0]


def test_consistency_inequality_by_hand():
    """b = (2, 0); c = (-2, 0) is consistent (d = 0); c = (-1, 0): |d|^2 = 1 > 0.01 (4 + 1) + 0.5 = 0.55; beta = 1 admits it; c = (-1.3, 0):
    0.49 <= 0.01 (4 + 1.69) + 0.5 holds."""
    H, W = 4, 8
    z = np.zeros((2, H, W))
    b = z.copy()
    b[0] = 2.0
    V, M = np.ones((H, W)), np.ones((H, W))
    inside = np.tile(np.arange(W) + 2 <= W - 1, (H, 1)).astype(np.float64)
    for cx, beta, ok in ((-2.0, 0.5, True), (-1.0, 0.5, False), (-1.0, 1.0, True), (-1.3, 0.5, True), (2.0, 0.5, False)):
        c = z.copy()
        c[0] = cx
        assert np.array_equal(mr.step(z, V, b, c, M, beta=beta)["V"], inside * ok), (cx, beta)
    assert np.array_equal(mr.step(z, V, b, None, M)["V"], inside)


def test_chain_limits():
    """Zero flow: every frame is the key frame.  T = 1: only the key frame.  An invalid pixel stays invalid down the chain."""
    rng = np.random.default_rng(5)
    M = rng.uniform(0, 1, (5, 7))
    zero = np.zeros((4, 2, 5, 7))
    for key in (0, 2, 4):
        r = mr.chain(M, key, zero, zero)
        assert all(np.array_equal(r["mask"][t], M) for t in range(5)) and not r["flow_to_key"].any() and r["valid"].all()
    r = mr.chain(M, 0, zero[:0], zero[:0])
    assert r["mask"].shape == (1, 5, 7) and np.array_equal(r["mask"][0], M)
    assert [len(s) for s in mr.track_plan(5, 2)] == [2, 2] and [len(s) for s in mr.track_plan(5, 0)] == [1] * 4 and mr.track_plan(1, 0) == []
    assert [len(s) for s in mr.track_plan(6, 1)] == [2, 1, 1, 1]
    # the scene moves right by 3 columns, then back: frame 2 shows the key frame again (F = 0), but its last three columns were outside
    # frame 1 on the way - what left the frame stays lost when it comes back, also in frame 3, which does not move
    tc = mr.translation_case(9, 13, 0, [(3, 0), (-3, 0), (0, 0)])
    assert not tc["valid"][1][:, :3].any() and tc["valid"][1][:, 3:].all()
    assert np.array_equal(tc["valid"][2], tc["valid"][3]) and not tc["valid"][3][:, 10:].any() and tc["valid"][3][:, :10].all()
    assert not tc["flow_to_key"][2].any() and not tc["flow_to_key"][3].any()
    assert np.array_equal(tc["mask"][3][:, :10], tc["M"][:, :10]) and not tc["mask"][3][:, 10:].any() and tc["M"][:, 10:].any()


EXACT = mr.EXACT_CASES


def _chain64(tc, key, occlusion, fill, mutate=None):
    return mr.chain(tc["M"].astype(np.float64), key, tc["fwd"].astype(np.float64), tc["bwd"].astype(np.float64), occlusion, fill=fill, mutate=mutate)


@pytest.mark.parametrize("H,W,key,disps,rect", EXACT)
def test_translations_are_index_arithmetic(H, W, key, disps, rect):
    """The definition on integer translations IS the integer expectation the GPU file's bit-exact cases use, with and without the
    consistency check, for a zero and a non-zero fill."""
    for fill in (0.0, 0.375):
        tc = mr.translation_case(H, W, key, disps, fill, bad_rect=rect)
        r, r0 = _chain64(tc, key, True, fill), _chain64(tc, key, False, fill)
        assert all(np.array_equal(r[k], tc[k]) for k in ("mask", "valid", "flow_to_key"))
        assert np.array_equal(r0["mask"], tc["mask_noocc"]) and np.array_equal(r0["valid"], tc["valid_noocc"])
        assert 0 < tc["valid"].mean() < 1
        if rect is not None:
            assert (tc["valid"] != tc["valid_noocc"]).sum() >= (rect[2] - rect[1]) * (rect[4] - rect[3])


# ------------------------------------------------------------------------------------------------------------------ planted mutations
@pytest.mark.parametrize("mutate", mr.MUTATIONS)
def test_mutations_are_caught_by_the_gpu_inputs(mutate):
    """Each misreading of the definition, run through the very comparison the GPU file applies to the kernel (``compare_step`` on the step
    cases; exact equality on the translation cases), fails it on at least one case."""
    caught_step = 0
    for shape in mr.STEP_SHAPES:
        inp = mr.step_inputs(*shape)
        for n in range(shape[0]):
            a = mr.chain_inputs(inp, n)
            got = mr.step(a["F_prev"], a["V_prev"], a["b"], a["c"], a["M"], inp["alpha"], inp["beta"], inp["fill"], mutate=mutate)
            caught_step += bool(mr.compare_step(inp, n, got)[0])
    caught_exact = 0
    for H, W, key, disps, rect in EXACT:
        tc = mr.translation_case(H, W, key, disps, 0.375, bad_rect=rect)
        r = _chain64(tc, key, True, 0.375, mutate)
        caught_exact += not all(np.array_equal(r[k], tc[k]) for k in ("mask", "valid", "flow_to_key"))
    print(f"[masktrack] mutation {mutate}: told apart in {caught_step} step chains and {caught_exact} of {len(EXACT)} exact cases")
    if mutate == "all_four":   # a weight of exactly zero never occurs on the smooth flows; only the integer translations show it
        assert caught_exact >= 4
    else:
        assert caught_step >= 5, mutate


def test_the_definition_itself_passes_the_comparison_and_few_pixels_are_excluded():
    """The float64 definition and its float32 restatement pass ``compare_step``; the share of pixels the guard leaves out is within the
    cap on every chain of every GPU case (a key that violates this is changed; the cap is not); both classes of V occur."""
    worst = 0.0
    for shape in mr.STEP_SHAPES:
        inp = mr.step_inputs(*shape)
        for n in range(shape[0]):
            a = mr.chain_inputs(inp, n)
            args = (a["F_prev"], a["V_prev"], a["b"], a["c"], a["M"], inp["alpha"], inp["beta"], inp["fill"])
            for dtype in (np.float64, np.float32):
                fails, share = mr.compare_step(inp, n, mr.step(*args, dtype=dtype))
                assert not fails, (shape, n, dtype, fails)
            assert share <= mr.MAX_EXCLUDED, (shape, n, share)
            worst = max(worst, share)
            V = mr.step(*args)["V"]
            assert 0 < V.mean() < 1, (shape, n)
    print(f"[masktrack] largest share of excluded pixels in a GPU chain: {worst:.4f}")


def test_measured_k_is_under_the_constant():
    ks = [mr.measure_k(mr.step_inputs(*shape), n) for shape in mr.STEP_SHAPES for n in range(shape[0])]
    print(f"[masktrack] measured K: F {max(k[0] for k in ks):.3f}  mask {max(k[1] for k in ks):.3f}  (constant {mr.K_MEASURED}, GPU bound uses {mr.K_GPU})")
    assert max(max(k) for k in ks) <= mr.K_MEASURED and mr.K_GPU == 4 * mr.K_MEASURED


# ------------------------------------------------------------------------------------------------------------------ interfaces
FIELDS = [("f_prev", "p"), ("v_prev", "p"), ("b", "p"), ("c", "p"), ("m", "p"), ("f_out", "p"), ("v_out", "p"), ("mask_out", "p"),
          ("N", "i"), ("H", "i"), ("W", "i"), ("alpha", "f"), ("beta", "f"), ("fill", "f")]


def test_header_ctypes_and_sources_agree_and_abi_is_15(tmp_path):
    import build
    from insv2v import _lib, ops
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    assert re.search(r"^int insv2v_mask_track_step\(const insv2v_masktrack_desc\* d, insv2v_stream_t stream\);", header, flags=re.M)
    assert _lib.SIGNATURES["insv2v_mask_track_step"] == (ctypes.c_int32, [ctypes.POINTER(_lib.MaskTrackDesc), ctypes.c_void_p])
    assert _lib.ABI_VERSION == 15 and "masktrack.hip" in build.SOURCES and callable(ops.mask_track_step)
    kind = {ctypes.c_void_p: "p", ctypes.c_int32: "i", ctypes.c_float: "f"}
    assert [(n, kind[t]) for n, t in _lib.MaskTrackDesc._fields_] == FIELDS
    body = re.search(r"typedef struct insv2v_masktrack_desc \{(.*?)\} insv2v_masktrack_desc;", header, flags=re.S).group(1)
    names = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        m = re.match(r"\s*(const\s+)?(float|int32_t)\s*(\*?)\s*(.*)", decl.strip())
        if m and m.group(4):
            names += [(v.strip(), "p" if m.group(3) else {"float": "f", "int32_t": "i"}[m.group(2)]) for v in m.group(4).split(",")]
    assert names == FIELDS
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc is not None, "no host C compiler to check the descriptor layout with"
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "insv2v_hip.h"', 'int main(void) {',
            '  printf("%zu\\n", sizeof(insv2v_masktrack_desc));']
    prog += [f'  printf("{n} %zu\\n", offsetof(insv2v_masktrack_desc, {n}));' for n, _ in FIELDS] + ['  return 0;', '}']
    (tmp_path / "layout.c").write_text("\n".join(prog))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    assert int(out[0]) == ctypes.sizeof(_lib.MaskTrackDesc)
    for line in out[1:]:
        if line:
            assert int(line.split()[1]) == getattr(_lib.MaskTrackDesc, line.split()[0]).offset, line
    src = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "masktrack.hip")).read()
    assert "atomic" not in src and "malloc" not in src.lower()   # plain loads and stores, nothing allocated


def test_entry_refuses_bad_arguments_before_any_launch():
    """The argument checks run on the host in front of the launch: the addresses below are never dereferenced."""
    from insv2v import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build
        build.build(verbose=False)
    lib = _lib.load()
    N, H, W = 2, 5, 7
    one, two = N * H * W * 4, N * 2 * H * W * 4
    base = dict(f_prev=0x100000, v_prev=0x200000, b=0x300000, c=0x400000, m=0x500000, f_out=0x600000, v_out=0x700000, mask_out=0x800000,
                N=N, H=H, W=W, alpha=0.01, beta=0.5, fill=0.0)

    def call(**kw):
        d = _lib.MaskTrackDesc()
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        return lib.insv2v_mask_track_step(ctypes.byref(d), None)
    assert lib.insv2v_mask_track_step(None, None) == -1
    for k in ("f_prev", "v_prev", "b", "m", "f_out", "v_out", "mask_out"):
        assert call(**{k: None}) == -1, k
    for kw in (dict(N=0), dict(N=-1), dict(H=1), dict(H=0), dict(W=1), dict(W=-4), dict(alpha=-0.01), dict(beta=-0.5), dict(alpha=float("nan")),
               dict(beta=float("inf")), dict(alpha=float("inf")), dict(beta=float("nan")), dict(fill=float("nan"))):
        assert call(**kw) == -1, kw
    assert call(N=1 << 20, H=1 << 20, W=1 << 20) == -1 and call(N=1, H=1 << 19, W=1 << 21) == -1   # beyond the grid
    size = dict(f_prev=two, v_prev=one, b=two, c=two, m=one, f_out=two, v_out=one, mask_out=one)
    for out in ("f_out", "v_out", "mask_out"):
        for inp in ("f_prev", "v_prev", "b", "c", "m"):
            assert call(**{out: base[inp]}) == -1, (out, inp)                          # the same buffer
            assert call(**{out: base[inp] + size[inp] - 4}) == -1, (out, inp)          # the last element of the input
            assert call(**{out: base[inp] - size[out] + 4}) == -1, (out, inp)          # the last element of the output
    assert call(v_out=base["f_out"] + two - 4) == -1 and call(mask_out=base["v_out"]) == -1 and call(mask_out=base["f_out"] + 4) == -1


class _Counting:
    """A flow estimator that counts its calls: flow = (index of img1's frame - index of img2's frame, 100 * index of img1's frame)."""

    def __init__(self, max_pairs=None):
        if max_pairs is not None:
            self.max_pairs = max_pairs
        self.calls = []

    def __call__(self, img1, img2):
        self.calls.append(img1.shape[0])
        assert img1.shape == img2.shape and img1.shape[1] == 3
        a, b = img1[:, 0, 0, 0], img2[:, 0, 0, 0]
        flow = torch.zeros((img1.shape[0], 2, *img1.shape[2:]))
        flow[:, 0], flow[:, 1] = (a - b)[:, None, None], (100 * a)[:, None, None]
        return flow


def test_pair_flows_chunks_and_order():
    from insv2v.mask_track import pair_flows, needed_pairs, track_plan
    T, H, W = 6, 4, 5
    frames = torch.arange(T, dtype=torch.float32).reshape(1, T, 1, 1, 1).expand(1, T, 3, H, W).clone()   # the frame index as its value, unscaled
    for max_pairs, calls in ((None, [1] * 10), (1, [1] * 10), (4, [4, 4, 2]), (48, [10]), (0, [1] * 10)):
        est = _Counting(max_pairs)
        r = pair_flows(frames, est)
        assert est.calls == calls and r["fwd"].shape == r["bwd"].shape == (T - 1, 2, H, W)
        for t in range(T - 1):   # fwd[t] = est(frame_t, frame_t+1), bwd[t] = est(frame_t+1, frame_t): the frames exactly as handed in
            assert (r["fwd"][t, 0] == -1).all() and (r["fwd"][t, 1] == 100 * t).all()
            assert (r["bwd"][t, 0] == 1).all() and (r["bwd"][t, 1] == 100 * (t + 1)).all()
    for key in range(T):
        est = _Counting(3)
        r = pair_flows(frames, est, both=False, key=key)
        fi, bi = needed_pairs(T, key)
        assert sum(est.calls) == T - 1 == len(fi) + len(bi) and max(est.calls) <= 3
        assert all((r["fwd"][t, 0] == (-1 if t in fi else 0)).all() and (r["bwd"][t, 0] == (1 if t in bi else 0)).all() for t in range(T - 1))
        used = [s for step in track_plan(T, key) for _, _, s, _ in step]
        assert sorted(used) == sorted([("fwd", t) for t in fi] + [("bwd", t) for t in bi])   # exactly what the chain reads as b
        assert track_plan(T, key) == mr.track_plan(T, key) and len(track_plan(T, key)) == max(key, T - 1 - key) <= T - 1
    est = _Counting(4)
    r = pair_flows(frames[:, :1], est)
    assert est.calls == [] and r["fwd"].shape == (0, 2, H, W)
    for bad in (frames[0], frames[:, :, :2], torch.cat([frames, frames])):
        with pytest.raises(ValueError, match="frames"):
            pair_flows(bad, est)
    with pytest.raises(ValueError, match="key"):
        pair_flows(frames, est, both=False)
    with pytest.raises(ValueError, match="key"):
        pair_flows(frames, est, both=False, key=T)


def test_propagate_mask_refuses_before_any_launch():
    """CPU tensors: a launch attempt would raise HipKernelError (ops._req), not ValueError."""
    from insv2v.mask_track import propagate_mask, TRACK_DEFAULTS
    par = inspect.signature(propagate_mask).parameters
    assert {k: par[k].default for k in TRACK_DEFAULTS} == TRACK_DEFAULTS == dict(occlusion=True, alpha=mr.ALPHA, beta=mr.BETA, fill=0.0)
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in TRACK_DEFAULTS) and par["bwd"].default is None
    H, W, T = 8, 16, 4
    M, f = torch.ones((H, W)), torch.zeros((T - 1, 2, H, W))
    with pytest.raises(ValueError, match="occlusion"):   # the occlusion check needs both flow sets
        propagate_mask(M, 0, None, f)
    with pytest.raises(ValueError, match="occlusion"):
        propagate_mask(M, 0, f)
    bad = [dict(key_mask=M[None]), dict(key_mask=torch.ones((1, T, H, W))), dict(key_mask=M.long()), dict(key_mask=M.numpy()),
           dict(key_mask=torch.ones((1, W))), dict(key=-1), dict(key=T), dict(key=1.0), dict(key=True), dict(fwd=f[:, :1]), dict(fwd=f[:2]),
           dict(fwd=torch.zeros((T - 1, 2, H, W + 1))), dict(fwd=None, bwd=None, occlusion=False), dict(alpha=-1.0), dict(alpha=float("nan")),
           dict(beta=-0.5), dict(beta=float("inf")), dict(fill=float("nan")), dict(fill=1.5), dict(fill=-0.1), dict(occlusion=1),
           dict(key=1, bwd=None, occlusion=False), dict(key=2, fwd=None, occlusion=False)]
    for kw in bad:
        a = dict(dict(key_mask=M, key=0, fwd=f, bwd=f), **kw)
        with pytest.raises(ValueError):
            propagate_mask(a.pop("key_mask"), a.pop("key"), a.pop("fwd"), a.pop("bwd"), **a)
    r = propagate_mask(M[None, None], 0, f[:0], f[:0])   # T = 1 launches nothing: it runs on the host
    assert r["mask"].shape == (1, 1, H, W) and torch.equal(r["mask"][0, 0], M) and r["valid"].all() and r["flow_to_key"].shape == (1, 2, H, W)


def test_check_edit_args_refusals():
    from insv2v.run_loveu_tgve import check_edit_args, edit_video, edit_videos, MASK_TRACK_KEYS
    assert MASK_TRACK_KEYS == ("occlusion", "alpha", "beta", "fill")
    par = inspect.signature(check_edit_args).parameters
    assert [par[k].default for k in ("mask_key", "mask_flows", "mask_track")] == [None, None, None]
    par = inspect.signature(edit_video).parameters
    assert [par[k].default for k in ("mask_key", "mask_flows", "flow_estimator", "mask_track")] == [None] * 4
    T, H, W = 6, 32, 48
    shape = (1, T, 3, H, W)
    frames = torch.zeros(shape)
    M, f = torch.ones((1, 1, H, W)), torch.zeros((T - 1, 2, H, W))
    check_edit_args(shape, M, mask_key=0)
    check_edit_args(shape, M, 0.5, "mean", None, T - 1, dict(fwd=f, bwd=f), dict(occlusion=True, alpha=0.0, beta=1.0, fill=0.5))
    check_edit_args(shape, M, mask_key=2, mask_flows=dict(fwd=f), mask_track=dict(occlusion=False))
    check_edit_args((1, 1, 3, H, W), M, mask_key=0)
    cases = [dict(mask="auto", mask_key=0), dict(mask=None, mask_key=0), dict(mask=torch.ones((1, T, H, W)), mask_key=0), dict(mask=M[0], mask_key=0),
             dict(mask=M, mask_key=-1), dict(mask=M, mask_key=T), dict(mask=M, mask_key=1.0), dict(mask=M, mask_key=True),
             dict(mask=M, mask_key=0, mask_track=dict(gamma=1.0)), dict(mask=M, mask_key=0, mask_track=[("alpha", 0.1)]),
             dict(mask=M, mask_key=0, mask_track=dict(alpha=-1.0)), dict(mask=M, mask_key=0, mask_track=dict(beta=float("nan"))),
             dict(mask=M, mask_key=0, mask_track=dict(fill=2.0)), dict(mask=M, mask_key=0, mask_track=dict(occlusion="yes")),
             dict(mask=M, mask_key=0, mask_flows=dict(fwd=f)), dict(mask=M, mask_key=0, mask_flows=dict(fwd=f, bwd=f[:2])),
             dict(mask=M, mask_key=0, mask_flows=dict(fwd=f, bwd=f, mid=f)), dict(mask=M, mask_key=0, mask_flows=[f, f]), dict(mask=M, mask_key=0, mask_flows={}),
             dict(mask=M, mask_key=0, mask_flows=dict(fwd=f, bwd=torch.zeros((T - 1, 2, H, W + 8)))),
             dict(mask=M, mask_flows=dict(fwd=f, bwd=f)), dict(mask=M, mask_track={}), dict(mask=torch.ones((1, 1, H, W + 8)), mask_key=0),
             dict(mask=M.long(), mask_key=0)]
    for kw in cases:
        with pytest.raises(ValueError, match="mask"):
            check_edit_args(shape, kw.get("mask"), 1.0, "max", None, kw.get("mask_key"), kw.get("mask_flows"), kw.get("mask_track"))
        with pytest.raises(ValueError, match="mask"):   # model and pipe are never touched
            edit_video(None, None, frames, None, None, **kw)
        with pytest.raises(ValueError, match="mask"):
            edit_videos(None, None, [dict(frames=frames), dict(frames=frames, **kw)])
    with pytest.raises(ValueError, match="auto_mask"):
        check_edit_args(shape, M, auto_mask={}, mask_key=0)


from driver_fakes import UnseededModel as _Model, RecordingPipe as _RecordingPipe   # noqa: E402


def test_a_call_without_the_new_keywords_is_what_it_was():
    """edit_video / edit_videos / the CLI defaults: the pipe sees exactly the keywords it saw before the feature existed, and nothing asks
    for a flow estimator."""
    from insv2v.run_loveu_tgve import edit_video, edit_videos, build_parser, check_args, mask_track_unit, load_mask_file, build_flow_estimator
    frames = torch.rand((1, 20, 3, 16, 24)) * 2 - 1
    tc = torch.zeros((1, 77, 8))
    first = ["img_cfg", "img_cond", "latent", "text_cfg", "text_cond", "text_uncond"]
    second = sorted(first + ["latent_ref", "noise_correct_step"])
    pipe = _RecordingPipe()
    out = edit_video(_Model(), pipe, frames, tc, tc)
    assert out.shape == frames.shape and pipe.calls == [("call", first), ("second", second)]
    pipe = _RecordingPipe()
    outs = edit_videos(_Model(), pipe, [dict(frames=frames, text_cond=tc, text_uncond=tc) for _ in range(2)])
    assert len(outs) == 2 and pipe.calls == [("stacked", [first, first], []), ("stacked", [second, second], [])]
    pipe = _RecordingPipe()
    edit_videos(_Model(), pipe, [dict(frames=frames, text_cond=tc, text_uncond=tc)])
    assert pipe.calls == [("call", first), ("second", second)]
    a = check_args(build_parser().parse_args([]))
    assert (a.mask_key, a.mask_file, a.mask_no_occlusion) == (None, None, False)
    assert mask_track_unit(a) == {} and load_mask_file(a) == {} and build_flow_estimator(a, "cpu") is None
    # a tracked mask without a flow source is refused like the optical-flow pipe's missing estimator, before anything runs
    M = torch.ones((1, 1, 16, 24))
    pipe = _RecordingPipe()
    with pytest.raises(RuntimeError, match="flow source"):
        edit_video(_Model(), pipe, frames, tc, tc, mask=M, mask_key=3)
    with pytest.raises(RuntimeError, match="flow source"):
        edit_videos(_Model(), pipe, [dict(frames=frames, text_cond=tc, text_uncond=tc), dict(frames=frames, text_cond=tc, text_uncond=tc, mask=M, mask_key=3)])
    assert pipe.calls == []


def test_cli():
    from insv2v.run_loveu_tgve import build_parser, check_args, mask_track_unit
    p = build_parser()
    a = check_args(p.parse_args(["--synthetic", "2", "--synthetic-mask", "--mask-key", "3", "--mask-out", "m.pt"]))
    assert mask_track_unit(a) == dict(mask_key=3, mask_track=dict(occlusion=True))
    a = check_args(p.parse_args(["--units", "u.pt", "--mask-file", "m.pt", "--mask-key", "0", "--mask-no-occlusion", "--raft-ckpt", "raft.pt"]))
    assert mask_track_unit(a) == dict(mask_key=0, mask_track=dict(occlusion=False)) and a.mask_file == "m.pt"
    check_args(p.parse_args(["--mask-file", "m.pt"]))   # drawn masks, not tracked: no estimator needed
    with pytest.raises(SystemExit, match="--mask-key needs a mask"):
        check_args(p.parse_args(["--mask-key", "0", "--raft-ckpt", "raft.pt"]))
    with pytest.raises(SystemExit, match="--mask-key needs a mask"):
        check_args(p.parse_args(["--mask-key", "0", "--synthetic", "2"]))
    with pytest.raises(SystemExit, match="--auto-mask"):
        check_args(p.parse_args(["--mask-key", "0", "--auto-mask", "--mask-file", "m.pt", "--raft-ckpt", "raft.pt"]))
    with pytest.raises(SystemExit, match="--raft-ckpt"):
        check_args(p.parse_args(["--mask-key", "0", "--mask-file", "m.pt"]))
    with pytest.raises(SystemExit, match="--mask-key"):
        check_args(p.parse_args(["--mask-key", "-1", "--mask-file", "m.pt", "--raft-ckpt", "raft.pt"]))
    with pytest.raises(SystemExit, match="--mask-no-occlusion"):
        check_args(p.parse_args(["--mask-no-occlusion"]))
    with pytest.raises(SystemExit, match="--mask-file"):
        check_args(p.parse_args(["--mask-file", "m.pt", "--synthetic", "2", "--synthetic-mask"]))
    with pytest.raises(SystemExit, match="--mask-out"):
        check_args(p.parse_args(["--mask-out", "m.pt", "--mask-file", "m.pt"]))
