"""Scoring an edit in pixel space, on the host: the float64 restatement (tests/pixel_score_ref.py) pinned against
independent formulations (scipy's Gaussian filter, torch's grid_sample, masktrack_ref's validity), its exact cases, planted misreadings
of both definitions that the GPU file's inputs must tell apart, the conditions the GPU file's comparison relies on (share of excluded
pixels, the measured errors behind the bounds), and the interfaces the feature adds: C header, ctypes mirror, exported symbols, every
refusal of the two entries, every ValueError of insv2v/pixel_score.py, and the driver's new flags."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import masktrack_ref as mr
import pixel_score_ref as pr
from conftest import ROOT


# ------------------------------------------------------------------------------------------------------------------ the restatements
def test_ssim_restatement_against_scipy():
    """An independent formulation: scipy.ndimage.gaussian_filter(sigma = 1.5, truncate = 3.5) has radius int(3.5 * 1.5 + 0.5) = 5 and the
    same normalised weights; cropped by 5 its border mode plays no part.  Tolerance: float64 round-off - the moments carry about 1e-16,
    the variances cancel from values <= 1 and are divided by at least C2 = 9e-4, so 1e-12 absolute is a loose cover."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(5)
    for H, W in ((11, 11), (19, 31)):
        X = rng.uniform(0, 1, (3, H, W))
        Y = np.clip(X + rng.normal(0, 0.1, X.shape), 0, 1)

        def gf(a):
            return np.stack([gaussian_filter(a[c], sigma=1.5, truncate=3.5)[5:-5, 5:-5] for c in range(3)])
        mx, my = gf(X), gf(Y)
        sx2, sy2, sxy = gf(X * X) - mx ** 2, gf(Y * Y) - my ** 2, gf(X * Y) - mx * my
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        want = (((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx ** 2 + my ** 2 + C1) * (sx2 + sy2 + C2))).mean(0)
        got = pr.ssim_map(X, Y)
        assert got.shape == (H - 10, W - 10) and np.abs(got - want).max() <= 1e-12
        assert np.abs(pr.ssim_map(X, X) - 1.0).max() <= 1e-12
    g = pr.gauss()
    assert len(g) == 11 and abs(g.sum() - 1) < 1e-15 and np.allclose(g[5] / g[4], np.exp(1 / 4.5)) and np.array_equal(g, g[::-1])


def test_warp_restatement_against_grid_sample_and_masktrack():
    """The sample is F.grid_sample(align_corners=True, padding_mode="border") in float64 (1e-11: the normalised grid rounds the
    coordinate by about 1e-15 W); ``valid`` is masktrack_ref.step's V with a valid previous frame."""
    import torch.nn.functional as F
    for T, H, W, dt in pr.WARP_CASES[1:]:
        inp = pr.warp_inputs(T, H, W, dt)
        V = pr.affine(inp["A"], pr.SIGNED)
        for t in range(T - 1):
            b, c = inp["fwd"][t], inp["bwd"][t]
            ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
            grid = np.stack([2 * (xs + b[0]) / (W - 1) - 1, 2 * (ys + b[1]) / (H - 1) - 1], -1)
            warped = F.grid_sample(torch.from_numpy(V[t + 1])[None], torch.from_numpy(grid)[None], mode="bilinear", padding_mode="border",
                                   align_corners=True)[0].numpy()
            want = ((V[t] - warped) ** 2).mean(0)
            r = pr.warp_pair(V[t], V[t + 1], b, c)
            step = mr.step(np.zeros((2, H, W)), np.ones((H, W)), b, c, np.zeros((H, W)))
            assert np.array_equal(r["valid"], step["V"] == 1)
            assert np.abs(r["err"] - np.where(r["valid"], want, 0.0)).max() <= 1e-11
            r0 = pr.warp_pair(V[t], V[t + 1], b, None)
            assert np.array_equal(r0["valid"], mr.step(np.zeros((2, H, W)), np.ones((H, W)), b, None, np.zeros((H, W)))["V"] == 1)
            assert (r0["valid"] >= r["valid"]).all()


@pytest.mark.parametrize("H,W,disps,deltas,dt,rect", pr.EXACT_CASES)
def test_exact_cases_in_the_restatement(H, W, disps, deltas, dt, rect):
    tc = pr.translation_video(H, W, disps, deltas, rect)
    assert np.array_equal(pr.stored(tc["A"], dt), tc["A"]) and tc["A"].min() >= 0 and tc["A"].max() <= 1   # exact in the operand's dtype
    for dtype in (np.float64, np.float32):
        r = pr.warp_video(tc["A"], tc["fwd"], tc["bwd"], affine_map=(1.0, 0.0), dtype=dtype)
        assert np.array_equal(r["valid"], tc["valid"])
        for t in range(len(disps)):
            assert np.array_equal(r["err"][t], np.where(tc["valid"][t], tc["err"][t], 0.0))
            dx, dy = disps[t]
            assert tc["valid_plain"][t].sum() == (H - abs(dy)) * (W - abs(dx))
        assert np.array_equal(r["warp_error"], tc["err"])
    if rect is not None:
        t, y0, y1, x0, x1 = rect
        assert tc["valid_plain"][t].sum() - tc["valid"][t].sum() == (y1 - y0) * (x1 - x0)   # exactly the rectangle's pixels


def test_fidelity_conventions_by_hand():
    """X == Y: mse 0, psnr inf, ssim 1; a change only inside a binary region: the outside sum is exactly 0; an empty region: nan inside."""
    H, W = 14, 15
    rng = np.random.default_rng(3)
    X = rng.integers(0, 257, (3, H, W)) / 128.0 - 1.0
    w = np.zeros((H, W))
    w[3:9, 4:11] = 1.0
    Y = X + 0.25 * w
    same, _ = pr.fidelity_frame(X, X, w)
    m = pr.fidelity_metrics(same, H, W)
    assert m["mse"] == 0 and m["psnr"] == np.inf and abs(m["ssim"] - 1) < 1e-12 and m["psnr_inside"] == np.inf and m["psnr_outside"] == np.inf
    sums, _ = pr.fidelity_frame(X, Y, w)
    m = pr.fidelity_metrics(sums, H, W)
    assert sums[2] == 0.0 and m["mse_outside"] == 0 and m["psnr_outside"] == np.inf and m["mse_inside"] > 0 and np.isfinite(m["psnr_inside"])
    assert sums[3] == 42 and sums[4] == H * W - 42 and sums[8] + sums[9] == (H - 10) * (W - 10)
    # mse inside by hand: the affine halves the change (clamped where x + 0.25 > 1)
    d = pr.affine(X, pr.SIGNED) - pr.affine(Y, pr.SIGNED)
    assert np.isclose(m["mse_inside"], (d ** 2).mean(0)[3:9, 4:11].mean(), rtol=1e-14, atol=0)
    empty, _ = pr.fidelity_frame(X, Y, np.zeros((H, W)))
    m = pr.fidelity_metrics(empty, H, W)
    assert np.isnan(m["mse_inside"]) and np.isnan(m["psnr_inside"]) and np.isnan(m["ssim_inside"]) and np.isfinite(m["mse_outside"]) and np.isfinite(m["ssim_outside"])


# ------------------------------------------------------------------------------------------------------------------ planted mutations
def _fidelity_metric_bounds(sums, bound, H, W):
    """The GPU bounds of the three SSIM metrics of a frame: the sum's bound over the (exact) denominator."""
    return dict(ssim=bound[5] / ((H - 10) * (W - 10)), ssim_inside=bound[6] / sums[8], ssim_outside=bound[7] / sums[9])


@pytest.mark.parametrize("mutate", pr.SSIM_MUTATIONS)
def test_ssim_mutations_move_the_result_beyond_ten_bounds(mutate):
    T, H, W, xdt, ydt = pr.MUTATION_FIDELITY_CASE
    inp = pr.fidelity_inputs(T, H, W, xdt, ydt)
    sums, bounds, _, _ = pr.fidelity_reference(T, H, W, xdt, ydt)
    moved = 0.0
    for t in range(T):
        mut, _ = pr.fidelity_frame(inp["X"][t], inp["Y"][t], inp["w"][t], mutate=mutate)
        ref_m = pr.fidelity_metrics(sums[t], H, W)
        mut_m = pr.fidelity_metrics(mut, H, W, n_centres=H * W if mutate == "same_pad" else None)
        for k, b in _fidelity_metric_bounds(sums[t], bounds[t], H, W).items():
            moved = max(moved, abs(mut_m[k] - ref_m[k]) / b)
    print(f"[pixel_score] SSIM mutation {mutate}: moves a metric by {moved:.3g} bounds")
    assert moved >= 10.0, (mutate, moved)


@pytest.mark.parametrize("mutate", [m for m in pr.WARP_MUTATIONS if m != "lt"])
def test_warp_mutations_move_the_result_beyond_ten_bounds(mutate):
    T, H, W, dt = pr.MUTATION_WARP_CASE
    inp = pr.warp_inputs(T, H, W, dt)
    ref = pr.warp_reference(T, H, W, dt)
    mut = pr.warp_video(inp["A"], inp["fwd"], inp["bwd"], inp["w"], mutate=mutate)
    bound = float(ref["elem_bound"].max())   # no weighted mean of err can move by more than the largest element bound
    moved = float((np.abs(mut["warp_error"] - ref["ref"]["warp_error"]) / bound).max())
    print(f"[pixel_score] warp mutation {mutate}: moves a pair's warp error by {moved:.3g} bounds")
    assert moved >= 10.0, (mutate, moved)


def test_strict_inequality_is_seen_on_the_boundary():
    """b = (2, 0), c = (-1, 0), alpha = 1/8, beta = 3/8: |d|^2 = 1 = (1/8)(4 + 1) + 3/8 exactly, in float32 too: ``<=`` holds, ``<`` does not."""
    H, W = 4, 8
    b, c = np.zeros((2, H, W)), np.zeros((2, H, W))
    b[0], c[0] = 2.0, -1.0
    A = np.zeros((3, H, W))
    inside = np.tile(np.arange(W) + 2 <= W - 1, (H, 1))
    for dtype in (np.float64, np.float32):
        assert np.array_equal(pr.warp_pair(A, A, b, c, 0.125, 0.375, dtype)["valid"], inside)
        assert not pr.warp_pair(A, A, b, c, 0.125, 0.375, dtype, mutate="lt")["valid"].any()
    m = mr.margins(np.zeros((2, H, W)), np.ones((H, W)), b, c, 0.125, 0.375)
    assert (m["cons"] == 0).all()   # such a pixel is never compared on random inputs: it needs this exact case


# ------------------------------------------------------------------------------------------------------------------ what the GPU comparison relies on
@pytest.mark.parametrize("T,H,W,dt", pr.WARP_CASES)
def test_excluded_share_and_measured_warp_errors(T, H, W, dt):
    for with_bwd in (True, False):
        r = pr.warp_reference(T, H, W, dt, with_bwd)
        inp = pr.warp_inputs(T, H, W, dt)
        r32 = pr.warp_video(inp["A"], inp["fwd"], inp["bwd"] if with_bwd else None, inp["w"], dtype=np.float32)
        print(f"[pixel_score] warp {T}x{H}x{W} {dt} bwd={with_bwd}: excluded {r['share']:.4f}, valid {r['ref']['valid'].mean():.2f}, "
              f"worst |f32 - f64| of err {r['worst']:.3e}, largest err {r['ref']['err'].max():.3e}")
        assert r["share"] <= mr.MAX_EXCLUDED
        assert np.array_equal(r32["valid"][~r["excluded"]], r["ref"]["valid"][~r["excluded"]])   # float32 flips no decision outside the guard
        assert r["worst"] <= 1e-5 and (H < 8 or 0.2 < r["ref"]["valid"].mean() < 1.0)
        if with_bwd and H >= 8:
            assert (r["ref"]["valid"] != pr.warp_reference(T, H, W, dt, False)["ref"]["valid"]).any()   # the planted rectangles act


@pytest.mark.parametrize("T,H,W,xdt,ydt", pr.FIDELITY_CASES)
def test_measured_fidelity_errors(T, H, W, xdt, ydt):
    sums, bounds, worst_se, worst_ssim = pr.fidelity_reference(T, H, W, xdt, ydt)
    m = pr.fidelity_metrics(sums, H, W)
    print(f"[pixel_score] fidelity {T}x{H}x{W} {xdt}/{ydt}: worst |f32 - f64| se {worst_se:.3e}, ssim {worst_ssim:.3e}; relative sum bounds "
          f"{(bounds / np.maximum(np.abs(sums), 1e-300)).max(0)[[0, 5]]}; ssim {m['ssim'].mean():.3f}, mse {m['mse'].mean():.4f}")
    assert worst_se <= 1e-6 and worst_ssim <= 1e-4 and np.isfinite(sums).all() and (bounds >= 0).all()
    assert (bounds[:, [0, 1, 2, 5, 6, 7]] <= 1e-4 * np.abs(sums[:, [0, 1, 2, 5, 6, 7]]) + 1e-6).all()   # the bounds stay tight
    inp = pr.fidelity_inputs(T, H, W, xdt, ydt)
    assert (inp["w"] == 0).any() or H < 20   # flat areas of the region
    assert np.abs(inp["X"]).max() > 1.0       # the clamp acts


def test_tile_shapes_are_named_from_the_kernel_tile():
    from insv2v import ops
    assert ops.frame_fidelity_tile() == pr.TILE
    th, tw = pr.TILE
    shapes = {(H, W) for _, H, W, _, _ in pr.FIDELITY_CASES}
    assert {(11, 11), (11, 12), (12, 11), (th + 10, tw + 10), (th + 9, tw + 9), (th + 11, tw + 10), (th + 10, tw + 11)} <= shapes
    assert any(H > 2 * th + 10 and W > 2 * tw + 10 and W % 2 for H, W in shapes)
    assert {T for T, *_ in pr.FIDELITY_CASES} == {1, 3}


# ------------------------------------------------------------------------------------------------------------------ the C interface
VIEW = [("p", "p"), ("stride_t", "q"), ("stride_c", "q"), ("stride_h", "q"), ("fp32", "i"), ("scale", "f"), ("shift", "f")]
WARP_FIELDS = [("a", "v"), ("fwd", "p"), ("bwd", "p"), ("w", "p"), ("sums", "p"), ("err_map", "p"), ("valid_map", "p"), ("workspace", "p"),
               ("workspace_bytes", "q"), ("T", "i"), ("H", "i"), ("W", "i"), ("alpha", "f"), ("beta", "f")]
FID_FIELDS = [("x", "v"), ("y", "v"), ("w", "p"), ("sums", "p"), ("workspace", "p"), ("workspace_bytes", "q"), ("T", "i"), ("H", "i"), ("W", "i")]


def _header_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    out = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        m = re.match(r"\s*(const\s+)?(void|float|double|int32_t|int64_t|insv2v_frames_view)\s*(\*?)\s*(.*)", decl.strip())
        if m and m.group(4):
            kind = "p" if m.group(3) else {"float": "f", "int32_t": "i", "int64_t": "q", "insv2v_frames_view": "v"}[m.group(2)]
            out += [(v.strip(), kind) for v in m.group(4).split(",")]
    return out


def test_header_ctypes_and_sources_agree_and_abi_is_15(tmp_path):
    import build
    from insv2v import _lib, ops, pixel_score
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    i32, i64, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    want = {"insv2v_warp_error": (i32, [ctypes.POINTER(_lib.WarpErrorDesc), p]), "insv2v_warp_error_workspace_bytes": (i64, [i32, i32, i32]),
            "insv2v_frame_fidelity": (i32, [ctypes.POINTER(_lib.FidelityDesc), p]), "insv2v_frame_fidelity_workspace_bytes": (i64, [i32, i32, i32]),
            "insv2v_frame_fidelity_tile": (i32, [ctypes.POINTER(i32), ctypes.POINTER(i32)])}
    for name, sig in want.items():
        assert re.search(r"^(int|int64_t) %s\(" % name, header, flags=re.M), name
        assert _lib.SIGNATURES[name] == sig, name
    assert re.search(r"^int insv2v_warp_error\(const insv2v_warp_error_desc\* d, insv2v_stream_t stream\);", header, flags=re.M)
    assert re.search(r"^int insv2v_frame_fidelity\(const insv2v_fidelity_desc\* d, insv2v_stream_t stream\);", header, flags=re.M)
    assert _lib.ABI_VERSION == 15 and "pixel_score.hip" in build.SOURCES
    assert callable(ops.warp_error) and callable(ops.frame_fidelity) and callable(pixel_score.score_pixels)
    assert int(re.search(r"#define INSV2V_FIDELITY_K (\d+)", header).group(1)) == _lib.FIDELITY_K == len(ops.FIDELITY_KEYS) == len(pr.FIDELITY_KEYS)
    assert ops.FIDELITY_KEYS == pr.FIDELITY_KEYS
    kind = {p: "p", i32: "i", i64: "q", ctypes.c_float: "f", _lib.FramesView: "v"}
    structs = (("insv2v_frames_view", _lib.FramesView, VIEW), ("insv2v_warp_error_desc", _lib.WarpErrorDesc, WARP_FIELDS),
               ("insv2v_fidelity_desc", _lib.FidelityDesc, FID_FIELDS))
    for cname, cls, fields in structs:
        assert [(n, kind[t]) for n, t in cls._fields_] == fields == _header_fields(header, cname), cname
    cc = next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    assert cc is not None, "no host C compiler to check the descriptor layouts with"
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "insv2v_hip.h"', 'int main(void) {']
    for cname, cls, fields in structs:
        prog += [f'  printf("{cname} size %zu\\n", sizeof({cname}));']
        prog += [f'  printf("{cname} {n} %zu\\n", offsetof({cname}, {n}));' for n, _ in fields]
    (tmp_path / "layout.c").write_text("\n".join(prog + ['  return 0;', '}']))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True,
                   capture_output=True, timeout=120)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    classes = {cname: cls for cname, cls, _ in structs}
    seen = 0
    for line in filter(None, out):
        cname, field, value = line.split()
        assert int(value) == (ctypes.sizeof(classes[cname]) if field == "size" else getattr(classes[cname], field).offset), line
        seen += 1
    assert seen == sum(len(f) + 1 for _, _, f in structs)
    src = open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", "pixel_score.hip")).read()
    assert "atomic" not in src.lower() and "malloc" not in src.lower()   # a fixed-order reduction, nothing allocated
    both = [open(os.path.join(ROOT, "instruct-video-to-video_amd", "csrc", f)).read() for f in ("pixel_score.hip", "masktrack.hip")]
    assert all("mt_consistent(" in s and '#include "flow_sample.h"' in s for s in both)   # ONE occlusion rule, in one place


def _lib_on_host():
    from insv2v import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import build
        build.build(verbose=False)
    return _lib, _lib.load()


def test_exported_symbols_and_workspace_queries():
    _lib, lib = _lib_on_host()
    for name in ("insv2v_warp_error", "insv2v_warp_error_workspace_bytes", "insv2v_frame_fidelity", "insv2v_frame_fidelity_workspace_bytes",
                 "insv2v_frame_fidelity_tile"):
        assert getattr(lib, name) is not None
    th, tw = pr.TILE
    assert lib.insv2v_frame_fidelity_workspace_bytes(1, 11, 11) == 8 * _lib.FIDELITY_K
    assert lib.insv2v_frame_fidelity_workspace_bytes(3, th + 11, tw + 11) == 3 * 4 * 8 * _lib.FIDELITY_K
    assert lib.insv2v_frame_fidelity_workspace_bytes(2, th + 10, tw + 10) == 2 * 8 * _lib.FIDELITY_K
    for bad in ((0, 11, 11), (1, 10, 11), (1, 11, 10), (-1, 64, 64), (70000, 11, 11)):
        assert lib.insv2v_frame_fidelity_workspace_bytes(*bad) == -1, bad
    assert lib.insv2v_warp_error_workspace_bytes(2, 2, 2) == 24 and lib.insv2v_warp_error_workspace_bytes(4, 64, 96) == 3 * 3 * 24
    for bad in ((1, 8, 8), (0, 8, 8), (2, 1, 8), (2, 8, 1), (2, -3, 8), (70000, 8, 8)):
        assert lib.insv2v_warp_error_workspace_bytes(*bad) == -1, bad


def test_entries_refuse_bad_arguments_before_any_launch():
    """The argument checks run on the host in front of the launch: the addresses below are never dereferenced, and every call here is
    one the entry must refuse."""
    _lib, lib = _lib_on_host()
    T, H, W = 3, 12, 16
    plane = H * W

    def view(v, at, p=-1, fp32=1, st=3 * plane, sc=plane, sh=W, scale=0.5, shift=0.5):
        p = at if p == -1 else p
        v.p, v.fp32, v.stride_t, v.stride_c, v.stride_h, v.scale, v.shift = p, fp32, st, sc, sh, scale, shift

    def warp(a=None, **kw):
        d = _lib.WarpErrorDesc()
        view(d.a, 0x100000, **(a or {}))
        base = dict(fwd=0x200000, bwd=0x300000, w=0x400000, sums=0x500000, err_map=0x600000, valid_map=0x700000, workspace=0x800000,
                    workspace_bytes=1 << 16, T=T, H=H, W=W, alpha=0.01, beta=0.5)
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        return lib.insv2v_warp_error(ctypes.byref(d), None)
    assert lib.insv2v_warp_error(None, None) == -1
    for k in ("fwd", "sums", "workspace"):
        assert warp(**{k: None}) == -1, k
    assert warp(a=dict(p=None)) == -1
    for kw in (dict(T=1), dict(T=0), dict(H=1), dict(W=1), dict(H=0), dict(W=-2), dict(alpha=-0.01), dict(beta=-1.0), dict(alpha=float("nan")),
               dict(beta=float("inf")), dict(alpha=float("inf")), dict(beta=float("nan")), dict(workspace_bytes=(T - 1) * 24 - 1), dict(workspace_bytes=0),
               dict(workspace=0x800004), dict(sums=0x500004), dict(T=70000, workspace_bytes=1 << 40)):
        assert warp(**kw) == -1, kw
    for a in (dict(st=-1), dict(sc=-1), dict(sh=W - 1), dict(scale=float("nan")), dict(shift=float("inf"))):
        assert warp(a=a) == -1, a
    frames_bytes = T * 3 * plane * 4
    for kw in (dict(sums=0x100000 + 8), dict(err_map=0x100000 + frames_bytes - 4), dict(valid_map=0x200000), dict(workspace=0x300000 + 8),
               dict(err_map=0x400000 + 16), dict(valid_map=0x600000 + 4 * plane), dict(workspace=0x500000), dict(sums=0x800000 + 8)):   # overlaps
        assert warp(**kw) == -1, kw
    assert warp(a=dict(fp32=0), err_map=0x100000 + frames_bytes // 2 - 4) == -1 and warp(a=dict(st=0), sums=0x100000 + 3 * plane * 4 - 8) == -1

    def fid(x=None, y=None, **kw):
        d = _lib.FidelityDesc()
        view(d.x, 0x100000, **(x or {}))
        view(d.y, 0x200000, **(y or {}))
        base = dict(w=0x400000, sums=0x500000, workspace=0x800000, workspace_bytes=1 << 16, T=T, H=H, W=W)
        for k, v in dict(base, **kw).items():
            setattr(d, k, v)
        return lib.insv2v_frame_fidelity(ctypes.byref(d), None)
    assert lib.insv2v_frame_fidelity(None, None) == -1
    for kw in (dict(sums=None), dict(workspace=None), dict(T=0), dict(T=-1), dict(H=10), dict(W=10), dict(H=1), dict(workspace_bytes=T * 80 - 1),
               dict(workspace=0x800004), dict(sums=0x500004), dict(sums=0x100000), dict(sums=0x200000 + 64), dict(workspace=0x400000 + 8),
               dict(sums=0x800000 + 16)):
        assert fid(**kw) == -1, kw
    for v in (dict(p=None), dict(st=-1), dict(sc=-3), dict(sh=W - 1), dict(scale=float("inf"))):
        assert fid(x=v) == -1 and fid(y=v) == -1, v


# ------------------------------------------------------------------------------------------------------------------ the Python interface
def test_every_value_error_is_raised_before_a_launch(monkeypatch):
    from insv2v import ops, pixel_score as ps
    launched = []
    monkeypatch.setattr(ops, "warp_error", lambda *a, **kw: launched.append("warp"))
    monkeypatch.setattr(ops, "frame_fidelity", lambda *a, **kw: launched.append("fidelity"))
    monkeypatch.setattr(ps, "pair_flows", lambda *a, **kw: launched.append("flows"))
    T, H, W = 3, 12, 14
    A = torch.zeros((T, 3, H, W))
    fwd, w = torch.zeros((T - 1, 2, H, W)), torch.zeros((T, H, W))
    bad_warp = [dict(frames=A[:1]), dict(frames=A[:, :2]), dict(frames=A.double()), dict(frames=A[0]), dict(frames=None), dict(frames=A[:, :, :1]),
                dict(frames=A[:, :, :, :1]), dict(fwd=fwd[:1]), dict(fwd=fwd[:, :1]), dict(fwd=None), dict(fwd=fwd.long()), dict(bwd=fwd[:, :, 1:]),
                dict(bwd="flows"), dict(region=w[:2]), dict(region=w.long()), dict(region=w[None]), dict(alpha=-1), dict(alpha=float("nan")),
                dict(beta=float("inf")), dict(beta="0.5"), dict(alpha=True), dict(affine=(1.0,)), dict(affine=(float("nan"), 0.0)), dict(affine=1.0)]
    for kw in bad_warp:
        a = dict(dict(frames=A, fwd=fwd, bwd=fwd, region=w), **kw)
        with pytest.raises(ValueError, match="warp_error"):
            ps.warp_error(a.pop("frames"), a.pop("fwd"), a.pop("bwd"), **a)
    bad_fid = [dict(source=A[:2]), dict(edited=A[:, :, :10]), dict(source=A[:, :, :10], edited=A[:, :, :10]), dict(source=A[..., :10], edited=A[..., :10]),
               dict(source=A[:0], edited=A[:0]), dict(source=A.double()), dict(edited=None), dict(region=w[:, :5]), dict(region=w.bool()),
               dict(source_affine=(1.0, None)), dict(edited_affine=(1.0, 2.0, 3.0))]
    for kw in bad_fid:
        a = dict(dict(source=A, edited=A, region=w), **kw)
        with pytest.raises(ValueError, match="fidelity"):
            ps.fidelity(a.pop("source"), a.pop("edited"), **a)
    V = torch.zeros((1, T, 3, H, W))
    flows = dict(fwd=fwd, bwd=fwd)
    bad_score = [dict(source_frames=V[0]), dict(edited_frames=V[:, :2]), dict(source_frames=V.double(), edited_frames=V.double()),
                 dict(source_frames=V[..., :10], edited_frames=V[..., :10]), dict(flows=flows, flow_estimator=lambda a, b: a), dict(flows=dict(bwd=fwd)),
                 dict(flows=dict(fwd=fwd)), dict(flows=dict(fwd=fwd[:1], bwd=fwd)), dict(flows=[fwd, fwd]), dict(flow_estimator="raft"),
                 dict(mask=torch.zeros((1, 2, H, W))), dict(mask=torch.zeros((H, W))), dict(mask=torch.zeros((1, 1, H, W)).bool()), dict(occlusion=1)]
    for kw in bad_score:
        a = dict(dict(source_frames=V, edited_frames=V), **kw)
        with pytest.raises(ValueError, match="score_pixels"):
            ps.score_pixels(a.pop("source_frames"), a.pop("edited_frames"), **a)
    assert launched == []
    ps.check_score_pixels_args(V, V, flows=dict(fwd=fwd), occlusion=False)   # half the flows do without the check
    ps.check_score_pixels_args(V[:, :1], V[:, :1], flows=None)               # T = 1: fidelity only
    ps.check_warp_error_args(A, fwd) and ps.check_fidelity_args(A, A.half(), w)
    assert ps.check_warp_error_args.__defaults__[2:4] == (mr.ALPHA, mr.BETA)
    from insv2v.mask_track import TRACK_DEFAULTS
    assert (TRACK_DEFAULTS["alpha"], TRACK_DEFAULTS["beta"]) == (pr.ALPHA, pr.BETA)


def test_check_args_for_the_new_flags():
    from insv2v.run_loveu_tgve import build_parser, check_args, build_flow_estimator, want_pixel_scores, PIXEL_FIDELITY_KEYS, PIXEL_WARP_KEYS
    p = build_parser()
    a = check_args(p.parse_args([]))
    assert (a.score_pixels, a.score_warp) == (False, False) and not want_pixel_scores(a) and build_flow_estimator(a, "cpu") is None
    a = check_args(p.parse_args(["--synthetic", "2", "--score-pixels", "--score-out", "s.json"]))   # no CLIP scorer needed
    assert want_pixel_scores(a) and build_flow_estimator(a, "cpu") is None
    check_args(p.parse_args(["--synthetic", "2", "--score-warp", "--score-out", "s.json"]))
    check_args(p.parse_args(["--units", "u.pt", "--score-warp", "--score-pixels", "--raft-ckpt", "raft.pt", "--score-out", "s.json"]))
    check_args(p.parse_args(["--synthetic", "2", "--score-synthetic", "--score-pixels", "--score-warp", "--score-out", "s.json"]))
    check_args(p.parse_args(["--units", "u.pt", "--score-pixels", "--score-out", "s.json"]))   # fidelity needs no flow source
    with pytest.raises(SystemExit, match="--score-warp needs --raft-ckpt"):
        check_args(p.parse_args(["--units", "u.pt", "--score-warp", "--score-out", "s.json"]))
    with pytest.raises(SystemExit, match="--score-pixels / --score-warp need --score-out"):
        check_args(p.parse_args(["--synthetic", "2", "--score-pixels"]))
    with pytest.raises(SystemExit, match="--score-pixels / --score-warp need --score-out"):
        check_args(p.parse_args(["--synthetic", "2", "--score-warp"]))
    with pytest.raises(SystemExit) as e:   # without both flags today's refusal stays word for word
        check_args(p.parse_args(["--synthetic", "2", "--score-out", "s.json"]))
    assert str(e.value) == "--score-out needs a scorer: --score-ckpt FILE (or --score-synthetic with --synthetic N)"
    assert PIXEL_FIDELITY_KEYS == ("mse", "psnr", "ssim") and "warp_error_source" in PIXEL_WARP_KEYS and "valid_fraction" in PIXEL_WARP_KEYS
