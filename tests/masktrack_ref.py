"""Float64 restatement of the key-frame mask chain (csrc/masktrack.hip is the kernel, insv2v/mask_track.py the host).

One step, from the chain's previous frame t' to frame t, per pixel (x, y); b = the flow on t into t', c = the opposite flow on t' (or None):

    p     = (x + b_x, y + b_y)
    inb   = 0 <= p_x <= W-1  and  0 <= p_y <= H-1
    pc    = p clamped to the frame
    S(G)  = bilinear sample of G at pc (x0 = floor, x1 = min(x0+1, W-1), same in y: border clamp, not zero padding)
            evaluated as two lerps in x and one in y, top + ay (bottom - top) with top = g00 + ax (g01 - g00): a constant region is
            sampled exactly, so a binary mask stays exactly 0 / 1 away from its edges
    cons  = true without c; else with cf = S(c), d = b + cf:   |d|^2 <= alpha * (|b|^2 + |cf|^2) + beta
    Vs    = min of V_t' over the (up to four) neighbours of pc whose bilinear weight is non-zero
    F_t   = b + S(F_t')
    V_t   = inb and cons and Vs
    mask_t = V_t ? bilinear sample of M at clamp((x, y) + F_t) : fill

``step`` is that in any dtype (float64: the definition; float32: the kernel's operation order, used only to calibrate the bound K),
``chain`` the whole video, ``margins`` how far each pixel's three decisions are from flipping, ``compare_step`` the check the GPU test
applies to the kernel's output - the CPU file applies the same check to planted mutations of the definition (``MUTATIONS``).
Everything here is numpy on the host; the inputs are seeded by name, so the CPU and the GPU file see the same arrays."""
import zlib

import numpy as np

ALPHA, BETA = 0.01, 0.5
GUARD_PX, GUARD_REL = 1e-3, 1e-3     # decisions closer than this to flipping are left out of the exact comparison ...
MAX_EXCLUDED = 0.02                  # ... and at most this share of a case's pixels may be left out
STEP_SHAPES = [(1, 2, 2), (1, 16, 24), (2, 40, 56), (3, 17, 33)]   # (N, H, W)
STEP_FILL = 0.25
MUTATIONS = ("c_sign", "c_at_x", "nearest", "zero_pad", "or_valid", "no_fill", "all_four")
# K: the largest ratio, over every element of every STEP_SHAPES case, by which the float32 restatement (the kernel's operation order
# without FMA contraction) departs from float64, in units of 2^-24 * (|b| + max|F_prev| over the neighbours), once the coordinate term
# 2^-23 * max(H,W) * spread has been taken off (``measure_k``).  Measured on these inputs: never above 0.1 - F's largest ratio is
# negative (-0.54), the mask's 0.043: the worst-case coordinate term alone already covers what float32 does here, because the fields
# vary from pixel to pixel wherever they are not exactly constant.  A K below 1 would claim less than the one rounding of the final
# sum, which is always there, so the constant is floored at 1; tests/test_masktrack_cpu.py asserts that the measurement stays at or
# under it.  The GPU bound uses 4 K: the compiler is free to contract a * b + c into one FMA in each of the three lerps.
K_MEASURED = 1.0
K_GPU = 4.0 * K_MEASURED


def _rng(key):
    return np.random.default_rng(zlib.crc32(key.encode()))


# ------------------------------------------------------------------------------------------------------------------ the definition
def _taps(px, py, H, W, dtype, clamp=True):
    """The four taps of a (clamped) point: integer indices, the fractions ax / ay and which taps have a non-zero bilinear weight
    ((1 - ax)(1 - ay), ax (1 - ay), (1 - ax) ay, ax ay with ax, ay in [0, 1): decided on ax and ay, never on a product that could underflow)."""
    if clamp:
        px = np.minimum(np.maximum(px, dtype(0)), dtype(W - 1))
        py = np.minimum(np.maximum(py, dtype(0)), dtype(H - 1))
    fx, fy = np.floor(px), np.floor(py)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = (np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)) if clamp else (x0 + 1, y0 + 1)
    ax, ay = (px - fx).astype(dtype), (py - fy).astype(dtype)
    nz = [np.ones(ax.shape, bool), ax != 0, ay != 0, (ax != 0) & (ay != 0)]
    return dict(x=[x0, x1, x0, x1], y=[y0, y0, y1, y1], ax=ax, ay=ay, nz=nz, cx=px, cy=py)


def _gather(G, yy, xx):
    """G[yy, xx], zero outside the frame (only the zero-padding mutation ever asks outside)."""
    H, W = G.shape
    ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    return np.where(ok, G[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], G.dtype.type(0))


def _sample(G, t, nearest=False):
    """top + ay (bottom - top), top = g00 + ax (g01 - g00), bottom = g10 + ax (g11 - g10) - the kernel's order."""
    if nearest:
        return _gather(G, np.rint(t["cy"]).astype(np.int64), np.rint(t["cx"]).astype(np.int64))
    g = [_gather(G, t["y"][k], t["x"][k]) for k in range(4)]
    top, bottom = g[0] + t["ax"] * (g[1] - g[0]), g[2] + t["ax"] * (g[3] - g[2])
    return top + t["ay"] * (bottom - top)


def step(F_prev, V_prev, b, c, M, alpha=ALPHA, beta=BETA, fill=0.0, dtype=np.float64, mutate=None):
    """One chain: F_prev, b, c [2,H,W] (c may be None), V_prev, M [H,W] -> dict(F [2,H,W], V [H,W], mask [H,W]) in ``dtype``."""
    assert mutate is None or mutate in MUTATIONS
    F_prev, V_prev, b, M = (np.asarray(a).astype(dtype) for a in (F_prev, V_prev, b, M))
    H, W = V_prev.shape
    ys, xs = (a.astype(dtype) for a in np.mgrid[0:H, 0:W])
    px, py = xs + b[0], ys + b[1]
    inb = (px >= 0) & (px <= dtype(W - 1)) & (py >= 0) & (py <= dtype(H - 1))
    clamp, nearest = mutate != "zero_pad", mutate == "nearest"
    t = _taps(px, py, H, W, dtype, clamp)
    cons = np.ones((H, W), dtype=bool)
    if c is not None:
        c = np.asarray(c).astype(dtype)
        tc = _taps(xs, ys, H, W, dtype) if mutate == "c_at_x" else t
        cfx, cfy = _sample(c[0], tc, nearest), _sample(c[1], tc, nearest)
        sign = dtype(-1) if mutate == "c_sign" else dtype(1)
        dx, dy = b[0] + sign * cfx, b[1] + sign * cfy
        cons = dx * dx + dy * dy <= dtype(alpha) * ((b[0] * b[0] + b[1] * b[1]) + (cfx * cfx + cfy * cfy)) + dtype(beta)
    if nearest:
        vs = _sample(V_prev, t, True)
    else:
        vs = np.ones((H, W), dtype=dtype)
        for k in range(4):
            counted = np.ones((H, W), dtype=bool) if mutate == "all_four" else t["nz"][k]
            vs = np.minimum(vs, np.where(counted, _gather(V_prev, t["y"][k], t["x"][k]), dtype(1)))
    F = np.stack([b[0] + _sample(F_prev[0], t, nearest), b[1] + _sample(F_prev[1], t, nearest)])
    V = (inb | cons | (vs > 0.5)) if mutate == "or_valid" else (inb & cons & (vs > 0.5))
    tq = _taps(xs + F[0], ys + F[1], H, W, dtype, clamp)
    mv = _sample(M, tq, nearest)
    mask = mv if mutate == "no_fill" else np.where(V, mv, dtype(fill))
    return dict(F=F, V=V.astype(dtype), mask=mask.astype(dtype))


def track_plan(T, key):
    """[(t, t', b set and index, c set and index)] per launch, as insv2v.mask_track.track_plan (restated, not imported)."""
    steps = []
    for j in range(1, max(key, T - 1 - key) + 1):
        s = []
        if key + j <= T - 1:
            s.append((key + j, key + j - 1, ("bwd", key + j - 1), ("fwd", key + j - 1)))
        if key - j >= 0:
            s.append((key - j, key - j + 1, ("fwd", key - j), ("bwd", key - j)))
        steps.append(s)
    return steps


def chain(M, key, fwd, bwd, occlusion=True, alpha=ALPHA, beta=BETA, fill=0.0, dtype=np.float64, mutate=None):
    """The whole video: M [H,W] on frame ``key``, fwd / bwd [T-1,2,H,W] -> dict(mask [T,H,W], valid [T,H,W], flow_to_key [T,2,H,W])."""
    sets = dict(fwd=fwd, bwd=bwd)
    T = (fwd if fwd is not None else bwd).shape[0] + 1
    H, W = M.shape
    mask, valid, flow = np.zeros((T, H, W), dtype), np.ones((T, H, W), dtype), np.zeros((T, 2, H, W), dtype)
    mask[key] = M
    for s in track_plan(T, key):
        for t, tp, (bs, bi), (cs, ci) in s:
            r = step(flow[tp], valid[tp], sets[bs][bi], sets[cs][ci] if occlusion else None, M, alpha, beta, fill, dtype, mutate)
            flow[t], valid[t], mask[t] = r["F"], r["V"], r["mask"]
    return dict(mask=mask, valid=valid, flow_to_key=flow)


# ------------------------------------------------------------------------------------------------------------------ decision margins
def margins(F_prev, V_prev, b, c, alpha=ALPHA, beta=BETA):
    """Per pixel, how far each of the three decisions behind V is from flipping (float64):
      border   distance of p to the nearest frame border, in pixels
      cons     |lhs - rhs| / rhs of the consistency inequality (inf without c)
      lattice  distance of pc to the nearest lattice line in x or y - where the set of taps with a non-zero weight changes - counted only
               where V_prev is not constant over the 3 x 3 pixels around the lattice point nearest to pc (every tap on either side of the
               line lies in that window), and only inside the frame (outside, V is 0 whatever the taps say); inf elsewhere."""
    f = np.float64
    V_prev, b = np.asarray(V_prev, f), np.asarray(b, f)
    H, W = V_prev.shape
    ys, xs = (a.astype(f) for a in np.mgrid[0:H, 0:W])
    px, py = xs + b[0], ys + b[1]
    border = np.minimum(np.minimum(np.abs(px), np.abs(px - (W - 1))), np.minimum(np.abs(py), np.abs(py - (H - 1))))
    inb = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    t = _taps(px, py, H, W, f)
    cons = np.full((H, W), np.inf)
    if c is not None:
        c = np.asarray(c, f)
        cfx, cfy = _sample(c[0], t), _sample(c[1], t)
        lhs = (b[0] + cfx) ** 2 + (b[1] + cfy) ** 2
        rhs = alpha * ((b[0] ** 2 + b[1] ** 2) + (cfx ** 2 + cfy ** 2)) + beta
        cons = np.abs(lhs - rhs) / rhs
    rx, ry = np.rint(t["cx"]).astype(np.int64), np.rint(t["cy"]).astype(np.int64)
    win = np.stack([V_prev[np.clip(ry + j, 0, H - 1), np.clip(rx + i, 0, W - 1)] for j in (-1, 0, 1) for i in (-1, 0, 1)])
    differs = (win.max(0) != win.min(0)) & inb
    dist = np.minimum(np.abs(t["cx"] - rx), np.abs(t["cy"] - ry))
    return dict(border=border, cons=cons, lattice=np.where(differs, dist, np.inf))


def excluded(m):
    """The pixels whose V the comparison leaves out: a decision margin under its guard."""
    return (m["border"] < GUARD_PX) | (m["cons"] < GUARD_REL) | (m["lattice"] < GUARD_PX)


def _window(G, px, py, g=GUARD_PX):
    """(max |G|, max G - min G) over the neighbours of the clamped point: its four taps, and the taps on the other side of a lattice
    line it lies within ``g`` of (a float32 coordinate may fall there)."""
    H, W = G.shape
    cx, cy = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
    xa, xb = np.clip(np.floor(cx - g), 0, W - 1).astype(np.int64), np.clip(np.floor(cx + g) + 1, 0, W - 1).astype(np.int64)
    ya, yb = np.clip(np.floor(cy - g), 0, H - 1).astype(np.int64), np.clip(np.floor(cy + g) + 1, 0, H - 1).astype(np.int64)
    vals = np.stack([G[np.minimum(ya + j, yb), np.minimum(xa + i, xb)] for j in range(3) for i in range(3)])
    return np.abs(vals).max(0), vals.max(0) - vals.min(0)


def bound_terms(F_prev, b, M, ref):
    """The two terms of the element-wise bound  K * 2^-24 * A + 2^-23 * max(H,W) * S  for F [2,H,W] and for mask [H,W]:
    A = |b| + max |F_prev| over the neighbours of pc, S = the spread of F_prev over them (per component); for the mask the same with M
    over the neighbours of clamp((x, y) + F) and |b| = |b_x| + |b_y|."""
    f = np.float64
    F_prev, b, M = np.asarray(F_prev, f), np.asarray(b, f), np.asarray(M, f)
    H, W = M.shape
    ys, xs = (a.astype(f) for a in np.mgrid[0:H, 0:W])
    px, py = xs + b[0], ys + b[1]
    A, S = np.zeros((2, H, W)), np.zeros((2, H, W))
    for k in range(2):
        mx, sp = _window(F_prev[k], px, py)
        A[k], S[k] = np.abs(b[k]) + mx, sp
    mx, sp = _window(M, xs + ref["F"][0], ys + ref["F"][1])
    scale = 2.0 ** -23 * max(H, W)
    return dict(F=(2.0 ** -24 * A, scale * S), mask=(2.0 ** -24 * (np.abs(b[0]) + np.abs(b[1]) + mx), scale * sp))


def compare_step(inp, n, got, K=K_GPU):
    """The GPU test's check of chain n of a step case: ``got`` = dict(F, V, mask) float arrays of that chain.  Returns (failures, share of
    excluded pixels): V and the valid / fill choice of mask exactly wherever the decision margins exceed the guard, F everywhere and mask
    on the valid pixels within the bound."""
    a = chain_inputs(inp, n)
    ref = step(a["F_prev"], a["V_prev"], a["b"], a["c"], a["M"], inp["alpha"], inp["beta"], inp["fill"])
    ex = excluded(margins(a["F_prev"], a["V_prev"], a["b"], a["c"], inp["alpha"], inp["beta"]))
    terms = bound_terms(a["F_prev"], a["b"], a["M"], ref)
    fails = []
    gF, gV, gm = (np.asarray(got[k], np.float64) for k in ("F", "V", "mask"))
    if not np.isfinite(gF).all() or not np.isfinite(gV).all() or not np.isfinite(gm).all():
        fails.append("non-finite output")
    if not np.isin(gV, (0.0, 1.0)).all():
        fails.append("V is not 0 / 1")
    bad = (gV != ref["V"]) & ~ex
    if bad.any():
        fails.append(f"V differs on {int(bad.sum())} pixels outside the guard")
    errF = np.abs(gF - ref["F"])
    over = errF > K * terms["F"][0] + terms["F"][1]
    if over.any():
        fails.append(f"F beyond the bound on {int(over.sum())} elements (worst excess {float((errF - K * terms['F'][0] - terms['F'][1]).max()):.3e})")
    inv = (ref["V"] == 0) & ~ex
    if (gm[inv] != inp["fill"]).any():
        fails.append(f"mask is not fill on {int((gm[inv] != inp['fill']).sum())} invalid pixels")
    val = (ref["V"] == 1) & ~ex
    errm = np.abs(gm - ref["mask"])
    over = val & (errm > K * terms["mask"][0] + terms["mask"][1])
    if over.any():
        fails.append(f"mask beyond the bound on {int(over.sum())} valid pixels (worst error {float(errm[over].max()):.3e})")
    return fails, float(ex.mean())


def measure_k(inp, n):
    """(K of F, K of mask) of chain n: the largest (|float32 restatement - float64| - coordinate term) / (2^-24 A); the mask on the pixels
    both precisions call valid."""
    a = chain_inputs(inp, n)
    args = (a["F_prev"], a["V_prev"], a["b"], a["c"], a["M"], inp["alpha"], inp["beta"], inp["fill"])
    r64, r32 = step(*args), step(*args, dtype=np.float32)
    terms = bound_terms(a["F_prev"], a["b"], a["M"], r64)
    out = []
    for name, sel in (("F", np.ones_like(r64["F"], bool)), ("mask", (r64["V"] == 1) & (r32["V"] == 1))):
        err = np.abs(r32[name].astype(np.float64) - r64[name]) - terms[name][1]
        unit = terms[name][0]
        assert not (sel & (unit == 0) & (err > 0)).any(), name   # nothing to scale by: the value must then be exact
        ratio = np.where(sel & (unit > 0), err / np.where(unit > 0, unit, 1.0), 0.0)
        out.append(float(ratio.max()))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------ inputs
def _smooth(rng, H, W, amp, cells=4):
    """A smooth field [H,W]: a coarse random grid (about ``cells`` pixels apart) interpolated bilinearly, scaled to +-amp."""
    gh, gw = max(2, H // cells + 2), max(2, W // cells + 2)
    g = rng.uniform(-1.0, 1.0, (gh, gw))
    y, x = np.linspace(0, gh - 1, H), np.linspace(0, gw - 1, W)
    t = _taps(*np.meshgrid(x, y), gh, gw, np.float64)
    return amp * _sample(g, t)


def step_inputs(N, H, W):
    """The inputs of one GPU step case, float32 values held as float64-exact arrays: smooth flows of a few pixels (scaled down on a tiny
    frame), c about -b resampled plus planted inconsistent rectangles, a V_prev with holes, an arbitrary smooth F_prev and a key mask
    whose values are 0 or at least 1/2 (so that the bound's scale never vanishes where the mask varies)."""
    rng = _rng(f"masktrack.step.{N}.{H}.{W}")
    amp = min(3.0, min(H, W) / 8.0)
    ys, xs = (a.astype(np.float64) for a in np.mgrid[0:H, 0:W])
    out = dict(F_prev=[], V_prev=[], b=[], c=[], M=[], alpha=ALPHA, beta=BETA, fill=STEP_FILL, N=N, H=H, W=W)
    for n in range(N):
        b = np.stack([_smooth(rng, H, W, amp) + 0.4 * amp, _smooth(rng, H, W, amp) - 0.3 * amp])
        t = _taps(xs - b[0], ys - b[1], H, W, np.float64)          # c(z) ~ -b(z - b(z))
        c = -np.stack([_sample(b[0], t), _sample(b[1], t)]) + rng.uniform(-0.05, 0.05, (2, H, W))
        for _ in range(2 if H >= 8 else 0):                         # planted inconsistent rectangles
            y0, x0 = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
            c[:, y0:y0 + max(3, H // 5), x0:x0 + max(3, W // 5)] += np.array([3.0, -2.0])[:, None, None]
        V = np.ones((H, W))
        for _ in range(3 if H >= 8 else 0):                         # holes (none on the tiny frame: one would leave no valid pixel)
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            V[y0:y0 + max(1, H // 6), x0:x0 + max(1, W // 6)] = 0.0
        Fp = np.stack([_smooth(rng, H, W, 2 * amp), _smooth(rng, H, W, 2 * amp)])
        s = 0.5 + 0.5 * _smooth(rng, H, W, 1.0, cells=6)
        M = np.where(s > 0.5, s, 0.0)
        for k, v in (("F_prev", Fp), ("V_prev", V), ("b", b), ("c", c), ("M", M)):
            out[k].append(v.astype(np.float32))
    for k in ("F_prev", "V_prev", "b", "c", "M"):
        out[k] = np.stack(out[k])
    return out


def chain_inputs(inp, n):
    return {k: inp[k][n].astype(np.float64) for k in ("F_prev", "V_prev", "b", "c", "M")}


# ------------------------------------------------------------------------------------------------------------------ the exact cases
# (H, W, key, disps, bad_rect) of the bit-exact cases: key first, in the middle and last; with and without a planted inconsistency
_DISPS = [(1, 0), (2, -1), (0, 1), (1, 1)]
EXACT_CASES = [(9, 13, 0, _DISPS, None), (9, 13, 2, _DISPS, None), (9, 13, 4, _DISPS, None), (9, 13, 1, _DISPS, (2, 3, 6, 4, 8)),
               (9, 13, 3, _DISPS, (2, 3, 6, 4, 8)), (5, 7, 1, [(-1, 2)], None)]


def translation_case(H, W, key, disps, fill=0.0, seed="masktrack.exact", bad_rect=None, M=None):
    """A scene that moves by the integer displacement ``disps[t]`` = (dx, dy) between frames t and t+1: fwd[t] = +d, bwd[t] = -d, constant
    over the frame.  Everything is exact in float32, so the expectation is integer index arithmetic, not the definition above: frame t
    shows the key mask shifted by the accumulated displacement; a pixel is valid iff every position on its way to the key frame lies in
    the frame; invalid pixels are ``fill``.  ``bad_rect`` = (t, y0, y1, x0, x1): there the flow set that serves as c on the chain's way
    to frame t (fwd for t > key: the rectangle is on frame t-1; bwd for t < key: on frame t+1) is made inconsistent (+ (5, 5)); with the
    occlusion check, what samples the rectangle is invalid from then on.
    ``M``: the key mask [H,W] (default: seeded multiples of 1/8 with holes).
    -> dict(M, fwd, bwd [T-1,2,H,W], mask, valid [T,H,W], flow_to_key [T,2,H,W], and the same three without the rectangle's effect)."""
    rng = _rng(f"{seed}.{H}.{W}")
    T = len(disps) + 1
    if M is None:
        M = np.round(rng.uniform(0, 1, (H, W)) * 8) / 8 * (rng.uniform(0, 1, (H, W)) > 0.4)
    M = np.asarray(M).astype(np.float32)
    d = np.asarray(disps, np.float32).reshape(T - 1, 2)
    fwd = np.broadcast_to(d[:, :, None, None], (T - 1, 2, H, W)).copy()
    bwd = -fwd
    ys, xs = np.mgrid[0:H, 0:W]

    def run(with_rect):
        mask, valid, flow = np.zeros((T, H, W), np.float32), np.ones((T, H, W), np.float32), np.zeros((T, 2, H, W), np.float32)
        mask[key] = M
        order = [(t, t - 1, -d[t - 1]) for t in range(key + 1, T)] + [(t, t + 1, d[t]) for t in range(key - 1, -1, -1)]
        for t, tp, bvec in order:
            sx, sy = xs + int(bvec[0]), ys + int(bvec[1])          # where frame t's pixel lies in t'
            ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
            cx, cy = np.clip(sx, 0, W - 1), np.clip(sy, 0, H - 1)
            flow[t] = bvec[:, None, None] + flow[tp][:, cy, cx]
            v = ok & (valid[tp][cy, cx] == 1)
            if with_rect and bad_rect is not None and bad_rect[0] == t:
                _, y0, y1, x0, x1 = bad_rect
                v &= ~((cy >= y0) & (cy < y1) & (cx >= x0) & (cx < x1))
            qx, qy = np.clip(xs + flow[t][0].astype(np.int64), 0, W - 1), np.clip(ys + flow[t][1].astype(np.int64), 0, H - 1)
            valid[t] = v
            mask[t] = np.where(v, M[qy, qx], np.float32(fill))
        return mask, valid, flow

    if bad_rect is not None:
        t, y0, y1, x0, x1 = bad_rect
        (fwd if t > key else bwd)[t - 1 if t > key else t][:, y0:y1, x0:x1] += 5.0
    mask, valid, flow = run(True)
    mask0, valid0, flow0 = run(False)
    return dict(M=M, fwd=fwd, bwd=bwd, mask=mask, valid=valid, flow_to_key=flow, mask_noocc=mask0, valid_noocc=valid0, flow_noocc=flow0)
