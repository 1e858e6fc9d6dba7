"""The editing drivers, traced on the CPU: what ``edit_video`` and ``edit_videos`` hand the model, the pipe, the flow estimator and the
eight ``ops`` entries they reach the GPU through, call by call.

Every fake and every stand-in appends one record to a trace: the callee, every argument by name (scalars as they are; tensors as shape,
dtype and ``zlib.crc32`` of their bytes) and the result in the same form.  The inputs are ``arange`` arithmetic on dyadic values and the
stand-ins only index and do element-wise arithmetic whose results are exact, so the checksums are the same on any CPU.

``tests/golden/driver_trace.json`` holds, per case, one ``[callee, crc32 of the record's canonical JSON]`` per record, and the result of
the call in the same form.  It was recorded with ``python tests/test_driver_trace_cpu.py --write`` BEFORE the drivers were rewritten
around one per-unit object (``_EditUnit``); the tests only read it.

  * every ``edit_video`` case and the single-unit ``edit_videos`` cases reproduce their recorded trace record for record;
  * a multi-unit ``edit_videos`` case reproduces its recorded pipe calls (``run_stacked``: keywords, shapes, checksums) and results, and
    the rest of its trace is its units' own ``edit_video`` traces merged by phase: cut each unit's trace at its pipe calls into segments;
    between two stacked pipe calls the stacked trace is the concatenation, in unit order, of the units' segments of that index.  One cut
    more is needed to phrase it: ``edit_videos`` prepares EVERY unit before it builds the first window call of any, while a unit alone
    builds its first window call right after its own preparation, so the segment before the first pipe call is cut once more, into the
    unit's preparation and its first window call (its trailing records of ``WINDOW_OPS``: building a window call draws noise and
    re-noises the source, nothing else, and a preparation ends with neither).  That is "per unit, bit for bit what ``edit_video`` does
    alone", written as an assertion.  Before the rewrite it failed for the cases named in ``MERGE_FAILED_BEFORE``.

The unseeded draw, ``torch.randn``, has a stand-in like the ``ops`` entries (a function of the shape alone), so that an unseeded unit
gets the same noise alone and in a stack.
"""
import json
import math
import os
import sys
import zlib

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "driver_trace.json")
FIB, REF = 4, 2           # frames_in_batch, num_ref_frames: 9 frames are three windows that carry over 2 frames, then 1
H, W = 16, 24
TRACE = []
OPS = ("randn", "add_noise", "mask_to_latent", "composite", "mask_track_step", "mask_shape", "temporal_filter", "keyframe_fill")
MERGE_FAILED_BEFORE = ("multi_mixed", "multi_key")


# ------------------------------------------------------------------------------------------------------------------ the trace
def _desc(v):
    if torch.is_tensor(v):
        t = v.detach().contiguous().cpu()
        return ["T", list(t.shape), str(t.dtype).replace("torch.", ""), zlib.crc32(t.numpy().tobytes())]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, dict):
        return {str(k): _desc(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_desc(x) for x in v]
    return type(v).__name__


def _rec(callee, args, result):
    TRACE.append({"callee": callee, "args": _desc(args), "result": _desc(result)})


def _short(records):
    return [[r["callee"], zlib.crc32(json.dumps(r, sort_keys=True).encode())] for r in records]


# ------------------------------------------------------------------------------------------------------------------ the fakes
class TraceModel:
    scale_factor = 0.5

    class unet:
        device = torch.device("cpu")

    def encode_image_to_latent(self, frames, noise=None, **kw):
        z = frames[:, :, :1].repeat(1, 1, 4, 1, 1)[..., ::8, ::8].contiguous()
        if noise is not None:
            z = z + noise * 0.25
        z = z + 0.125 * (kw.get("seed", 0) % 4) + 0.0625 * (kw.get("unit", 0) % 4)
        _rec("model.encode_image_to_latent", dict(frames=frames, noise=noise, **kw), z)
        return z

    def decode_latent_to_image(self, latent):
        image = latent[:, :, :3].repeat_interleave(8, -1).repeat_interleave(8, -2)
        _rec("model.decode_latent_to_image", dict(latent=latent), image)
        return image


class TraceEstimator:
    def __init__(self, name="estimator"):
        self.name = name

    def __call__(self, a, b):
        flow = (a[:, :2] - b[:, :2]) * 2
        _rec(self.name, dict(a=a, b=b), flow)
        return flow


class TracePipe:
    """``pipe="plain"``; ``"est"`` also has a ``flow_estimator`` of its own."""
    num_ddim_steps = 4

    class scheduler:
        timesteps = [750, 500, 250, 0]

        @staticmethod
        def start_coefficients(t):
            return {250: (0.5, 0.75)}.get(t, (0.25, 0.875))

    def __init__(self, estimator=False):
        self.flow_estimator = TraceEstimator("pipe.flow_estimator") if estimator else None

    @staticmethod
    def _step(kw):
        return kw["latent"] * 0.5 + kw["img_cond"] * 0.25

    def __call__(self, **kw):
        out = {"latent": self._step(kw)}
        _rec("pipe.__call__", kw, out)
        return out

    def second_clip_forward(self, **kw):
        out = {"latent": self._step(kw)}
        _rec("pipe.second_clip_forward", kw, out)
        return out

    def run_stacked(self, calls, **kw):
        outs = [{"latent": self._step(c)} for c in calls]
        _rec("pipe.run_stacked", dict(calls=calls, **kw), outs)
        return outs

    def estimate_mask(self, z, text_cond, text_uncond, cond, **kw):
        latent = (z[:, :, 0] > 0).to(torch.float32)
        out = dict(raw=z[:, :, 0] * 0.5, soft=z[:, :, 0] * 0.25 + 0.5, mask_latent=latent,
                   mask=latent.repeat_interleave(8, -1).repeat_interleave(8, -2))
        _rec("pipe.estimate_mask", dict(z=z, text_cond=text_cond, text_uncond=text_uncond, cond=cond, **kw), out)
        return out


class TraceFlowPipe(TracePipe):
    """``pipe="flow"`` / ``"flow_est"``: the optical-flow pipe, without and with an estimator of its own."""

    def obtain_flow_batched(self, *a, **k):
        raise AssertionError("the drivers do not compute the correction's flows themselves")


def _pipe(kind):
    return {"plain": lambda: TracePipe(), "est": lambda: TracePipe(True), "flow": lambda: TraceFlowPipe(), "flow_est": lambda: TraceFlowPipe(True)}[kind]()


# ------------------------------------------------------------------------------------------------------------------ the ops stand-ins
def _randn(shape, seed, stream, offset=0, raw=False, device=None):
    n = math.prod(shape)
    out = (((torch.arange(n, dtype=torch.int64) * 7 + seed * 3 + stream % 1021) % 64) - 32).to(torch.float32).div(32).reshape(tuple(shape))
    _rec("ops.randn", dict(shape=tuple(shape), seed=seed, stream=stream, device=device), out)
    return out


def _add_noise(z, noise, ka, kb):
    out = ka * z + kb * noise
    _rec("ops.add_noise", dict(z=z, noise=noise, ka=ka, kb=kb), out)
    return out


def _mask_to_latent(mask, mode="max"):
    out = (mask[..., ::8, ::8] if mode == "max" else (mask[..., 3::8, 3::8] + mask[..., 4::8, 4::8]) * 0.5).contiguous()
    _rec("ops.mask_to_latent", dict(mask=mask, mode=mode), out)
    return out


def _composite(edited, original, mask, out=None):
    args = _desc(dict(edited=edited, original=original, mask=mask, out_is_edited=out is edited))
    r = (mask[:, None] * edited + (1 - mask[:, None]) * original).clip(-1, 1)
    out = r if out is None else out.copy_(r)
    TRACE.append({"callee": "ops.composite", "args": args, "result": _desc(out)})
    return out


def _mask_track_step(f_prev, v_prev, b, c, m, *, alpha=0.01, beta=0.5, fill=0.0, out=None):
    F = f_prev + b
    V = v_prev if c is None else v_prev * ((b + c)[:, 0].abs() <= 1.0).to(torch.float32)
    mask = m * V + fill * (1 - V)
    _rec("ops.mask_track_step", dict(f_prev=f_prev, v_prev=v_prev, b=b, c=c, m=m, alpha=alpha, beta=beta, fill=fill), (F, V, mask))
    return F, V, mask


def _mask_shape(mask, *, grow=0.0, feather=0.0, threshold=0.5, profile="smooth"):
    inside = (mask > threshold).to(torch.float32)
    support = inside.clone()
    if grow + feather > 0:   # one pixel to the right, whatever the distance: enough to tell the two masks apart
        support[..., 1:] = torch.maximum(inside[..., 1:], inside[..., :-1])
    shaped = (inside + support) * 0.5
    _rec("ops.mask_shape", dict(mask=mask, grow=grow, feather=feather, threshold=threshold, profile=profile), (shaped, support))
    return shaped, support


def _temporal_filter(edited, guide, flow, valid, offsets, *, sigma=0.1, strength=1.0, guide_affine=(1.0, 0.0), out=None):
    T = edited.shape[0]
    acc = edited * 0.5
    for i, k in enumerate(offsets):
        rows = torch.tensor([min(max(t + k, 0), T - 1) for t in range(T)], dtype=torch.long)
        acc = acc + valid[i][:, None].to(edited.dtype) * edited.index_select(0, rows) * 0.125
    _rec("ops.temporal_filter", dict(edited=edited, guide=guide, flow=flow, valid=valid, offsets=offsets, sigma=sigma, strength=strength,
                                     guide_affine=guide_affine), acc)
    return acc


def _keyframe_fill(source, edited_keys, flow, valid, key_frame, frames, slots, weights, *, sigma=0.1, mode="residual", guide_affine=(1.0, 0.0),
                   out=None, conf=None):
    args = _desc(dict(source=source, edited_keys=edited_keys, flow=flow, valid=valid, key_frame=key_frame, frames=frames, slots=slots,
                      weights=weights, sigma=sigma, mode=mode, guide_affine=guide_affine))
    conf = torch.zeros((len(frames), *source.shape[-2:]), dtype=torch.float32)
    for i, t in enumerate(frames):
        row = source[t] * (0.5 if mode == "residual" else 0.0)
        for s in (0, 1):
            if slots[i][s] >= 0:
                row = row + edited_keys[slots[i][s]] * 0.25
                conf[i] += valid[i, s] * 0.5
        out[t] = row
    TRACE.append({"callee": "ops.keyframe_fill", "args": args, "result": _desc((out, conf))})
    return out, conf


def _torch_randn(*shape, device=None, dtype=None):
    shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape)
    out = _grid(shape, 11, 64, 32)
    _rec("torch.randn", dict(shape=shape, device=str(device), dtype=str(dtype)), out)
    return out


STAND_INS = dict(randn=_randn, add_noise=_add_noise, mask_to_latent=_mask_to_latent, composite=_composite, mask_track_step=_mask_track_step,
                 mask_shape=_mask_shape, temporal_filter=_temporal_filter, keyframe_fill=_keyframe_fill)
assert tuple(STAND_INS) == OPS


def _patch(setattr_):
    from insv2v import ops
    for name, fn in STAND_INS.items():
        setattr_(ops, name, fn)
    setattr_(torch, "randn", _torch_randn)


@pytest.fixture(autouse=True)
def _cpu_ops(monkeypatch):
    _patch(monkeypatch.setattr)


# ------------------------------------------------------------------------------------------------------------------ the inputs
def _grid(shape, mul, mod, div, shift=0):
    n = math.prod(shape)
    return (((torch.arange(n, dtype=torch.int64) * mul + shift) % mod) - mod // 2).to(torch.float32).div(div).reshape(shape)


def _frames(T):
    return _grid((1, T, 3, H, W), 5, 128, 64)


def _flows(T, shift=0):
    return dict(fwd=_grid((T - 1, 2, H, W), 3, 8, 4, shift), bwd=_grid((T - 1, 2, H, W), 5, 8, 4, shift + 1))


def _still():
    m = torch.zeros((1, 1, H, W))
    m[..., 4:12, 6:18] = 1.0
    m[..., 12:14, 6:18] = 0.5
    return m


def _moving(T):
    m = torch.zeros((1, T, H, W))
    for t in range(T):
        m[0, t, 4:12, 2 + t:14 + t] = 1.0
    return m


def _unit(T=9, **kw):
    return dict(frames=_frames(T), text_cond=_grid((1, 77, 8), 3, 32, 16), text_uncond=_grid((1, 77, 8), 3, 32, 16, 5), **kw)


def _latents(T, mul):
    return _grid((1, T, 4, H // 8, W // 8), mul, 32, 16)


EST = "<estimator>"       # stands for a fresh TraceEstimator in a case's options
SHAPE = dict(grow=2.0, feather=3.0)
ALL = dict(keyframes=2, mask=None, mask_key=4, mask_shape=SHAPE, stabilize=dict(radius=1))   # (mask: filled in, a fresh tensor per run)

# name -> (pipe kind, the unit's keywords, the call's keywords); built anew for every run, so that no run sees another's tensors
SINGLE = {
    "plain": lambda: ("plain", _unit(), {}),
    "seeded": lambda: ("plain", _unit(), dict(seed=3, unit=2)),
    "mask_still": lambda: ("plain", _unit(mask=_still()), {}),
    "mask_frames": lambda: ("plain", _unit(mask=_moving(9), mask_mode="mean"), {}),
    "strength_half": lambda: ("plain", _unit(strength=0.5), {}),
    "strength_half_mask": lambda: ("plain", _unit(strength=0.5, mask=_still()), dict(seed=1)),
    "auto": lambda: ("plain", _unit(mask="auto", auto_mask=dict(n_maps=2, dilate=0)), dict(seed=4, unit=1, return_mask=True)),
    "track_flows": lambda: ("plain", _unit(mask=_still(), mask_key=4, mask_flows=_flows(9)), dict(return_mask=True)),
    "track_estimator": lambda: ("plain", _unit(mask=_still(), mask_key=3), dict(flow_estimator=EST)),
    "track_no_occlusion": lambda: ("est", _unit(mask=_still(), mask_key=3, mask_track=dict(occlusion=False)), {}),
    "stabilize_flows": lambda: ("plain", _unit(stabilize=True, stabilize_flows=_flows(9)), {}),
    "stabilize_estimator": lambda: ("est", _unit(stabilize=dict(radius=1, occlusion=False)), {}),
    "stabilize_track_share": lambda: ("plain", _unit(mask=_still(), mask_key=4, stabilize=True), dict(flow_estimator=EST, return_mask=True)),
    "stabilize_track_mask_flows": lambda: ("plain", _unit(mask=_still(), mask_key=4, mask_flows=_flows(9), stabilize=True), {}),
    "shape_drawn": lambda: ("plain", _unit(mask=_still(), mask_shape=SHAPE), dict(return_mask=True)),
    "shape_auto": lambda: ("plain", _unit(mask="auto", mask_shape=SHAPE), dict(return_mask=True)),
    "shape_tracked": lambda: ("plain", _unit(mask=_still(), mask_key=0, mask_flows=_flows(9), mask_shape=dict(grow=-1.0)), dict(return_mask=True)),
    "key_key_flows": lambda: ("plain", _unit(keyframes=2, key_flows=_flows(9), stabilize_flows=_flows(9, 2), stabilize=True), dict(return_mask=True)),
    "key_stabilize_flows": lambda: ("plain", _unit(keyframes=4, stabilize=True, stabilize_flows=_flows(9)), {}),
    "key_mask_flows": lambda: ("plain", _unit(keyframes=2, mask=_still(), mask_key=4, mask_flows=_flows(9)), dict(return_mask=True)),
    "key_estimator": lambda: ("est", _unit(keyframes=dict(stride=4, mode="warp", occlusion=False)), dict(flow_estimator=EST, return_latent=True)),
    "key_pipe_estimator": lambda: ("est", _unit(keyframes=2, mask=_moving(9)), dict(seed=2)),
    "key_all": lambda: ("plain", _unit(**dict(ALL, mask=_still())), dict(seed=6, unit=3, flow_estimator=EST, return_latent=True, return_mask=True)),
    "key_all_stride4": lambda: ("est", _unit(**dict(ALL, mask=_still(), keyframes=4)), dict(return_mask=True)),
    "key_injected": lambda: ("plain", _unit(keyframes=2, key_flows=_flows(9), cond=_latents(9, 3), enc_noise=_latents(9, 7), mask=_still(),
                                            init_noises=[_latents(4, 5), _latents(1, 9)]), dict(seed=9)),
    "injected_noises": lambda: ("plain", _unit(init_noises=[_latents(4, 5), _latents(2, 9), _latents(3, 11)], enc_noise=_latents(9, 7)), dict(seed=9)),
    "injected_cond": lambda: ("plain", _unit(cond=_latents(9, 3), mask=_still(), strength=0.5), dict(return_latent=True)),
    "flow_pipe_given": lambda: ("flow", _unit(flows_per_window=[[_grid((2, 2, H, W), 3, 8, 4, q) for q in range(2)],
                                                                 [_grid((1, 2, H, W), 3, 8, 4, q) for q in range(3)]]), {}),
    "flow_pipe_estimator": lambda: ("flow_est", _unit(), dict(seed=2)),
    "flow_pipe_one_window": lambda: ("flow", _unit(T=4), {}),
    "returns": lambda: ("plain", _unit(mask=_still()), dict(return_latent=True, return_mask=True)),
    "no_source_key": lambda: ("plain", _unit(keyframes=2), {}),
    "no_source_stabilize": lambda: ("plain", _unit(stabilize=True), {}),
    "no_source_track": lambda: ("plain", _unit(mask=_still(), mask_key=4), {}),
    "no_source_flow_pipe": lambda: ("flow", _unit(), {}),
    "one_frame": lambda: ("plain", _unit(T=1, **dict(ALL, mask=_still(), mask_key=0)), dict(return_mask=True)),
    "two_frames": lambda: ("plain", _unit(T=2, **dict(ALL, mask=_still(), mask_key=1)), dict(flow_estimator=EST, return_mask=True)),
    "two_frames_plain": lambda: ("plain", _unit(T=2), {}),
}
RAISES = {"no_source_key": "key_flows=", "no_source_stabilize": "stabilize_flows=", "no_source_track": "mask_flows=", "no_source_flow_pipe": "flows_per_window="}

# name -> (pipe kind, the units, the call's keywords)
STACKED = {
    "videos_one_plain": lambda: ("plain", [_unit()], {}),
    "videos_one": lambda: ("plain", [_unit(mask=_still(), mask_key=4, stabilize=True, text_cfg=5.0)],
                           dict(seed=3, flow_estimator=EST, return_mask=True, max_clips=2)),
    "videos_one_key": lambda: ("est", [_unit(keyframes=2, unit=5)], dict(seed=3, return_latent=True)),
    "multi_plain": lambda: ("plain", [_unit(), _unit(mask=_still(), mask_shape=SHAPE), _unit(mask=_moving(9), video_cfg=1.5)], {}),
    "multi_mixed": lambda: ("plain", [_unit(), _unit(mask=_still(), mask_key=4, stabilize=True, unit=7),
                                      _unit(stabilize=True, stabilize_flows=_flows(9)), _unit(mask="auto")],
                            dict(seed=5, max_clips=2, flow_estimator=EST, return_mask=True)),
    "multi_key": lambda: ("est", [_unit(**dict(ALL, mask=_still())), _unit(T=5, mask=_still()), _unit(keyframes=2, key_flows=_flows(9))],
                          dict(seed=5, return_latent=True, return_mask=True)),
    "multi_partial": lambda: ("plain", [_unit(strength=0.5), _unit(strength=0.5, mask=_still()), _unit(strength=0.5, mask="auto")], dict(max_clips=3)),
    "multi_flow_pipe": lambda: ("flow_est", [_unit(flows_per_window=[[_grid((2, 2, H, W), 3, 8, 4)] * 2, [_grid((1, 2, H, W), 3, 8, 4)] * 3]),
                                             _unit(init_noises=[_latents(4, 5), _latents(2, 9), _latents(3, 11)])], dict(seed=1)),
}
MULTI = tuple(n for n in STACKED if n.startswith("multi_"))


# ------------------------------------------------------------------------------------------------------------------ running a case
def _opts(opts):
    return {k: (TraceEstimator() if v is EST else v) for k, v in opts.items()}


def _traced(fn):
    del TRACE[:]
    try:
        result = _desc(fn())
    except RuntimeError as e:
        result = {"raised": str(e)}
    return {"trace": list(TRACE), "result": result}


def run_video(pipe_kind, u, opts):
    from insv2v.run_loveu_tgve import edit_video
    u = dict(u)
    return _traced(lambda: edit_video(TraceModel(), _pipe(pipe_kind), u.pop("frames"), u.pop("text_cond"), u.pop("text_uncond"),
                                      frames_in_batch=FIB, num_ref_frames=REF, **u, **_opts(opts)))


def run_videos(pipe_kind, units, opts):
    from insv2v.run_loveu_tgve import edit_videos
    return _traced(lambda: edit_videos(TraceModel(), _pipe(pipe_kind), units, FIB, REF, **_opts(opts)))


def _alone(case):
    """The units of a stacked case, each through ``edit_video`` with the id and the options ``edit_videos`` gives it."""
    kind, units, opts = STACKED[case]()
    opts = {k: v for k, v in opts.items() if k in ("seed", "flow_estimator")}
    return [run_video(kind, {k: v for k, v in u.items() if k != "unit"}, dict(opts, unit=u.get("unit", j), return_latent=True, return_mask=True))
            for j, u in enumerate(units)]


PIPE_CALLS = ("pipe.__call__", "pipe.second_clip_forward", "pipe.run_stacked")
WINDOW_OPS = ("ops.randn", "torch.randn", "ops.add_noise")


def _cut(trace):
    segments = [[]]
    for r in trace:
        if r["callee"] in PIPE_CALLS:
            segments.append([])
        else:
            segments[-1].append(r)
    first = segments[0]
    n = next((i for i in range(len(first), 0, -1) if first[i - 1]["callee"] not in WINDOW_OPS), 0)
    return [first[:n], first[n:]] + segments[1:]   # the preparation, window 0, the later windows, the finish


def merged(case, stacked_trace):
    """None if the stacked trace, outside its pipe calls, is its units' own traces merged by phase - else what differs."""
    got, alone = _cut(stacked_trace), [_cut(r["trace"]) for r in _alone(case)]
    if {len(a) for a in alone} != {len(got)}:
        return f"{len(got) - 2} stacked pipe calls, but the units alone make {[len(a) - 2 for a in alone]}"
    for i, seg in enumerate(got):
        want = [r for a in alone for r in a[i]]
        if seg != want:
            return f"phase {i}: stacked {[r['callee'] for r in seg]} != alone, in unit order {[r['callee'] for r in want]}"
    return None


def _compare(case, got, want):
    """Record for record; the first record that differs is shown in full."""
    short = _short(got)
    for i, (g, w) in enumerate(zip(short, want)):
        assert g == w, f"{case}: record {i} is {json.dumps(got[i], sort_keys=True)}, recorded {w}"
    assert [c for c, _ in short] == [c for c, _ in want], f"{case}: the trace has {len(short)} records, recorded {len(want)}"


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", sorted(SINGLE))
def test_edit_video_reproduces_its_recorded_trace(case, recorded):
    run = run_video(*SINGLE[case]())
    _compare(case, run["trace"], recorded[case]["trace"])
    assert run["result"] == recorded[case]["result"]
    if case in RAISES:   # before the pipe is called at all
        assert RAISES[case] in run["result"]["raised"] and not [r for r in run["trace"] if r["callee"].startswith("pipe.")]
    else:
        assert "raised" not in json.dumps(run["result"])


@pytest.mark.parametrize("case", sorted(set(STACKED) - set(MULTI)))
def test_edit_videos_of_one_unit_reproduces_its_recorded_trace(case, recorded):
    run = run_videos(*STACKED[case]())
    _compare(case, run["trace"], recorded[case]["trace"])
    assert run["result"] == recorded[case]["result"]
    assert not [r for r in run["trace"] if r["callee"] == "pipe.run_stacked"]   # the shortcut into edit_video


@pytest.mark.parametrize("case", MULTI)
def test_edit_videos_reproduces_its_recorded_pipe_calls_and_results(case, recorded):
    run = run_videos(*STACKED[case]())
    _compare(case, [r for r in run["trace"] if r["callee"] in PIPE_CALLS], recorded[case]["pipe"])
    assert run["result"] == recorded[case]["result"]
    kw = STACKED[case]()[2]
    for r in run["trace"]:
        if r["callee"] == "pipe.run_stacked":   # max_clips is passed on only when the caller gave it
            assert ("max_clips" in r["args"]) == ("max_clips" in kw) and set(r["args"]) <= {"calls", "max_clips"}


@pytest.mark.parametrize("case", MULTI)
def test_edit_videos_is_its_units_edit_video_traces_merged_by_phase(case):
    assert merged(case, run_videos(*STACKED[case]())["trace"]) is None


@pytest.mark.parametrize("case", MULTI)
def test_every_unit_of_edit_videos_gets_the_result_of_edit_video(case):
    """The stand-in pipe treats a stacked call like a single one, so the results must agree too."""
    kind, units, opts = STACKED[case]()
    run = run_videos(kind, units, dict(opts, return_latent=True, return_mask=True))
    assert run["result"] == [r["result"] for r in _alone(case)]


def _write():
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "instruct-video-to-video_amd")]
    _patch(setattr)
    out = {}
    for case in sorted(SINGLE):
        run = run_video(*SINGLE[case]())
        out[case] = {"trace": _short(run["trace"]), "result": run["result"]}
    for case in sorted(STACKED):
        run = run_videos(*STACKED[case]())
        if case in MULTI:
            out[case] = {"pipe": _short([r for r in run["trace"] if r["callee"] in PIPE_CALLS]), "result": run["result"]}
            print(f"{case}: merged by phase: {merged(case, run['trace']) or 'yes'}")
        else:
            out[case] = {"trace": _short(run["trace"]), "result": run["result"]}
    for case, r in out.items():
        print(f"{case}: {len(r.get('trace', r.get('pipe')))} records, result {json.dumps(r['result'])[:100]}")
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        raise SystemExit("usage: python tests/test_driver_trace_cpu.py --write   (only before a change of the drivers; the tests read the file)")
    _write()
