"""Sampling pipelines: drop-in for pl_trainer/inference/inference.py (same class names, constructor
and call signatures, same returned dict keys).

  Inference.__init__                                   inference.py:26-51
  InferenceIP2PVideo.__call__                          inference.py:162-218
  InferenceIP2PVideo.second_clip_forward               inference.py:220-289
  InferenceIP2PVideoOpticalFlow.second_clip_forward    inference.py:313-398

Per DDIM step the host issues: one input-assembly kernel, one hipGraph replay of the whole UNet
forward (the 3 CFG branches run as three concurrent kernel chains on three HIP streams captured in
ONE graph, so their latency-bound kernels overlap and fill each other's tails: +10 % over batching
them in every launch; text K/V hoisted out of the loop), and one fused CFG-combine +
noise-correction + scheduler-step kernel.  Latents stay fp32 in the reference
layout [1,F,4,h,w]; there is no host<->device traffic inside the loop.
"""
import os
import weakref

import torch

from . import ops
from .fused import check_operand_windows
from .rng import stream_id, STEP, MASK, WINDOW_BITS, STEP_BITS
from .schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, strength_to_start
from .flow_utils import resize_flow


class GraphedUNet:
    """One captured hipGraph of UNet3DConditionModel.forward_cl for fixed (B,F,H,W,ctx_len).

    Static inputs: x_in (channels-last fp16), t (device fp32), per-layer text K/V; static output eps.
    """

    def __init__(self, unet, B, F, H, W, ctx_len, use_graph=True, branch_streams=False, cfg_clips=0):
        dev = unet.device
        self.branch_streams = branch_streams and B > 1
        # cfg_clips = n: the B = 3 n samples are the CFG branches of n clips, BRANCH-major, with the inputs of branches 1 and 2 identical
        # (what build_unet_input writes): UNet3DConditionModel.forward_cl computes their common prefix once
        self.cfg_clips = cfg_clips if (cfg_clips > 0 and B == 3 * cfg_clips and not self.branch_streams) else 0
        self._streams = None
        # weak: the process-wide graph cache (shared_runner) must not keep a UNet - 2.5 GB of weights - alive
        try:
            self._unet = weakref.ref(unet)
        except TypeError:
            self._unet = lambda u=unet: u
        self.key = (B, F, H, W, ctx_len)
        self.x_in = torch.zeros((B * F * H * W, unet.in_pad), device=dev, dtype=torch.float16)
        self.t = torch.zeros((B,), device=dev, dtype=torch.float32)
        self.kvs = None   # per-layer text K/V (tensor, or (K/V, fragment streams) where the fused cross-attention runs): set_context
        self.use_graph = use_graph
        self.graph = None
        self.eps = None
        self.start = 0
        # split-K scratch owned by this runner (one per concurrently running branch), allocated outside any capture
        self._ws = [ops.new_workspace(dev) for _ in range(B if self.branch_streams else 1)]

    @property
    def unet(self):
        u = self._unet()
        if u is None:
            raise RuntimeError("GraphedUNet: its UNet has been garbage collected")
        return u

    def set_context(self, ctx):
        kvs, L = self.unet.project_context(ctx)
        assert L == self.key[4] and ctx.shape[0] == self.key[0]
        if self.kvs is None:   # static buffers of the captured graph, shaped like the first projection
            self.kvs = [tuple(torch.zeros_like(t) for t in kv) if isinstance(kv, tuple) else torch.zeros_like(kv) for kv in kvs]
        for dst, src in zip(self.kvs, kvs):
            for d, s_ in zip(dst, src) if isinstance(dst, tuple) else ((dst, src),):
                d.copy_(s_)

    def _forward(self):
        B, F, H, W, L = self.key
        if not self.branch_streams:
            with ops.workspace(self._ws[0]):
                return self.unet.forward_cl(self.x_in, self.t, self.kvs, L, B, F, H, W, start=self.start, cfg_clips=self.cfg_clips)
        # one HIP stream per CFG branch: the branches are independent, so their (latency-bound) kernels
        # overlap and fill each other's tails; fork/join is captured into the same hipGraph.
        if self._streams is None:
            self._streams = [torch.cuda.Stream() for _ in range(B)]
        main = torch.cuda.current_stream()
        rows = F * H * W
        outs = [None] * B
        for b, st in enumerate(self._streams):
            st.wait_stream(main)
            with torch.cuda.stream(st), ops.workspace(self._ws[b]):
                kvs = [(kv[0][b * L:(b + 1) * L], kv[1][b:b + 1]) if isinstance(kv, tuple) else kv[b * L:(b + 1) * L] for kv in self.kvs]
                outs[b] = self.unet.forward_cl(self.x_in[b * rows:(b + 1) * rows], self.t[b:b + 1], kvs, L, 1, F, H, W,
                                               start=self.start)
        for st in self._streams:
            main.wait_stream(st)
        return torch.cat(outs, 0)

    def run(self):
        """eps [B*F*H*W, 4] fp32 for the current contents of x_in / t / kvs."""
        if not self.use_graph:
            return self._forward()
        if self.graph is None:
            # warm-up on a side stream (sets lazy kernel attributes, primes the allocator), then capture
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                self._forward()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self.eps = self._forward()
            self.graph = g
        self.graph.replay()
        return self.eps


class Inference:
    def __init__(self, unet, scheduler="ddim", beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear",
                 num_ddim_steps=20, guidance_scale=5, use_graph=True, branch_streams=True, solver_order=2):
        """``scheduler``: "ddim" / "ddpm" (the reference's two), or "dpmsolver++" / "sde-dpmsolver++": DPM-Solver++ multistep of order
        ``solver_order`` (1 or 2; ignored by the other two) on DDIM's time grid - schedulers.DPMSolverMultistepScheduler."""
        self.unet = unet
        if scheduler == "ddim":
            cls, kw = DDIMScheduler, {"set_alpha_to_one": False, "steps_offset": 1, "clip_sample": False}
        elif scheduler == "ddpm":
            cls, kw = DDPMScheduler, {"clip_sample": False}
        elif scheduler in ("dpmsolver++", "sde-dpmsolver++"):
            cls, kw = DPMSolverMultistepScheduler, {"solver_order": solver_order, "algorithm_type": scheduler, "lower_order_final": True,
                                                    "steps_offset": 1}
        else:
            raise NotImplementedError()
        self.scheduler = cls(beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule, **kw)
        self.scheduler.set_timesteps(num_ddim_steps)
        self.num_ddim_steps = num_ddim_steps
        self.guidance_scale = guidance_scale
        self.use_graph = use_graph
        self.branch_streams = branch_streams
        self.variance_noises = None  # optional injected DDPM noises, one [1,F,4,h,w] tensor (or None) per step

    def _runner(self, B, F, H, W, L, slot=0):
        return shared_runner(self.unet, B, F, H, W, L, slot, self.use_graph, self.branch_streams)


# Threading: ONE host thread drives the pipelines of a process (like the reference): runners share static input / output
# buffers, and ops._WS_OVERRIDE (the split-K scratch selection) is a plain module global.
# Captured UNet graphs are shared process-wide, keyed by (UNet object, its weights version, shape, slot, mode): pipe
# objects are cheap and short-lived (one per clip / scheduler setting in the drivers and tests), the captured hipGraph of a
# full-size 3-stream forward is not - and capturing the same shape again right after destroying a graph crashed inside
# hipGraphLaunch on ROCm 7.2 (first replay of the new graph; reproducible with tests/test_full_size_gpu.py followed by
# tests/test_model_gpu.py, also on the round-1 code).  Entries die with their UNet or when its weights are reloaded:
# a captured graph holds the OLD weight pointers.
_RUNNERS = {}
_FINALIZERS = {}
_DEAD = set()   # UNets collected while a stream capture was in progress: their runners are purged at the next shared_runner() call


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


# hipGraphLaunch of a NEW graph segfaults on ROCm 7.2 once a captured graph of this process has been destroyed and the same shape is
# captured again (tests/test_model_gpu.py followed by tests/test_full_size_gpu.py: crash with destruction at collection time, at the next
# shared_runner() call, and with an empty_cache() in between; no crash when the dead graphs are merely parked - gpurun_out of round 3,
# tools/r03_run18.sh).  Retired graphs are therefore PARKED here, never destroyed (their static buffers and split-K scratch go with the
# runner; the graph's private activation pool - a few GB for a 3-branch full-size forward - stays until the process ends or
# release_dead_graphs() is called).  INSV2V_GRAPH_PURGE=destroy restores immediate destruction.
_GRAVEYARD = []
_PURGE_MODE = os.environ.get("INSV2V_GRAPH_PURGE", "keep")   # keep | destroy
# The park is bounded: beyond INSV2V_GRAPH_PARK_MAX graphs the OLDEST is destroyed behind a device synchronize.  A process that
# keeps ONE UNet never parks anything but the graphs of reloaded weights / retired stack sizes; the bound only bites in processes that
# build many models (test suites), where the oldest graphs belong to models collected long ago.
_PARK_MAX = int(os.environ.get("INSV2V_GRAPH_PARK_MAX", "32"))


def parked_graphs():
    """Number of retired hipGraphs currently parked (each holds its private activation pool)."""
    return len(_GRAVEYARD)


def _park(graph):
    _GRAVEYARD.append(graph)
    if len(_GRAVEYARD) > _PARK_MAX:
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        while len(_GRAVEYARD) > _PARK_MAX:
            _GRAVEYARD.pop(0)


def release_dead_graphs():
    """Destroy the parked graphs of retired runners (frees their activation pools).  Safe when no further graph will be captured in
    this process, or on a ROCm without the hipGraphLaunch crash described above."""
    if _GRAVEYARD and torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()
    _GRAVEYARD.clear()


def _purge_runners(uid, keep_version=None):
    dead = [k for k in _RUNNERS if k[0] == uid and k[1] != keep_version]
    if dead:
        gpu = torch.cuda.is_available() and torch.cuda.is_initialized()
        if gpu:
            torch.cuda.synchronize()  # never destroy a graph that may still be executing
        for k in dead:
            r = _RUNNERS.pop(k)
            if _PURGE_MODE == "keep" and getattr(r, "graph", None) is not None:
                _park(r.graph)
            del r


def _unet_collected(uid):
    """weakref.finalize callback of a UNet.  Its graphs are destroyed right away - EXCEPT when the collector happens to run inside a
    stream capture, where the device synchronize of _purge_runners is illegal: then the id is parked in _DEAD for the next
    shared_runner() call.  (Destroying them only there as a rule - i.e. immediately before the next capture of the same shapes - ran
    into the hipGraphLaunch crash described above: tests/test_model_gpu.py followed by tests/test_full_size_gpu.py.)"""
    _FINALIZERS.pop(uid, None)
    if _capturing():
        _DEAD.add(uid)
    else:
        _purge_runners(uid)


def shared_runner(unet, B, F, H, W, L, slot=0, use_graph=True, branch_streams=True, cfg_clips=0):
    """Process-wide runner of (unet, shape, slot).  One host thread drives a process's pipes (the runners' static buffers, ops' workspace
    override and this cache are plain module state)."""
    uid, ver = id(unet), getattr(unet, "weights_version", 0)
    while _DEAD:   # (an id can be reused by a NEW UNet: stale entries go first, so it never sees another model's graphs)
        _purge_runners(_DEAD.pop())
    if uid not in _FINALIZERS:
        try:
            fin = weakref.finalize(unet, _unet_collected, uid)
            fin.atexit = False  # at interpreter exit the HIP runtime may already be gone
            _FINALIZERS[uid] = fin
        except TypeError:  # not weak-referenceable (test doubles): entries live as long as the process
            _FINALIZERS[uid] = None
    _purge_runners(uid, keep_version=ver)
    key = (uid, ver, B, F, H, W, L, slot, bool(use_graph), bool(branch_streams), int(cfg_clips))
    r = _RUNNERS.get(key)
    if r is None:
        r = _RUNNERS[key] = GraphedUNet(unet, B, F, H, W, L, use_graph, branch_streams, cfg_clips)
    return r


MAX_CLIPS_IN_FLIGHT = int(os.environ.get("INSV2V_MAX_CLIPS", "20"))


def max_clips_in_flight(frames=16, h=32, w=48):
    """Clips that are stacked into one launch chain BY DEFAULT: at most 20 (5 -> 10 clips gave +1.4 %, 10 -> 20 fills the last round of the
    level-0 tile grids - 22.5 -> 23 rounds instead of 11.25 -> 12 - and halves the launches per clip: +0.9 %, profiles/r04_clips20.txt), and few enough that every
    [3 * clips * F * h * w, 640] fp16 tensor would fit ONE 2 GiB buffer descriptor: 20 for C2 (B = 60, 1.89 GB), 9 at 360 x 640, 7 for C5.
    The window term is a default, not a kernel requirement: no kernel addresses a whole operand through one descriptor any more
    (insv2v_rowlin and insv2v_attention rebase theirs; insv2v_gemm and the launchers of the fused row kernels run a problem beyond the
    window as row / image / tile / sample ranges: DESIGN.md section 12), so ``run_stacked(calls, max_clips=N)`` may stack more.  What
    cannot run at all is refused up front by ``fused.check_operand_windows``."""
    return max(1, min(MAX_CLIPS_IN_FLIGHT, (2 ** 31 - 2 ** 20) // (3 * frames * h * w * 640 * 2)))


def stack_groups(n, cap):
    """Sizes of the launch chains ``run_stacked`` runs n clips as under a cap of `cap` clips per chain: as few chains as the cap allows,
    as even as possible (every distinct stack size captures its own graph), the larger ones first."""
    n, cap = int(n), int(cap)
    if cap < 1:
        raise ValueError(f"a stack holds at least one clip, not {cap}")
    if n <= cap:
        return [n] if n > 0 else []
    ng = -(-n // cap)
    return [n // ng + (1 if g < n % ng else 0) for g in range(ng)]


def _unet_channels(unet):
    """block_out_channels of a UNet3DConditionModel (test doubles without a config: the full-width default)."""
    cfg = getattr(unet, "cfg", None)
    return tuple(cfg["ch"]) if isinstance(cfg, dict) and "ch" in cfg else (320, 640, 1280, 1280)


def _rng_of(kw):
    """(seed, unit, window) of a call's kwargs, or None without a seed."""
    if kw.get("seed") is None:
        return None
    return (kw["seed"], kw.get("unit", 0), kw.get("window", 0))


def check_known_region(latent, mask=None, source_latent=None, known_noise=None, release=None):
    """Host-side check of a call's masked-edit arguments (no launch): ``mask`` [1,F,h,w] at latent resolution, ``source_latent`` and
    ``known_noise`` [1,F,4,h,w] like ``latent``; a mask needs both of the others, and they mean nothing without one.  ``release`` (an
    int32 [1,F,h,w] release map) is a known region too, with or without a mask: it needs both of the others."""
    if mask is None and release is None:
        if source_latent is not None or known_noise is not None:
            raise ValueError("source_latent / known_noise are the known region of a masked edit: pass mask= (or release=) with them")
        return
    if source_latent is None or known_noise is None:
        raise ValueError(("a mask needs" if release is None else "a release map needs") +
                         " source_latent= (the scaled source latent) and known_noise= (the window's initial noise)")
    b, F, _, h, w = latent.shape
    if release is not None:
        if not torch.is_tensor(release) or tuple(release.shape) != (b, F, h, w):
            raise ValueError(f"release {tuple(getattr(release, 'shape', ()))} must be [{b},{F},{h},{w}]: one release step per latent cell of latent {tuple(latent.shape)}")
        if release.dtype != torch.int32:
            raise ValueError(f"release must be an int32 tensor (ops.strength_release's), not {release.dtype}")
    if mask is not None and (not torch.is_tensor(mask) or tuple(mask.shape) != (b, F, h, w)):
        raise ValueError(f"mask {tuple(getattr(mask, 'shape', ()))} must be [{b},{F},{h},{w}]: one latent-resolution plane per frame of latent {tuple(latent.shape)}")
    for name, t in (("source_latent", source_latent), ("known_noise", known_noise)):
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(latent.shape):
            raise ValueError(f"{name} {tuple(getattr(t, 'shape', ()))} must be shaped like the latent {tuple(latent.shape)}")


_KNOWN_KEYS = ("mask", "source_latent", "known_noise", "release")


def _known_of(kw):
    """The ``known=`` tuple of a call's kwargs (``_KNOWN_KEYS``' order), or None for a call without a known region: a mask or a release map."""
    return tuple(kw.get(k) for k in _KNOWN_KEYS) if kw.get("mask") is not None or kw.get("release") is not None else None

# ---- a mask estimated from the prompt -------------------------------------------------------------------------
# Starting values, not findings: nobody has tuned them on a real checkpoint.
AUTO_MASK_DEFAULTS = dict(n_maps=4, mask_strength=0.5, clamp_ratio=3.0, threshold=0.5, smooth=True, dilate=1)


def check_automask_args(n_maps=4, mask_strength=0.5, clamp_ratio=3.0, threshold=0.5, smooth=True, dilate=1, frames_in_batch=16):
    """Host-side check of ``estimate_mask``'s parameters (nothing is launched): ValueError naming the parameter."""
    def integer(v, name):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"estimate_mask: {name} must be an integer, got {v!r}")
        return v
    if not 1 <= integer(n_maps, "n_maps") < (1 << STEP_BITS):
        raise ValueError(f"estimate_mask: n_maps = {n_maps} outside [1, 2^{STEP_BITS}) (the draw index of the MASK stream)")
    try:
        strength_to_start(mask_strength, 1)
    except (TypeError, ValueError):
        raise ValueError(f"estimate_mask: mask_strength must be in (0, 1], not {mask_strength!r}") from None
    for name, v, ok in (("clamp_ratio", clamp_ratio, lambda x: x > 0.0 and x != float("inf")), ("threshold", threshold, lambda x: 0.0 < x < 1.0)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(float(v)):   # (NaN fails every comparison)
            raise ValueError(f"estimate_mask: {name} must be " + ("a positive number" if name == "clamp_ratio" else "inside (0, 1)") + f", not {v!r}")
    if integer(dilate, "dilate") < 0:
        raise ValueError(f"estimate_mask: dilate = {dilate} must not be negative")
    if not isinstance(smooth, bool):
        raise ValueError(f"estimate_mask: smooth must be True or False, not {smooth!r}")
    if integer(frames_in_batch, "frames_in_batch") < 1:
        raise ValueError(f"estimate_mask: frames_in_batch = {frames_in_batch} must be positive")


def mask_plan(T, frames_in_batch, n_maps, cap):
    """The UNet launches of one mask estimate, in order: ``(chunk, start, frames, draw0, clips)`` - chunk ``chunk`` = frames
    [start, start + frames) of the video (consecutive chunks of ``frames_in_batch`` frames, no overlap, the last one whatever remains)
    runs its draws [draw0, draw0 + clips) as the clips of one stacked launch; a chunk's ``n_maps`` draws are grouped by
    ``stack_groups(n_maps, cap)``.  Pure arithmetic."""
    T, fib, n_maps = int(T), int(frames_in_batch), int(n_maps)
    if T < 1 or fib < 1 or n_maps < 1:
        raise ValueError(f"mask_plan: {T} frames in chunks of {fib} with {n_maps} draws is not a plan")
    groups = stack_groups(n_maps, cap)
    plan = []
    for k, start in enumerate(range(0, T, fib)):
        d0 = 0
        for m in groups:
            plan.append((k, start, min(fib, T - start), d0, m))
            d0 += m
    return plan


class InferenceIP2PVideo(Inference):
    def zeros(self, x):
        return torch.zeros_like(x)

    def _known_tensors(self, latent, mask=None, source_latent=None, known_noise=None, release=None):
        """The known region of ONE clip on the device - dict(mask [F,h,w], src [F,4,h,w], noise [F,4,h,w]), with a release map also
        release (int32 [F,h,w]; mask may then be None) - or None without a mask and a release map.  The public entry points have checked
        it (``check_known_region``)."""
        if mask is None and release is None:
            return None
        to = lambda t: t[0].to(device=self.unet.device, dtype=torch.float32).contiguous()
        known = dict(mask=None if mask is None else to(mask), src=to(source_latent), noise=to(known_noise))
        if release is not None:
            known["release"] = release[0].to(device=self.unet.device, dtype=torch.int32).contiguous()
        return known

    # ---- shared loop ------------------------------------------------------------------------------
    def _clip_tensors(self, latent, img_cond):
        dev = self.unet.device
        if latent.shape[0] != 1:
            raise ValueError("internal: one clip per entry (a batch is split into clips by the callers)")
        lat = latent[0].to(device=dev, dtype=torch.float32).contiguous()
        cond = img_cond[0].to(device=dev, dtype=torch.float32).contiguous()
        if lat.shape != cond.shape or lat.shape[1] != 4:
            raise ValueError(f"latent {tuple(latent.shape)} and img_cond {tuple(img_cond.shape)} must both be [1,F,4,h,w]")
        return lat, cond

    def _latent_flows(self, flows, n_query, h, w):
        """Image-resolution flows (one [R,2,H,W] per query frame) -> [n_query,R,2,h,w] at latent resolution, resized ONCE per window
        (the reference repeats this loop-invariant resize every corrected step, inference.py:374-378)."""
        if len(flows) != n_query:
            raise ValueError("need one [R,2,H,W] flow per query frame")
        dev = self.unet.device
        return torch.stack([resize_flow(f.to(device=dev, dtype=torch.float32), (h, w)) for f in flows], 0).contiguous()

    def _prep(self, latent, text_cond, text_uncond, img_cond, slot=0):
        lat, cond = self._clip_tensors(latent, img_cond)
        ctx = torch.cat([text_uncond, text_uncond, text_cond], dim=0)
        F, _, h, w = lat.shape
        check_operand_windows(3, F, h, w, _unet_channels(self.unet), ctx.shape[1])   # a frame that cannot run is refused before the first launch
        runner = self._runner(3, F, h, w, ctx.shape[1], slot)
        runner.set_context(ctx)
        return lat, cond, runner

    def _loop(self, *args, **kwargs):
        gen = self._loop_gen(*args, **kwargs)
        try:
            while True:
                next(gen)
        except StopIteration as done:
            return done.value

    def _loop_gen(self, latent, text_cond, text_uncond, img_cond, text_cfg, img_cfg, start_time, guidance_rescale,
                  latent_ref=None, noise_correct_step=0.0, flows=None, slot=0, rng=None, known=None):
        """One sampling loop as a generator that yields after enqueueing each step's (asynchronous) GPU work,
        so several independent clips can be interleaved from one host thread (``run_concurrent``).
        ``rng`` = (seed, unit, window) or None: where a stochastic scheduler's variance noise comes from (``_finish_step``).
        ``known`` = (mask, source_latent, known_noise, release) or None: the known region of a masked edit (``_finish_step``)."""
        known = self._known_tensors(latent, *known) if known is not None else None
        lat, cond, runner = self._prep(latent, text_cond, text_uncond, img_cond, slot)
        dev = lat.device
        F, _, h, w = lat.shape
        ref = None
        if latent_ref is not None:
            ref = latent_ref[0].to(device=dev, dtype=torch.float32).contiguous()
        stats = torch.empty(2, device=dev, dtype=torch.float32) if guidance_rescale > 0 else None
        all_latent, all_pred = [], []
        hist = t_last = None   # a multistep scheduler's history: the previous executed step's x0 prediction (kept in all_pred) and timestep
        for i, t in enumerate(self.scheduler.timesteps[start_time:]):
            t = int(t)
            ops.build_unet_input(lat, cond, runner.x_in, runner.t, t, 3)
            eps = runner.run()
            lat, pred = self._finish_step(i, t, eps, lat, text_cfg, img_cfg, guidance_rescale, stats, ref, noise_correct_step, flows, rng=rng,
                                          hist=hist, t_last=t_last, known=known, start_time=start_time)
            hist, t_last = pred, t
            all_latent.append(lat[None])
            all_pred.append(pred[None])
            yield i
        return {"latent": lat[None], "all_latent": all_latent, "all_pred": all_pred}

    def _finish_step(self, i, t, eps, lat, text_cfg, img_cfg, guidance_rescale, stats, ref, noise_correct_step, flows, noise=None, bstride=0,
                     rng=None, hist=None, t_last=None, known=None, start_time=0):
        """Everything of one sampling step behind the UNet for ONE clip: CFG combine (+ rescale), noise correction, scheduler
        step (inference.py:197-213, 270-277, 367-386).  eps: the clip's three branch predictions [3*F*h*w, 4] fp32, or (bstride > 0,
        the branch-major stack) a view that starts at its first branch with bstride fp32 elements between the branches.
        Variance noise of a stochastic scheduler, in order of precedence: an injected tensor (``noise`` / ``variance_noises[i]``), the
        seeded stream of ``rng`` = (seed, unit, window) - generated inside the step kernel, no tensor -, a ``torch.randn`` draw.
        ``hist`` / ``t_last``: the clip's x0 prediction (from the CORRECTED eps, this function's second result) and timestep of the previous
        executed step, None on the first: what a multistep scheduler (DPM-Solver++ 2M) builds its second-order term from.
        ``known`` (``_known_tensors``): a masked edit - inside the step kernel the new latent becomes
        ``mask * prev + (1 - mask) * (k_src * src + k_noise * noise)`` with the scheduler's ``known_coefficients(t)``; the x0 prediction
        stays the model's own.  None: the launches of an unmasked call, unchanged.  With a release map in ``known`` the step kernel also
        gets ``step = start_time + i``, the step's GLOBAL index in ``scheduler.timesteps`` (``i`` counts the executed steps of a partial
        edit, a release map counts all of them): a cell stays held until ``release <= step``."""
        dev = lat.device
        F, _, h, w = lat.shape
        if stats is not None:
            ops.cfg_stats(eps, stats, F, h, w, text_cfg, img_cfg, branch_stride=bstride)
        ms = {}
        if getattr(self.scheduler, "multistep", False):
            co = self.scheduler.coefficients(t, t_last if hist is not None else None)
            if co["c_hist"] != 0.0:   # (order 1 - the first executed step, the lower-order final step - is the plain step kernel)
                ms = dict(x0_hist=hist, c_hist=co["c_hist"])
        else:
            co = self.scheduler.coefficients(t)
        seeded = {}
        if self.scheduler.stochastic and co["coef"][3] != 0.0:
            if noise is None:
                inj = self.variance_noises[i] if self.variance_noises is not None else None
                if inj is not None:
                    noise = inj[0].to(device=dev, dtype=torch.float32).contiguous()
                elif rng is not None:
                    # This runs OUTSIDE the captured UNet graph, so the step index is a host integer packed into the stream id.  Should
                    # the step kernel ever move inside a capture, the index has to come from device memory: a captured launch replays
                    # the arguments it was captured with.
                    seeded = dict(noise_seed=rng[0], noise_stream=stream_id(STEP, rng[1], rng[2], i))
                else:
                    noise = torch.randn(lat.shape, device=dev, dtype=torch.float32)
        else:
            noise = None
        if known is not None:
            k_src, k_noise = self.scheduler.known_coefficients(t)
            ms = dict(ms, mask=known["mask"], src=known["src"], known_noise=known["noise"], k_src=k_src, k_noise=k_noise)
            if known.get("release") is not None:
                ms.update(release=known["release"], step=start_time + i)
        new_lat, pred = torch.empty_like(lat), torch.empty_like(lat)
        correct = ref is not None and noise_correct_step * self.num_ddim_steps > i
        common = dict(text_cfg=text_cfg, img_cfg=img_cfg, sqrt_a=co["sqrt_a"], sqrt_1ma=co["sqrt_1ma"],
                      rescale_stats=stats, guidance_rescale=guidance_rescale, branch_stride=bstride)
        if correct and flows is not None:
            # combine -> flow-warped correction of the query frames -> step (inference.py:367-386)
            eps_cfg = torch.empty_like(lat)
            ops.cfg_step(eps, lat, nbranch=3, eps_out=eps_cfg, **common)
            dq = ops.flow_correction(eps_cfg, lat, ref, flows, co["sqrt_a"], co["sqrt_1ma"])
            ops.cfg_step(eps_cfg, lat, nbranch=0, coef=co["coef"], latent_out=new_lat, pred_x0=pred, latent_ref=ref,
                         correct=2, delta_q=dq, noise=noise, sqrt_a=co["sqrt_a"], sqrt_1ma=co["sqrt_1ma"], **seeded, **ms)
        else:
            ops.cfg_step(eps, lat, nbranch=3, coef=co["coef"], latent_out=new_lat, pred_x0=pred,
                         latent_ref=ref if correct else None, correct=1 if correct else 0, noise=noise, **seeded, **ms, **common)
        return new_lat, pred

    @torch.no_grad()
    def run_stacked(self, calls, max_clips=None):
        """Run several independent ``__call__`` / ``second_clip_forward`` invocations (list of kwargs dicts as for
        ``run_concurrent``) as ONE batch: the 3 CFG branches of all n clips are stacked into every UNet launch
        (B = 3n; statistics stay per sample), so weights are read once per group of clips, every launch fills the chip
        and the lowest UNet levels need no split-K.  All clips must share shapes, ``start_time`` and the scheduler;
        guidance scales may differ; each clip may or may not carry a known region (``mask`` / ``source_latent`` / ``known_noise``, as for
        ``__call__``).  A call's ``seed`` / ``unit`` / ``window`` select its seeded noise streams as in ``__call__``: a unit's
        result then does not depend on what it is stacked with.  Also the path of a batched ``__call__`` (inference.py:183-187 works for any b).
        (Round 4 measured two stacks of 5 clips running concurrently on two HIP streams against one stack of 10: 14.02 vs 14.50 frames/s -
        the persistent kernels own every CU, a second chain only fills tails and pays for it with half-sized launches.)
        ``max_clips``: clips per launch chain.  None (default): ``max_clips_in_flight`` of the clips' shape; an integer replaces that cap -
        any stack that fits in memory runs (``stack_groups`` gives the chains; a geometry no kernel can address raises ValueError before
        anything is launched, ``fused.check_operand_windows``)."""
        n = len(calls)
        if n == 0:
            return []
        for kw in calls:   # a malformed known region is refused before the first launch of the first chain
            check_known_region(kw["latent"], *(kw.get(k) for k in _KNOWN_KEYS))
        gen = self._stacked_gen(calls, 0, max_clips)
        while True:
            try:
                next(gen)
            except StopIteration as done:
                return done.value

    def _stacked_gen(self, calls, slot, max_clips=None):
        """Generator behind run_stacked: yields after every DDIM step (so several stacks can be interleaved), returns the result dicts."""
        n = len(calls)
        # no more clips per launch chain than the cap - by default max_clips_in_flight, or the caller's max_clips: larger
        # stacks run as several, as even as possible (stack_groups)
        Fc, hc, wc = calls[0]["latent"].shape[1], calls[0]["latent"].shape[-2], calls[0]["latent"].shape[-1]
        cap = max_clips_in_flight(Fc, hc, wc) if max_clips is None else int(max_clips)
        groups = stack_groups(n, cap)
        for m in set(groups):   # every chain's geometry is checked before the first one is launched
            check_operand_windows(3 * m, Fc, hc, wc, _unet_channels(self.unet), calls[0]["text_cond"].shape[1])
        if len(groups) > 1:
            out, k = [], 0
            for m in groups:
                out += yield from self._stacked_gen(calls[k:k + m], slot, m)
                k += m
            return out
        dev = self.unet.device
        st0 = calls[0].get("start_time", 0)
        clips = []
        for kw in calls:
            if kw.get("start_time", 0) != st0:
                raise ValueError("run_stacked: all clips must share start_time")
            lat, cond = self._clip_tensors(kw["latent"], kw["img_cond"])
            if clips and lat.shape != clips[0]["lat"].shape:
                raise ValueError("run_stacked: all clips must have the same [F,4,h,w]")
            ref = kw.get("latent_ref")
            gr = kw.get("guidance_rescale", 0.0)
            # optical-flow correction is per-clip elementwise work behind the shared UNet launch (inference.py:367-386): a clip's flows
            # ride with it (precomputed ``flows``, or ``ref_images`` / ``query_images`` for the pipe's estimator)
            fl = kw.get("flows")
            if fl is None and kw.get("ref_images") is not None:
                if kw["ref_images"].shape[0] != 1:
                    raise ValueError("only support batch size 1")   # inference.py:334
                if not hasattr(self, "obtain_flow_batched"):
                    raise ValueError("ref_images / query_images need the optical-flow pipe (InferenceIP2PVideoOpticalFlow)")
                fl = self.obtain_flow_batched(kw["ref_images"][0], kw["query_images"][0])
            if fl is not None:
                if ref is None:
                    raise ValueError("run_stacked: flows need latent_ref (second_clip_forward)")
                fl = self._latent_flows(fl, lat.shape[0] - ref.shape[1], lat.shape[-2], lat.shape[-1])
            clips.append(dict(lat=lat, cond=cond, flows=fl, ref=None if ref is None else ref[0].to(device=dev, dtype=torch.float32).contiguous(),
                              ncs=kw.get("noise_correct_step", 1.0) if ref is not None else 0.0,
                              text_cfg=kw.get("text_cfg", 7.5), img_cfg=kw.get("img_cfg", 1.2), gr=gr,
                              stats=torch.empty(2, device=dev, dtype=torch.float32) if gr > 0 else None,
                              noises=kw.get("noises"), rng=_rng_of(kw), all_latent=[], all_pred=[], hist=None,
                              known=self._known_tensors(kw["latent"], *(kw.get(k) for k in _KNOWN_KEYS))))
        F, _, h, w = clips[0]["lat"].shape
        # BRANCH-major stack: sample br * n + c = branch br of clip c - the branches (no text, video) and (text, video), whose UNet inputs
        # are identical (inference.py:183-194), are the contiguous samples [n, 3n): the UNet computes their common prefix once (cfg_clips)
        ctx = torch.cat([torch.cat([kw["text_uncond"] for kw in calls], dim=0)] * 2 + [torch.cat([kw["text_cond"] for kw in calls], dim=0)], dim=0)
        runner = shared_runner(self.unet, 3 * n, F, h, w, ctx.shape[1], slot, self.use_graph, False, cfg_clips=n)
        runner.set_context(ctx)
        rows1 = F * h * w
        t_last = None   # (the clips of a stack share start_time, so one previous timestep serves them all; the x0 history is per clip)
        for i, t in enumerate(self.scheduler.timesteps[st0:]):
            t = int(t)
            for c, cl in enumerate(clips):
                ops.build_unet_input(cl["lat"], cl["cond"], runner.x_in[c * rows1:], runner.t[c:], t, 3, branch_rows=n * rows1, t_stride=n)
            eps = runner.run()
            for c, cl in enumerate(clips):
                noise = cl["noises"][i] if cl["noises"] is not None else None
                cl["lat"], pred = self._finish_step(i, t, eps[c * rows1:], cl["lat"], cl["text_cfg"], cl["img_cfg"], cl["gr"],
                                                    cl["stats"], cl["ref"], cl["ncs"], cl["flows"], noise=noise, bstride=n * rows1 * 4,
                                                    rng=cl["rng"], hist=cl["hist"], t_last=t_last, known=cl["known"], start_time=st0)
                cl["hist"] = pred
                cl["all_latent"].append(cl["lat"][None])
                cl["all_pred"].append(pred[None])
            t_last = t
            yield
        return [{"latent": cl["lat"][None], "all_latent": cl["all_latent"], "all_pred": cl["all_pred"]} for cl in clips]

    def _batched_call(self, latent, text_cond, text_uncond, img_cond, latent_ref=None, **kw):
        """b > 1: the reference stacks the batch into the UNet call (inference.py:183-194); here every batch entry is a clip of
        ``run_stacked``.  A stochastic scheduler draws ONE [b,F,4,h,w] normal per step like the reference and slices it - or, with
        ``seed``, batch entry j takes the streams of unit ``unit`` + j."""
        b = latent.shape[0]
        check_known_region(latent, *(kw.get(k) for k in _KNOWN_KEYS))   # (before the noise draws below: nothing is launched for a malformed call)
        noises = None
        seed, unit = kw.pop("seed", None), kw.pop("unit", 0)
        if seed is not None:
            kw["seed"] = seed
        if self.scheduler.stochastic and self.variance_noises is None and seed is None:
            dev = self.unet.device
            steps = len(self.scheduler.timesteps[kw.get("start_time", 0):])
            draws = [torch.randn(latent.shape, device=dev, dtype=torch.float32) for _ in range(steps)]
            noises = [[d[j].contiguous() for d in draws] for j in range(b)]
        elif self.variance_noises is not None:
            noises = [[(v[j] if v is not None else None) for v in self.variance_noises] for j in range(b)]
            noises = [[(x.to(device=self.unet.device, dtype=torch.float32).contiguous() if x is not None else None) for x in nj] for nj in noises]
        calls = []
        for j in range(b):
            c = dict(kw, latent=latent[j:j + 1], text_cond=text_cond[j:j + 1], text_uncond=text_uncond[j:j + 1], img_cond=img_cond[j:j + 1])
            if latent_ref is not None:
                c["latent_ref"] = latent_ref[j:j + 1]
            for k in ("ref_images", "query_images") + _KNOWN_KEYS:   # (the optical-flow pipe's batched form: one estimator pass per batch entry; a batched known region: one slice per entry)
                if kw.get(k) is not None:
                    c[k] = kw[k][j:j + 1]
            if noises is not None:
                c["noises"] = noises[j]
            if seed is not None:
                c["unit"] = unit + j
            calls.append(c)
        res = self.run_stacked(calls)
        steps = len(res[0]["all_latent"])
        return {"latent": torch.cat([r["latent"] for r in res], 0),
                "all_latent": [torch.cat([r["all_latent"][k] for r in res], 0) for k in range(steps)],
                "all_pred": [torch.cat([r["all_pred"][k] for r in res], 0) for k in range(steps)]}

    @torch.no_grad()
    def run_concurrent(self, calls):
        """Run several independent ``__call__`` / ``second_clip_forward`` invocations (list of kwargs dicts, the
        optional key ``latent_ref`` selects ``second_clip_forward``) CONCURRENTLY: each gets its own HIP stream
        set and captured UNet graph and the steps are interleaved, so the GPU overlaps the kernels of
        different clips (units are independent: insv2v_run_loveu_tgve.py:83,101).  Returns the result dicts."""
        if not hasattr(self, "_slot_streams"):
            self._slot_streams = {}
        for kw in calls:   # a malformed known region is refused before the first launch
            check_known_region(kw["latent"], *(kw.get(k) for k in _KNOWN_KEYS))
        main = torch.cuda.current_stream()
        gens = []
        for slot, kw in enumerate(calls):
            kw = dict(kw)
            st = self._slot_streams.setdefault(slot, torch.cuda.Stream())
            st.wait_stream(main)
            args = dict(latent=kw["latent"], text_cond=kw["text_cond"], text_uncond=kw["text_uncond"], img_cond=kw["img_cond"],
                        text_cfg=kw.get("text_cfg", 7.5), img_cfg=kw.get("img_cfg", 1.2), start_time=kw.get("start_time", 0),
                        guidance_rescale=kw.get("guidance_rescale", 0.0), slot=slot, rng=_rng_of(kw),
                        known=_known_of(kw))
            if kw.get("latent_ref") is not None:
                args.update(latent_ref=kw["latent_ref"], noise_correct_step=kw.get("noise_correct_step", 1.0))
            gens.append((st, self._loop_gen(**args)))
        results = [None] * len(gens)
        active = list(range(len(gens)))
        while active:
            for i in list(active):
                st, g = gens[i]
                with torch.cuda.stream(st):
                    try:
                        next(g)
                    except StopIteration as done:
                        results[i] = done.value
                        active.remove(i)
        for st, _ in gens:
            main.wait_stream(st)
        return results

    # ---- a mask estimated from the prompt ---------------------------------------------------------------
    @torch.no_grad()
    def estimate_mask(self, source_latent, text_cond, text_uncond, img_cond, *, n_maps=4, mask_strength=0.5, clamp_ratio=3.0, threshold=0.5,
                      smooth=True, dilate=1, frames_in_batch=16, noises=None, seed=None, unit=0):
        """Where does the instruction act?  -> dict(raw, soft, mask_latent [1,T,h,w], mask [1,T,8h,8w]) for a whole video's SCALED
        source latent ``source_latent`` [1,T,4,h,w] and its condition ``img_cond`` = source_latent / scale_factor (DESIGN.md section 18;
        tests/automask_ref.py is the definition).  Branches 1 and 2 of the CFG stack differ only in the text, so
        ``raw = 1/(4 n_maps) sum_draws sum_c |eps3 - eps2|`` at the source latent noised to the level of ``mask_strength``
        (``timesteps[strength_to_start(mask_strength, steps)[1]]``) is the instruction's footprint; it is normalised by
        ``clamp_ratio`` x the VIDEO's mean, smoothed (``smooth``), thresholded (strict ``>``) and dilated by ``dilate`` cells.
        ``mask`` feeds ``edit_video(mask=...)`` / ``__call__(mask=...)`` unchanged; ``ops.mask_to_latent`` of it is ``mask_latent`` in both modes.

        The video is cut into consecutive chunks of ``frames_in_batch`` frames (no overlap); a chunk's draws are the clips of the
        branch-major stacked runner (``mask_plan``).  The estimate runs in launches of its own - never stacked with another unit or with
        sampling - so with a ``seed`` the mask is a pure function of (seed, unit, inputs, parameters).  Noise, in order of precedence:
        ``noises[chunk][draw]`` ([1,F,4,h,w] or [F,4,h,w] tensors), the seeded stream ``stream_id(MASK, unit, chunk, draw)`` generated
        inside the input kernel, ``torch.randn``.  The defaults are starting values, not findings."""
        check_automask_args(n_maps, mask_strength, clamp_ratio, threshold, smooth, dilate, frames_in_batch)
        if not torch.is_tensor(source_latent) or source_latent.dim() != 5 or source_latent.shape[0] != 1:
            raise ValueError(f"estimate_mask: source_latent {tuple(getattr(source_latent, 'shape', ()))} must be [1,T,4,h,w] (one unit per estimate)")
        z, cond = self._clip_tensors(source_latent, img_cond)
        T, _, h, w = z.shape
        nchunks = -(-T // frames_in_batch)
        if nchunks > (1 << WINDOW_BITS):
            raise ValueError(f"estimate_mask: {T} frames in chunks of {frames_in_batch} are {nchunks} chunks, more than the 2^{WINDOW_BITS} a stream id numbers")
        if noises is not None:
            if len(noises) != nchunks or any(len(nc) != n_maps for nc in noises):
                raise ValueError(f"estimate_mask: noises must hold {nchunks} chunks of {n_maps} draws each")
            for k, nc in enumerate(noises):
                want = (min(frames_in_batch, T - k * frames_in_batch), 4, h, w)
                if any(not torch.is_tensor(x) or tuple(x.shape[-4:]) != want or x.numel() != want[0] * 4 * h * w for x in nc):
                    raise ValueError(f"estimate_mask: every draw of chunk {k} must be shaped {want}")
        elif seed is not None:
            stream_id(MASK, unit, nchunks - 1, n_maps - 1)   # the ranges, before anything is launched
        L = text_cond.shape[1]
        plan = mask_plan(T, frames_in_batch, n_maps, max_clips_in_flight(min(T, frames_in_batch), h, w))
        for F, m in sorted({(p[2], p[4]) for p in plan}):   # every launch's geometry is checked before the first one
            check_operand_windows(3 * m, F, h, w, _unet_channels(self.unet), L)
        dev = z.device
        t = int(self.scheduler.timesteps[strength_to_start(mask_strength, self.num_ddim_steps)[1]])
        ka, kb = self.scheduler.start_coefficients(t)
        raw = torch.empty((T, h, w), device=dev, dtype=torch.float32)   # (the first draw of every chunk writes, the others add: no memset)
        scale = 1.0 / (4.0 * n_maps)
        ready = set()
        for k, start, F, d0, m in plan:
            runner = shared_runner(self.unet, 3 * m, F, h, w, L, 0, self.use_graph, False, cfg_clips=m)
            if id(runner) not in ready:   # the context of a stack of m draws depends on m alone
                runner.set_context(torch.cat([text_uncond] * (2 * m) + [text_cond] * m, dim=0))
                ready.add(id(runner))
            rows1 = F * h * w
            zc, cc = z[start:start + F], cond[start:start + F]
            for c in range(m):
                src = {}
                if noises is not None:
                    src["noise"] = noises[k][d0 + c].to(device=dev, dtype=torch.float32).reshape(F, 4, h, w).contiguous()
                elif seed is not None:
                    src.update(seed=seed, stream=stream_id(MASK, unit, k, d0 + c))
                else:
                    src["noise"] = torch.randn((F, 4, h, w), device=dev, dtype=torch.float32)
                ops.build_unet_input_noised(zc, cc, runner.x_in[c * rows1:], runner.t[c:], t, ka, kb, branch_rows=m * rows1, t_stride=m, **src)
            eps = runner.run()
            for c in range(m):
                ops.eps_absdiff_accum(eps[c * rows1:], raw[start:start + F], scale, accumulate=d0 + c > 0, branch_stride=m * rows1 * 4)
        soft, mask_latent, mask = ops.automask_finish(raw, clamp_ratio=float(clamp_ratio), threshold=float(threshold), smooth=smooth, dilate=dilate)
        return {"raw": raw[None], "soft": soft[None], "mask_latent": mask_latent[None], "mask": mask[None]}

    # ---- reference call surface ----------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, latent, text_cond, text_uncond, img_cond, text_cfg=7.5, img_cfg=1.2, start_time=0,
                 guidance_rescale=0.0, seed=None, unit=0, window=0, mask=None, source_latent=None, known_noise=None, release=None):
        """``mask`` [1,F,h,w] in [0,1] at latent resolution (1 = edit, 0 = keep) with ``source_latent`` [1,F,4,h,w] (the SCALED source
        latent, ``model.encode_image_to_latent``'s result) and ``known_noise`` [1,F,4,h,w] (the fixed noise it is re-noised with: the
        window's initial noise): after every step the latent outside the mask is the source's, re-noised to that step's level - inside
        the step kernel, no extra launch.  Without a mask the call launches exactly what it launched before.
        ``seed`` (default None: the draws of ``torch.randn``, as before): a stochastic scheduler's variance noise of step i comes from
        the seeded stream ``rng.stream_id(STEP, unit, window, i)`` - a pure function of (seed, unit, window, step, element), whatever
        else runs.  Injected ``variance_noises`` win over it; a deterministic scheduler ignores it.
        ``release`` int32 [1,F,h,w] (``ops.strength_release``'s) with ``source_latent`` and ``known_noise``, with or
        without a mask: cell c is held like a cell outside the mask through the steps before ``timesteps[release_c]`` and belongs to the
        model (under its mask value) from that step on - a per-cell ``strength``.  The index is global: ``start_time`` decides which steps
        run, a release index below it changes nothing more.  Without ``release`` the call launches exactly what it launched before."""
        if latent.shape[0] != 1:
            return self._batched_call(latent, text_cond, text_uncond, img_cond, text_cfg=text_cfg, img_cfg=img_cfg, start_time=start_time,
                                      guidance_rescale=guidance_rescale, seed=seed, unit=unit, window=window,
                                      mask=mask, source_latent=source_latent, known_noise=known_noise, release=release)
        check_known_region(latent, mask, source_latent, known_noise, release)
        return self._loop(latent, text_cond, text_uncond, img_cond, text_cfg, img_cfg, start_time, guidance_rescale,
                          rng=_rng_of(dict(seed=seed, unit=unit, window=window)),
                          known=_known_of(dict(mask=mask, source_latent=source_latent, known_noise=known_noise, release=release)))

    @torch.no_grad()
    def second_clip_forward(self, latent, text_cond, text_uncond, img_cond, latent_ref, noise_correct_step=1.0,
                            text_cfg=7.5, img_cfg=1.2, start_time=0, guidance_rescale=0.0, seed=None, unit=0, window=0,
                            mask=None, source_latent=None, known_noise=None, release=None):
        if latent.shape[0] != 1:
            return self._batched_call(latent, text_cond, text_uncond, img_cond, latent_ref=latent_ref, noise_correct_step=noise_correct_step,
                                      text_cfg=text_cfg, img_cfg=img_cfg, start_time=start_time, guidance_rescale=guidance_rescale,
                                      seed=seed, unit=unit, window=window, mask=mask, source_latent=source_latent, known_noise=known_noise, release=release)
        check_known_region(latent, mask, source_latent, known_noise, release)
        return self._loop(latent, text_cond, text_uncond, img_cond, text_cfg, img_cfg, start_time, guidance_rescale,
                          latent_ref=latent_ref, noise_correct_step=noise_correct_step, rng=_rng_of(dict(seed=seed, unit=unit, window=window)),
                          known=_known_of(dict(mask=mask, source_latent=source_latent, known_noise=known_noise, release=release)))


class InferenceIP2PVideoOpticalFlow(InferenceIP2PVideo):
    """Motion-compensated noise correction (inference.py:291-398).  The reference builds a torchvision RAFT estimator with downloaded
    weights here (inference.py:294, flow_utils.py:134-189).  This build carries the network itself on the HIP kernels (insv2v/raft.py,
    round 5) but no weights: pass ``raft_state_dict=`` (torchvision's ``raft_large`` checkpoint, its own key names) and the pipe builds
    ``RAFTFlow`` like the reference; or inject any ``flow_estimator(query[R,3,H,W], refs[R,3,H,W]) -> flow[R,2,H,W]`` (RAFTFlow's call
    signature); or hand precomputed ``flows=`` to ``second_clip_forward``."""

    def __init__(self, *args, flow_estimator=None, raft_state_dict=None, **kwargs):
        super().__init__(*args, **kwargs)
        if flow_estimator is None and raft_state_dict is not None:
            from .raft import RAFTFlow
            flow_estimator = RAFTFlow(self.unet.device).load_state_dict(raft_state_dict)
        self.flow_estimator = flow_estimator

    def obtain_flow_batched(self, ref_images, query_images):
        """One [R,2,H,W] flow set per query frame (inference.py:303-311: the query frame repeated against the R reference frames).  An
        estimator that advertises ``max_pairs`` (this build's RAFTFlow) gets several query frames per call: every (query, reference)
        pair is independent - InstanceNorm is per image, BatchNorm in eval mode - so the values are those of the per-query loop."""
        est = self.flow_estimator
        if est is None:
            raise RuntimeError("InferenceIP2PVideoOpticalFlow needs raft_state_dict= (the estimator's weights are not bundled), flow_estimator= or flows=")
        R = len(ref_images)
        per = getattr(est, "max_pairs", 0) // max(R, 1)
        if per >= 2:
            flows = []
            for i in range(0, len(query_images), per):
                qs = query_images[i:i + per]
                out = est(qs.repeat_interleave(R, dim=0), ref_images.repeat(len(qs), 1, 1, 1))
                flows += list(out.reshape(len(qs), R, *out.shape[1:]))
            return flows
        flows = []
        for q in query_images:
            flows.append(est(q.unsqueeze(0).repeat(R, 1, 1, 1), ref_images))
        return flows

    @torch.no_grad()
    def second_clip_forward(self, latent, text_cond, text_uncond, img_cond, latent_ref, ref_images=None,
                            query_images=None, noise_correct_step=1.0, text_cfg=7.5, img_cfg=1.2, start_time=0,
                            guidance_rescale=0.0, flows=None, seed=None, unit=0, window=0, mask=None, source_latent=None, known_noise=None,
                            release=None):
        check_known_region(latent, mask, source_latent, known_noise, release)
        if flows is None:
            assert ref_images.shape[0] == 1, "only support batch size 1"
            flows = self.obtain_flow_batched(ref_images[0], query_images[0])
        h, w = latent.shape[-2:]
        small = self._latent_flows(flows, latent.shape[1] - latent_ref.shape[1], h, w)
        return self._loop(latent, text_cond, text_uncond, img_cond, text_cfg, img_cfg, start_time, guidance_rescale,
                          latent_ref=latent_ref, noise_correct_step=noise_correct_step, flows=small,
                          rng=_rng_of(dict(seed=seed, unit=unit, window=window)),
                          known=_known_of(dict(mask=mask, source_latent=source_latent, known_noise=known_noise, release=release)))
