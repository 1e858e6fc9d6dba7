#!/usr/bin/env python3
"""Time of the parts of ``keyframes=`` (insv2v/keyfill.py) for 16 frames at 256 x 384 and at 1024 x 2112, stride 4
(key frames 0, 4, 8, 12, 15: 11 frames in between), fp32 frames - and of the whole thing:

  keyframe_fill   one call of insv2v_keyframe_fill, beside a plain device-to-device copy that moves the same number of bytes
  key_flows       the max gap - 1 = 3 launches of the chain (``ops.mask_track_step``) with the host-side stacking around them
  pair_flows      the 2 (T - 1) RAFT pairs the flows come from (key-hashed weights: the time does not depend on them)
  edit_video      delivered frames per second of ``edit_video`` on the synthetic full-width models, T = 17 at 256 x 384, 20 DDIM steps,
                  with ``keyframes=4`` (5 frames denoised, 12 filled, the RAFT pairs included) and without, alternating in one process

Bytes of the fill are what the algorithm needs, counted from the shapes: A, E, G and U read once, the in-between frames and conf written
once (the gather's re-reads of the keys' taps, which mostly hit the cache, are not counted).  Device events around REPS back-to-back calls
after WARM warm-up calls; the median of ROUNDS such windows; ``pair_flows`` and ``edit_video`` are timed as single calls.  No target is
set: nobody has measured this kernel before, the table is a record.

Every measurement runs in a child process of its own under its own time limit, one after the other; the first one that fails or runs out
of time ends the run.  Prints the lines of profiles/keyfill_gpu.txt; an optional argument names a file to write them to as well
(``--no-e2e`` before it leaves the ``edit_video`` measurement out; ``--e2e`` runs that one alone, ``--e2e DIR`` the plain call alone on
another checkout of the project, such as the parent commit)."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, STRIDE, SIZES, WARM, REPS, ROUNDS, LIMIT = 16, 4, [(256, 384), (1024, 2112)], 3, 10, 5, 300
KINDS = ("keyframe_fill", "key_flows", "pair_flows")
E2E = dict(T=17, H=256, W=384, steps=20, stride=4, rounds=3, limit=900)


def _timed(torch, fn, warm=WARM, reps=REPS, rounds=ROUNDS):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ms), min(ms), max(ms)


def measure(kind, H, W):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
    import torch
    from insv2v import ops, keyfill
    dev = "cuda:0"
    assert torch.cuda.is_available(), "bench_keyfill.py measures on the GPU"
    g = torch.Generator(device=dev).manual_seed(H * 131 + W)
    src = torch.rand((T, 3, H, W), device=dev, generator=g) * 2 - 1
    keys = keyfill.key_frames(T, STRIDE)
    head = f"{T} x {H} x {W}  stride {STRIDE}  {kind:14s}"
    if kind == "pair_flows":
        from insv2v import synth, shapes
        from insv2v.raft import RAFTFlow
        from insv2v.mask_track import pair_flows
        raft = RAFTFlow(dev, synth.synth_raft_state_dict(shapes.raft_shapes()))
        k = _timed(torch, lambda: pair_flows(src[None], raft, both=True), warm=1, reps=1, rounds=2)
        print(f"{head} {2 * (T - 1)} RAFT pairs  median {k[0]:9.1f} ms (min {k[1]:.1f}, max {k[2]:.1f})", flush=True)
        return
    # a sub-pixel translation per pair (all four taps are read), bwd = -fwd: the trajectories are consistent, so nearly every side is
    # active and the kernel does all of its work (independent random flows fail the consistency check almost everywhere)
    d = torch.tensor([[1.5 - 0.25 * (t % 3), -0.75 + 0.5 * (t % 2)] for t in range(T - 1)], device=dev)
    fwd = d[:, :, None, None].expand(T - 1, 2, H, W).contiguous()
    bwd = -fwd
    if kind == "key_flows":
        plan = keyfill.fill_plan(T, keys)
        k = _timed(torch, lambda: keyfill.key_flows(fwd, bwd, keys))
        print(f"{head} {len(plan)} launches of {', '.join(str(len(s)) for s in plan)} chains  median {k[0] * 1e3:9.1f} us (min {k[1] * 1e3:.1f}, max {k[2] * 1e3:.1f})", flush=True)
        return
    edt = (src[keys] + 0.1 * torch.rand((len(keys), 3, H, W), device=dev, generator=g)).clamp_(-1, 1)
    kf = keyfill.key_flows(fwd, bwd, keys)
    n, Tk = len(kf["frames"]), len(keys)
    out, conf = torch.empty_like(src), torch.empty((n, H, W), device=dev)
    plane = H * W * 4
    nbytes = plane * (3 * T + 3 * Tk + 4 * n + 2 * n + 3 * n + n)
    fn = lambda: ops.keyframe_fill(src, edt, kf["flow"], kf["valid"], keys, kf["frames"], kf["slots"], kf["weights"], sigma=0.1, guide_affine=(0.5, 0.5),   # noqa: E731
                                   out=out, conf=conf)
    a = torch.empty(nbytes // 8, device=dev, dtype=torch.float32).normal_()   # nbytes / 2 read + nbytes / 2 written
    b = torch.empty_like(a)
    k, c = _timed(torch, fn), _timed(torch, lambda: b.copy_(a))
    print(f"{head} n={n} active {float(kf['valid'].mean()):.2f}  {nbytes / 2 ** 20:9.1f} MiB  median {k[0] * 1e3:9.1f} us (min {k[1] * 1e3:.1f}, max {k[2] * 1e3:.1f})  "
          f"{nbytes / k[0] / 1e6:8.1f} GB/s | copy of the same bytes {c[0] * 1e3:9.1f} us  {nbytes / c[0] / 1e6:8.1f} GB/s  (ratio {c[0] / k[0]:.2f})", flush=True)


def measure_e2e(root=None):
    """``root``: another checkout of the project (the parent commit): only the plain call is timed there, to show that it did not move."""
    plain_only, root = root is not None, os.path.abspath(root or ROOT)
    sys.path[:0] = [root, os.path.join(root, "instruct-video-to-video_amd")]
    import torch
    from insv2v import synth, shapes
    from insv2v.model import create_model
    from insv2v.inference import InferenceIP2PVideo
    from insv2v.raft import RAFTFlow
    from insv2v.run_loveu_tgve import edit_video
    c, dev = E2E, "cuda:0"
    ucfg, vcfg = synth.UNET_FULL, synth.VAE_FULL
    model = create_model({"unet": {"params": ucfg}, "vae": {"params": vcfg}}, device=dev)
    model.unet.load_state_dict(synth.synth_state_dict(shapes.unet_shapes(**ucfg)))
    model.vae.load_state_dict(synth.synth_state_dict(shapes.vae_shapes(**vcfg)))
    pipe = InferenceIP2PVideo(model.unet, scheduler="ddim", num_ddim_steps=c["steps"])
    raft = RAFTFlow(dev, synth.synth_raft_state_dict(shapes.raft_shapes()))
    frames = synth.synth_input("bench_keyfill.frames", (1, c["T"], 3, c["H"], c["W"]), kind="uniform").to(dev)
    tc = synth.synth_input("bench_keyfill.tc", (1, 77, ucfg["cross_attention_dim"])).to(dev)
    tu = synth.synth_input("bench_keyfill.tu", (1, 77, ucfg["cross_attention_dim"])).to(dev)
    keys = sorted(set(range(0, c["T"], c["stride"])) | {c["T"] - 1})
    sub = frames[:, keys].contiguous()
    runs = {"plain": lambda: edit_video(model, pipe, frames, tc, tu, 7.5, 1.5, seed=1)}
    if plain_only:
        print(f"edit_video  the checkout at {os.path.relpath(root, ROOT)}:", flush=True)
    else:
        runs[f"keyframes={c['stride']}"] = lambda: edit_video(model, pipe, frames, tc, tu, 7.5, 1.5, seed=1, keyframes=c["stride"], flow_estimator=raft)
        runs["keys alone"] = lambda: edit_video(model, pipe, sub, tc, tu, 7.5, 1.5, seed=1)   # the sub-video's edit: what the key frames cost
    ms = {k: [] for k in runs}
    for k, fn in runs.items():   # warm-up: graph capture, workspaces
        fn()
    torch.cuda.synchronize()
    for _ in range(c["rounds"]):
        for k, fn in runs.items():   # alternating
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
            assert out.shape == (sub if k == "keys alone" else frames).shape
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        nf = len(keys) if k == "keys alone" else c["T"]
        print(f"edit_video  {c['T']} x {c['H']} x {c['W']}  {c['steps']} steps  {k:12s} median {med[k]:9.1f} ms (min {min(v):.1f}, max {max(v):.1f})  "
              f"{nf / med[k] * 1e3:7.2f} delivered frames/s ({nf} frames)", flush=True)
    if plain_only:
        return
    p, q, s = med["plain"], med[f"keyframes={c['stride']}"], med["keys alone"]
    nk = len(keys)
    per_between = (q - s) / (c["T"] - nk)
    print(f"edit_video  ratio of delivered frames/s {p / q:.2f}; a denoised frame costs {p / c['T']:.1f} ms in the plain call and {s / nk:.1f} ms in the "
          f"key frames' own, an in-between frame {per_between:.2f} ms (the call's time less the key frames' own, over {c['T'] - nk} frames: "
          f"{2 * (c['T'] - 1)} RAFT pairs, the chain, the fill): a factor of {p / c['T'] / per_between:.1f} and {s / nk / per_between:.1f}", flush=True)


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--one":
        return measure(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    if len(sys.argv) in (2, 3) and sys.argv[1] == "--e2e":
        return measure_e2e(*sys.argv[2:])
    argv = [a for a in sys.argv[1:] if a != "--no-e2e"]
    lines = [f"fp32 frames in [-1, 1], a sub-pixel translation of up to 1.5 px per pair (bwd = -fwd); device events around {REPS} calls after {WARM} warm-up calls, median of {ROUNDS} "
             f"windows (pair_flows: 2 single calls after 1; edit_video: wall clock around single synchronised calls, {E2E['rounds']} per form, alternating); bytes counted from the shapes"]
    jobs = [(["--one", kind, str(H), str(W)], LIMIT, f"{kind} at {H} x {W}") for H, W in SIZES for kind in KINDS]
    if "--no-e2e" not in sys.argv:
        jobs.append((["--e2e"], E2E["limit"], "edit_video"))
    print(lines[0], flush=True)
    for args, limit, what in jobs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], capture_output=True, text=True, timeout=limit)
        new = [ln for ln in r.stdout.splitlines() if ln.strip()]
        print("\n".join(new), flush=True)
        lines += new
        if r.returncode != 0:
            sys.exit(f"{what} ended with status {r.returncode}: nothing more is run\n{r.stderr[-2000:]}")
    if argv:
        open(argv[0], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
