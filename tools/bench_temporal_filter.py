#!/usr/bin/env python3
"""Time of the three parts of ``stabilize=`` (insv2v/temporal_filter.py) for 16 frames at 256 x 384 and at
1024 x 2112, radius 2 (K = 4 neighbours), fp32 frames:

  temporal_filter   one launch of insv2v_temporal_filter, beside a plain device-to-device copy that moves the same number of bytes
  neighbour_flows   the R = 2 launches of the chain (``ops.mask_track_step``) with the host-side stacking around them
  pair_flows        the 2 (T - 1) RAFT pairs the flows come from (key-hashed weights: the time does not depend on them)

Bytes of the filter are what the algorithm needs, counted from the shapes: E, A, G and U read once, the output written once (the
gather's re-reads of neighbouring frames, which mostly hit the cache, are not counted).  Device events around REPS back-to-back calls after
WARM warm-up calls; the median of ROUNDS such windows; ``pair_flows`` is timed as single calls.  No target is set: nobody has measured this
kernel before, the table is a record.

Every measurement runs in a child process of its own under its own time limit, one after the other; the first one that fails or runs out
of time ends the run.  Prints the lines of profiles/temporal_filter_gpu.txt; an optional argument names a file to write them to as well."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, R, SIZES, WARM, REPS, ROUNDS, LIMIT = 16, 2, [(256, 384), (1024, 2112)], 3, 10, 5, 300
KINDS = ("temporal_filter", "neighbour_flows", "pair_flows")


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
    from insv2v import ops, temporal_filter as tf
    dev = "cuda:0"
    assert torch.cuda.is_available(), "bench_temporal_filter.py measures on the GPU"
    g = torch.Generator(device=dev).manual_seed(H * 131 + W)
    src = torch.rand((T, 3, H, W), device=dev, generator=g) * 2 - 1
    head = f"{T} x {H} x {W}  R={R}  {kind:16s}"
    if kind == "pair_flows":
        from insv2v import synth, shapes
        from insv2v.raft import RAFTFlow
        from insv2v.mask_track import pair_flows
        raft = RAFTFlow(dev, synth.synth_raft_state_dict(shapes.raft_shapes()))
        k = _timed(torch, lambda: pair_flows(src[None], raft, both=True), warm=1, reps=1, rounds=2)
        print(f"{head} {2 * (T - 1)} RAFT pairs  median {k[0]:9.1f} ms (min {k[1]:.1f}, max {k[2]:.1f})", flush=True)
        return
    # a sub-pixel translation per pair (all four taps are read), bwd = -fwd: the trajectories are consistent, so nearly every neighbour is
    # valid and the filter does all of its work (independent random flows fail the consistency check almost everywhere)
    d = torch.tensor([[1.5 - 0.25 * (t % 3), -0.75 + 0.5 * (t % 2)] for t in range(T - 1)], device=dev)
    fwd = d[:, :, None, None].expand(T - 1, 2, H, W).contiguous()
    bwd = -fwd
    if kind == "neighbour_flows":
        k = _timed(torch, lambda: tf.neighbour_flows(fwd, bwd, radius=R))
        print(f"{head} {R} launches of {2 * (T - 1)} and {2 * (T - 2)} chains  median {k[0] * 1e3:9.1f} us (min {k[1] * 1e3:.1f}, max {k[2] * 1e3:.1f})", flush=True)
        return
    edt = (src + 0.1 * torch.rand((T, 3, H, W), device=dev, generator=g)).clamp_(-1, 1)
    nb = tf.neighbour_flows(fwd, bwd, radius=R)
    K = len(nb["offsets"])
    out = torch.empty_like(edt)
    plane = H * W * 4
    nbytes = T * plane * (3 + 3 + 3 * K + 3)
    fn = lambda: ops.temporal_filter(edt, src, nb["flow"], nb["valid"], nb["offsets"], sigma=0.1, strength=1.0, guide_affine=(0.5, 0.5), out=out)   # noqa: E731
    a = torch.empty(nbytes // 8, device=dev, dtype=torch.float32).normal_()   # nbytes / 2 read + nbytes / 2 written
    b = torch.empty_like(a)
    k, c = _timed(torch, fn), _timed(torch, lambda: b.copy_(a))
    print(f"{head} valid {float(nb['valid'].mean()):.2f}  {nbytes / 2 ** 20:9.1f} MiB  median {k[0] * 1e3:9.1f} us (min {k[1] * 1e3:.1f}, max {k[2] * 1e3:.1f})  "
          f"{nbytes / k[0] / 1e6:8.1f} GB/s | copy of the same bytes {c[0] * 1e3:9.1f} us  {nbytes / c[0] / 1e6:8.1f} GB/s", flush=True)


def main():
    if len(sys.argv) == 5 and sys.argv[1] == "--one":
        return measure(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    lines = [f"fp32 frames in [-1, 1], a sub-pixel translation of up to 1.5 px per pair (bwd = -fwd); device events around {REPS} calls after {WARM} warm-up calls, median of {ROUNDS} "
             f"windows (pair_flows: 2 single calls after 1); bytes counted from the shapes"]
    for H, W in SIZES:
        for kind in KINDS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, str(H), str(W)], capture_output=True, text=True, timeout=LIMIT)
            lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
            if r.returncode != 0:
                print("\n".join(lines))
                sys.exit(f"{kind} at {H} x {W} ended with status {r.returncode}: nothing more is run\n{r.stderr[-2000:]}")
    out = "\n".join(lines)
    print(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out + "\n")


if __name__ == "__main__":
    main()
