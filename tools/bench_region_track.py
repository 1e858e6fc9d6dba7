#!/usr/bin/env python3
"""What a box per frame costs (insv2v/region_track.py, csrc/region.hip): 16 frames of 3 x 1080 x 1920 fp32, a
384 x 384 working clip and a 480 x 480 box, for the resample, the residual paste and the replace paste with a mask.  In ONE process per
kind, one after the other:

  track, moving     the track entry with a fractional box per frame that travels 37.3 x 11.7 pixels a frame
  track, static     the track entry with the same integer box for every frame
  static entry      the entry of section 26 on that integer box
  copy              a ``torch`` device-to-device copy of the same number of bytes (half read, half written)

Bytes are counted from the shapes as box bytes read plus written, as tools/bench_region.py counts them (the moving boxes' covers are one
pixel larger per axis; the count uses the box).  Device events around REPS back-to-back calls after WARM warm-up calls; the median of
ROUNDS such windows.  The ratio of the track entry to the static entry is RECORDED, not asserted: the arithmetic per tile is the same,
so the expectation is a ratio of 1, and that expectation is a supposition until this file's output says so.

Every kind runs in a child process of its own under its own time limit; the first one that fails or runs out of time ends the run.
Prints the lines of profiles/region_track_gpu.txt; an optional argument names a file to write them to as well."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W, SIZE, WARM, REPS, ROUNDS, LIMIT = 16, 1080, 1920, (384, 384), 3, 10, 5, 240
BOX = (300, 300, 780, 780)
MOVING = [(300.0 + 37.3125 * t, 300.0 + 11.6875 * t, 780.0 + 37.3125 * t, 780.0 + 11.6875 * t) for t in range(T)]
KINDS = ("resample", "paste", "paste_replace")


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


def measure(kind):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
    import torch
    from insv2v import ops
    dev = "cuda:0"
    assert torch.cuda.is_available(), "bench_region_track.py measures on the GPU"
    g = torch.Generator(device=dev).manual_seed(1080 * 131 + 1920)
    bw, bh = BOX[2] - BOX[0], BOX[3] - BOX[1]
    w, h = SIZE
    src = torch.rand((T, 3, H, W), device=dev, generator=g) * 2 - 1
    still = [tuple(float(v) for v in BOX)] * T
    box_bytes, work_bytes = T * 3 * bh * bw * 4, T * 3 * h * w * 4
    if kind == "resample":
        out = torch.empty((T, 3, h, w), device=dev)
        nbytes = box_bytes + work_bytes
        track = lambda boxes: (lambda: ops.region_resample_track(src, boxes, SIZE, clamp=(-1.0, 1.0), out=out))   # noqa: E731
        static = lambda: ops.region_resample(src, BOX, SIZE, clamp=(-1.0, 1.0), out=out)   # noqa: E731
    else:
        down = ops.region_resample(src, BOX, SIZE, clamp=(-1.0, 1.0))
        edit = (down + 0.1 * torch.rand(down.shape, device=dev, generator=g)).clamp_(-1, 1)
        if kind == "paste":   # (in place: every call adds the residual again)
            nbytes = 2 * work_bytes + 2 * box_bytes
            track = lambda boxes: (lambda: ops.region_paste_track(src, edit, down, boxes, mode="residual", blend=8))   # noqa: E731
            static = lambda: ops.region_paste(src, edit, down, BOX, mode="residual", blend=8)   # noqa: E731
        else:
            mask = torch.rand((T, h, w), device=dev, generator=g)
            nbytes = work_bytes + T * h * w * 4 + 2 * box_bytes
            track = lambda boxes: (lambda: ops.region_paste_track(src, edit, None, boxes, mode="replace", blend=8, mask_w=mask))   # noqa: E731
            static = lambda: ops.region_paste(src, edit, None, BOX, mode="replace", blend=8, mask_w=mask)   # noqa: E731
    a = torch.empty(nbytes // 8, device=dev, dtype=torch.float32).normal_()   # nbytes / 2 read + nbytes / 2 written
    b = torch.empty_like(a)
    runs = (("track, moving", track(MOVING)), ("track, static", track(still)), ("static entry", static), ("copy", lambda: b.copy_(a)))
    times = {name: _timed(torch, fn) for name, fn in runs}
    for name, (med, lo, hi) in times.items():
        print(f"{T} x 3 x {H} x {W} -> {w} x {h}  box {bw} x {bh}  {kind:14s} {name:14s} {nbytes / 2 ** 20:7.1f} MiB  median {med * 1e3:8.1f} us "
              f"(min {lo * 1e3:.1f}, max {hi * 1e3:.1f})  {nbytes / med / 1e6:8.1f} GB/s", flush=True)
    s = times["static entry"][0]
    print(f"{kind:14s} time / static entry's: track moving {times['track, moving'][0] / s:.3f}, track static {times['track, static'][0] / s:.3f}; "
          f"static entry / copy rate {times['copy'][0] / s:.2f}", flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        return measure(sys.argv[2])
    lines = [f"fp32 frames in [-1, 1]; device events around {REPS} calls after {WARM} warm-up calls, median of {ROUNDS} windows; bytes counted from the "
             "shapes as box bytes read plus written (halos and cache hits not counted); all four of a kind in the same process"]
    print(lines[0], flush=True)
    for kind in KINDS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind], capture_output=True, text=True, timeout=LIMIT)
        new = [ln for ln in r.stdout.splitlines() if ln.strip()]
        print("\n".join(new), flush=True)
        lines += new
        if r.returncode != 0:
            sys.exit(f"{kind} ended with status {r.returncode}: nothing more is run\n{r.stderr[-2000:]}")
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
