#!/usr/bin/env python3
"""Time of the two resampling entries of the region edit (insv2v/region.py, csrc/region.hip) for 16 frames of
3 x 1080 x 1920 fp32 and a 384 x 384 working clip, for the whole frame and for a 480 x 480 box:

  region_resample   the box of every frame and channel resampled to the working size (antialiased bicubic, clamped): one launch
  region_paste      the working-resolution residual resampled to the box and blended into the frames (residual mode, blend 8): one
                    launch; and the replace mode with a mask

Bytes are what the algorithm needs, counted from the shapes, as BOX bytes read plus written: the resample reads the box of the source
once and writes the working clip; the paste reads the working clips (edit and down, or edit and mask) and reads and writes the box of
the frames.  The tiles' halos and the re-reads that hit the cache are not counted.  Next to every kernel: a ``torch`` device-to-device
copy that moves the same number of bytes (half read, half written) in the same process - the yardstick, since nobody has measured these
kernels before.  Device events around REPS back-to-back calls after WARM warm-up calls; the median of ROUNDS such windows.

Every measurement runs in a child process of its own under its own time limit, one after the other; the first one that fails or runs out
of time ends the run.  Prints the lines of profiles/region_gpu.txt; an optional argument names a file to write them to as well."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, H, W, SIZE, WARM, REPS, ROUNDS, LIMIT = 16, 1080, 1920, (384, 384), 3, 10, 5, 240
BOXES = {"whole": (0, 0, 1920, 1080), "box480": (720, 300, 1200, 780)}
KINDS = ("region_resample", "region_paste", "region_paste_replace")


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


def measure(kind, where):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
    import torch
    from insv2v import ops
    dev = "cuda:0"
    assert torch.cuda.is_available(), "bench_region.py measures on the GPU"
    g = torch.Generator(device=dev).manual_seed(1080 * 131 + 1920)
    box = BOXES[where]
    bw, bh = box[2] - box[0], box[3] - box[1]
    w, h = SIZE
    src = torch.rand((T, 3, H, W), device=dev, generator=g) * 2 - 1
    box_bytes, work_bytes = T * 3 * bh * bw * 4, T * 3 * h * w * 4
    if kind == "region_resample":
        out = torch.empty((T, 3, h, w), device=dev)
        nbytes = box_bytes + work_bytes
        fn = lambda: ops.region_resample(src, box, SIZE, clamp=(-1.0, 1.0), out=out)   # noqa: E731
    else:
        down = ops.region_resample(src, box, SIZE, clamp=(-1.0, 1.0))
        edit = (down + 0.1 * torch.rand(down.shape, device=dev, generator=g)).clamp_(-1, 1)
        if kind == "region_paste":
            nbytes = 2 * work_bytes + 2 * box_bytes
            fn = lambda: ops.region_paste(src, edit, down, box, mode="residual", blend=8)   # noqa: E731  (in place: every call adds the residual again)
        else:
            mask = torch.rand((T, h, w), device=dev, generator=g)
            nbytes = work_bytes + T * h * w * 4 + 2 * box_bytes
            fn = lambda: ops.region_paste(src, edit, None, box, mode="replace", blend=8, mask_w=mask)   # noqa: E731
    a = torch.empty(nbytes // 8, device=dev, dtype=torch.float32).normal_()   # nbytes / 2 read + nbytes / 2 written
    b = torch.empty_like(a)
    k, c = _timed(torch, fn), _timed(torch, lambda: b.copy_(a))
    print(f"{T} x 3 x {H} x {W} -> {w} x {h}  {where:7s} box {bw} x {bh}  {kind:21s} {nbytes / 2 ** 20:8.1f} MiB  median {k[0] * 1e3:9.1f} us "
          f"(min {k[1] * 1e3:.1f}, max {k[2] * 1e3:.1f})  {nbytes / k[0] / 1e6:8.1f} GB/s | copy of the same bytes {c[0] * 1e3:9.1f} us  "
          f"{nbytes / c[0] / 1e6:8.1f} GB/s  (kernel / copy rate {c[0] / k[0]:.2f})", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        return measure(sys.argv[2], sys.argv[3])
    lines = [f"fp32 frames in [-1, 1]; device events around {REPS} calls after {WARM} warm-up calls, median of {ROUNDS} windows; bytes counted from the "
             "shapes as box bytes read plus written (halos and cache hits not counted); the copy moves the same number of bytes in the same process"]
    print(lines[0], flush=True)
    for where in BOXES:
        for kind in KINDS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", kind, where], capture_output=True, text=True, timeout=LIMIT)
            new = [ln for ln in r.stdout.splitlines() if ln.strip()]
            print("\n".join(new), flush=True)
            lines += new
            if r.returncode != 0:
                sys.exit(f"{kind} at {where} ended with status {r.returncode}: nothing more is run\n{r.stderr[-2000:]}")
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
