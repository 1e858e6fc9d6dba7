#!/usr/bin/env python3
"""Time and bytes moved of the two pixel-score entries (insv2v/pixel_score.py) - insv2v_frame_fidelity and
insv2v_warp_error, each with its finalize launch - for 16 frames at 256 x 384 and at 1024 x 2112, fp32 frames with a region, each row
beside a plain device-to-device copy that moves the same number of bytes (read + written).  No target is set: the small size is
launch-bound and sits in the last-level cache, the table is a record.

Bytes are what the algorithm needs, counted from the shapes: fidelity reads X, Y and w once; the warp error reads, per pair, both
frames, both flows and w (halo re-reads, the gather's neighbours and the partial sums are not counted).  Device events around REPS
back-to-back calls after WARM warm-up calls; the median of ROUNDS such windows.

Every measurement runs in a child process of its own under its own time limit, one after the other; the first one that fails or runs out
of time ends the run.  Prints the lines of profiles/pixel_score_gpu.txt; an optional argument names a file to write them to as well."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, SIZES, WARM, REPS, ROUNDS, LIMIT = 16, [(256, 384), (1024, 2112)], 3, 10, 5, 300


def measure(H, W):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
    import torch
    from insv2v import ops
    dev = "cuda:0"
    assert torch.cuda.is_available(), "bench_pixel_score.py measures on the GPU"
    g = torch.Generator(device=dev).manual_seed(H * 131 + W)
    x = torch.rand((T, 3, H, W), device=dev, generator=g) * 2 - 1
    y = (x + 0.1 * torch.rand((T, 3, H, W), device=dev, generator=g)).clamp_(-1, 1)
    w = (torch.rand((T, H, W), device=dev, generator=g) > 0.5).float()
    fwd = torch.rand((T - 1, 2, H, W), device=dev, generator=g) * 4 - 2
    bwd = -fwd
    fid_out = torch.empty((T, 10), device=dev, dtype=torch.float64)
    fid_ws = torch.empty(ops.frame_fidelity_workspace_elems(T, H, W), device=dev, dtype=torch.float64)
    we_out = (torch.empty((T - 1, 3), device=dev, dtype=torch.float64), None, None)
    we_ws = torch.empty(ops.warp_error_workspace_elems(T, H, W), device=dev, dtype=torch.float64)
    plane = H * W * 4
    runs = [("frame_fidelity", 2 * T * 3 * plane + T * plane,
             lambda: ops.frame_fidelity(x, y, w, x_affine=(0.5, 0.5), y_affine=(0.5, 0.5), out=fid_out, workspace=fid_ws)),
            ("warp_error (fwd + bwd)", (T - 1) * (2 * 3 + 2 * 2 + 1) * plane,
             lambda: ops.warp_error(y, fwd, bwd, w, scale=0.5, shift=0.5, out=we_out, workspace=we_ws))]

    def timed(fn):
        for _ in range(WARM):
            fn()
        ms = []
        for _ in range(ROUNDS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / REPS)
        return statistics.median(ms), min(ms), max(ms)

    for name, nbytes, fn in runs:
        src = torch.empty(nbytes // 8, device=dev, dtype=torch.float32).normal_()   # nbytes / 2 read + nbytes / 2 written
        dst = torch.empty_like(src)
        k, c = timed(fn), timed(lambda: dst.copy_(src))
        print(f"{T} x {H} x {W}  {name:24s} {nbytes / 2 ** 20:9.1f} MiB  median {k[0] * 1e3:9.1f} us (min {k[1] * 1e3:.1f}, max {k[2] * 1e3:.1f})  "
              f"{nbytes / k[0] / 1e6:8.1f} GB/s | copy of the same bytes {c[0] * 1e3:9.1f} us  {nbytes / c[0] / 1e6:8.1f} GB/s", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        return measure(int(sys.argv[2]), int(sys.argv[3]))
    lines = [f"fp32 frames in [-1, 1] with a region; us per call (kernel + finalize launch), device events around {REPS} calls after {WARM} warm-up calls, "
             f"median of {ROUNDS} windows; bytes counted from the shapes"]
    for H, W in SIZES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(H), str(W)], capture_output=True, text=True, timeout=LIMIT)
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            print("\n".join(lines))
            sys.exit(f"{H} x {W} ended with status {r.returncode}: nothing more is run\n{r.stderr[-2000:]}")
    out = "\n".join(lines)
    print(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out + "\n")


if __name__ == "__main__":
    main()
