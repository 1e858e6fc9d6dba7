#!/usr/bin/env python3
"""Time of ``ops.mask_shape`` (insv2v_mask_shape: the column pass and the row pass) for 16 frames at 256 x 384 and
at 1024 x 2112, with ``grow=4, feather=8`` (R = 12, 25 taps per pixel in the row pass) and ``grow=0, feather=32`` (R = 32, 65 taps),
beside a plain device-to-device copy that moves the same number of bytes.

Bytes are what the algorithm needs, counted from the shapes: the mask read once, ``shaped`` and ``support`` written once (12 bytes per
pixel; the workspace's byte per pixel, written and read back, and the column pass's re-reads of its halo are not counted).  The outputs and
the workspace are preallocated.  Device events around REPS back-to-back calls after WARM warm-up calls; the median of ROUNDS such windows.
No target is set: nobody has measured this kernel before, the table is a record.

Every measurement runs in a child process of its own under its own time limit, one after the other; the first one that fails or runs out
of time ends the run.  Prints the lines of profiles/mask_shape_gpu.txt; an optional argument names a file to write them to as well."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, SIZES, PARAMS, WARM, REPS, ROUNDS, LIMIT = 16, [(256, 384), (1024, 2112)], [(4.0, 8.0), (0.0, 32.0)], 3, 10, 5, 120


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


def measure(H, W, grow, feather):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
    import torch
    from insv2v import ops, _lib
    dev = "cuda:0"
    assert torch.cuda.is_available(), "bench_mask_shape.py measures on the GPU"
    # a centred rectangle of half the height and width that drifts by a pixel per frame, and a scatter of single pixels
    g = torch.Generator(device=dev).manual_seed(H * 131 + W)
    m = (torch.rand((T, H, W), device=dev, generator=g) > 0.9995).float()
    for t in range(T):
        m[t, H // 4:H - H // 4, W // 4 + t:W - W // 4 + t] = 1.0
    out = (torch.empty_like(m), torch.empty_like(m))
    ws = torch.empty(_lib.load().insv2v_mask_shape_workspace_bytes(T, H, W), device=dev, dtype=torch.uint8)
    plan = ops.mask_shape_plan(grow, feather)
    nbytes = T * H * W * 12
    fn = lambda: ops.mask_shape(m, grow=grow, feather=feather, out=out, workspace=ws)   # noqa: E731
    a = torch.empty(nbytes // 8, device=dev, dtype=torch.float32).normal_()   # nbytes / 2 read + nbytes / 2 written
    b = torch.empty_like(a)
    k, c = _timed(torch, fn), _timed(torch, lambda: b.copy_(a))
    soft = float(((out[0] > 0) & (out[0] < 1)).float().mean())
    print(f"{T} x {H} x {W}  grow={grow:g} feather={feather:g}  R={plan['R']:2d}  feathered {soft:.3f}  {nbytes / 2 ** 20:8.1f} MiB  median {k[0] * 1e3:9.1f} us "
          f"(min {k[1] * 1e3:.1f}, max {k[2] * 1e3:.1f})  {nbytes / k[0] / 1e6:8.1f} GB/s | copy of the same bytes {c[0] * 1e3:9.1f} us  "
          f"{nbytes / c[0] / 1e6:8.1f} GB/s", flush=True)


def main():
    if len(sys.argv) == 6 and sys.argv[1] == "--one":
        return measure(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), float(sys.argv[5]))
    lines = [f"fp32 masks (a drifting rectangle and scattered pixels), profile smooth; device events around {REPS} calls after {WARM} warm-up calls, median of "
             f"{ROUNDS} windows; bytes counted from the shapes (mask read, shaped and support written)"]
    for H, W in SIZES:
        for grow, feather in PARAMS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(H), str(W), str(grow), str(feather)], capture_output=True,
                               text=True, timeout=LIMIT)
            lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
            if r.returncode != 0:
                print("\n".join(lines))
                sys.exit(f"grow={grow} feather={feather} at {H} x {W} ended with status {r.returncode}: nothing more is run\n{r.stderr[-2000:]}")
    out = "\n".join(lines)
    print(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out + "\n")


if __name__ == "__main__":
    main()
