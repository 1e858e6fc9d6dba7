#!/usr/bin/env python3
"""Time of a tracked mask (insv2v/mask_track.py), its two parts apart: ``pair_flows`` - the 2 (T - 1) adjacent-frame
pairs through RAFT on the HIP kernels, key-hashed weights - and the chain of ``propagate_mask`` (T - 1 launches of insv2v_mask_track_step
from a key frame at 0, T / 2 launches from one in the middle), for 16 and 32 frames at 256 x 384.  No target is set: the figures are
recorded.  Host clock around calls that end in a device synchronise, one warm-up call, median of REPS.

Every measurement runs in a child process of its own under its own time limit, one after the other; the first one that fails or runs out
of time ends the run.  Prints the lines of profiles/masktrack_gpu.txt; an optional argument names a file to write them to as well."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, REPS, LIMIT = 256, 384, 5, 300
CASES = [(what, T) for T in (16, 32) for what in ("pair_flows", "chain")]


def measure(what, T):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
    import torch
    from insv2v import synth, shapes
    from insv2v.mask_track import pair_flows, propagate_mask
    dev = "cuda:0"
    assert torch.cuda.is_available(), "bench_masktrack.py measures on the GPU"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if what == "pair_flows":
        from insv2v.raft import RAFTFlow
        est = RAFTFlow(dev, synth.synth_raft_state_dict(shapes.raft_shapes()))
        frames = synth.synth_input("bench.masktrack.frames", (1, T, 3, H, W), kind="uniform").to(dev)
        runs = {f"pair_flows T={T}: {2 * (T - 1)} pairs, RAFT 12 updates": lambda: pair_flows(frames, est),
                f"pair_flows T={T}: {T - 1} pairs (no occlusion check)": lambda: pair_flows(frames, est, both=False, key=0)}
    else:
        fwd = synth.synth_input("bench.masktrack.fwd", (T - 1, 2, H, W)).to(dev) * 2.0
        bwd = -fwd
        M = torch.zeros((H, W), device=dev)
        M[H // 4:H - H // 4, W // 4:W - W // 4] = 1.0
        runs = {f"chain T={T} key=0: {T - 1} launches": lambda: propagate_mask(M, 0, fwd, bwd),
                f"chain T={T} key={T // 2}: {T // 2} launches": lambda: propagate_mask(M, T // 2, fwd, bwd),
                f"chain T={T} key=0, no occlusion check": lambda: propagate_mask(M, 0, fwd, bwd, occlusion=False)}
    for name, fn in runs.items():
        fn()
        t = [timed(fn) for _ in range(REPS)]
        print(f"{name:58s} median {statistics.median(t):9.2f} ms  min {min(t):9.2f}  max {max(t):9.2f}", flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        return measure(sys.argv[2], int(sys.argv[3]))
    lines = [f"{H} x {W} frames; ms per call (host clock, device-synchronised), median of {REPS} calls after one warm-up; RAFT with key-hashed weights"]
    for what, T in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what, str(T)], capture_output=True, text=True, timeout=LIMIT)
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            print("\n".join(lines))
            sys.exit(f"{what} T={T} ended with status {r.returncode}: nothing more is run\n{r.stderr[-2000:]}")
    out = "\n".join(lines)
    print(out)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(out + "\n")


if __name__ == "__main__":
    main()
