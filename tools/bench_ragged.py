#!/usr/bin/env python3
"""Full-width UNet forward (B = 3, F = 16) at latent sizes whose pixel counts do not line up with the row kernels' tiles, e.g. 60x60
(480x480 frames) and 45x80 (360x640): ms per forward as a replayed hipGraph on one stream (median of REPS replays) and the per-launch
table of an eager forward (HIP events around every launch; per shape the fastest of three recorded forwards, as tools/profile_unet.py).

    python tools/bench_ragged.py 60x60 45x80          # SHAPES; env: NB, F, REPS, TABLE=0 for the forward time only
Run it from two checkouts alternately to compare them on one box (profiles/ragged_rows_ab.txt)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
import torch  # noqa: E402
from insv2v import synth, shapes, ops  # noqa: E402
from insv2v.unet import UNet3DConditionModel  # noqa: E402
from insv2v.inference import GraphedUNet  # noqa: E402

NB, F, REPS = int(os.environ.get("NB", 3)), int(os.environ.get("F", 16)), int(os.environ.get("REPS", 9))
TABLE = os.environ.get("TABLE", "1") != "0"
LABEL = os.environ.get("LABEL", os.path.basename(ROOT))
sizes = [tuple(int(v) for v in s.split("x")) for s in (sys.argv[1:] or ["60x60", "45x80"])]
unet = UNet3DConditionModel(**synth.UNET_FULL, device="cuda:0").load_state_dict(synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_FULL)))
ctx = synth.synth_input("p.ctx", (NB, 77, 768))


def runner(h, w, use_graph):
    r = GraphedUNet(unet, NB, F, h, w, 77, use_graph=use_graph, branch_streams=False, cfg_clips=0)
    r.set_context(ctx)
    r.x_in.normal_()
    r.t.fill_(500.0)
    return r


for h, w in sizes:
    r = runner(h, w, True)
    for _ in range(2):
        r.run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r.run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(f"[{LABEL}] B={NB} F={F} latent {h}x{w}: forward {statistics.median(ms):.3f} ms (median of {REPS} graph replays; min {min(ms):.3f}, max {max(ms):.3f})", flush=True)
    del r
    if not TABLE:
        continue
    r = runner(h, w, False)
    r.run()
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        rec = []
        ops.set_launch_recorder(rec)
        r.run()
        torch.cuda.synchronize()
        ops.set_launch_recorder(None)
        groups = {}
        for name, work, e0, e1, tag in rec:
            g = groups.setdefault(tag, [0, 0.0, 0.0])
            g[0] += 1
            g[1] += e0.elapsed_time(e1)
            g[2] += work
        runs.append((groups, len(rec)))
    groups = {tag: min((run[0][tag] for run in runs), key=lambda g: g[1]) for tag in runs[0][0]}
    tot = sum(g[1] for g in groups.values())
    print(f"[{LABEL}] latent {h}x{w}: {tot:.2f} ms in {runs[0][1]} eager launches (per shape: fastest of 3 forwards)")
    for tag, (n, t, work) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
        print(f"{t:8.3f} ms {100 * t / tot:5.1f}%  n={n:3d}  {t / n * 1e3:8.1f} us/launch  {work / t / 1e9 if t else 0:8.1f} TF/s  {tag}")
    del r
    torch.cuda.empty_cache()
