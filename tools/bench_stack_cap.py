#!/usr/bin/env python3
"""Stacks beyond the default cap (inference.max_clips_in_flight): the full-width UNet forward of n clips' CFG triples (B = 3 n, branch-major
with the shared CFG prefix, as run_stacked launches it) as a replayed hipGraph on one stream, ms per forward and per clip (median of REPS).

    python tools/bench_stack_cap.py 24x48x64:7,10,14 16x45x80:9,14,20      # FxHxW:clips,...   env: REPS
The first count of each geometry is its default cap; nothing here changes a default."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
import torch  # noqa: E402
from insv2v import synth, shapes  # noqa: E402
from insv2v.unet import UNet3DConditionModel  # noqa: E402
from insv2v.inference import GraphedUNet, max_clips_in_flight  # noqa: E402

REPS = int(os.environ.get("REPS", 7))
specs = sys.argv[1:] or ["24x48x64:7,10,14", "16x45x80:9,14,20"]
unet = UNet3DConditionModel(**synth.UNET_FULL, device="cuda:0").load_state_dict(synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_FULL)))

for spec in specs:
    geo, counts = spec.split(":")
    F, h, w = (int(v) for v in geo.split("x"))
    print(f"F={F} latent {h}x{w}: default cap {max_clips_in_flight(F, h, w)} clips", flush=True)
    for n in (int(v) for v in counts.split(",")):
        r = GraphedUNet(unet, 3 * n, F, h, w, 77, use_graph=True, branch_streams=False, cfg_clips=n)
        one = synth.synth_input("p.ctx", (3, 77, 768))
        r.set_context(torch.cat([one[b:b + 1].repeat(n, 1, 1) for b in range(3)], 0))
        r.x_in.normal_()
        r.x_in[2 * n * F * h * w:] = r.x_in[n * F * h * w:2 * n * F * h * w]   # branches 1 and 2 share their inputs (cfg_clips)
        r.t.fill_(500.0)
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
        med = statistics.median(ms)
        gb = 3 * n * F * h * w * 320 * 2 / 1e9
        print(f"  {n:2d} clips (B = {3 * n:3d}, level-0 token matrix {gb:.2f} GB): forward {med:9.2f} ms = {med / n:7.2f} ms per clip "
              f"(median of {REPS} graph replays; min {min(ms):.2f}, max {max(ms):.2f})", flush=True)
        del r
        torch.cuda.empty_cache()
