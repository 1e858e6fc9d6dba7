#!/usr/bin/env python3
"""Time of a mask estimate (InferenceIP2PVideo.estimate_mask) against the edit it precedes: the full-width
random-init UNet, one clip of 16 frames at 32 x 48 latents (C2), n_maps = 4 and 10, seeded noise; the edit is the 20-step DDIM sampling
loop of the same clip (``pipe(...)``, one window, three branch streams - no VAE on either side).  Host clock around calls that end in a
device synchronise, every shape warmed up (graphs captured) first, the three variants alternating, median of REPS.  The expectation
``n_maps / steps`` of an edit is arithmetic; what this prints is the measurement.  Prints the figures of profiles/automask_gpu.txt; an
optional argument names a file to write them to as well."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
import torch  # noqa: E402
from insv2v import synth, shapes  # noqa: E402
from insv2v.unet import UNet3DConditionModel  # noqa: E402
from insv2v.inference import InferenceIP2PVideo  # noqa: E402

F, h, w, STEPS, REPS = 16, 32, 48, 20, 7
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_automask.py measures on the GPU"
unet = UNet3DConditionModel(**synth.UNET_FULL, device=dev).load_state_dict(synth.synth_state_dict(shapes.unet_shapes(**synth.UNET_FULL)))
pipe = InferenceIP2PVideo(unet, scheduler="ddim", num_ddim_steps=STEPS)
z, cond, noise = (synth.synth_input(f"bench.automask.{k}", (1, F, 4, h, w)).to(dev) for k in ("z", "cond", "noise"))
tc, tu = (synth.synth_input(f"bench.automask.{k}", (1, 77, synth.UNET_FULL["cross_attention_dim"])).to(dev) for k in ("tc", "tu"))
variants = {"estimate_mask n_maps=4": lambda: pipe.estimate_mask(z, tc, tu, cond, n_maps=4, seed=1, unit=0),
            "estimate_mask n_maps=10": lambda: pipe.estimate_mask(z, tc, tu, cond, n_maps=10, seed=1, unit=0),
            f"edit, {STEPS} DDIM steps": lambda: pipe(noise, tc, tu, cond, text_cfg=7.5, img_cfg=1.5)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


for fn in variants.values():   # warm-up: kernel attributes, allocator, graph capture of every shape
    fn(), fn()
times = {k: [] for k in variants}
for _ in range(REPS):
    for name, fn in variants.items():   # alternating
        times[name].append(timed(fn))
med = {k: statistics.median(t) for k, t in times.items()}
edit = med[f"edit, {STEPS} DDIM steps"]
lines = [f"full-width random-init UNet, one clip F={F} h={h} w={w}; ms per call (host clock, device-synchronised), median of {REPS} alternating calls"]
for name, t in times.items():
    lines.append(f"{name:26s} median {med[name]:9.2f} ms  min {min(t):9.2f}  max {max(t):9.2f}")
for n in (4, 10):
    m = med[f"estimate_mask n_maps={n}"]
    lines.append(f"n_maps={n:2d}: {m / edit:.3f} of the edit (arithmetic expectation n_maps / steps = {n / STEPS:.3f}); {m / n:.2f} ms per draw, "
                 f"{edit / STEPS:.2f} ms per edit step; a third of every draw's forward is branch 0, which the estimate does not use: ~{m / 3:.1f} ms")
out = "\n".join(lines)
print(out)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(out + "\n")
