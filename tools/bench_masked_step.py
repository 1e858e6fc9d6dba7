#!/usr/bin/env python3
"""Per-CALL time (ops.cfg_step: host work included, not a kernel time) of the masked step kernel (insv2v_cfg_step_mask) against insv2v_cfg_step_ms at the C2 clip shape (F = 16, h = 32,
w = 48; 3 branches, history present): alternating windows of back-to-back launches between device events, median per call, in one
process.  For kernel time run it under `rocprofv3 --kernel-trace --stats` (a run of its own) and read the kernel_stats table.  Prints the figures of profiles/masked_step_gpu.txt; an optional argument names a file to write them to as well."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
import torch  # noqa: E402
from insv2v import ops  # noqa: E402

F, h, w = 16, 32, 48
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *s: torch.randn(s, device=dev, generator=g)
eps, lat, hist, src, kn = rn(3, F, h, w, 4), rn(F, 4, h, w), rn(F, 4, h, w), rn(F, 4, h, w), rn(F, 4, h, w)
mask = torch.rand((F, h, w), device=dev, generator=g)
new, pred = torch.empty_like(lat), torch.empty_like(lat)
base = dict(nbranch=3, text_cfg=7.5, img_cfg=1.5, sqrt_a=0.8, sqrt_1ma=0.6, coef=(0.83, 0.0, 0.41, 0.0), latent_out=new, pred_x0=pred,
            x0_hist=hist, c_hist=-0.37)
known = dict(mask=mask, src=src, known_noise=kn, k_src=0.93, k_noise=0.37)
variants = {"cfg_step_ms": lambda: ops.cfg_step(eps, lat, **base), "cfg_step_mask": lambda: ops.cfg_step(eps, lat, **base, **known)}
INNER, REPS = 500, 31
for fn in variants.values():
    for _ in range(200):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in variants}
for _ in range(REPS):
    for name, fn in variants.items():   # alternating
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        e1.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3 / INNER)
elems = F * 4 * h * w
bytes_ms = (3 + 1 + 1 + 2) * elems * 4            # 3 eps planes + latent + history read, latent_out + pred_x0 written
bytes_mask = bytes_ms + (2 * elems + F * h * w) * 4
lines = [f"shape F={F} h={h} w={w} (C2 clip), nbranch=3, history present, {REPS} windows of {INNER} back-to-back launches each, alternating; us per call (host work included)"]
med = {}
for name, t in times.items():
    med[name] = statistics.median(t)
    lines.append(f"{name:14s} median {med[name]:.3f} us  min {min(t):.3f}  max {max(t):.3f}")
lines.append(f"ratio masked / unmasked (medians): {med['cfg_step_mask'] / med['cfg_step_ms']:.3f}")
lines.append(f"bytes moved: unmasked {bytes_ms} B, masked {bytes_mask} B, ratio {bytes_mask / bytes_ms:.3f}")
lines.append(f"achieved: unmasked {bytes_ms / med['cfg_step_ms'] / 1e3:.1f} GB/s, masked {bytes_mask / med['cfg_step_mask'] / 1e3:.1f} GB/s")
out = "\n".join(lines)
print(out)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(out + "\n")
