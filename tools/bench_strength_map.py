#!/usr/bin/env python3
"""Per-CALL time (ops.cfg_step: host work included, not a kernel time) of the released step kernel (insv2v_cfg_step_release, with and
without a mask next to the release map) against insv2v_cfg_step_mask at the C2 clip shape (F = 16, h = 32, w = 48; 3 branches, history
present), and of insv2v_strength_release (with and without an image mask) against insv2v_mask_to_latent at 16 x 256 x 384: alternating
windows of back-to-back launches between device events, median per call, in one process - the method of profiles/masked_step_gpu.txt.
Prints the figures of profiles/strength_map_gpu.txt; an optional argument names a file to write them to as well."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
import torch  # noqa: E402
from insv2v import ops  # noqa: E402

F, h, w = 16, 32, 48
STEPS = 20
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(0)
rn = lambda *s: torch.randn(s, device=dev, generator=g)
eps, lat, hist, src, kn = rn(3, F, h, w, 4), rn(F, 4, h, w), rn(F, 4, h, w), rn(F, 4, h, w), rn(F, 4, h, w)
mask = torch.rand((F, h, w), device=dev, generator=g)
release = torch.randint(0, STEPS + 1, (F, h, w), device=dev, generator=g, dtype=torch.int32)
new, pred = torch.empty_like(lat), torch.empty_like(lat)
base = dict(nbranch=3, text_cfg=7.5, img_cfg=1.5, sqrt_a=0.8, sqrt_1ma=0.6, coef=(0.83, 0.0, 0.41, 0.0), latent_out=new, pred_x0=pred,
            x0_hist=hist, c_hist=-0.37, src=src, known_noise=kn, k_src=0.93, k_noise=0.37)
smap = torch.rand((F, 8 * h, 8 * w), device=dev, generator=g)
smap[smap < 0.2] = 0.0
image_mask = torch.rand((F, 8 * h, 8 * w), device=dev, generator=g)
INNER, REPS = 500, 31


def measure(variants):
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
    return times


def table(times, width):
    med = {name: statistics.median(t) for name, t in times.items()}
    return med, [f"{name:{width}s} median {med[name]:.3f} us  min {min(t):.3f}  max {max(t):.3f}" for name, t in times.items()]


elems, cells, pixels = F * 4 * h * w, F * h * w, F * 64 * h * w
lines = [f"shape F={F} h={h} w={w} (C2 clip), nbranch=3, history present, step {STEPS // 2} of a release map with values in [0, {STEPS}], {REPS} windows of "
         f"{INNER} back-to-back launches each, alternating; us per call (host work included)"]
med, rows = table(measure({"cfg_step_mask": lambda: ops.cfg_step(eps, lat, mask=mask, **base),
                           "cfg_step_release": lambda: ops.cfg_step(eps, lat, mask=mask, release=release, step=STEPS // 2, **base),
                           "cfg_step_release, no mask": lambda: ops.cfg_step(eps, lat, release=release, step=STEPS // 2, **base)}), 26)
lines += rows
bytes_mask = ((3 + 1 + 1 + 2 + 2) * elems + cells) * 4   # 3 eps planes, latent, history, src, known_noise read, latent_out and pred_x0 written, the mask
lines.append(f"ratio released / masked (medians): {med['cfg_step_release'] / med['cfg_step_mask']:.3f}   without a mask: {med['cfg_step_release, no mask'] / med['cfg_step_mask']:.3f}")
lines.append(f"bytes moved: masked {bytes_mask} B, released {bytes_mask + cells * 4} B (the release map: one int32 per cell), ratio {(bytes_mask + cells * 4) / bytes_mask:.3f}")
lines.append("")
lines.append(f"strength image {F} x {8 * h} x {8 * w} fp32, steps={STEPS}, mode max; us per call (host work and the allocation of the outputs included)")
med, rows = table(measure({"mask_to_latent": lambda: ops.mask_to_latent(smap, "max"),
                           "strength_release": lambda: ops.strength_release(smap, STEPS, "max"),
                           "strength_release, mask": lambda: ops.strength_release(smap, STEPS, "max", mask=image_mask)}), 26)
lines += rows
lines.append(f"bytes moved: mask_to_latent {(pixels + cells) * 4} B, strength_release {(3 * pixels + cells) * 4} B (the map read twice, the gate written), "
             f"with an image mask {(4 * pixels + cells) * 4} B")
lines.append(f"achieved: mask_to_latent {(pixels + cells) * 4 / med['mask_to_latent'] / 1e3:.1f} GB/s, strength_release {(3 * pixels + cells) * 4 / med['strength_release'] / 1e3:.1f} GB/s, "
             f"with an image mask {(4 * pixels + cells) * 4 / med['strength_release, mask'] / 1e3:.1f} GB/s")
out = "\n".join(lines)
print(out)
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(out + "\n")
