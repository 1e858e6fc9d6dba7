#!/usr/bin/env python3
"""The VAE's mid AttnBlock alone (insv2v/vae.py VAttn, full width C = 512) on its two forms - "scores" (three batched GEMMs around a row
softmax, the [N, h*w, h*w] scores in memory) and "flash" (insv2v_attention at head_dim = 512) - with N = the frames one VAE call batches
at that frame size:  milliseconds per call (device events; both forms warmed, then timed alternately in the same process, median of the
rounds with the range) and torch.cuda.max_memory_allocated above the pre-call baseline.  With --decode: one VAE decode call of the same N
frames at 720p / 1080p and the block's share of it.

    python tools/bench_vae_attn.py [--decode] [--rounds 3] > profiles/vae_flash_attn.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "instruct-video-to-video_amd")]
import torch  # noqa: E402
from insv2v import synth, shapes, vae as V  # noqa: E402

dev = torch.device("cuda:0")
C = 512
# latent h x w -> h*w: the benched geometries (C2, C5), the first default-flash size, 720p, 1080p, and one beyond the score path's window
GEOMS = [(32, 48), (48, 64), (64, 66), (90, 160), (135, 240), (128, 264)]


def events(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def measure(forms, rounds):
    """forms: {name: fn}.  Warm every form (twice), size the timed window to ~0.3 s per form from one timed call, then `rounds` rounds that
    alternate the forms.  Returns {name: (median ms, min, max, peak bytes)}."""
    res = {}
    iters = {}
    for name, fn in forms.items():
        fn(), fn()
        torch.cuda.synchronize()
        iters[name] = max(2, min(50, int(300.0 / max(events(fn, 1), 1e-3))))
    ms = {name: [] for name in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            ms[name].append(events(fn, iters[name]))
    for name, fn in forms.items():
        res[name] = (statistics.median(ms[name]), min(ms[name]), max(ms[name]), peak_of(fn))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decode", action="store_true", help="also time one VAE decode call at 720p and 1080p (synthetic full-width weights)")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_vae_attn.py needs a GPU"
    sd = synth.synth_state_dict(shapes.vae_shapes(**synth.VAE_FULL))
    full = V.AutoencoderKL(**synth.VAE_FULL, device=dev).load_state_dict(sd)
    key = "decoder.mid.attn_1"
    att = {"scores": V.VAttn(sd, key, C, dev, flash=False), "flash": V.VAttn(sd, key, C, dev, flash=True)}
    print(f"# {torch.cuda.get_device_name(0)}; VAttn C = {C}; ms = median of {a.rounds} alternating rounds [min .. max]; peak = max_memory_allocated above the baseline")
    print(f"# {'h x w':>9} {'h*w':>6} {'N':>3} | {'scores ms':>26} {'peak MB':>9} | {'flash ms':>26} {'peak MB':>9} | flash / scores   flash TFLOP/s")
    block_ms = {}
    for h, w in GEOMS:
        HW = h * w
        ns = [full._frames_per_call(8 * h, 8 * w)]
        if HW == 32400:
            ns.append(1)
        for N in ns:
            x = (torch.randn(N * HW, C, device=dev) * 1.5).half()
            forms = {}
            for name, m in att.items():
                try:
                    V.attn_plan(C, HW, m.flash)
                except ValueError:
                    continue
                forms[name] = (lambda m=m: m(x, (N, h, w)))
            r = measure(forms, a.rounds)
            cell = lambda k: (f"{r[k][0]:9.3f} [{r[k][1]:7.3f} ..{r[k][2]:8.3f}] {r[k][3] / 2 ** 20:9.1f}" if k in r else f"{'refused (window)':>26} {'-':>9}")
            ratio = f"{r['flash'][0] / r['scores'][0]:6.2f}" if "scores" in r else "     -"
            tf = 4.0 * N * HW * HW * C / (r["flash"][0] * 1e-3) / 1e12     # the two contractions of the attention alone, over the whole block's time
            print(f"  {h:>4}x{w:<4} {HW:>6} {N:>3} | {cell('scores')} | {cell('flash')} | {ratio}           {tf:7.1f}")
            block_ms[(HW, N)] = {k: v[0] for k, v in r.items()}
            del x
            torch.cuda.empty_cache()
    if a.decode:
        print("# one VAE decode call (default dispatch: flash above 4096 tokens) and the mid AttnBlock's share of it")
        for h, w in ((90, 160), (135, 240)):
            N = full._frames_per_call(8 * h, 8 * w)
            z = torch.randn(N, 4, h, w)
            fn = lambda: full.decode(z)
            r = measure({"decode": fn}, a.rounds)["decode"]
            b = block_ms[(h * w, N)]
            print(f"  {8 * h}x{8 * w} N = {N}: decode {r[0]:9.2f} ms [{r[1]:.2f} .. {r[2]:.2f}] = {r[0] / N:8.2f} ms per frame; AttnBlock flash {b['flash']:8.3f} ms = "
                  f"{100 * b['flash'] / r[0]:5.1f} %"
                  + (f"; with the score form {b['scores']:8.3f} ms = {100 * b['scores'] / (r[0] - b['flash'] + b['scores']):5.1f} % of that decode" if "scores" in b else ""))


if __name__ == "__main__":
    main()
