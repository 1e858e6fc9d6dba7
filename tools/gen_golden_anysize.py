#!/usr/bin/env python3
"""Generate the any-frame-size fixtures under tests/golden/ by running the UNMODIFIED reference on CPU.

Built like tools/gen_golden.py: same sys.path recipe (the reference tree plus the stand-ins of tests/oracle_shim for its missing
third-party leaves), weights regenerated from crc32(key) by insv2v.synth and never stored, outputs only (float32).  It runs only where
the reference tree is present (INSV2V_REFERENCE, default /root/reference).  The oracle restatement is NOT consulted here: oracle/unet3d.py
never learnt `upsample_size` and cannot run latents whose sides are not multiples of 8, so the expected values are the reference's own.

  unet_tiny_anysize.npz   tiny-UNet forwards at latents (2,8,4,20,14) [H even down to 5 and cropped on the way up, W cropped at another
                          level: 14 -> 7 -> 4 -> 2], (1,8,5,18,22) with video_start_index = 3 [both sides odd at level 1] and a
                          3-sample branch-major input (3,8,4,12,20) whose samples 1 and 2 carry the same latent (the shared CFG prefix);
                          plus the size table of the planning helper: per-level sizes the reference's tensors had, read with forward hooks
  vae_tiny_anysize.npz    VAE_TINY encoder output (mean path: the moments) and decoder output at image 40x56 (latent 5x7, h*w = 35)
  pipelines_anysize.npz   4-step DDIM InferenceIP2PVideo.__call__ (text 7.5 / image 1.5: latent and all_pred[-1]) and 4-step
                          second_clip_forward (R = 2, noise_correct_step = 0.5) on the tiny UNet at latent [1,6,4,20,14]
  unet_full_anysize.npz   full-width UNet forward of a branch-major CFG triple (3,8,16,9,8): the row kernels' dispatch at a ragged size
  blocks_anysize.npz      one Upsample3D at 1280 channels, input 5x7, output_size 9x14, one image (fp16 storage, as blocks_wide.npz)

usage: python tools/gen_golden_anysize.py [--only NAME]
The committed files were written with GOLDEN_THREADS=16 (torch.set_num_threads(16)); another thread count changes fp32 summation order
inside torch's CPU kernels by ~1e-6 of the values.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("INSV2V_REFERENCE", "/root/reference")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "oracle_shim"), REF,
                os.path.join(ROOT, "instruct-video-to-video_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from insv2v import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)

# latents whose per-level sizes are recorded for the size-planning helper (insv2v.unet.plan_sizes)
SIZE_TABLE = [(45, 80), (60, 106), (20, 14), (18, 22), (12, 20), (45, 45), (90, 160), (16, 24), (1, 1), (5, 7)]


def save(name, **arrs):
    out = {k: (v.detach().cpu().numpy().astype(np.float32) if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    np.savez(os.path.join(GOLD, name + ".npz"), **out)
    print(f"  wrote {name}.npz ({sum(a.nbytes for a in out.values()) / 1e3:.0f} KB)")


def load_synth(module, prefix=""):
    sd = {k: synth.synth_tensor(prefix + k, v) for k, v in module.state_dict().items()}
    module.load_state_dict(sd)
    return module.eval()


def ref_unet():
    from modules.video_unet_temporal.unet import UNet3DConditionModel as RefUNet
    return load_synth(RefUNet(**synth.UNET_TINY))


def level_sizes(unet, H, W):
    """(h, w) of the tensor every down block receives and of the tensor every upsampler produces, read from the running reference."""
    down, up, hooks = [], [], []
    for blk in unet.down_blocks:
        hooks.append(blk.register_forward_pre_hook(lambda m, args, kw: down.append(tuple((args[0] if args else kw["hidden_states"]).shape[-2:])),
                                                   with_kwargs=True))
    for blk in unet.up_blocks:
        if getattr(blk, "upsamplers", None):
            hooks.append(blk.upsamplers[0].register_forward_hook(lambda m, args, out: up.append(tuple(out.shape[-2:]))))
    x = torch.zeros(1, 8, 1, H, W)
    unet(x, torch.zeros(1, dtype=torch.long), encoder_hidden_states=torch.zeros(1, 2, 64))
    for h in hooks:
        h.remove()
    return down, up


def case_unet():
    unet = ref_unet()
    out = {}
    x = synth.synth_input("anysize.a.sample", (2, 8, 4, 20, 14))
    ctx = synth.synth_input("anysize.a.ctx", (2, 77, 64))
    out["a"] = unet(x, torch.full((2,), 481, dtype=torch.long), encoder_hidden_states=ctx).sample
    x = synth.synth_input("anysize.b.sample", (1, 8, 5, 18, 22))
    ctx = synth.synth_input("anysize.b.ctx", (1, 77, 64))
    out["b"] = unet(x, torch.full((1,), 481, dtype=torch.long), encoder_hidden_states=ctx, video_start_index=3).sample
    # branch-major CFG triple: (no text, no video) / (no text, video) / (text, video) - samples 1 and 2 share the latent, 0 and 1 the text
    lat = synth.synth_input("anysize.c.latent", (1, 4, 4, 12, 20))
    cond = synth.synth_input("anysize.c.cond", (1, 4, 4, 12, 20))
    tu, tc = synth.synth_input("anysize.c.tu", (1, 77, 64)), synth.synth_input("anysize.c.tc", (1, 77, 64))
    x = torch.cat([torch.cat([lat, torch.zeros_like(cond)], 1), torch.cat([lat, cond], 1), torch.cat([lat, cond], 1)], 0)
    out["c"] = unet(x, torch.full((3,), 481, dtype=torch.long), encoder_hidden_states=torch.cat([tu, tu, tc], 0)).sample
    for k, v in out.items():
        assert torch.isfinite(v).all()
        print(f"  {k}: {tuple(v.shape)} max|y| = {v.abs().max().item():.3f}")
    table = []
    for H, W in SIZE_TABLE:
        down, up = level_sizes(unet, H, W)
        assert len(down) == 4 and len(up) == 3
        table.append([H, W] + [s for hw in down for s in hw] + [s for hw in up for s in hw])
    out["size_table"] = np.asarray(table, dtype=np.int32)   # rows: H, W, 4 x (h, w) down, 3 x (h, w) upsampler outputs
    save("unet_tiny_anysize", **out)


def case_vae():
    from modules.vqvae.model import Encoder as RefEnc, Decoder as RefDec
    from insv2v import shapes
    dd = synth.VAE_TINY["ddconfig"]
    sd = synth.synth_state_dict(shapes.vae_shapes(**synth.VAE_TINY))
    renc, rdec = RefEnc(**dd).eval(), RefDec(**dd).eval()
    renc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
    rdec.load_state_dict({k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.")})
    x = synth.synth_input("anysize.vae.x", (2, 3, 40, 56), kind="uniform")
    h = renc(x)
    moments = torch.nn.functional.conv2d(h, sd["quant_conv.weight"], sd["quant_conv.bias"])      # autoencoder.py:89-93
    assert moments.shape == (2, 8, 5, 7)
    z = synth.synth_input("anysize.vae.z", (1, 4, 5, 7))
    dec = rdec(torch.nn.functional.conv2d(z, sd["post_quant_conv.weight"], sd["post_quant_conv.bias"]))   # autoencoder.py:97-100
    assert dec.shape == (1, 3, 40, 56)
    save("vae_tiny_anysize", moments=moments, dec=dec)


def case_pipelines():
    import pl_trainer.inference.inference as ref_inf
    unet = ref_unet()
    F, h, w, R = 6, 20, 14, 2
    lat = synth.synth_input("anysize.pipe.latent", (1, F, 4, h, w))
    cond = synth.synth_input("anysize.pipe.cond", (1, F, 4, h, w))
    tc = synth.synth_input("anysize.pipe.text_cond", (1, 77, 64))
    tu = synth.synth_input("anysize.pipe.text_uncond", (1, 77, 64))
    lref = synth.synth_input("anysize.pipe.latent_ref", (1, R, 4, h, w))
    rp = ref_inf.InferenceIP2PVideo(unet, scheduler="ddim", num_ddim_steps=4)
    r = rp(lat, tc, tu, cond, text_cfg=7.5, img_cfg=1.5)
    out = {"ddim4_latent": r["latent"], "ddim4_pred_last": r["all_pred"][-1]}
    r = rp.second_clip_forward(lat, tc, tu, cond, latent_ref=lref, noise_correct_step=0.5, text_cfg=7.5, img_cfg=1.5)
    out["second_clip_latent"] = r["latent"]
    save("pipelines_anysize", **out)


def case_blocks():
    from modules.video_unet_temporal.resnet import Upsample3D
    up = load_synth(Upsample3D(1280, use_conv=True, out_channels=1280), "up1280.")
    x = synth.synth_input("up1280.x", (1, 1280, 1, 5, 7))
    y = up(x, output_size=(1, 9, 14))   # the reference's UNet hands over the skip's shape[2:] of a 5-D tensor: (f, h, w)
    assert y.shape == (1, 1280, 1, 9, 14)
    save("blocks_anysize", up1280=y.half().numpy())


def case_unet_full():
    """Full width: a branch-major CFG triple of 16 frames at latent 9x8 (72 and 20 pixels per frame at the row-kernel levels: samples of 1152
    and 320 rows in the fused text cross-attention's 128-row tiles, ragged 32-row wave blocks in the GroupNorm fold; every upsampler crops
    its rows: 2 -> 3 -> 5 -> 9)."""
    from modules.video_unet_temporal.unet import UNet3DConditionModel as RefUNet
    unet = load_synth(RefUNet(**synth.UNET_FULL))
    lat = synth.synth_input("anysize.full.latent", (1, 4, 16, 9, 8))   # [b, c, f, h, w]
    cond = synth.synth_input("anysize.full.cond", (1, 4, 16, 9, 8))
    tu, tc = synth.synth_input("anysize.full.tu", (1, 77, 768)), synth.synth_input("anysize.full.tc", (1, 77, 768))
    x = torch.cat([torch.cat([lat, torch.zeros_like(cond)], 1), torch.cat([lat, cond], 1), torch.cat([lat, cond], 1)], 0)
    t0 = time.time()
    y = unet(x, torch.full((3,), 481, dtype=torch.long), encoder_hidden_states=torch.cat([tu, tu, tc], 0)).sample
    print(f"  reference full-width forward (3,8,16,9,8) {time.time() - t0:.0f}s, max|y| = {y.abs().max().item():.3f}")
    assert torch.isfinite(y).all()
    save("unet_full_anysize", out=y)


CASES = dict(unet=case_unet, vae=case_vae, pipelines=case_pipelines, blocks=case_blocks, unet_full=case_unet_full)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    os.makedirs(GOLD, exist_ok=True)
    torch.set_num_threads(int(os.environ.get("GOLDEN_THREADS", 16)))
    for name, fn in CASES.items():
        if a.only and a.only != name:
            continue
        t0 = time.time()
        print(f"[{name}]")
        fn()
        print(f"  done in {time.time() - t0:.1f}s")
