#!/usr/bin/env python3
"""Generate tests/golden/clip_score_{tiny,full}.npz: the REAL transformers ``CLIPVisionModelWithProjection`` and
``CLIPTextModelWithProjection`` (third party, needed here and only here) on key-hashed weights, behind the reference's own pixel front end
(F.interpolate bicubic + mean / std, misc_utils/clip_similarity.py:29-31).  The float64 restatement tests/clip_score_ref.py runs on the
same inputs and must agree to 2e-5, which is how the restatement is pinned (the figure tools/gen_golden.py: case_clip_text uses).

Weights are never stored (insv2v.synth regenerates them from crc32(key)); the files hold small inputs and outputs only: two 4-frame clips
at 40 x 72 (source and "edit": one noise image under a brightness ramp and the reversed ramp, stored as the fp16 values every side reads),
two prompts' token ids, the preprocessed pixels of source frame 0, the image / text embeddings and the scores.

The gains are chosen so that the directional score is a meaningful test: it divides by |f1 - f0|, so its error is ~ 2 eps / gap for a
feature error eps; asserted here and again by the GPU test: every frame has |f1 - f0| >= 0.2 and |t1 - t0| >= 0.2, and the cosines of
consecutive frames differ from 1 and from the skip-two cosines (an off-by-one in the frame pairing is visible).

usage: python tools/gen_golden_clip_score.py [--only tiny|full]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "instruct-video-to-video_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from insv2v import shapes, synth  # noqa: E402
import clip_score_ref as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_grad_enabled(False)

# per config: the brightness ramp of the source clip (the edit runs it backwards)
GAINS = {"full": (1.0, 0.65, 0.38, 0.2), "tiny": (1.0, 0.55, 0.25, 0.08)}
CONFIGS = {"tiny": (synth.CLIP_VISION_TINY, synth.CLIP_TINY), "full": (synth.CLIP_VISION_FULL, synth.CLIP_FULL)}


def import_transformers():
    """transformers must not see the torchvision stand-in of tests/oracle_shim while it probes its optional dependencies."""
    shim = os.path.join(ROOT, "tests", "oracle_shim")
    saved_path = list(sys.path)
    saved_mods = {m: sys.modules[m] for m in list(sys.modules) if m == "torchvision" or m.startswith("torchvision.")}
    sys.path[:] = [p for p in sys.path if os.path.abspath(p) != shim]
    for m in saved_mods:
        del sys.modules[m]
    try:
        import transformers as tr
        tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(hidden_size=8, intermediate_size=8, num_hidden_layers=1, num_attention_heads=1,
                                                             image_size=4, patch_size=2, projection_dim=4))   # lazy sub-imports happen here
        tr.CLIPTextModelWithProjection(tr.CLIPTextConfig(vocab_size=8, hidden_size=8, intermediate_size=8, num_hidden_layers=1,
                                                         num_attention_heads=1, projection_dim=4))
    finally:
        sys.path[:] = saved_path
        for m in [m for m in sys.modules if m == "torchvision" or m.startswith("torchvision.")]:
            del sys.modules[m]
        sys.modules.update(saved_mods)
    return tr


def state_dicts(vis, txt):
    sd = synth.synth_state_dict(shapes.clip_vision_shapes(**vis))
    sd.update(synth.synth_state_dict(shapes.clip_text_shapes(**dict(txt, prefix="text_model.", with_projection=True))))
    return sd


def check(tag, ref, ours, tol=2e-5):
    err = (ref.double() - ours.double()).abs().max().item()
    scale = ref.abs().max().item()
    print(f"  {tag}: max|transformers - restatement| = {err:.3e} (max {scale:.3f})")
    assert err <= tol * max(1.0, scale), f"the restatement disagrees with transformers on {tag}"


def case(name, tr):
    vis, txt = CONFIGS[name]
    sd = state_dicts(vis, txt)
    S = vis["image_size"]
    hv = tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(**vis, hidden_act="quick_gelu")).eval()
    hv.load_state_dict({k: v for k, v in sd.items() if k.startswith("vision_model.") or k.startswith("visual_projection.")}, strict=True)
    ht = tr.CLIPTextModelWithProjection(tr.CLIPTextConfig(**txt, hidden_act="quick_gelu", eos_token_id=2, bos_token_id=0, pad_token_id=1)).eval()
    ht.load_state_dict({k: v for k, v in sd.items() if k.startswith("text_model.") or k.startswith("text_projection.")}, strict=True)
    src = R.ramp_frames(name, GAINS[name]).half()
    edit = R.ramp_frames(name, GAINS[name], reverse=True).half()
    ids = synth.synth_token_ids("clip_score." + name, 2, 77, txt["vocab_size"])

    def reference_pixels(frames):   # clip_similarity.py:29-31 on the frames mapped to [0, 1]
        img = F.interpolate(frames.float() * 0.5 + 0.5, size=S, mode="bicubic", align_corners=False)
        return (img - torch.tensor(R.CLIP_MEAN)[None, :, None, None]) / torch.tensor(R.CLIP_STD)[None, :, None, None]

    emb, ours = {}, {}
    for tag, frames in (("src", src), ("edit", edit)):
        px = reference_pixels(frames)
        px64 = R.front_end(frames, S, 0.5, 0.5)
        check(f"{name} {tag} pixels", px, px64, tol=1e-5)
        emb[tag] = hv(pixel_values=px).image_embeds
        ours[tag] = R.vision_forward(sd, px64, vis)
        check(f"{name} {tag} image_embeds", emb[tag], ours[tag])
    temb = ht(input_ids=ids).text_embeds
    tours = R.text_forward(sd, ids, txt)
    check(f"{name} text_embeds", temb, tours)
    sc = R.scores(emb["src"], emb["edit"], temb[0], temb[1])
    check(f"{name} scores", sc, R.scores(ours["src"], ours["edit"], tours[0], tours[1]), tol=2e-4)
    # the input condition of the end-to-end test, on the reference itself
    nz = lambda v: v.double() / v.double().norm(dim=-1, keepdim=True)
    gap = (nz(emb["edit"]) - nz(emb["src"])).norm(dim=-1)
    tgap = (nz(temb[1]) - nz(temb[0])).norm().item()
    b = nz(emb["edit"])
    skip2 = R.cosine(b[:-2], b[2:])
    print(f"  {name}: image gaps {[round(v, 3) for v in gap.tolist()]}, text gap {tgap:.3f}")
    print(f"  {name}: consecutive cosines {[round(v, 4) for v in sc[:-1, 4].tolist()]}, skip-two {[round(v, 4) for v in skip2.tolist()]}")
    assert gap.min().item() >= 0.2 and tgap >= 0.2, "the gains do not separate source and edit: sim_direction would be ill-conditioned"
    out = dict(src_frames=src.numpy(), edit_frames=edit.numpy(), input_ids=ids.numpy(), pixels0=reference_pixels(src[:1])[0].numpy(),
               image_embeds_src=emb["src"].numpy(), image_embeds_edit=emb["edit"].numpy(), text_embeds=temb.numpy(), scores=sc.numpy())
    np.savez(os.path.join(GOLD, f"clip_score_{name}.npz"), **out)
    print(f"  wrote clip_score_{name}.npz ({sum(a.nbytes for a in out.values()) / 1e3:.0f} KB)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=("tiny", "full"))
    a = ap.parse_args()
    tr = import_transformers()
    for name in ("tiny", "full"):
        if a.only in (None, name):
            print(f"[{name}]")
            case(name, tr)
