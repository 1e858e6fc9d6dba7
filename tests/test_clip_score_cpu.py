"""CLIP scoring, the parts that need no GPU: the float64 restatement (tests/clip_score_ref.py) against torch's own bicubic resize and
cosine similarity, planted mistakes that the comparison must catch, the committed goldens against the restatement, the OpenAI <->
transformers key map, the CLI and the C ABI additions."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "instruct-video-to-video_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import clip_score_ref as R  # noqa: E402

# (H, W, S): upscale, non-square downscale (both directions at once), identity, odd sizes with border taps on every side, the real patch grid
GEOMETRIES = [(8, 8, 28), (40, 72, 28), (28, 28, 28), (15, 9, 28), (64, 96, 224)]
FRONT_TOL = 1e-5


def _frames(H, W, n=2):
    g = torch.Generator().manual_seed(H * 1000 + W)
    return torch.rand((n, 3, H, W), generator=g, dtype=torch.float64)


def _torch_front_end(x, S):
    """clip_similarity.py:29-31 with torch's own kernels, in float64."""
    img = F.interpolate(x, size=S, mode="bicubic", align_corners=False)
    m, s = torch.tensor(R.CLIP_MEAN, dtype=torch.float64), torch.tensor(R.CLIP_STD, dtype=torch.float64)
    return (img - m[None, :, None, None]) / s[None, :, None, None]


@pytest.mark.parametrize("H,W,S", GEOMETRIES)
def test_front_end_matches_torch_bicubic(H, W, S):
    x = _frames(H, W)
    err = (R.front_end(x, S) - _torch_front_end(x, S)).abs().max().item()
    print(f"[parity] front end {H}x{W} -> {S}: max abs err vs F.interpolate {err:.3e}")
    assert err <= FRONT_TOL
    # the affine map of frames in [-1, 1]
    err = (R.front_end(x * 2 - 1, S, 0.5, 0.5) - _torch_front_end(x, S)).abs().max().item()
    assert err <= FRONT_TOL
    if (H, W) == (S, S):   # identity: the normalised input itself
        m, s = torch.tensor(R.CLIP_MEAN, dtype=torch.float64), torch.tensor(R.CLIP_STD, dtype=torch.float64)
        assert (R.front_end(x, S) - (x - m[None, :, None, None]) / s[None, :, None, None]).abs().max().item() <= 1e-12


MUTATIONS = {
    "A = -0.5": dict(A=-0.5),
    "align_corners mapping": dict(align_corners=True),
    "clamped source coordinate": dict(clamp_coord=True),
    "result clamped to [0, 1]": dict(clamp_result=True),
    "mean / std swapped between channels": dict(mean=R.CLIP_MEAN[::-1], std=R.CLIP_STD[::-1]),
}


@pytest.mark.parametrize("what", list(MUTATIONS))
def test_planted_front_end_mistakes_are_caught(what):
    """Each classic mistake moves the front end past the bound at the resampling geometries (the identity resample cannot see A, the
    mapping or the clamps - its weights are (0, 1, 0, 0) - so it is not asked to; a pure downscale never has a source coordinate outside
    the image - (dst + 0.5) * in / out - 0.5 >= 0 for in >= out - so the clamped coordinate is asked of the geometries that upscale)."""
    for H, W, S in GEOMETRIES:
        if (H, W) == (S, S) and "swapped" not in what:
            continue
        if "coordinate" in what and H >= S and W >= S:
            continue
        x = _frames(H, W)
        err = (R.front_end(x, S, **MUTATIONS[what]) - _torch_front_end(x, S)).abs().max().item()
        assert err > 100 * FRONT_TOL, f"{what} at {H}x{W} -> {S}: only {err:.3e}"


def test_patch_rows_are_the_flattened_conv_weight_order():
    px = torch.randn((2, 3, 28, 28), dtype=torch.float64)
    w = torch.randn((5, 3, 14, 14), dtype=torch.float64)
    rows = R.patch_rows(px, 14, ld=640)
    assert rows.shape == (8, 640) and rows[:, 588:].abs().max() == 0
    ref = F.conv2d(px, w, stride=14).flatten(2).transpose(1, 2).reshape(8, 5)   # transformers' CLIPVisionEmbeddings
    assert (rows[:, :588] @ w.reshape(5, -1).T - ref).abs().max() < 1e-10


def test_scores_restate_torch_cosine_similarity():
    g = torch.Generator().manual_seed(3)
    n, D = 5, 32
    a, b = torch.randn((n, D), generator=g, dtype=torch.float64), torch.randn((n, D), generator=g, dtype=torch.float64)
    s, t = torch.randn((D,), generator=g, dtype=torch.float64), torch.randn((D,), generator=g, dtype=torch.float64)
    nz = lambda v: v / v.norm(dim=-1, keepdim=True)
    out = R.scores(a, b, s, t)
    an, bn, sn, tn = nz(a), nz(b), nz(s)[None].expand(n, -1), nz(t)[None].expand(n, -1)
    want = torch.stack([F.cosine_similarity(an, sn), F.cosine_similarity(bn, tn), F.cosine_similarity(bn - an, tn - sn),
                        F.cosine_similarity(an, bn), torch.cat([F.cosine_similarity(bn[:-1], bn[1:]), torch.zeros(1, dtype=torch.float64)])], 1)
    assert (out - want).abs().max().item() < 1e-14
    assert out[-1, 4] == 0
    # the clamping rule of the installed torch: each norm on its own (restated in clip_score_ref.cosine)
    x, y = torch.tensor([[1e-9, 0.0]], dtype=torch.float64), torch.tensor([[1e3, 0.0]], dtype=torch.float64)
    assert abs(F.cosine_similarity(x, y).item() - 0.1) < 1e-12 and abs(R.cosine(x, y).item() - 0.1) < 1e-12
    # img0 == img1: the direction has no length; torch's eps rule gives a finite 0, not nan
    same = R.scores(a, a, s, t)
    assert torch.isfinite(same).all() and same[:, 2].abs().max() == 0 and (same[:, 3] - 1).abs().max() < 1e-14
    assert torch.equal(torch.nan_to_num(F.cosine_similarity(an - an, tn - sn)), same[:, 2])


def _configs(name):
    from insv2v import synth
    return (synth.CLIP_VISION_TINY, synth.CLIP_TINY) if name == "tiny" else (synth.CLIP_VISION_FULL, synth.CLIP_FULL)


def _state_dict(name):
    from insv2v import shapes, synth
    vis, txt = _configs(name)
    sd = synth.synth_state_dict(shapes.clip_vision_shapes(**vis))
    sd.update(synth.synth_state_dict(shapes.clip_text_shapes(**dict(txt, prefix="text_model.", with_projection=True))))
    return sd


def _golden(name):
    return dict(np.load(os.path.join(HERE, "golden", f"clip_score_{name}.npz")))


@pytest.mark.parametrize("name", ["tiny", "full"])
def test_goldens_match_the_restatement(name):
    """The committed outputs of the real transformers models vs the float64 restatement, 2e-5 as tools/gen_golden.py: case_clip_text."""
    g = _golden(name)
    vis, txt = _configs(name)
    sd = _state_dict(name)
    src = torch.from_numpy(g["src_frames"])
    assert src.dtype == torch.float16 and tuple(src.shape) == (4, 3, 40, 72)
    px = R.front_end(src[:1], vis["image_size"], 0.5, 0.5)
    pref = torch.from_numpy(g["pixels0"]).double()
    assert (px[0] - pref).abs().max().item() <= 1e-5 * max(1.0, pref.abs().max().item())   # (the stored pixels are torch's fp32 resize)
    nfr = 4 if name == "tiny" else 1   # (one frame of the 24-layer tower keeps this CPU test quick; the generator checked all of them)
    emb = R.vision_forward(sd, R.front_end(src[:nfr], vis["image_size"], 0.5, 0.5), vis)
    ref = torch.from_numpy(g["image_embeds_src"][:nfr]).double()
    assert (emb - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    temb = R.text_forward(sd, torch.from_numpy(g["input_ids"]).long(), txt)
    tref = torch.from_numpy(g["text_embeds"]).double()
    assert (temb - tref).abs().max().item() <= 2e-5 * max(1.0, tref.abs().max().item())
    sc = R.scores(torch.from_numpy(g["image_embeds_src"]), torch.from_numpy(g["image_embeds_edit"]), tref[0], tref[1])
    assert (sc - torch.from_numpy(g["scores"])).abs().max().item() <= 1e-12
    # the input condition of the end-to-end GPU test holds on the reference itself
    nz = lambda v: v / v.norm(dim=-1, keepdim=True)
    gap = (nz(torch.from_numpy(g["image_embeds_edit"]).double()) - nz(torch.from_numpy(g["image_embeds_src"]).double())).norm(dim=-1)
    assert gap.min().item() >= 0.2 and (nz(tref[1]) - nz(tref[0])).norm().item() >= 0.2


def test_live_transformers_agrees_with_the_restatement():
    """The tiny towers against the installed transformers (skipped where it is absent; the goldens pin the same thing everywhere)."""
    tr = pytest.importorskip("transformers")
    vis, txt = _configs("tiny")
    sd = _state_dict("tiny")
    try:
        hv = tr.CLIPVisionModelWithProjection(tr.CLIPVisionConfig(**vis, hidden_act="quick_gelu")).eval()
        ht = tr.CLIPTextModelWithProjection(tr.CLIPTextConfig(**txt, hidden_act="quick_gelu", eos_token_id=2, bos_token_id=0, pad_token_id=1)).eval()
    except Exception as e:   # an optional dependency of transformers that the test environment shadows
        pytest.skip(f"transformers cannot build its CLIP models here: {e}")
    hv.load_state_dict({k: v for k, v in sd.items() if k.startswith("vision_model.") or k.startswith("visual_projection.")}, strict=True)
    ht.load_state_dict({k: v for k, v in sd.items() if k.startswith("text_model.") or k.startswith("text_projection.")}, strict=True)
    from insv2v import synth
    px = R.front_end(_frames(15, 9, 3), 28)
    ids = synth.synth_token_ids("clip_score.live", 3, 77, txt["vocab_size"], salt=1)
    with torch.no_grad():
        e, t = hv(pixel_values=px.float()).image_embeds, ht(input_ids=ids).text_embeds
    assert (R.vision_forward(sd, px, vis) - e).abs().max().item() <= 2e-5 * max(1.0, e.abs().max().item())
    assert (R.text_forward(sd, ids, txt) - t).abs().max().item() <= 2e-5 * max(1.0, t.abs().max().item())


def test_openai_layout_maps_back_key_for_key():
    from insv2v.clip_vision import is_openai_layout, openai_to_transformers
    sd = _state_dict("tiny")
    oa = R.transformers_to_openai(sd)
    assert is_openai_layout(oa) and not is_openai_layout(sd)
    assert "visual.transformer.resblocks.1.attn.in_proj_weight" in oa and "transformer.resblocks.0.mlp.c_fc.bias" in oa
    assert tuple(oa["visual.proj"].shape) == (64, 32) and tuple(oa["text_projection"].shape) == (64, 32)   # stored [width, embed]
    back = openai_to_transformers(dict(oa, input_resolution=torch.tensor(28), context_length=torch.tensor(77), vocab_size=torch.tensor(1000),
                                       logit_scale=torch.tensor(4.6)))
    assert back.pop("logit_scale").item() == pytest.approx(4.6)
    assert set(back) == set(sd)
    for k in sd:
        assert back[k].shape == sd[k].shape and torch.equal(back[k], sd[k]), k
    for bad in ("visual.transformer.resblocks.0.attn.rel_pos", "visual.attnpool.k_proj.weight", "unknown.weight", "transformer.resblocks.x.ln_1.weight"):
        with pytest.raises(KeyError, match="OpenAI CLIP layout"):
            openai_to_transformers(dict(oa, **{bad: torch.zeros(1)}))


def test_shapes_and_synth_keep_existing_keys():
    from insv2v import shapes, synth
    v = shapes.clip_vision_shapes(**synth.CLIP_VISION_TINY)
    assert v["vision_model.embeddings.position_embedding.weight"] == (5, 64) and v["visual_projection.weight"] == (32, 64)
    assert v["vision_model.embeddings.patch_embedding.weight"] == (64, 3, 14, 14) and "vision_model.pre_layrnorm.weight" in v
    full = shapes.clip_vision_shapes(**synth.CLIP_VISION_FULL)
    assert full["vision_model.embeddings.position_embedding.weight"] == (257, 1024) and full["visual_projection.weight"] == (768, 1024)
    assert sum(1 for k in full if k.endswith("mlp.fc1.weight")) == 24
    assert synth.CLIP_FULL["projection_dim"] == 768 and synth.CLIP_TINY["projection_dim"] == 32
    # the text configs carry their projection width, the state dict of the embedder (and so its goldens) is what it was
    t = shapes.clip_text_shapes(**synth.CLIP_TINY)
    assert "text_projection.weight" not in t and len(t) == 2 + 16 * 2 + 2
    assert shapes.clip_text_shapes(**dict(synth.CLIP_TINY, with_projection=True))["text_projection.weight"] == (32, 64)
    # the two new norms get gammas around 1; a key that is no norm keeps its value
    w = synth.synth_tensor("vision_model.pre_layrnorm.weight", (64,))
    assert abs(w.mean().item() - 1) < 0.1 and abs(synth.synth_tensor("vision_model.post_layernorm.weight", (64,)).mean().item() - 1) < 0.1
    g = torch.Generator().manual_seed(__import__("zlib").crc32(b"mid_block.attentions.0.proj_in.bias") & 0x7FFFFFFF)
    assert torch.equal(synth.synth_tensor("mid_block.attentions.0.proj_in.bias", (8,)), 0.1 * torch.randn((8,), generator=g))


def test_cli():
    from insv2v.run_loveu_tgve import build_parser, check_args
    p = build_parser()
    a = check_args(p.parse_args([]))
    assert a.score_ckpt is None and a.score_out is None and a.score_synthetic is False and a.score_name == "ViT-L/14" and a.synthetic_tiny is False
    a = check_args(p.parse_args(["--score-ckpt", "clip.pt", "--score-out", "s.json"]))
    assert (a.score_ckpt, a.score_out) == ("clip.pt", "s.json")
    a = check_args(p.parse_args(["--synthetic", "2", "--score-synthetic", "--score-out", "s.json", "--synthetic-tiny"]))
    assert a.score_synthetic and a.synthetic_tiny
    with pytest.raises(SystemExit, match="--score-out needs a scorer"):
        check_args(p.parse_args(["--score-out", "s.json"]))
    with pytest.raises(SystemExit, match="--score-out needs a scorer"):
        check_args(p.parse_args(["--synthetic", "2", "--score-out", "s.json"]))
    with pytest.raises(SystemExit, match="--score-synthetic needs --synthetic"):
        check_args(p.parse_args(["--score-synthetic", "--score-out", "s.json"]))
    with pytest.raises(SystemExit, match="need --score-out"):
        check_args(p.parse_args(["--score-ckpt", "clip.pt"]))
    with pytest.raises(SystemExit, match="two scorers"):
        check_args(p.parse_args(["--synthetic", "1", "--score-synthetic", "--score-ckpt", "c.pt", "--score-out", "s.json"]))
    with pytest.raises(SystemExit, match="--synthetic-tiny"):
        check_args(p.parse_args(["--synthetic-tiny"]))


def test_clip_similarity_names():
    from insv2v import clip_score
    assert clip_score.NAMES == ("RN50", "RN101", "RN50x4", "RN50x16", "RN50x64", "ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px")
    assert clip_score.VIT_CONFIGS["ViT-L/14@336px"][0]["image_size"] == 336 and clip_score.VIT_CONFIGS["ViT-L/14"][0]["image_size"] == 224
    for rn in clip_score.NAMES[:5]:
        with pytest.raises(NotImplementedError, match="ResNet"):
            clip_score.ClipSimilarity(name=rn, device="cpu")
    with pytest.raises(ValueError):
        clip_score.ClipSimilarity(name="ViT-H/14", device="cpu")
    s = clip_score.ClipSimilarity(name="ViT-L/14@336px", device="cpu")
    assert s.size == 336
    with pytest.raises(RuntimeError, match="tokenizer"):
        s.encode_text(["no tokenizer offline"])


def _c_struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(void|float|int64_t|int32_t)\s*(\*?)\s*(.*)", decl)
        ctype = "ptr" if m.group(3) or "*" in m.group(4) else m.group(2)
        for var in m.group(4).split(","):
            var = var.strip().lstrip("*").strip()
            arr = re.fullmatch(r"(\w+)\[(\d+)\]", var)
            fields.append((arr.group(1), ctype, int(arr.group(2))) if arr else (var, ctype, 0))
    return fields


def test_abi_additions():
    from insv2v import _lib
    header = open(os.path.join(ROOT, "include", "insv2v_hip.h")).read()
    assert _lib.ABI_VERSION == 15
    i32, i64, f32, p = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    want = {
        "insv2v_clip_preprocess": (i32, [ctypes.POINTER(_lib.ClipPreprocessDesc), p]),
        "insv2v_clip_scores": (i32, [p, p, p, p, i32, i64, i64, i64, i32, i32, f32, p, p]),
        "insv2v_l2_normalize": (i32, [p, i32, i64, p, i64, i32, i32, p]),
    }
    kind = {"void": p, "float": f32, "int64_t": i64, "int32_t": i32, "insv2v_stream_t": p}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig
        proto = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.S | re.M).group(1)
        args = []
        for a in proto.split(","):
            a = a.strip()
            args.append(p if "*" in a else kind[re.sub(r"^const\s+", "", a).split()[0]])
        if name == "insv2v_clip_preprocess":
            args[0] = sig[1][0]
        assert args == sig[1], name
    py = []
    for n, t in _lib.ClipPreprocessDesc._fields_:
        py.append((n, "float", t._length_) if hasattr(t, "_length_") else (n, {p: "ptr", i64: "int64_t", i32: "int32_t", f32: "float"}[t], 0))
    assert py == _c_struct_fields(header, "insv2v_clip_preprocess_desc")
    assert ctypes.sizeof(_lib.ClipPreprocessDesc) == 2 * 8 + 5 * 8 + 6 * 4 + 2 * 4 + 6 * 4
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for name in want:
            assert getattr(lib, name) is not None
