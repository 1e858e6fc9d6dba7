"""float64 restatement (torch on the CPU) of what insv2v/clip_score.py computes: the bicubic pixel front end of
``ClipSimilarity.encode_image``, the CLIP image and text towers with their projections (transformers ``CLIPVisionModelWithProjection`` /
``CLIPTextModelWithProjection`` semantics, quick-GELU), and the scores.  tools/gen_golden_clip_score.py checks it against the real
transformers models; the tests check the HIP kernels against it.

``front_end`` takes its few constants as keywords so that tests can plant the classic mistakes (another A, the align_corners mapping, a
clamped coordinate, a clamped result, swapped channel statistics) and see the comparison with F.interpolate catch each of them.
"""
import math
import re

import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
F64 = torch.float64


def cubic_weights(t, A=-0.75):
    """The four cubic-convolution weights of taps floor(x) - 1 .. floor(x) + 2 for the fraction t (Keys; torch uses A = -0.75)."""
    def near(x):   # |x| <= 1
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def far(x):    # 1 < |x| < 2
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return torch.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], -1)


def _axis(n_in, n_out, A, align_corners, clamp_coord):
    """Per output index: the four clamped tap indices [n_out, 4] and weights [n_out, 4] of one axis."""
    dst = torch.arange(n_out, dtype=F64)
    if align_corners:
        src = dst * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        src = (dst + 0.5) * (n_in / n_out) - 0.5   # NOT clamped: bicubic extrapolates the coordinate, only the taps are clamped
    if clamp_coord:
        src = src.clamp(0, n_in - 1)
    fl = torch.floor(src)
    idx = (fl.long()[:, None] + torch.arange(-1, 3)[None]).clamp(0, n_in - 1)
    return idx, cubic_weights(src - fl, A)


def resize_bicubic(x, size, A=-0.75, align_corners=False, clamp_coord=False):
    """F.interpolate(x, size=(size, size), mode="bicubic", align_corners=False) for x [n, c, H, W], in float64."""
    x = x.to(F64)
    iy, wy = _axis(x.shape[2], size, A, align_corners, clamp_coord)
    ix, wx = _axis(x.shape[3], size, A, align_corners, clamp_coord)
    rows = (x[:, :, iy, :] * wy[None, None, :, :, None]).sum(3)          # [n, c, S, W]
    return (rows[:, :, :, ix] * wx[None, None, None, :, :]).sum(4)       # [n, c, S, S]


def front_end(frames, size, in_scale=1.0, in_shift=0.0, mean=CLIP_MEAN, std=CLIP_STD, A=-0.75, align_corners=False, clamp_coord=False,
              clamp_result=False):
    """frames [n,3,H,W] -> the normalised size x size pixels [n,3,size,size] float64 (clip_similarity.py:29-31 after the affine map of
    the frames to [0, 1])."""
    img = resize_bicubic(frames.to(F64) * in_scale + in_shift, size, A, align_corners, clamp_coord)
    if clamp_result:
        img = img.clamp(0, 1)
    m, s = torch.tensor(mean, dtype=F64), torch.tensor(std, dtype=F64)
    return (img - m[None, :, None, None]) / s[None, :, None, None]


def patch_rows(pixels, patch, ld=None):
    """[n,3,S,S] -> [n * (S/P)^2, ld]: row (frame, patch row, patch column), column c*P*P + py*P + px, zero pad columns."""
    n, c, S, _ = pixels.shape
    g = S // patch
    rows = pixels.reshape(n, c, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, c * patch * patch)
    if ld is not None and ld > rows.shape[1]:
        rows = torch.cat([rows, torch.zeros((rows.shape[0], ld - rows.shape[1]), dtype=rows.dtype)], 1)
    return rows


def _ln(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w + b


def _encoder(sd, p, x, layers, heads, causal):
    n, L, C = x.shape
    d = C // heads
    g = lambda k: sd[p + k].to(F64)
    for i in range(layers):
        q = f"encoder.layers.{i}."
        h = _ln(x, g(q + "layer_norm1.weight"), g(q + "layer_norm1.bias"))
        qkv = [(h @ g(q + f"self_attn.{t}_proj.weight").T + g(q + f"self_attn.{t}_proj.bias")).reshape(n, L, heads, d).transpose(1, 2) for t in "qkv"]
        s = qkv[0] @ qkv[1].transpose(-1, -2) * d ** -0.5
        if causal:
            s = s + torch.full((L, L), -math.inf, dtype=F64).triu(1)
        a = (torch.softmax(s, -1) @ qkv[2]).transpose(1, 2).reshape(n, L, C)
        x = x + a @ g(q + "self_attn.out_proj.weight").T + g(q + "self_attn.out_proj.bias")
        h = _ln(x, g(q + "layer_norm2.weight"), g(q + "layer_norm2.bias"))
        h = h @ g(q + "mlp.fc1.weight").T + g(q + "mlp.fc1.bias")
        h = h * torch.sigmoid(1.702 * h)
        x = x + h @ g(q + "mlp.fc2.weight").T + g(q + "mlp.fc2.bias")
    return x


def vision_forward(sd, pixels, cfg):
    """transformers layout state dict, normalised pixels [n,3,S,S] -> image_embeds [n, projection_dim] float64 (un-normalised)."""
    p, P = "vision_model.", cfg["patch_size"]
    C = cfg["hidden_size"]
    n = pixels.shape[0]
    w = sd[p + "embeddings.patch_embedding.weight"].to(F64).reshape(C, -1)
    x = (patch_rows(pixels.to(F64), P) @ w.T).reshape(n, -1, C)
    cls = sd[p + "embeddings.class_embedding"].to(F64).expand(n, 1, C)
    x = torch.cat([cls, x], 1) + sd[p + "embeddings.position_embedding.weight"].to(F64)[None]
    x = _ln(x, sd[p + "pre_layrnorm.weight"].to(F64), sd[p + "pre_layrnorm.bias"].to(F64))
    x = _encoder(sd, p, x, cfg["num_hidden_layers"], cfg["num_attention_heads"], causal=False)
    pooled = _ln(x[:, 0], sd[p + "post_layernorm.weight"].to(F64), sd[p + "post_layernorm.bias"].to(F64))
    return pooled @ sd["visual_projection.weight"].to(F64).T


def text_forward(sd, ids, cfg):
    """transformers layout state dict (``text_model.*``, ``text_projection.weight``), ids [n, L] -> text_embeds [n, projection_dim]
    float64 (un-normalised); the pooled token is the one with the highest id (the legacy eos_token_id == 2 pooling)."""
    p = "text_model."
    L = ids.shape[1]
    x = sd[p + "embeddings.token_embedding.weight"].to(F64)[ids] + sd[p + "embeddings.position_embedding.weight"].to(F64)[:L][None]
    x = _encoder(sd, p, x, cfg["num_hidden_layers"], cfg["num_attention_heads"], causal=True)
    x = _ln(x, sd[p + "final_layer_norm.weight"].to(F64), sd[p + "final_layer_norm.bias"].to(F64))
    pooled = x[torch.arange(ids.shape[0]), ids.argmax(-1)]
    return pooled @ sd["text_projection.weight"].to(F64).T


def cosine(x, y, eps=1e-8):
    """F.cosine_similarity(x, y, dim=-1, eps) as the installed torch (2.x) defines it: EACH norm is clamped to eps on its own,
    ``sum(x / max(|x|, eps) * y / max(|y|, eps))`` - not the older ``x.y / max(|x| |y|, eps)``: with |x| = 1e-9 and |y| = 1e3 (parallel) the
    first gives 0.1, the second 1."""
    x, y = x.to(F64), y.to(F64)
    return ((x / x.norm(dim=-1, keepdim=True).clamp_min(eps)) * (y / y.norm(dim=-1, keepdim=True).clamp_min(eps))).sum(-1)


def scores(img0, img1, txt0, txt1, eps=1e-8):
    """Features [n, D] / [n, D] / [D] or [n, D] (any float dtype; taken to float64 as they are) -> [n, 5] float64:
    sim_0, sim_1, sim_direction, sim_image (clip_similarity.py:43-46 on operands L2-normalised as :25, :33 do) and the cosine of
    consecutive img1 rows (0 for the last)."""
    nz = lambda v: v.to(F64) / v.to(F64).norm(dim=-1, keepdim=True)
    a, b, s, t = nz(img0), nz(img1), nz(txt0), nz(txt1)
    n = a.shape[0]
    s, t = s.expand(n, -1) if s.dim() == 2 else s[None].expand(n, -1), t.expand(n, -1) if t.dim() == 2 else t[None].expand(n, -1)
    cons = torch.zeros(n, dtype=F64)
    if n > 1:
        cons[:-1] = cosine(b[:-1], b[1:], eps)
    return torch.stack([cosine(a, s, eps), cosine(b, t, eps), cosine(b - a, t - s, eps), cosine(a, b, eps), cons], 1)


def ramp_frames(name, gains, H=40, W=72, reverse=False):
    """The test clips: ONE key-hashed uniform-noise image in [-1, 1] times a gain per frame (a brightness ramp; random-weight ViTs
    collapse on plain noise, a ramp moves the features).  ``reverse``: the same noise with the gains in reverse order (the "edit")."""
    from insv2v import synth
    base = synth.synth_input("clip_score." + name, (1, 3, H, W), kind="uniform")
    g = torch.tensor(list(reversed(gains)) if reverse else list(gains), dtype=torch.float32)
    return base * g[:, None, None, None]


def transformers_to_openai(sd):
    """The tests' own inverse of clip_vision.openai_to_transformers: a transformers-layout state dict as the OpenAI ``clip`` package stores
    it (fused in_proj, ``visual.proj`` / ``text_projection`` as [width, embed])."""
    out = {}
    blk = {"layer_norm1": "ln_1", "layer_norm2": "ln_2", "self_attn.out_proj": "attn.out_proj", "mlp.fc1": "mlp.c_fc", "mlp.fc2": "mlp.c_proj"}
    top = {"vision_model.embeddings.patch_embedding.weight": "visual.conv1.weight", "vision_model.embeddings.class_embedding": "visual.class_embedding",
           "vision_model.embeddings.position_embedding.weight": "visual.positional_embedding", "vision_model.pre_layrnorm": "visual.ln_pre",
           "vision_model.post_layernorm": "visual.ln_post", "text_model.embeddings.token_embedding.weight": "token_embedding.weight",
           "text_model.embeddings.position_embedding.weight": "positional_embedding", "text_model.final_layer_norm": "ln_final"}
    for k, v in sd.items():
        m = re.fullmatch(r"(vision_model|text_model)\.encoder\.layers\.(\d+)\.(.+)\.(weight|bias)", k)
        if m:
            base = ("visual.transformer" if m.group(1) == "vision_model" else "transformer") + f".resblocks.{m.group(2)}."
            if m.group(3) in blk:
                out[f"{base}{blk[m.group(3)]}.{m.group(4)}"] = v
            elif m.group(3) == "self_attn.q_proj":
                stem = k[:-len(f"q_proj.{m.group(4)}")]
                out[f"{base}attn.in_proj_{m.group(4)}"] = torch.cat([sd[f"{stem}{n}_proj.{m.group(4)}"] for n in "qkv"], 0)
            else:
                assert m.group(3) in ("self_attn.k_proj", "self_attn.v_proj"), k
        elif k == "visual_projection.weight":
            out["visual.proj"] = v.t().contiguous()
        elif k == "text_projection.weight":
            out["text_projection"] = v.t().contiguous()
        elif k in top:
            out[top[k]] = v
        else:
            stem, leaf = k.rsplit(".", 1)
            out[f"{top[stem]}.{leaf}"] = v
    return out
