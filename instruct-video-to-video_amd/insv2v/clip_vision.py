"""CLIP image tower on the HIP kernels: transformers ``CLIPVisionModelWithProjection`` / OpenAI ``clip`` ``model.encode_image``
(the model behind ``ClipSimilarity``, misc_utils/clip_similarity.py:16,32).

Frames go through ``insv2v_clip_preprocess`` (bicubic resize, mean / std, patch rows), the patch embedding is one batched
``insv2v_gemm`` that writes rows 1 .. of every frame's token block and adds the position table as its row bias, the class row is a
copy of ``class_embedding + position[0]``.  Then ``pre_layrnorm`` (transformers' own spelling), N pre-LN blocks built exactly like the
text tower's (LayerNorm folded into the QKV / fc1 GEMMs, ``insv2v_attention`` without the causal flag, quick-GELU), ``post_layernorm``
on the class token only and ``visual_projection``.

``openai_to_transformers`` rewrites a state dict of the OpenAI ``clip`` package (``visual.*``, ``transformer.*``, ``text_projection``)
into the transformers layout; both layouts give the same bits.
"""
import re

import torch

from . import ops
from .unet import fold_layernorm, _dev, prep_linear, prep_norm

_OPENAI_META = ("input_resolution", "context_length", "vocab_size")   # scalars the JIT archives carry; no weights
_BLOCK = {"ln_1.weight": "layer_norm1.weight", "ln_1.bias": "layer_norm1.bias", "ln_2.weight": "layer_norm2.weight",
          "ln_2.bias": "layer_norm2.bias", "attn.out_proj.weight": "self_attn.out_proj.weight", "attn.out_proj.bias": "self_attn.out_proj.bias",
          "mlp.c_fc.weight": "mlp.fc1.weight", "mlp.c_fc.bias": "mlp.fc1.bias", "mlp.c_proj.weight": "mlp.fc2.weight",
          "mlp.c_proj.bias": "mlp.fc2.bias"}
_VISUAL = {"conv1.weight": "embeddings.patch_embedding.weight", "class_embedding": "embeddings.class_embedding",
           "positional_embedding": "embeddings.position_embedding.weight", "ln_pre.weight": "pre_layrnorm.weight",
           "ln_pre.bias": "pre_layrnorm.bias", "ln_post.weight": "post_layernorm.weight", "ln_post.bias": "post_layernorm.bias"}
_TEXT = {"token_embedding.weight": "embeddings.token_embedding.weight", "positional_embedding": "embeddings.position_embedding.weight",
         "ln_final.weight": "final_layer_norm.weight", "ln_final.bias": "final_layer_norm.bias"}


def is_openai_layout(sd):
    return any(k.startswith("visual.") or k.startswith("transformer.resblocks.") for k in sd)


def openai_to_transformers(sd):
    """OpenAI ``clip`` state dict -> transformers ``CLIPModel`` layout (``vision_model.*``, ``visual_projection.weight``, ``text_model.*``,
    ``text_projection.weight``, ``logit_scale``).  Pure: tensors are split / transposed views of the input's, nothing is rounded.  The fused
    ``attn.in_proj_*`` become q / k / v, ``visual.proj`` and ``text_projection`` (stored [width, embed]) are transposed to Linear weights.
    A key that belongs to neither tower raises KeyError."""
    out = {}

    def block(dst, rest, v):
        m = re.fullmatch(r"(\d+)\.(.+)", rest)
        if m is None:
            raise KeyError(rest)
        p, name = f"{dst}.encoder.layers.{m.group(1)}.", m.group(2)
        if name in ("attn.in_proj_weight", "attn.in_proj_bias"):
            if v.shape[0] % 3:
                raise KeyError(f"{rest}: fused q/k/v of {v.shape[0]} rows")
            c = v.shape[0] // 3
            for i, n in enumerate("qkv"):
                out[f"{p}self_attn.{n}_proj.{'weight' if name.endswith('weight') else 'bias'}"] = v[i * c:(i + 1) * c]
        elif name in _BLOCK:
            out[p + _BLOCK[name]] = v
        else:
            raise KeyError(rest)

    for k, v in sd.items():
        try:
            if k in _OPENAI_META:
                continue
            if k == "logit_scale":
                out[k] = v
            elif k == "text_projection":
                out["text_projection.weight"] = v.t()
            elif k == "visual.proj":
                out["visual_projection.weight"] = v.t()
            elif k.startswith("visual.transformer.resblocks."):
                block("vision_model", k[len("visual.transformer.resblocks."):], v)
            elif k.startswith("transformer.resblocks."):
                block("text_model", k[len("transformer.resblocks."):], v)
            elif k.startswith("visual.") and k[len("visual."):] in _VISUAL:
                out["vision_model." + _VISUAL[k[len("visual."):]]] = v
            elif k in _TEXT:
                out["text_model." + _TEXT[k]] = v
            else:
                raise KeyError(k)
        except KeyError:
            raise KeyError(f"openai_to_transformers: {k!r} is not a key of the OpenAI CLIP layout") from None
    return out


class CLIPVisionTransformer:
    """transformers CLIPVisionModelWithProjection forward (quick_gelu) on device; weights fp16, statistics / accumulation fp32.
    ``__call__`` takes frames [n,3,H,W] (fp16 / fp32, any strides) with the affine map that brings them to [0, 1] and returns the
    projected, un-normalised ``image_embeds`` [n, projection_dim] fp32."""

    def __init__(self, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=224,
                 patch_size=14, projection_dim=768, layer_norm_eps=1e-5, device="cuda", **unused):
        if hidden_size % num_attention_heads or (hidden_size // num_attention_heads) not in (16, 32, 64, 128):
            raise ValueError("head_dim must be one of 16/32/64/128")
        if image_size % patch_size:
            raise ValueError(f"image_size {image_size} is no multiple of patch_size {patch_size}")
        self.cfg = dict(hidden_size=hidden_size, intermediate_size=intermediate_size, num_hidden_layers=num_hidden_layers,
                        num_attention_heads=num_attention_heads, image_size=image_size, patch_size=patch_size, projection_dim=projection_dim)
        self.eps, self.device, self.layers = layer_norm_eps, torch.device(device), None
        self.ld = -(-3 * patch_size * patch_size // 64) * 64   # K of the patch GEMM, zero-padded

    def load_state_dict(self, state_dict, strict=True):
        sd = openai_to_transformers(state_dict) if is_openai_layout(state_dict) else state_dict
        dev, c, f32 = self.device, self.cfg, torch.float32
        C, P, npos = c["hidden_size"], c["patch_size"], (c["image_size"] // c["patch_size"]) ** 2 + 1
        v = "vision_model."
        wp = sd[v + "embeddings.patch_embedding.weight"]
        pos = sd[v + "embeddings.position_embedding.weight"].float()
        if tuple(wp.shape) != (C, 3, P, P) or tuple(pos.shape) != (npos, C):
            raise RuntimeError(f"patch_embedding is {tuple(wp.shape)} and position_embedding {tuple(pos.shape)}, config says "
                               f"{(C, 3, P, P)} and {(npos, C)}")
        w = torch.zeros((C, self.ld), dtype=torch.float32)
        w[:, :3 * P * P] = wp.float().reshape(C, -1)
        self.w_patch = _dev(w, torch.float16, dev)
        self.pos_rows = _dev(pos[1:], f32, dev)                                                                   # row bias of the patch GEMM
        self.cls_row = _dev((sd[v + "embeddings.class_embedding"].float() + pos[0])[None], torch.float16, dev)   # [1, C]
        self.pre_ln = prep_norm(sd, v + "pre_layrnorm", dev)
        self.layers = []
        for i in range(c["num_hidden_layers"]):
            p = f"{v}encoder.layers.{i}."
            wqkv = torch.cat([sd[p + f"self_attn.{n}_proj.weight"].float() for n in "qkv"], 0)
            bqkv = torch.cat([sd[p + f"self_attn.{n}_proj.bias"].float() for n in "qkv"], 0)
            wf, cs, b = fold_layernorm(wqkv, sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"], bqkv)
            w1, cs1, b1 = fold_layernorm(sd[p + "mlp.fc1.weight"], sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"],
                                         sd[p + "mlp.fc1.bias"])
            self.layers.append(dict(
                wqkv=_dev(wf, torch.float16, dev), qkv_cs=_dev(cs, f32, dev), qkv_b=_dev(b, f32, dev),
                wo=prep_linear(sd, p + "self_attn.out_proj", dev),
                w1=_dev(w1, torch.float16, dev), cs1=_dev(cs1, f32, dev), b1=_dev(b1, f32, dev),
                w2=prep_linear(sd, p + "mlp.fc2", dev)))
        self.post_ln = prep_norm(sd, v + "post_layernorm", dev)
        wproj = sd["visual_projection.weight"]
        if tuple(wproj.shape) != (c["projection_dim"], C):
            raise RuntimeError(f"visual_projection is {tuple(wproj.shape)}, config says {(c['projection_dim'], C)}")
        self.w_proj = _dev(wproj, torch.float16, dev)
        return self

    def embed(self, frames, in_scale=1.0, in_shift=0.0):
        """Frames -> the token matrix [n * (patches + 1), C] entering ``pre_layrnorm``."""
        c = self.cfg
        C, S, P = c["hidden_size"], c["image_size"], c["patch_size"]
        n, npatch = frames.shape[0], (S // P) ** 2
        L = npatch + 1
        rows = ops.clip_preprocess(frames, S, P, ld=self.ld, in_scale=in_scale, in_shift=in_shift)
        x = torch.empty((n * L, C), device=self.device, dtype=torch.float16)
        # frame z's patches -> rows z * L + 1 ..: batched output behind a one-row offset; the position table is the row bias
        ops.gemm(rows, self.w_patch, None, row_bias=self.pos_rows, rows_per_group=1, out=x[1:], batch=n, M=npatch,
                 a_bs=npatch * self.ld, c_bs=L * C)
        ops.copy_rows(x.view(n, L, C)[:, 0], self.cls_row.expand(n, C))
        return x

    def __call__(self, frames, in_scale=1.0, in_shift=0.0):
        if self.layers is None:
            raise RuntimeError("CLIPVisionTransformer: load_state_dict() first")
        c = self.cfg
        C, H = c["hidden_size"], c["num_attention_heads"]
        d, n, L = C // H, frames.shape[0], (c["image_size"] // c["patch_size"]) ** 2 + 1
        x = ops.layernorm(self.embed(frames, in_scale, in_shift), *self.pre_ln, eps=self.eps)
        for ly in self.layers:
            qkv = ops.gemm(x, ly["wqkv"], ly["qkv_b"], row_stats=ops.layernorm_stats(x, self.eps), col_sum=ly["qkv_cs"])
            a = torch.empty((n * L, C), device=x.device, dtype=torch.float16)
            p = qkv.data_ptr()
            addr = (1, L * 3 * C, 0)
            ops.attention(p, p + 2 * C, p + 4 * C, a, batch=n, heads=H, head_dim=d, seq_q=L, seq_k=L, scale=d ** -0.5,
                          q_rs=3 * C, k_rs=3 * C, v_rs=3 * C, o_rs=C, q_addr=addr, kv_addr=addr, o_addr=(1, L * C, 0), causal=False)
            x = ops.gemm(a, *ly["wo"], residual=x)
            h = ops.gemm(x, ly["w1"], ly["b1"], act=ops.ACT_QUICK_GELU, row_stats=ops.layernorm_stats(x, self.eps), col_sum=ly["cs1"])
            x = ops.gemm(h, *ly["w2"], residual=x)
        pooled = ops.layernorm(x.view(n, L, C)[:, 0], *self.post_ln, eps=self.eps)   # the class token only
        return ops.gemm(pooled, self.w_proj, None, out_fp32=True)
