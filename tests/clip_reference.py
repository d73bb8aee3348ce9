"""TEST INFRASTRUCTURE: plain-torch CPU restatement of the two CLIP encoders the pipeline calls in encode_clip (reference
svd/pipeline_stable_video_diffusion_controlnet.py:130-185): transformers' CLIPVisionModelWithProjection and CLIPTextModel
(models/clip/modeling_clip.py), with the parameter names of the shipped checkpoints (``vision_model.*`` / ``visual_projection.weight``,
``text_model.*``).  The product classes (this_and_that_vdm_amd/clip.py) are tested against it on identical weights; its own leaves are
pinned against transformers' classes by tests/golden/make_clip_golden.py -> tests/golden/clip_tiny.npz.

Pre-LayerNorm transformer layers: x += out_proj(attn(LN1 x)); x += fc2(act(fc1(LN2 x))).  Vision: patch conv (no bias) -> class token
in front -> + positions -> pre_layrnorm -> layers -> last_hidden_state (no norm) ; post_layernorm on the class row -> visual_projection
(no bias).  Text: token + position embeddings -> layers under a causal mask -> final_layer_norm."""
from __future__ import annotations

from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F

# the tiny configurations the tests share (ISSUE: V17 / V257 / T77)
VISION_TINY = dict(hidden_size=160, intermediate_size=320, num_hidden_layers=2, num_attention_heads=2, patch_size=14, projection_dim=64,
                   hidden_act="gelu", layer_norm_eps=1e-5)
TINY = {
    "V17": dict(VISION_TINY, image_size=56),
    "V257": dict(VISION_TINY, image_size=224),
    "T77": dict(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5),
}
BATCH = {"V17": 2, "V257": 1, "T77": 2}


def act_fn(name: str):
    if name == "gelu":
        return F.gelu
    if name == "quick_gelu":
        return lambda x: x * torch.sigmoid(1.702 * x)
    raise ValueError(name)


class Attention(nn.Module):
    def __init__(self, c: int, heads: int):
        super().__init__()
        self.heads = heads
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)

    def forward(self, x, causal: bool):
        n, l, c = x.shape
        split = lambda t: t.view(n, l, self.heads, c // self.heads).transpose(1, 2)
        o = F.scaled_dot_product_attention(split(self.q_proj(x)), split(self.k_proj(x)), split(self.v_proj(x)), is_causal=causal)
        return self.out_proj(o.transpose(1, 2).reshape(n, l, c))


class MLP(nn.Module):
    def __init__(self, c: int, inner: int, act: str):
        super().__init__()
        self.fc1, self.fc2, self.act = nn.Linear(c, inner), nn.Linear(inner, c), act_fn(act)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class EncoderLayer(nn.Module):
    def __init__(self, c, inner, heads, act, eps):
        super().__init__()
        self.self_attn = Attention(c, heads)
        self.layer_norm1 = nn.LayerNorm(c, eps=eps)
        self.mlp = MLP(c, inner, act)
        self.layer_norm2 = nn.LayerNorm(c, eps=eps)

    def forward(self, x, causal):
        x = x + self.self_attn(self.layer_norm1(x), causal)
        return x + self.mlp(self.layer_norm2(x))


class Encoder(nn.Module):
    def __init__(self, n, *a):
        super().__init__()
        self.layers = nn.ModuleList([EncoderLayer(*a) for _ in range(n)])

    def forward(self, x, causal):
        for layer in self.layers:
            x = layer(x, causal)
        return x


class VisionEmbeddings(nn.Module):
    def __init__(self, c, image, patch):
        super().__init__()
        self.class_embedding = nn.Parameter(torch.zeros(c))
        self.patch_embedding = nn.Conv2d(3, c, patch, stride=patch, bias=False)
        self.position_embedding = nn.Embedding((image // patch) ** 2 + 1, c)

    def forward(self, pixel_values):
        p = self.patch_embedding(pixel_values).flatten(2).transpose(1, 2)
        x = torch.cat([self.class_embedding.expand(p.shape[0], 1, -1), p], 1)
        return x + self.position_embedding.weight[None]


class VisionTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.embeddings = VisionEmbeddings(c, cfg["image_size"], cfg["patch_size"])
        self.pre_layrnorm = nn.LayerNorm(c, eps=eps)
        self.encoder = Encoder(cfg["num_hidden_layers"], c, cfg["intermediate_size"], cfg["num_attention_heads"], cfg["hidden_act"], eps)
        self.post_layernorm = nn.LayerNorm(c, eps=eps)


class CLIPVisionModelWithProjection(nn.Module):
    def __init__(self, **cfg):
        super().__init__()
        self.vision_model = VisionTransformer(cfg)
        self.visual_projection = nn.Linear(cfg["hidden_size"], cfg["projection_dim"], bias=False)

    def forward(self, pixel_values):
        v = self.vision_model
        h = v.encoder(v.pre_layrnorm(v.embeddings(pixel_values)), False)
        return SimpleNamespace(image_embeds=self.visual_projection(v.post_layernorm(h[:, 0])), last_hidden_state=h)


class TextEmbeddings(nn.Module):
    def __init__(self, vocab, positions, c):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, c)
        self.position_embedding = nn.Embedding(positions, c)

    def forward(self, ids):
        return self.token_embedding(ids) + self.position_embedding.weight[None, :ids.shape[1]]


class TextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        c, eps = cfg["hidden_size"], cfg["layer_norm_eps"]
        self.embeddings = TextEmbeddings(cfg["vocab_size"], cfg["max_position_embeddings"], c)
        self.encoder = Encoder(cfg["num_hidden_layers"], c, cfg["intermediate_size"], cfg["num_attention_heads"], cfg["hidden_act"], eps)
        self.final_layer_norm = nn.LayerNorm(c, eps=eps)


class CLIPTextModel(nn.Module):
    def __init__(self, **cfg):
        super().__init__()
        self.text_model = TextTransformer(cfg)

    def forward(self, input_ids):
        t = self.text_model
        h = t.final_layer_norm(t.encoder(t.embeddings(input_ids), True))
        return SimpleNamespace(last_hidden_state=h)


def build(name: str, round_to=None, dtype=torch.float32, **override):
    """the restatement of tiny config `name` with the repository's hash fill (salt "clip.")"""
    from this_and_that_vdm_amd.utils.synthetic import fill_parameters_
    cfg = dict(TINY[name], **override)
    m = (CLIPTextModel if "vocab_size" in cfg else CLIPVisionModelWithProjection)(**cfg).eval()
    with torch.no_grad():
        fill_parameters_(m, "clip.", round_to=round_to)
    return m.to(dtype), cfg


def inputs(name: str, cfg=None, batch=None):
    """deterministic inputs: pixel values in CLIP's normalised range, or token ids"""
    from this_and_that_vdm_amd.utils.synthetic import hash_uniform
    cfg = TINY[name] if cfg is None else cfg
    n = BATCH.get(name, 1) if batch is None else batch
    if "vocab_size" in cfg:
        l = cfg["max_position_embeddings"]
        u = hash_uniform(n * l, 77)
        return ((u + 1.0) * 0.5 * cfg["vocab_size"]).long().clamp_(0, cfg["vocab_size"] - 1).view(n, l)
    s = cfg["image_size"]
    return (hash_uniform(n * 3 * s * s, 224) * 2.0).view(n, 3, s, s)
