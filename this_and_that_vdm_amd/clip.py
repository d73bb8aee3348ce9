"""MI355X-native CLIP encoders: drop-ins for the two transformers classes ``encode_clip`` calls (reference
svd/pipeline_stable_video_diffusion_controlnet.py:130-185) --

  CLIPVisionModelWithProjection   the SVD image encoder (test_code/inference.py:325; ViT-H/14: width 1280, 16 heads of 80, 32 layers,
                                  257 tokens): ``image_encoder(pixel_values).image_embeds``
  CLIPTextModel                   the SD-2.1 text encoder (test_code/inference.py:348; width 1024, 16 heads of 64, 23 layers, 77 tokens,
                                  causal): ``text_encoder(input_ids)[0]``

(train_code/train_svd.py:214-231 picks the classes per checkpoint).  Parameter names are the checkpoints', so a stock ``image_encoder/`` /
``text_encoder/`` folder loads strictly (``config.json`` + ``model[.variant].safetensors``, single file or sharded index).  Every layer runs on
libttvdm: tt_patch_tokens / tt_embed_rows build the token rows, LayerNorms are tt_layernorm, the Linear layers tt_gemm (Q | K | V as one
launch, residuals updated in place), attention tt_encoder_attention, the MLP activation tt_act_rows.  There is no CPU fallback.

Not computed: ``pooler_output`` of the text model (the end-of-text row; the pipeline reads ``[0]`` only) and hidden-state / attention lists."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from .packing import presplit_f32
from .svd.modeling_utils import BaseOutput, ConfigMixin, ModelMixin, _load_weights, register_to_config

CLIP_WEIGHTS = "model"                     # transformers' file stem: model[.variant].safetensors / model.safetensors.index[.variant].json


@dataclass
class CLIPVisionModelOutput(BaseOutput):
    image_embeds: torch.Tensor = None
    last_hidden_state: torch.Tensor = None


@dataclass
class CLIPTextModelOutput(BaseOutput):
    last_hidden_state: torch.Tensor = None


def _check_common(hidden_size, num_attention_heads, hidden_act):
    if num_attention_heads <= 0 or hidden_size % num_attention_heads:
        raise ValueError(f"hidden_size {hidden_size} is not a whole number of {num_attention_heads} heads")
    d = hidden_size // num_attention_heads
    if d not in (64, 80):
        raise NotImplementedError(f"head dimension {d}: tt_encoder_attention serves 64 (SD-2.1 text encoder) and 80 (ViT-H/14)")
    if hidden_act not in ops.ACTS:
        raise NotImplementedError(f"hidden_act {hidden_act!r}: tt_act_rows has {sorted(ops.ACTS)}")


# ---- parameter containers with transformers' names
class _Attention(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c), nn.Linear(c, c)


class _MLP(nn.Module):
    def __init__(self, c, inner):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(c, inner), nn.Linear(inner, c)


class _EncoderLayer(nn.Module):
    def __init__(self, c, inner, eps):
        super().__init__()
        self.self_attn = _Attention(c)
        self.layer_norm1 = nn.LayerNorm(c, eps=eps)
        self.mlp = _MLP(c, inner)
        self.layer_norm2 = nn.LayerNorm(c, eps=eps)

    def pack(self, dtype, wcv):
        """kernel-ready buffers (plain attributes: state_dict() is unchanged).  16-bit storage: Q | K | V are one [3C, C] projection whose
        output tt_encoder_attention reads as three column slices.  fp32 storage: Q | K are one [2C, C] projection and V^T is written by a
        launch with swapped operands (weights as the row operand); v_proj's bias then enters through out_proj's, b_o + W_o b_v -- softmax
        rows sum to one, so a constant added to every value row passes through the attention unchanged."""
        a, f32 = self.self_attn, lambda t: t.detach().float().contiguous()
        self.f32 = dtype == torch.float32
        nq = 2 if self.f32 else 3
        projs = (a.q_proj, a.k_proj, a.v_proj)[:nq]
        self.wqkv = wcv(torch.cat([p.weight.detach() for p in projs], 0))
        self.bqkv = torch.cat([f32(p.bias) for p in projs], 0).contiguous()
        bo = f32(a.out_proj.bias)
        if self.f32:
            self.wv = a.v_proj.weight.detach().to(dtype).contiguous()          # the ROW operand of the swapped launch: never pre-split
            bo = (bo.double() + a.out_proj.weight.detach().double() @ a.v_proj.bias.detach().double()).float().contiguous()
        self.wo, self.bo = wcv(a.out_proj.weight), bo
        self.g1, self.b1, self.g2, self.b2 = f32(self.layer_norm1.weight), f32(self.layer_norm1.bias), f32(self.layer_norm2.weight), f32(self.layer_norm2.bias)
        self.w1, self.bf1 = wcv(self.mlp.fc1.weight), f32(self.mlp.fc1.bias)
        self.w2, self.bf2 = wcv(self.mlp.fc2.weight), f32(self.mlp.fc2.bias)

    def run(self, x, s: "_Scratch", dst=None):
        """x [rows_pad, C] is updated in place and returned -- or, with ``dst``, left as it is: the block's output goes to dst"""
        c, eps = x.shape[1], self.layer_norm1.eps
        h = ops.layernorm(x, self.g1, self.b1, eps)
        qkv = ops.gemm(h, self.wqkv, bias=self.bqkv, out=s.qkv)
        if self.f32:
            ops.gemm(self.wv, h, out=s.vt, out_col_pad=(s.l, s.lpad))           # V^T [C, sequence-padded columns]
            v, vstride = s.vt, s.lpad
        else:
            v, vstride = qkv[:, 2 * c:], s.l
        ops.encoder_attention(qkv[:, :c], qkv[:, c:2 * c], v, s.att, nseq=s.nseq, l=s.l, heads=s.heads, head_dim=c // s.heads,
                              causal=s.causal, k_seq_stride=s.l, v_seq_stride=vstride)
        x = ops.gemm(s.att, self.wo, bias=self.bo, residual=x, out=x if dst is None else dst)
        h = ops.layernorm(x, self.g2, self.b2, eps)
        f = ops.gemm(h, self.w1, bias=self.bf1, out=s.ff)
        ops.act_rows(f, s.act, out=f)
        return ops.gemm(f, self.w2, bias=self.bf2, residual=x, out=x)


class _Encoder(nn.Module):
    def __init__(self, n, c, inner, eps):
        super().__init__()
        self.layers = nn.ModuleList([_EncoderLayer(c, inner, eps) for _ in range(n)])


class _Scratch:
    """buffers shared by the layers of one forward; a model keeps the set of its last (sequences, tokens, dtype, device) and reuses it, so
    an encode launches library kernels only (the zero fills below run when the shape changes, not per encode).  Rows are padded to a
    multiple of 4 (the swapped V^T launch has the token rows as its N).  Padding rows of x / att and padding columns of vt start as zeros
    and stay finite -- x's and att's are never written (the blocks update y or a fresh tensor), vt's receive the padding rows' values --
    and nothing reads them back into a real row."""

    def __init__(self, nseq, l, c, inner, heads, causal, act, dtype, device):
        self.nseq, self.l, self.heads, self.causal, self.act = nseq, l, heads, causal, act
        self.rows = nseq * l
        self.rows_pad = (self.rows + 3) // 4 * 4
        f32 = dtype == torch.float32
        self.x = torch.zeros((self.rows_pad, c), dtype=dtype, device=device)
        self.qkv = torch.empty((self.rows_pad, (2 if f32 else 3) * c), dtype=dtype, device=device)
        self.y = torch.empty((self.rows_pad, c), dtype=dtype, device=device)      # the hidden states from the first block on (every row written)
        self.att = torch.zeros((self.rows_pad, c), dtype=dtype, device=device)
        self.ff = torch.empty((self.rows_pad, inner), dtype=dtype, device=device)
        self.lpad = (l + 3) // 4 * 4
        # V^T [C, pseudo-sequences * lpad]: token row n of the swapped launch lands in column (n / l) * lpad + n % l, the padding rows too
        self.vt = torch.zeros((c, -(-self.rows_pad // l) * self.lpad), dtype=dtype, device=device) if f32 else None


class _ClipModel(ModelMixin, ConfigMixin):
    """what the two encoders share: loading, packing, dtype selection"""

    _ignored_suffix = "embeddings.position_ids"       # a buffer older transformers versions saved; it is arange(positions)

    def _init_runtime(self):
        self.compute_dtype: Optional[torch.dtype] = None      # None: the parameter dtype if 16-bit, else bf16; float32 = TT_F32 mode
        self._packed_key = None

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, subfolder: str = None, torch_dtype=None, variant: str = None, **kwargs):
        """transformers-format local folder: ``config.json`` (a combined CLIPConfig's ``vision_config`` / ``text_config`` is unwrapped) and
        ``model[.variant].safetensors`` or its sharded index."""
        import inspect
        path = os.path.join(pretrained_model_name_or_path, subfolder) if subfolder else pretrained_model_name_or_path
        cfg_file = os.path.join(path, "config.json")
        if not os.path.isfile(cfg_file):
            raise OSError(f"{cfg_file} not found: from_pretrained needs a local transformers-format folder")
        with open(cfg_file) as f:
            cfg = json.load(f)
        cfg = dict(cfg, **cfg.get(cls._sub_config, {})) if isinstance(cfg.get(cls._sub_config), dict) else cfg
        accepted = set(inspect.signature(cls.__init__).parameters) - {"self"}
        init_kwargs = {k: v for k, v in cfg.items() if k in accepted}
        init_kwargs.update({k: v for k, v in kwargs.items() if k in accepted})
        model = cls(**init_kwargs)
        model.load_state_dict(_load_weights(path, variant, name=CLIP_WEIGHTS), strict=True)
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        return model.eval()

    def save_pretrained(self, save_directory: str, variant: str = None, **_):
        from safetensors.torch import save_file
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(dict(self.config), f, indent=2, sort_keys=True)
        sd = {k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}
        save_file(sd, os.path.join(save_directory, CLIP_WEIGHTS + (f".{variant}" if variant else "") + ".safetensors"), metadata={"format": "pt"})

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._packed_key = None
        sd = {k: v for k, v in state_dict.items() if not k.endswith(self._ignored_suffix)}
        return super().load_state_dict(sd, strict=strict, **kw)

    def _apply(self, fn, *a, **k):
        self._packed_key = None
        return super()._apply(fn, *a, **k)

    def _run_dtype(self) -> torch.dtype:
        if self.compute_dtype is not None:
            return self.compute_dtype
        dt = next(self.parameters()).dtype
        return dt if dt in (torch.float16, torch.bfloat16) else torch.bfloat16

    def prepare(self, force: bool = False):
        p0 = next(self.parameters())
        key = (p0.device, self._run_dtype(), sum(p._version for p in self.parameters()), p0.data_ptr(), ops.f32_split())
        if force or self._packed_key != key:
            if p0.device.type != "cuda":
                raise RuntimeError(f"{type(self).__name__} runs on the MI355X only (no CPU fallback)")
            dtype = key[1]
            split = dtype == torch.float32 and ops.f32_split()         # split16: constant operands are split once, not in every launch
            wcv = lambda w: presplit_f32(w.detach().float().contiguous()) if split else w.detach().to(dtype).contiguous()
            self._pack(dtype, wcv)
            self._packed_key = key
        return self

    def _layers(self):
        raise NotImplementedError

    def _scratch(self, nseq, l, causal, dtype, device) -> _Scratch:
        cfg = self.config
        key = (nseq, l, dtype, device)
        if self.__dict__.get("_scratch_key") != key:
            self.__dict__["_scratch_buf"] = _Scratch(nseq, l, cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, causal,
                                                     cfg.hidden_act, dtype, device)
            self.__dict__["_scratch_key"] = key
        return self.__dict__["_scratch_buf"]

    def _run_layers(self, x, s: _Scratch, keep_input: bool = False):
        """keep_input: x is the scratch set's own zero-padded buffer -- the first block writes to s.y, so x's padding rows stay zeros"""
        for i, layer in enumerate(self._layers()):
            x = layer.run(x, s, dst=s.y if keep_input and i == 0 else None)
        return x


class CLIPVisionModelWithProjection(_ClipModel):
    _sub_config = "vision_config"

    @register_to_config
    def __init__(self, hidden_size: int = 1280, intermediate_size: int = 5120, num_hidden_layers: int = 32, num_attention_heads: int = 16,
                 image_size: int = 224, patch_size: int = 14, projection_dim: int = 1024, hidden_act: str = "gelu",
                 layer_norm_eps: float = 1e-5, num_channels: int = 3):
        super().__init__()
        _check_common(hidden_size, num_attention_heads, hidden_act)
        if patch_size <= 0 or image_size % patch_size:
            raise ValueError(f"image_size {image_size} is not a whole number of {patch_size}-pixel patches")
        if hidden_size % 8 or intermediate_size % 8 or projection_dim % 4:
            raise NotImplementedError("widths must be multiples of 8 (projection_dim: of 4)")
        c = hidden_size
        vm = nn.Module()
        vm.embeddings = nn.Module()
        vm.embeddings.class_embedding = nn.Parameter(torch.zeros(c))
        vm.embeddings.patch_embedding = nn.Conv2d(num_channels, c, patch_size, stride=patch_size, bias=False)
        vm.embeddings.position_embedding = nn.Embedding((image_size // patch_size) ** 2 + 1, c)
        vm.pre_layrnorm = nn.LayerNorm(c, eps=layer_norm_eps)
        vm.encoder = _Encoder(num_hidden_layers, c, intermediate_size, layer_norm_eps)
        vm.post_layernorm = nn.LayerNorm(c, eps=layer_norm_eps)
        self.vision_model = vm
        self.visual_projection = nn.Linear(c, projection_dim, bias=False)
        self._init_runtime()

    def _layers(self):
        return self.vision_model.encoder.layers

    def _pack(self, dtype, wcv):
        vm, f32 = self.vision_model, lambda t: t.detach().float().contiguous()
        w = vm.embeddings.patch_embedding.weight.detach().flatten(1)             # [C, 3 p^2], k = (c, ky, kx)
        self.kpad = (w.shape[1] + 7) // 8 * 8
        wp = torch.zeros((w.shape[0], self.kpad), dtype=w.dtype, device=w.device)
        wp[:, :w.shape[1]] = w
        self.w_patch = wcv(wp)
        self.cls = vm.embeddings.class_embedding.detach().to(dtype).contiguous()
        self.pos = vm.embeddings.position_embedding.weight.detach().to(dtype).contiguous()
        self.g_pre, self.b_pre = f32(vm.pre_layrnorm.weight), f32(vm.pre_layrnorm.bias)
        self.g_post, self.b_post = f32(vm.post_layernorm.weight), f32(vm.post_layernorm.bias)
        self.w_proj = wcv(self.visual_projection.weight)
        for layer in vm.encoder.layers:
            layer.pack(dtype, wcv)

    @torch.no_grad()
    def forward(self, pixel_values: torch.Tensor, return_dict: bool = True, **_):
        cfg = self.config
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (cfg.num_channels, cfg.image_size, cfg.image_size):
            raise ValueError(f"pixel_values: expected [N, {cfg.num_channels}, {cfg.image_size}, {cfg.image_size}], got {tuple(pixel_values.shape)}")
        if not pixel_values.is_cuda:
            raise RuntimeError("CLIPVisionModelWithProjection runs on the MI355X only (no CPU fallback): pixel_values must be on the device")
        self.prepare()
        dtype, out_dtype = self._run_dtype(), next(self.parameters()).dtype
        n, c = pixel_values.shape[0], cfg.hidden_size
        l = (cfg.image_size // cfg.patch_size) ** 2 + 1
        s = self._scratch(n, l, False, dtype, pixel_values.device)
        patches = ops.gemm(ops.patch_tokens(pixel_values, cfg.patch_size, dtype, self.kpad), self.w_patch)     # the stride-p conv
        ops.embed_rows(patches, self.pos, cls=self.cls, l=l, out=s.x[:s.rows])
        x = ops.layernorm(s.x, self.g_pre, self.b_pre, cfg.layer_norm_eps)     # a fresh tensor: the outputs below are views of it
        self._run_layers(x, s)
        hidden = x[:s.rows].view(n, l, c)
        pooled = ops.layernorm(hidden[:, 0], self.g_post, self.b_post, cfg.layer_norm_eps)                      # class rows, stride l * C
        embeds = ops.gemm(pooled, self.w_proj)
        out = CLIPVisionModelOutput(image_embeds=embeds.to(out_dtype), last_hidden_state=hidden.to(out_dtype))
        return out if return_dict else out.to_tuple()


class CLIPTextModel(_ClipModel):
    _sub_config = "text_config"

    @register_to_config
    def __init__(self, vocab_size: int = 49408, hidden_size: int = 1024, intermediate_size: int = 4096, num_hidden_layers: int = 23,
                 num_attention_heads: int = 16, max_position_embeddings: int = 77, hidden_act: str = "gelu", layer_norm_eps: float = 1e-5):
        super().__init__()
        _check_common(hidden_size, num_attention_heads, hidden_act)
        if hidden_size % 8 or intermediate_size % 8:
            raise NotImplementedError("widths must be multiples of 8")
        c = hidden_size
        tm = nn.Module()
        tm.embeddings = nn.Module()
        tm.embeddings.token_embedding = nn.Embedding(vocab_size, c)
        tm.embeddings.position_embedding = nn.Embedding(max_position_embeddings, c)
        tm.encoder = _Encoder(num_hidden_layers, c, intermediate_size, layer_norm_eps)
        tm.final_layer_norm = nn.LayerNorm(c, eps=layer_norm_eps)
        self.text_model = tm
        self._init_runtime()

    def _layers(self):
        return self.text_model.encoder.layers

    def _pack(self, dtype, wcv):
        tm, f32 = self.text_model, lambda t: t.detach().float().contiguous()
        self.table = tm.embeddings.token_embedding.weight.detach().to(dtype).contiguous()
        self.pos = tm.embeddings.position_embedding.weight.detach().to(dtype).contiguous()
        self.g_fin, self.b_fin = f32(tm.final_layer_norm.weight), f32(tm.final_layer_norm.bias)
        for layer in tm.encoder.layers:
            layer.pack(dtype, wcv)

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, return_dict: bool = True, **_):
        cfg = self.config
        if input_ids.dim() != 2 or input_ids.dtype != torch.int64:
            raise ValueError(f"input_ids: expected int64 [N, l], got {tuple(input_ids.shape)} {input_ids.dtype}")
        n, l = input_ids.shape
        if l < 1 or l > cfg.max_position_embeddings:
            raise ValueError(f"input_ids: {l} tokens, the model has {cfg.max_position_embeddings} positions")
        if not input_ids.is_cuda:
            raise RuntimeError("CLIPTextModel runs on the MI355X only (no CPU fallback): input_ids must be on the device")
        self.prepare()
        dtype, out_dtype = self._run_dtype(), next(self.parameters()).dtype
        s = self._scratch(n, l, True, dtype, input_ids.device)
        ops.embed_rows(self.table, self.pos, ids=input_ids.contiguous().view(-1), l=l, out=s.x[:s.rows])
        x = self._run_layers(s.x, s, keep_input=True)
        y = ops.layernorm(x, self.g_fin, self.b_fin, cfg.layer_norm_eps)
        out = CLIPTextModelOutput(last_hidden_state=y[:s.rows].view(n, l, cfg.hidden_size).to(out_dtype))
        return out if return_dict else out.to_tuple()
