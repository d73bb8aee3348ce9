"""MI355X-native VAE *encoder*: what ``vae.encode(x).latent_dist`` runs for the conditioning image and the gesture frames
(reference svd/pipeline_stable_video_diffusion_controlnet.py:200,652, svd/pipeline_stable_video_diffusion.py:189) and for the
training videos (train_code/train_svd.py:207,728).

diffusers==0.25.1's ``Encoder`` (models/vae.py; ``AutoencoderKLTemporalDecoder`` builds it with ``double_z=True``) is not vendored
by the reference and not installed here, so its published layout is restated with the same module / parameter names -- a stock
``vae/`` checkpoint's ``encoder.*`` keys load by name:

  conv_in 3x3 (3 -> C0) -> down_blocks[i] = DownEncoderBlock2D: layers_per_block x ResnetBlock2D (no time embedding, eps 1e-6),
  then (all but the last) Downsample2D(padding=0): F.pad(x, (0, 1, 0, 1)) + 3x3 stride-2 conv, ONE tt_gemm mode-3 launch
  -> mid_block = UNetMidBlock2D: ResnetBlock2D, single-head attention over h*w tokens (d = C), ResnetBlock2D
  -> GroupNorm + SiLU -> conv_out 3x3 (C -> 8: mean | logvar of the 4 latent channels).

The encoder is 2D: every image of the batch is independent (Geom(batch=N, frames=1, h, w)), GroupNorms are per image.
PARITY UNPINNED, like every diffusers leaf: tests/vae_encoder_reference.py is the CPU restatement it is tested against."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..packing import pack_conv3x3
from .layers import Geom, ResnetBlock2D, _f32, _Packable
from .pipeline_utils import randn_tensor


def _resnet(cin: int, cout: int) -> ResnetBlock2D:
    return ResnetBlock2D(in_channels=cin, out_channels=cout, temb_channels=None, eps=1e-6, groups=32)


class EncoderDownsample2D(_Packable):
    """diffusers Downsample2D(use_conv=True, padding=0): zero row / column appended at the bottom / right, then a 3x3 stride-2
    conv without padding -- tt_gemm mode 3 reads pixel (2y + ky, 2x + kx) and treats the ones past the edge as zeros."""

    def __init__(self, channels: int, out_channels: Optional[int] = None):
        super().__init__()
        self.conv = nn.Conv2d(channels, out_channels or channels, 3, stride=2, padding=0)

    def pack(self, reg, dtype):
        self.w, self.b = pack_conv3x3(self.conv.weight.detach().to(dtype)), _f32(self.conv.bias)

    def forward(self, x, g: Geom):
        ho, wo = (g.h + 1 - 3) // 2 + 1, (g.w + 1 - 3) // 2 + 1
        out = ops.gemm(x, self.w, mode=3, conv=(g.n, g.h, g.w, ho, wo, 2, 0), bias=self.b, stats=ho * wo)    # (next block's norm1)
        return out, Geom(g.batch, g.frames, ho, wo)


class DownEncoderBlock2D(_Packable):
    def __init__(self, in_channels: int, out_channels: int, num_layers: int, add_downsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([_resnet(in_channels if i == 0 else out_channels, out_channels) for i in range(num_layers)])
        self.downsamplers = nn.ModuleList([EncoderDownsample2D(out_channels, out_channels)]) if add_downsample else None

    def pack(self, reg, dtype):
        for m in self.resnets:
            m.pack(reg, dtype)
        if self.downsamplers is not None:
            self.downsamplers[0].pack(reg, dtype)

    def forward(self, x, g: Geom):
        for r in self.resnets:
            x = r(x, None, g, None)
        if self.downsamplers is not None:
            x, g = self.downsamplers[0](x, g)
        return x, g


class UNetMidBlock2D(_Packable):
    def __init__(self, channels: int):
        super().__init__()
        from .autoencoder_kl_temporal_decoder import VaeAttention
        self.resnets = nn.ModuleList([_resnet(channels, channels), _resnet(channels, channels)])
        self.attentions = nn.ModuleList([VaeAttention(channels, 1, channels, eps=1e-6, norm_num_groups=32)])

    def pack(self, reg, dtype):
        for m in list(self.resnets) + list(self.attentions):
            m.pack(reg, dtype)

    def forward(self, x, g: Geom):
        x = self.resnets[0](x, None, g, None)
        x = self.attentions[0](x, g)
        return self.resnets[1](x, None, g, None)


class Encoder(_Packable):
    """diffusers Encoder(in_channels, out_channels=latent_channels, down_block_types=("DownEncoderBlock2D",) * len(block_out_channels),
    block_out_channels, layers_per_block, norm_num_groups=32, act_fn="silu", double_z=True).

    pack() folds the VAE's ``quant_conv`` (1x1, 2L -> 2L) into conv_out: W' = Q W, b' = Q b + b_q in fp32 before the storage rounding,
    so the moments leave ONE launch (``quant_conv`` is passed in, it stays the parent's sub-module)."""

    CIN_PAD = 8        # image channels (3) padded to one 16-byte chunk of 16-bit tokens

    def __init__(self, in_channels: int = 3, out_channels: int = 4, block_out_channels: Tuple[int, ...] = (128, 256, 512, 512),
                 layers_per_block: int = 2):
        super().__init__()
        if in_channels > self.CIN_PAD or 2 * out_channels > 8:
            raise NotImplementedError("image channels <= 8 and latent channels <= 4")
        self.in_channels, self.z_channels = in_channels, 2 * out_channels
        self.conv_in = nn.Conv2d(in_channels, block_out_channels[0], 3, padding=1)
        self.down_blocks = nn.ModuleList([])
        out_ch = block_out_channels[0]
        for i, ch in enumerate(block_out_channels):
            prev, out_ch = out_ch, ch
            self.down_blocks.append(DownEncoderBlock2D(prev, out_ch, layers_per_block, add_downsample=i != len(block_out_channels) - 1))
        self.mid_block = UNetMidBlock2D(block_out_channels[-1])
        self.conv_norm_out = nn.GroupNorm(32, block_out_channels[-1], eps=1e-6)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(block_out_channels[-1], 2 * out_channels, 3, padding=1)

    def pack(self, reg, dtype, quant_conv: nn.Conv2d):
        w = self.conv_in.weight.detach()
        wp = torch.zeros((w.shape[0], self.CIN_PAD, 3, 3), dtype=w.dtype, device=w.device)
        wp[:, :self.in_channels] = w
        self.w_in, self.b_in = pack_conv3x3(wp.to(dtype)), _f32(self.conv_in.bias)
        for b in self.down_blocks:
            b.pack(reg, dtype)
        self.mid_block.pack(reg, dtype)
        self.g_out, self.be_out = _f32(self.conv_norm_out.weight), _f32(self.conv_norm_out.bias)
        q = quant_conv.weight.detach().float().flatten(1)                                    # [2L, 2L]
        w = torch.einsum("oj,jchw->ochw", q, self.conv_out.weight.detach().float())
        b = q @ self.conv_out.bias.detach().float() + quant_conv.bias.detach().float()
        wo = torch.zeros((8,) + tuple(w.shape[1:]), dtype=torch.float32, device=w.device)    # 2L rows padded to 8 (zero rows)
        wo[:self.z_channels] = w
        bo = torch.zeros(8, dtype=torch.float32, device=w.device)
        bo[:self.z_channels] = b
        self.w_out, self.b_out = pack_conv3x3(wo.to(dtype)), bo.contiguous()

    def forward(self, x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """x [N, C_in, H, W] (any float dtype) -> fp32 moments [N, 2L, H/2^k, W/2^k] (quant_conv applied)."""
        n, _, h, w = x.shape
        g = Geom(n, 1, h, w)
        t = ops.nchw_to_tokens(x, dtype, ld=self.CIN_PAD)
        t = ops.gemm(t, self.w_in, mode=1, conv=(n, h, w, h, w, 1, 0), bias=self.b_in, stats=g.hw)
        for blk in self.down_blocks:
            t, g = blk(t, g)
        t = self.mid_block(t, g)
        t = ops.groupnorm(t, None, g.n, g.hw, 1, self.g_out, self.be_out, 1e-6, True)
        t = ops.gemm(t, self.w_out, mode=1, conv=(n, g.h, g.w, g.h, g.w, 1, 0), bias=self.b_out)               # [M, 8]
        return ops.tokens_to_nchw(t, n, self.z_channels, g.h, g.w, torch.float32)

    def max_tokens_bytes(self, h: int, w: int, es: int) -> int:
        """bytes of the largest token tensor one image produces (every level's h*w x channels; the input's 8-wide tokens)"""
        chans = [self.conv_in.out_channels] + [b.resnets[-1].out_channels for b in self.down_blocks]
        big = h * w * max(self.CIN_PAD, chans[0])
        for i, blk in enumerate(self.down_blocks):
            big = max(big, (h >> i) * (w >> i) * max(r.out_channels for r in blk.resnets))
        return big * es


class DiagonalGaussianDistribution:
    """diffusers' DiagonalGaussianDistribution (models/vae.py) in plain torch: the ``latent_dist`` of ``encode``."""

    def __init__(self, parameters: torch.Tensor, deterministic: bool = False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if self.deterministic:
            self.var = self.std = torch.zeros_like(self.mean, device=self.parameters.device, dtype=self.parameters.dtype)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        noise = randn_tensor(self.mean.shape, generator=generator, device=self.parameters.device, dtype=self.parameters.dtype)
        return self.mean + self.std * noise

    def kl(self, other: Optional["DiagonalGaussianDistribution"] = None) -> torch.Tensor:
        if self.deterministic:
            return torch.Tensor([0.0])
        if other is None:
            return 0.5 * torch.sum(torch.pow(self.mean, 2) + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.sum(torch.pow(self.mean - other.mean, 2) / other.var + self.var / other.var - 1.0 - self.logvar + other.logvar,
                               dim=[1, 2, 3])

    def nll(self, sample: torch.Tensor, dims=(1, 2, 3)) -> torch.Tensor:
        if self.deterministic:
            return torch.Tensor([0.0])
        logtwopi = np.log(2.0 * np.pi)
        return 0.5 * torch.sum(logtwopi + self.logvar + torch.pow(sample - self.mean, 2) / self.var, dim=list(dims))

    def mode(self) -> torch.Tensor:
        return self.mean
