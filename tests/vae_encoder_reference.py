"""TEST INFRASTRUCTURE: plain fp32 CPU restatement of diffusers==0.25.1's VAE encoder path (models/vae.py `Encoder` with
double_z=True, models/unet_2d_blocks.py `DownEncoderBlock2D` / `UNetMidBlock2D`, models/resnet.py `Downsample2D(padding=0)`,
`AutoencoderKL*.encode` -> quant_conv -> DiagonalGaussianDistribution) with diffusers' module / parameter names, composed from the
audited oracle leaves (oracle.leaves.ResnetBlock2D, oracle.vae.VaeAttention).  The product encoder
(this_and_that_vdm_amd/svd/vae_encoder.py) is tested against it on identical weights.

Note: oracle.leaves.Downsample2D(padding=0) is NOT the encoder's downsample (it omits the (0, 1, 0, 1) zero pad and returns
H/2 - 1 rows); the one here pads first."""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.leaves import ResnetBlock2D
from oracle.vae import VaeAttention


def _resnet(cin, cout):
    return ResnetBlock2D(in_channels=cin, out_channels=cout, temb_channels=None, eps=1e-6)


class Downsample2D(nn.Module):
    def __init__(self, channels: int, out_channels: int):
        super().__init__()
        self.conv = nn.Conv2d(channels, out_channels, 3, stride=2, padding=0)

    def forward(self, x):
        return self.conv(F.pad(x, (0, 1, 0, 1), mode="constant", value=0.0))


class DownEncoderBlock2D(nn.Module):
    def __init__(self, cin: int, cout: int, num_layers: int, add_downsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([_resnet(cin if i == 0 else cout, cout) for i in range(num_layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(cout, cout)]) if add_downsample else None

    def forward(self, x):
        for r in self.resnets:
            x = r(x, None)
        if self.downsamplers is not None:
            x = self.downsamplers[0](x)
        return x


class UNetMidBlock2D(nn.Module):
    def __init__(self, c: int):
        super().__init__()
        self.resnets = nn.ModuleList([_resnet(c, c), _resnet(c, c)])
        self.attentions = nn.ModuleList([VaeAttention(c, 1, c, eps=1e-6, norm_num_groups=32)])

    def forward(self, x):
        x = self.resnets[0](x, None)
        x = self.attentions[0](x)
        return self.resnets[1](x, None)


class Encoder(nn.Module):
    def __init__(self, in_channels: int = 3, out_channels: int = 4, block_out_channels: Tuple[int, ...] = (128, 256, 512, 512),
                 layers_per_block: int = 2):
        super().__init__()
        self.conv_in = nn.Conv2d(in_channels, block_out_channels[0], 3, padding=1)
        self.down_blocks = nn.ModuleList([])
        out_ch = block_out_channels[0]
        for i, ch in enumerate(block_out_channels):
            prev, out_ch = out_ch, ch
            self.down_blocks.append(DownEncoderBlock2D(prev, out_ch, layers_per_block, i != len(block_out_channels) - 1))
        self.mid_block = UNetMidBlock2D(block_out_channels[-1])
        self.conv_norm_out = nn.GroupNorm(32, block_out_channels[-1], eps=1e-6)
        self.conv_act = nn.SiLU()
        self.conv_out = nn.Conv2d(block_out_channels[-1], 2 * out_channels, 3, padding=1)

    def forward(self, x):
        x = self.conv_in(x)
        for b in self.down_blocks:
            x = b(x)
        x = self.mid_block(x)
        return self.conv_out(self.conv_act(self.conv_norm_out(x)))


class DiagonalGaussian:
    def __init__(self, moments: torch.Tensor):
        self.parameters = moments
        self.mean, logvar = torch.chunk(moments, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def mode(self):
        return self.mean

    def kl(self):
        return 0.5 * torch.sum(self.mean ** 2 + self.var - 1.0 - self.logvar, dim=[1, 2, 3])

    def nll(self, sample):
        return 0.5 * torch.sum(np.log(2.0 * np.pi) + self.logvar + (sample - self.mean) ** 2 / self.var, dim=[1, 2, 3])


class EncoderVAE(nn.Module):
    """The encoder half of diffusers' AutoencoderKLTemporalDecoder: ``encoder.*`` + ``quant_conv.*`` keys, ``encode(x)``."""

    def __init__(self, in_channels: int = 3, block_out_channels: Tuple[int, ...] = (128, 256, 512, 512), layers_per_block: int = 2,
                 latent_channels: int = 4, **_):
        super().__init__()
        self.encoder = Encoder(in_channels, latent_channels, tuple(block_out_channels), layers_per_block)
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1)

    @torch.no_grad()
    def encode(self, x: torch.Tensor) -> DiagonalGaussian:
        return DiagonalGaussian(self.quant_conv(self.encoder(x.float())))
