"""Conditional UNet "C-UNet" (reference networks/nets/unet_vanilla.py): a pre-convolution, residual down path, nearest-upsample + concat +
residual up path, 1x1x1 head.

The children, their names and order are the reference's (``pre_conv``, ``down_path.{i}.{j}``, ``up_path.{i}.0`` an ``nn.Upsample`` /
``.1``, ``out``), so its published checkpoint loads with ``strict=True``.  The containers and the ``_run_*`` walkers are UNet's
(networks/nets/unet.py): every convolution, norm, activation and dropout runs on the HIP kernels over channels-last activations.  The decoder
step ``torch.concat((skip, upsample(x)), dim=1)`` is one launch (``miseg_upsample_cat``) whose backward sums the upsampled half's gradient
without atomics; the skip's two gradients (next down layer, concat) meet in ``HF.fork``'s add kernel."""
import warnings
from typing import Sequence

import numpy as np
import torch
import torch.nn as nn

from ...hip import functional as HF
from ...hip import ops
from ..norms.conditional_instance_norm import _ConditionalInstanceNorm, styles_limit, styles_to_device
from ..norms.utils import parse_normalization
from .unet import Convolution, ResidualUnit, SequentialWIthModalities, _conv_layer, _run_convolution, _run_residual_unit

__all__ = ["UNetVanilla"]


def _scalar_kernel(k):
    return k[0] if isinstance(k, (list, tuple)) and len(k) == 1 else k


class UNetVanilla(nn.Module):
    def __init__(self, spatial_dims: int, in_channels: int, out_channels: int, channels: Sequence[int], strides: Sequence[int], kernel_size=3,
                 up_kernel_size=3, num_res_units: int = 0, act="PRELU", norm_down="INSTANCE", norm_up="INSTANCE", dropout: float = 0.0,
                 bias: bool = True, adn_ordering: str = "NDA") -> None:
        super().__init__()
        if len(channels) < 2:
            raise ValueError("the length of `channels` should be no less than 2.")
        if len(strides) < len(channels):
            # the reference indexes strides[0] (pre_conv) and strides[1 .. len(channels) - 1] (down path): an IndexError there
            raise ValueError(f"UNetVanilla needs one stride per channel entry: {len(strides)} strides for {len(channels)} channels")
        if len(strides) > len(channels):
            warnings.warn(f"`len(strides) > len(channels)`, the last {len(strides) - len(channels)} values of strides will not be used.")
        kernel_size, up_kernel_size = _scalar_kernel(kernel_size), _scalar_kernel(up_kernel_size)
        if spatial_dims != 3 or isinstance(kernel_size, (list, tuple)) or isinstance(up_kernel_size, (list, tuple)):
            raise NotImplementedError("only spatial_dims=3 with scalar kernel sizes is reproduced")
        for s in strides[:len(channels)]:      # strides[1:] are also the decoder's upsample factors
            if s not in (1, 2):
                raise NotImplementedError(f"UNetVanilla: stride / upsample factor {s} (the MI355X path has 1 and 2)")
        self.dimensions, self.in_channels, self.out_channels = spatial_dims, in_channels, out_channels
        self.channels, self.strides, self.kernel_size, self.up_kernel_size = channels, strides, kernel_size, up_kernel_size
        self.num_res_units, self.act, self.norm_down, self.norm_up = num_res_units, act, norm_down, norm_up
        self.dropout, self.bias, self.adn_ordering = dropout, bias, adn_ordering

        def ru(cin, cout, s, norm):
            return ResidualUnit(3, cin, cout, strides=s, kernel_size=kernel_size, subunits=2, act=act, norm=norm, dropout=dropout, bias=bias,
                                adn_ordering=adn_ordering)

        self.pre_conv = Convolution(3, in_channels, channels[0], strides=strides[0], kernel_size=kernel_size, conv_only=True)
        self.down_path = nn.Sequential()
        self.saved_strides = []
        for scale in range(1, len(channels)):            # unet_vanilla.py:58-98
            layer = SequentialWIthModalities(ru(channels[scale - 1], channels[scale], strides[scale], norm_down))
            self.saved_strides.append(strides[scale])
            for _ in range(1, num_res_units):
                layer.append(ru(channels[scale], channels[scale], 1, norm_down))
            self.down_path.append(layer)
        self.up_path = nn.Sequential()
        for scale in range(len(channels) - 2, -1, -1):   # unet_vanilla.py:100-117
            self.up_path.append(nn.Sequential(nn.Upsample(scale_factor=self.saved_strides[scale]),
                                              ru(channels[scale + 1] + channels[scale], channels[scale], 1, norm_up)))
        self.out = Convolution(3, channels[0], out_channels, kernel_size=1, strides=1, conv_only=True)

    @classmethod
    def from_argparse_args(cls, args):
        d = parse_normalization(args.decoder_norm_name, not args.decoder_norm_no_affine, args.num_groups, args.num_styles)
        e = parse_normalization(args.encoder_norm_name, not args.encoder_norm_no_affine, args.num_groups, args.num_styles)
        fs = args.feature_size
        channels = list(fs) if isinstance(fs, (list, tuple)) else [fs]
        return cls(spatial_dims=args.spatial_dims, in_channels=args.in_channels, out_channels=args.out_channels, channels=channels,
                   strides=args.strides, kernel_size=args.kernel_size, up_kernel_size=args.up_kernel_size, num_res_units=args.num_res_units,
                   act=args.activation, norm_down=e, norm_up=d, dropout=args.dropout_rate, bias=not args.no_bias, adn_ordering=args.adn_ordering)

    # ------------------------------------------------------------------------------------------------------------------
    compute_dtype = torch.float32

    def set_compute_dtype(self, dtype):
        """torch.float32 (parity mode) or torch.bfloat16 (bf16 activations / MFMA, fp32 statistics and parameters)."""
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("compute dtype must be float32 or bfloat16")
        self.compute_dtype = dtype
        return self

    def check_grid(self, grid):
        """every stride-2 layer halves the grid and its upsample doubles it back: the grid must be a multiple of the strides' product (the
        reference's torch.concat fails otherwise)"""
        div = int(np.prod([int(s) for s in self.strides[:len(self.channels)]]))
        if any(int(v) % div for v in grid):
            raise ValueError(f"UNetVanilla: grid {tuple(int(v) for v in grid)} is not a multiple of {div}, the product of the strides "
                             f"{list(self.strides[:len(self.channels)])}")

    def forward(self, x: torch.Tensor, modalities=None) -> torch.Tensor:
        """x [B, C, D, H, W] float; modalities None | list[int] | int64 Tensor[B].  Returns fp32 logits [B, out, D', H', W'] with D' = D /
        strides[0] (unet_vanilla.py:152-169)."""
        self.check_grid(x.shape[2:])
        cond = any(isinstance(m, _ConditionalInstanceNorm) for m in self.modules())
        if cond and modalities is None:
            raise ValueError("Modalities must be passed to the forward step when a norm type is 'instance_cond'.")
        if not x.is_cuda:
            raise RuntimeError("UNetVanilla (MI355X path) needs a HIP device tensor; there is no CPU fallback")
        styles = styles_to_device(modalities, x.device, x.shape[0], styles_limit(self)) if modalities is not None else None
        ops.begin_forward(self.parameters())      # statistics-pool lifetime: hip/ops.py::_ZeroPool
        x = x.float().contiguous()
        if self.in_channels > 4:      # (up to 4 channels the first convolution reads the NCDHW image itself)
            h = _run_convolution(self.pre_conv, HF.image_rows(x, self.compute_dtype), styles)
        else:
            h = _run_convolution(self.pre_conv, None, styles, image=x, dtype=self.compute_dtype)
        skips = []
        for layer in self.down_path:
            # the layer's input is also a skip: its two gradients are summed by the fork's add kernel, not by autograd
            h, skip = HF.fork(h) if h.requires_grad else (h, h)
            skips.append(skip)
            for unit in layer:
                h = _run_residual_unit(unit, h, styles)
        for scale, (up, unit) in enumerate(self.up_path):
            h = HF.upsample_cat(skips[len(self.channels) - 2 - scale], h, _factor(up.scale_factor))
            h = _run_residual_unit(unit, h, styles)
        return HF.to_ncdhw(_conv_layer(self.out.conv, h))


def _factor(scale_factor):
    f = scale_factor[0] if isinstance(scale_factor, (tuple, list)) else scale_factor
    if float(f) not in (1.0, 2.0):
        raise NotImplementedError(f"UNetVanilla: upsample factor {scale_factor} (1 or 2)")
    return int(f)
