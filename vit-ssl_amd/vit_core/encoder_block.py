"""Pre-LN transformer encoder block (reference: vit_core/encoder_block.py:9-53).

Inside ViT / SimMIMViT / DINOViT the blocks are pure parameter containers: the owning
model runs all blocks through one EncoderStack schedule.  Called on its own, a block
builds a private one-block stack on first use."""
import math
from typing import Optional

import torch
from torch import nn

from . import _runtime as R
from .attention import MultiHeadedAttention
from .feed_forward import FeedForwardBlock
from ._functions import StackRunner


def check_layer_scale_init(value):
    """None (no LayerScale) or the finite float > 0 every gamma starts from; anything else is a ValueError"""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not math.isfinite(value) or not value > 0:
        raise ValueError(f"layer_scale_init must be None or a finite float > 0, got {value!r}")
    return float(value)


class LayerScale(nn.Module):
    """The learnable per-channel scale of one residual branch (timm's LayerScale / init_values): a parameter container with one
    `gamma` [dim] filled with `init`.  The multiply itself happens in the residual GEMM's epilogue (include/vitssl_layerscale.h)."""

    def __init__(self, dim: int, init: float):
        super().__init__()
        self.gamma = nn.Parameter(torch.full((dim,), check_layer_scale_init(float(init))))


class EncoderBlock(nn.Module):
    # (layer_scale_init is keyword-only and sits in front of drop_path, which stays the last parameter of the signature)
    def __init__(self, d_model: int = 512, num_heads: int = 8, mlp_dim: int = 3072, dropout: float = 0.1, *,
                 layer_scale_init: Optional[float] = None, drop_path: float = 0.0):
        super().__init__()
        self.self_attention = MultiHeadedAttention(d_model, num_heads)
        self.feed_forward = FeedForwardBlock(d_model, mlp_dim, dropout)
        self.layer_norm1 = nn.LayerNorm(d_model)
        self.layer_norm2 = nn.LayerNorm(d_model)
        self.drop1 = nn.Dropout(dropout)
        self.drop2 = nn.Dropout(dropout)
        # stochastic depth of a block called on its own: the probability of dropping a sample from each residual branch
        # (inside a model the owning stack holds the per-block rates; not a parameter, no state_dict key)
        self.drop_path = float(drop_path)
        if not 0.0 <= self.drop_path < 1.0:
            raise ValueError(f"drop_path must lie in [0, 1), got {drop_path}")
        # LayerScale: x + gamma1 (.) attention branch, x + gamma2 (.) MLP branch.  Registered after every other submodule, so the
        # fused-QKV span and every existing offset of the flat store stay where they are; None: no parameter, no key, no launch.
        self.layer_scale_init = check_layer_scale_init(layer_scale_init)
        if self.layer_scale_init is not None:
            self.layer_scale1 = LayerScale(d_model, self.layer_scale_init)
            self.layer_scale2 = LayerScale(d_model, self.layer_scale_init)
        self._cfg = (d_model, num_heads, mlp_dim, dropout)
        self._runner = None

    def forward(self, x: torch.Tensor, return_attn=False):
        R.require_gpu(x, "EncoderBlock")
        if self._runner is None or not self._runner.valid_for(x.device):
            d, h, f, p = self._cfg
            object.__setattr__(self, "_runner", StackRunner(self, [""], d, h, f, p, x.device, drop_path=[self.drop_path],
                                                                layer_scale=self.layer_scale_init is not None))
        return self._runner(x, self.training, return_attn)
