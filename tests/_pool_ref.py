"""Torch restatement of global average pooling (csrc/pool.hip, include_addons/vitssl_pool.h) and of the ViT forward that reads
its head input through it, for the pooling tests.  fp32 on the CPU; the scale is the fp32 quotient the entry points compute."""
import numpy as np
import torch

from oracle import vit_oracle as O

POOLS = ("cls", "avg")


def scale(T):
    """r = 1.0f / (float)(T - 1) as an fp32 value"""
    return float(np.float32(1) / np.float32(T - 1))


def pool_fwd(x, B, T):
    """x f32 [B*T, D] -> f32 [B, D]: r * (fp32 sum of the rows 1 .. T-1 of every image); row 0, the CLS row, is not read."""
    x = x.view(B, T, -1)
    assert x.dtype == torch.float32
    return x[:, 1:].sum(1, dtype=torch.float32) * torch.tensor(scale(T), dtype=torch.float32)


def pool_bwd(dout, B, T):
    """dout f32 [B, D] -> g f32 [B*T, D]: +0 in every CLS row, r * dout[b] in every other row of image b."""
    assert dout.dtype == torch.float32 and dout.shape[0] == B
    g = torch.zeros(B, T, dout.shape[1], dtype=torch.float32)
    g[:, 1:] = (dout * torch.tensor(scale(T), dtype=torch.float32))[:, None]
    return g.view(B * T, -1)


def vit_forward(sd, x, patch, heads, pool, emu, return_attn=False):
    """oracle.vit_oracle.vit_forward with the head input chosen by `pool`: "cls" = row 0 of the last block's output (the oracle's
    own arithmetic, operation for operation), "avg" = r * the sum of its patch rows, taken in fp32 on the unrounded stream."""
    assert pool in POOLS
    h = O.conv_patch_embed(x, sd["patch_embedding.conv.weight"], sd["patch_embedding.conv.bias"], sd["patch_embedding.cls_token"],
                           sd["patch_embedding.positional_embedding"], patch, emu)
    probs = None
    for i in range(O.num_blocks_of(sd)):
        h, probs = O.encoder_block(h, sd, f"encoder_blocks.{i}.", heads, emu, return_attn=return_attn)
    c = h[:, 0] if pool == "cls" else h[:, 1:].sum(1) * scale(h.shape[1])
    c = O.rnd(O.layer_norm(c, sd["classification_head.norm.weight"], sd["classification_head.norm.bias"]), emu)
    logits = O.linear(c, sd["classification_head.linear.weight"], sd["classification_head.linear.bias"], emu)
    return (logits, probs) if return_attn else logits
