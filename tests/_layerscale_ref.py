"""LayerScale, restated for the tests (no GPU code).

The unchanged oracle expresses LayerScale: oracle.vit_oracle.encoder_block multiplies the two residual branches by arbitrary
float tensors keep[0] / keep[2], so keep = (g1.view(1, 1, D) * k1, k_inner, g2.view(1, 1, D) * k2) with g1 / g2 leaves that
require grad gives x + g (.) drop(branch) and gamma's gradient through autograd (k1 / k2: the dropout masks times the drop-path
branch scales of tests/_droppath_ref.py, or ones).  Compositions for the supervised ViT, SimMIM, the DINO student and teacher
and a lone block, next to those of tests/_droppath_ref.py."""
import torch

import _droppath_ref as DP
from oracle import vit_oracle as O


def gamma_names(pre, i):
    return f"{pre}encoder_blocks.{i}.layer_scale1.gamma", f"{pre}encoder_blocks.{i}.layer_scale2.gamma"


def random_gammas(sd, D, seed=21, pre=""):
    """per-channel values in +-[0.5, 1.5], different for every branch: with init-sized gammas the branches vanish and a broken
    kernel would pass"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in sd:
        if k.startswith(pre) and k.endswith(("layer_scale1.gamma", "layer_scale2.gamma")):
            mag = 0.5 + torch.rand(D, generator=g)
            sign = torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0)
            out[k] = mag * sign
    return out


def keeps(sd, L, B, T, D, F, pre="", base=None, swap=None, block_names=None):
    """the oracle's per-block keep triples with the block's gammas folded into keep[0] / keep[2]; `base` = the triples of
    _droppath_ref.oracle_keeps (dropout masks x drop-path scales) or None = ones; `swap` = a block whose g1 / g2 are exchanged
    (the negative control of the model tests)"""
    out = []
    for i in range(L):
        n1, n2 = gamma_names(pre, i) if block_names is None else block_names[i]
        if swap == i:
            n1, n2 = n2, n1
        k1, ki, k2 = base[i] if base is not None else (torch.ones(B, T, D), torch.ones(B, T, F), torch.ones(B, T, D))
        out.append((sd[n1].view(1, 1, D) * k1, ki, sd[n2].view(1, 1, D) * k2))
    return out


def vit_forward(sd, x, patch, num_heads, D, F, base=None, p_drop=0.0, emu="bf16", swap=None):
    L = O.num_blocks_of(sd)
    T = (x.shape[2] // patch) * (x.shape[3] // patch) + 1
    return DP.vit_forward(sd, x, patch, num_heads, keeps(sd, L, x.shape[0], T, D, F, base=base, swap=swap), p_drop=p_drop, emu=emu)


def simmim_forward(sd, x, mask, patch, num_heads, D, F, base=None, p_drop=0.0, emu="bf16"):
    L = O.num_blocks_of(sd)
    return O.simmim_forward(sd, x, mask, patch, num_heads, emu=emu, keeps=keeps(sd, L, x.shape[0], mask.shape[1], D, F, base=base),
                            p_drop=p_drop)


def simmim_inference(sd, x, patch, num_heads, D, F, emu="bf16", return_patch_features=False):
    """oracle.vit_oracle.simmim_inference with the gammas (the oracle's own passes no keeps)"""
    patches = O.patchify(x, patch)
    h = O.linear(patches, sd["projection.weight"], sd["projection.bias"], emu) + sd["positional_embedding"]
    L = O.num_blocks_of(sd)
    ks = keeps(sd, L, x.shape[0], h.shape[1], D, F)
    for i in range(L):
        h, _ = O.encoder_block(h, sd, f"encoder_blocks.{i}.", num_heads, emu, keep=ks[i], p_drop=0.0)
    return h if return_patch_features else h.mean(dim=1)


def dino_branch(sd, who, x, patch, num_heads, grid, D, F, base=None, emu="bf16"):
    """`who`_head of `who`_backbone (student or teacher) with the gammas"""
    pre = f"{who}_backbone."
    h = O.dynamic_patch_embed(x, sd, pre + "patch_embedding.", patch, grid, emu)
    L = O.num_blocks_of(sd, pre + "encoder_blocks.")
    ks = keeps(sd, L, x.shape[0], h.shape[1], D, F, pre=pre, base=base)
    for i in range(L):
        h, _ = O.encoder_block(h, sd, pre + f"encoder_blocks.{i}.", num_heads, emu, keep=ks[i], p_drop=0.0)
    return O.dino_head(sd, f"{who}_head.", h[:, 0], emu)


def block_forward(sd, x, num_heads, D, F, emu="bf16"):
    """a lone EncoderBlock (keys without a prefix)"""
    B, T, _ = x.shape
    ks = keeps(sd, 1, B, T, D, F, block_names=[("layer_scale1.gamma", "layer_scale2.gamma")])
    return O.encoder_block(x, sd, "", num_heads, emu, keep=ks[0], p_drop=0.0)[0]


def plain_block(x, sd, pre, num_heads):
    """x + g (.) branch in plain torch, fp32: the restatement the oracle's keep route is checked against"""
    h = torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[pre + "layer_norm1.weight"], sd[pre + "layer_norm1.bias"])
    a, _ = O.mha(h, sd, pre + "self_attention.", num_heads, None)
    x = x + sd[pre + "layer_scale1.gamma"] * a
    h = torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[pre + "layer_norm2.weight"], sd[pre + "layer_norm2.bias"])
    f = O.feed_forward(h, sd, pre + "feed_forward.", None)
    return x + sd[pre + "layer_scale2.gamma"] * f
