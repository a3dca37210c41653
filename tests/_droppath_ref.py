"""Stochastic depth (drop path), restated for the tests (no GPU code).

  * the table of per-sample branch scales (include/vitssl_droppath.h) in NumPy, from the dropout stream's restatement in
    tests/test_dropout_stream.py: scale[b] = keep_mask(1, B, r, seed, site)[b] ? fp32(65536 / (65536 - round(r * 65536))) : 0;
  * the oracle's `keep` triples that express drop path: oracle.vit_oracle.encoder_block multiplies the two branches by
    arbitrary float tensors keep[0] / keep[2] (times 1 / (1 - p_drop)), so k0 = keep1 * s_att[b] broadcast over [B, T, 1];
  * compositions of the oracle's pieces for the models it has no keeps argument for: the supervised ViT
    (conv_patch_embed + encoder_block + head) and the DINO student backbone (dynamic_patch_embed + encoder_block)."""
import numpy as np
import torch

from oracle import vit_oracle as O
from test_dropout_stream import keep_mask

SITE_BIT = 0x80000000


def site(block, branch, site_base=0):
    """VITSSL_DROPPATH_SITE: branch 0 = attention, 1 = MLP; the high bit keeps the family apart from every dropout site"""
    return SITE_BIT | (site_base + 2 * block + branch)


def rates(rate, layers):
    """linspace(0, rate, layers)"""
    return [0.0] if layers == 1 else [float(v) for v in np.linspace(0.0, rate, layers)]


def r_eff(rate):
    return min(int(rate * 65536.0 + 0.5), 65535) / 65536.0 if rate > 0 else 0.0


def path_scales(B, rate, seed, site_id):
    """f32 [B]: the scales of one (rate, site) row of the table"""
    thr = min(int(rate * 65536.0 + 0.5), 65535) if rate > 0 else 0
    if thr == 0:
        return np.ones(B, np.float32)
    keep = keep_mask(1, (B + 3) // 4 * 4, rate, seed, site_id)[0, :B]         # element b of a [1, B] tensor: group b // 4
    scale = np.float32(65536.0) / np.float32(65536 - thr)                    # one fp32 division, as make_drop_key does it
    return np.where(keep != 0, scale, np.float32(0)).astype(np.float32)


def table(block_rates, B, seed, site_base=0):
    """f32 [2 L, B]: row 2 i = attention branch of block i, row 2 i + 1 = its MLP branch"""
    return np.stack([path_scales(B, r, seed, site(i, br, site_base)) for i, r in enumerate(block_rates) for br in (0, 1)])


def mixed(tab, block_rates):
    """every row of a block with a nonzero rate holds a kept and a dropped sample"""
    return all((tab[2 * i + br] == 0).any() and (tab[2 * i + br] != 0).any()
               for i, r in enumerate(block_rates) if r > 0 for br in (0, 1))


def pick_seed(block_rates, B, start=1, site_base=0, offsets=(0,)):
    """the first seed >= start whose table(s) (one per seed offset: DINO's passes) are mixed(); chosen on the CPU"""
    for seed in range(start, start + 100000):
        if all(mixed(table(block_rates, B, seed + o, site_base), block_rates) for o in offsets):
            return seed
    raise AssertionError("no seed found")


def seed_for_next_draw(block_rates, B, offsets=(0,), start=1):
    """a torch.manual_seed value after which vit_core._runtime.next_seed() returns a pick_seed()-quality step seed"""
    from vit_core import _runtime as R
    for ms in range(start, start + 100000):
        torch.manual_seed(ms)
        seed = R.next_seed()
        if all(mixed(table(block_rates, B, seed + o), block_rates) for o in offsets):
            return ms, seed
    raise AssertionError("no seed found")


def oracle_keeps(tab, T, D, F, dropout_keeps=None):
    """the oracle's per-block (keep1, keep_inner, keep2) for a table [2 L, B] (NumPy or tensor): the dropout masks
    ([B, T, cols] float 0/1, or None = dropout off) times the branch scales broadcast over [B, T, 1]"""
    tab = torch.as_tensor(np.asarray(tab), dtype=torch.float32)
    L, B = tab.shape[0] // 2, tab.shape[1]
    out = []
    for i in range(L):
        k1, ki, k2 = dropout_keeps[i] if dropout_keeps is not None else (torch.ones(B, T, D), torch.ones(B, T, F), torch.ones(B, T, D))
        out.append((k1 * tab[2 * i].view(B, 1, 1), ki, k2 * tab[2 * i + 1].view(B, 1, 1)))
    return out


def vit_forward(sd, x, patch, num_heads, keeps=None, p_drop=0.0, emu="bf16"):
    """oracle.vit_oracle.vit_forward with per-block keeps (the oracle's own takes none)"""
    h = O.conv_patch_embed(x, sd["patch_embedding.conv.weight"], sd["patch_embedding.conv.bias"], sd["patch_embedding.cls_token"],
                           sd["patch_embedding.positional_embedding"], patch, emu)
    for i in range(O.num_blocks_of(sd)):
        h, _ = O.encoder_block(h, sd, f"encoder_blocks.{i}.", num_heads, emu, keep=None if keeps is None else keeps[i], p_drop=p_drop)
    c = O.rnd(O.layer_norm(h[:, 0], sd["classification_head.norm.weight"], sd["classification_head.norm.bias"]), emu)
    return O.linear(c, sd["classification_head.linear.weight"], sd["classification_head.linear.bias"], emu)


def dino_student(sd, x, patch, num_heads, grid, keeps=None, p_drop=0.0, emu="bf16"):
    """student head of the student backbone with per-block keeps (oracle.vit_oracle.dino_backbone takes none)"""
    pre = "student_backbone."
    h = O.dynamic_patch_embed(x, sd, pre + "patch_embedding.", patch, grid, emu)
    for i in range(O.num_blocks_of(sd, pre + "encoder_blocks.")):
        h, _ = O.encoder_block(h, sd, pre + f"encoder_blocks.{i}.", num_heads, emu, keep=None if keeps is None else keeps[i], p_drop=p_drop)
    return O.dino_head(sd, "student_head.", h[:, 0], emu)
