"""MAEViT restated from the pieces of oracle/vit_oracle.py (patchify, linear, layer_norm, encoder_block; emu=None: fp32,
emu="bf16": rounded where the HIP path stores bf16), the fixed sin-cos table in NumPy and the loss in fp64.  No GPU code; the
oracle is imported, not changed."""
import numpy as np
import torch

from oracle import vit_oracle as O


def sincos_table(dim, gh, gw):
    """NumPy restatement of the paper's 2-D sin-cos table with a zero CLS row: f32 [1, gh*gw + 1, dim]."""
    def one_d(d, pos):
        omega = 1.0 / 10000 ** (np.arange(d // 2, dtype=np.float64) / (d / 2.0))
        out = pos.reshape(-1)[:, None] * omega[None, :]
        return np.concatenate([np.sin(out), np.cos(out)], axis=1)
    rows = np.repeat(np.arange(gh, dtype=np.float64), gw)          # row-major patches: row index, column index
    cols = np.tile(np.arange(gw, dtype=np.float64), gh)
    table = np.concatenate([one_d(dim // 2, cols), one_d(dim // 2, rows)], axis=1)
    return torch.from_numpy(np.concatenate([np.zeros((1, dim)), table], axis=0)).float()[None]


def shuffle(noise, K):
    """the paper's random_masking on given noise: keep [B, K], restore [B, N], mask bool [B, N]"""
    ids_shuffle = torch.argsort(noise, dim=1)
    ids_restore = torch.argsort(ids_shuffle, dim=1)
    return ids_shuffle[:, :K], ids_restore, ids_restore >= K


def normalise(t):
    """per-row (t - mean) / sqrt(var + 1e-6), unbiased variance, in the input's dtype"""
    mu = t.mean(dim=-1, keepdim=True)
    var = t.var(dim=-1, keepdim=True)
    return (t - mu) / (var + 1.0e-6) ** 0.5


def forward(sd, x, keep, restore, patch, heads, dec_heads, emu=None):
    """-> (pred [Mm, Pd], raw pixel targets [Mm, Pd]); rows are the masked patches in ascending (b, n) order."""
    patches = O.patchify(x, patch)
    B, N, _ = patches.shape
    K = keep.shape[1]
    mask = restore >= K
    D = sd["projection.weight"].shape[0]
    kept = torch.gather(patches, 1, keep[:, :, None].expand(B, K, patches.shape[2]))
    pos = sd["pos_embed"]
    tok = O.linear(kept, sd["projection.weight"], sd["projection.bias"], emu) + torch.gather(pos[0, 1:][None].expand(B, N, D), 1, keep[:, :, None].expand(B, K, D))
    h = torch.cat([(sd["cls_token"] + pos[:, :1]).expand(B, 1, D), tok], dim=1)
    for i in range(O.num_blocks_of(sd, "encoder_blocks.")):
        h, _ = O.encoder_block(h, sd, f"encoder_blocks.{i}.", heads, emu)
    h = O.rnd(O.layer_norm(h, sd["norm.weight"], sd["norm.bias"]), emu)
    y = O.linear(h, sd["decoder_embed.weight"], sd["decoder_embed.bias"], emu)
    Dd = y.shape[-1]
    full = torch.cat([y[:, 1:], sd["mask_token"].expand(B, N - K, Dd)], dim=1)
    full = torch.gather(full, 1, restore[:, :, None].expand(B, N, Dd))
    y = torch.cat([y[:, :1], full], dim=1) + sd["decoder_pos_embed"]
    for i in range(O.num_blocks_of(sd, "decoder_blocks.")):
        y, _ = O.encoder_block(y, sd, f"decoder_blocks.{i}.", dec_heads, emu)
    sel = y[:, 1:][mask]
    hs = O.rnd(O.layer_norm(sel, sd["decoder_norm.weight"], sd["decoder_norm.bias"]), emu)
    return O.linear(hs, sd["decoder_pred.weight"], sd["decoder_pred.bias"], emu), patches[mask]


def inference(sd, x, patch, heads, emu=None):
    """the unmasked encode through `norm`: patch tokens [B, N, D]"""
    patches = O.patchify(x, patch)
    B = patches.shape[0]
    pos = sd["pos_embed"]
    tok = O.linear(patches, sd["projection.weight"], sd["projection.bias"], emu) + pos[:, 1:]
    h = torch.cat([(sd["cls_token"] + pos[:, :1]).expand(B, 1, -1), tok], dim=1)
    for i in range(O.num_blocks_of(sd, "encoder_blocks.")):
        h, _ = O.encoder_block(h, sd, f"encoder_blocks.{i}.", heads, emu)
    return O.rnd(O.layer_norm(h, sd["norm.weight"], sd["norm.bias"]), emu)[:, 1:]


def loss64(pred, targets, norm_pix):
    """fp64: (mean over the rows of mean_c (pred - t)^2, the targets the loss saw)"""
    t = targets.double()
    if norm_pix:
        t = normalise(t)
    return ((pred.double() - t) ** 2).mean(dim=-1).mean(), t
