#!/usr/bin/env python3
"""Generate tests/golden/simmim_p14.npz from the reference itself: its SimMIMViT at patch 14 on 42 x 42 RGB images (a 3 x 3
grid, patch width 588), a geometry whose patch side is no multiple of 4 and whose patch width is no multiple of 64.

Run ONLY where the reference is present (VITSSL_REFERENCE, default /root/reference):

    python tests/golden/make_golden_patch.py

Imports the reference's vit_core at generation time only.  The fixture holds the input, the mask the reference drew, the whole
state_dict, prediction, targets, loss, the mean-pooled inference features and the gradients of the patch-facing parameters and
of one tensor of every other kind (the layout of simmim_tiny.npz, gradients restricted to keep the file small)."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("VITSSL_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
OUT = os.path.dirname(os.path.abspath(__file__))

from vit_core.ssl.simmim.model import SimMIMViT  # noqa: E402

GRADS = ("projection.weight", "projection.bias", "simmim_head.bias", "mask_token", "positional_embedding",
         "encoder_blocks.0.self_attention.w_query.weight", "encoder_blocks.1.feed_forward.linear_out.bias",
         "encoder_blocks.1.layer_norm2.weight")
HEAD_ROWS = (0, 13, 195, 196, 391, 392, 587)       # rows of d(simmim_head.weight): first / last feature of every channel


def npy(t):
    return t.detach().cpu().numpy()


def main():
    seed, B, img, patch, D, H, F, blocks, ratio = 41, 3, 42, 14, 64, 1, 64, 2, 0.6
    torch.manual_seed(seed)
    model = SimMIMViT(num_blocks=blocks, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H, mlp_dim=F,
                      dropout=0.0, mask_ratio=ratio)
    model.train()
    g = torch.Generator().manual_seed(seed + 1)
    xu8 = torch.randint(0, 256, (B, 3, img, img), generator=g, dtype=torch.uint8)
    x = xu8.float() / 256.0
    torch.manual_seed(seed + 2)                     # the masking RNG state the oracle must replay
    pred, tgt, bm = model(x, return_bool_mask=True)
    loss = torch.nn.L1Loss(reduction="mean")(pred, tgt)
    loss.backward()
    with torch.no_grad():
        model.eval()
        feat = model.inference_forward(x)
    grads = {k: p.grad for k, p in model.named_parameters()}
    arrs = dict(x_u8=npy(xu8), mask=npy(bm[..., 0]), pred=npy(pred), targets=npy(tgt), loss=npy(loss), feat=npy(feat),
                cfg=np.array([B, img, patch, D, H, F, blocks], dtype=np.int64), ratio=np.array(ratio), mask_seed=np.array(seed + 2),
                head_rows=np.array(HEAD_ROWS, dtype=np.int64))
    arrs.update({"sd/" + k: npy(v) for k, v in model.state_dict().items()})
    arrs.update({"grad/" + k: npy(grads[k]) for k in GRADS})
    arrs["gradrows/simmim_head.weight"] = npy(grads["simmim_head.weight"][list(HEAD_ROWS)])
    path = os.path.join(OUT, "simmim_p14.npz")
    np.savez_compressed(path, **arrs)
    print(f"simmim_p14: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays, loss {float(loss.detach()):.4f}")


if __name__ == "__main__":
    main()
