#!/usr/bin/env python3
"""Generate tests/golden/vit_dh32.npz from the reference itself: the ViT of the reference's own tests/test_vit.py
(embed_dim 128, 4 heads: head dim 32).

Run ONLY where the reference is present (VITSSL_REFERENCE, default /root/reference):

    python tests/golden/make_golden_hd.py

Imports the reference's vit_core at generation time only.  The large matrices are overwritten with the closed-form fill of
synth_hd.py before the forward and are not stored; the fixture holds the input, the small tensors of the state_dict, the
shapes of all of them, logits, last-block attention probabilities, the loss and a handful of parameter gradients (whole for the
small tensors, rows / columns / checksums of synth.summarize for the attention weights)."""
import os
import sys

import numpy as np
import torch

REF = os.environ.get("VITSSL_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
OUT = os.path.dirname(os.path.abspath(__file__))

from vit_core.vit import ViT  # noqa: E402

sys.path.insert(0, OUT)
from synth import summarize  # noqa: E402
from synth_hd import big_weights  # noqa: E402

WHOLE_GRADS = ("patch_embedding.cls_token", "patch_embedding.positional_embedding", "classification_head.linear.weight",
               "classification_head.linear.bias", "encoder_blocks.0.layer_norm1.weight", "encoder_blocks.1.layer_norm2.bias",
               "encoder_blocks.1.feed_forward.linear_in.bias")
SUMMARY_GRADS = tuple(f"encoder_blocks.{i}.self_attention.{w}.weight" for i in (0, 1) for w in ("w_query", "w_key", "w_value", "final_linear"))


def npy(t):
    return t.detach().cpu().numpy()


def main():
    torch.manual_seed(31)
    B, img, patch, D, H, F, blocks, C = 4, 32, 8, 128, 4, 256, 2, 10
    model = ViT(num_classes=C, num_blocks=blocks, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H,
                mlp_dim=F, dropout=0.0)
    sd = model.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    big = big_weights(shapes)
    with torch.no_grad():
        for k, a in big.items():
            sd[k].copy_(torch.from_numpy(a))
        for k, v in sd.items():                       # biases and the class token start at zero in the reference: give them values
            if k not in big and float(v.abs().max()) == 0.0:
                v.copy_(0.1 * torch.randn(v.shape))
    g = torch.Generator().manual_seed(32)
    xu8 = torch.randint(0, 256, (B, 3, img, img), generator=g, dtype=torch.uint8)
    x = xu8.float() / 256.0
    labels = torch.tensor([7, 0, 3, 7])
    logits, attn = model(x, return_attn=True)
    loss = torch.nn.CrossEntropyLoss()(logits, labels)
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    arrs = dict(x_u8=npy(xu8), labels=npy(labels), logits=npy(logits), attn=npy(attn), loss=npy(loss),
                cfg=np.array([B, img, patch, D, H, F, blocks, C], dtype=np.int64),
                keys=np.array(list(shapes)), shapes=np.array([",".join(str(s) for s in shapes[k]) for k in shapes]))
    arrs.update({"sd/" + k: npy(v) for k, v in model.state_dict().items() if k not in big})
    arrs.update({"grad/" + k: npy(grads[k]) for k in WHOLE_GRADS})
    for k in SUMMARY_GRADS:
        for part, a in summarize(npy(grads[k])).items():
            arrs[f"gradsum/{k}/{part}"] = a
    path = os.path.join(OUT, "vit_dh32.npz")
    np.savez_compressed(path, **arrs)
    print(f"vit_dh32: {os.path.getsize(path) / 1024:.0f} KiB, {len(arrs)} arrays, loss {float(loss.detach()):.4f}, "
          f"max prob {float(attn.max()):.3f}")


if __name__ == "__main__":
    main()
