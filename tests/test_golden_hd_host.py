"""No GPU needed: the CPU oracle against tests/golden/vit_dh32.npz, the reference's own outputs for the ViT of its
tests/test_vit.py (embed_dim 128, 4 heads: head dim 32; tests/golden/make_golden_hd.py), and the fixture's size."""
import os

import _hd_golden as G
from _util import GOLDEN, rel_l2, t
from oracle import vit_oracle as O

TOL = 2e-5          # the bar of tests/test_oracle_golden.py


def test_fixture_is_small():
    size = os.path.getsize(os.path.join(GOLDEN, "vit_dh32.npz"))
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f != "vit_dh32.npz")
    assert size <= largest and size < (1 << 20)


def test_oracle_matches_the_reference_at_dh32():
    g, sd, (B, img, patch, D, H, F, blocks, C) = G.load()
    assert D // H == 32
    x = t(g["x_u8"]).float() / 256.0
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logits, attn = O.vit_forward(leaves, x, patch, H, return_attn=True)
    assert attn.shape == (B, H, 17, 17)
    assert rel_l2(logits, t(g["logits"])) < TOL and rel_l2(attn, t(g["attn"])) < TOL
    loss = O.cross_entropy_mean(logits, t(g["labels"]))
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5
    loss.backward()
    G.check_grads({k: v.grad for k, v in leaves.items()}, g, 2e-4)
