"""The CPU oracle reproduces the reference-written patch-14 fixture (tests/golden/simmim_p14.npz, made by
tests/golden/make_golden_patch.py) at the fp32 bars of tests/test_oracle_golden.py: the oracle is the comparator of the GPU
tests at the new geometries, this ties it to the reference there."""
import numpy as np
import torch

from _util import load_golden, split_prefix, t, rel_l2
from oracle import vit_oracle as O

TOL = 2e-5     # tests/test_oracle_golden.py


def test_tolerance_is_the_one_of_the_oracle_golden_tests():
    import test_oracle_golden as G
    assert TOL == G.TOL


def test_simmim_patch14():
    g = load_golden("simmim_p14")
    B, img, patch, D, H, F, blocks = (int(v) for v in g["cfg"])
    assert (patch, img) == (14, 42) and g["targets"].shape[1] == 588
    x = t(g["x_u8"]).float() / 256.0
    torch.manual_seed(int(g["mask_seed"]))
    mask = O.simple_masking(B, (img // patch) ** 2, float(g["ratio"]))
    assert np.array_equal(mask.numpy(), g["mask"])
    sd = split_prefix(g, "sd/")
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pred, tgt = O.simmim_forward(leaves, x, mask, patch, H)
    assert np.array_equal(tgt.numpy(), g["targets"])          # pure gather: bit-exact
    assert rel_l2(pred, t(g["pred"])) < TOL
    loss = O.l1_loss_mean(pred, tgt)
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-6 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    for k, gr in split_prefix(g, "grad/").items():
        assert rel_l2(leaves[k].grad, gr) < 2e-4, k
    rows = [int(r) for r in g["head_rows"]]
    assert rel_l2(leaves["simmim_head.weight"].grad[rows], t(g["gradrows/simmim_head.weight"])) < 2e-4
    assert rel_l2(O.simmim_inference(sd, x, patch, H), t(g["feat"])) < TOL
    pred_e, _ = O.simmim_forward(sd, x, mask, patch, H, emu="bf16")
    assert rel_l2(pred_e, t(g["pred"])) < 3e-2
