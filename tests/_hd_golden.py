"""Loader of tests/golden/vit_dh32.npz (no GPU code): the stored small tensors plus the large matrices rebuilt by
tests/golden/synth_hd.py, and the comparison of a set of gradients with the stored ones."""
import torch

from _util import load_golden, rel_l2, split_prefix, t
from synth import summarize
from synth_hd import big_weights


def load():
    """-> (arrays, state_dict in the reference's key order, cfg = (B, img, patch, D, H, F, blocks, C))"""
    g = load_golden("vit_dh32")
    shapes = {str(k): tuple(int(x) for x in str(s).split(",") if x) for k, s in zip(g["keys"], g["shapes"])}
    small, big = split_prefix(g, "sd/"), big_weights(shapes)
    sd = {k: (t(big[k]) if k in big else small[k]) for k in shapes}
    assert all(tuple(sd[k].shape) == shapes[k] for k in shapes)
    return g, sd, tuple(int(v) for v in g["cfg"])


def check_grads(grads, g, tol):
    """grads: {key: tensor}; whole tensors under grad/, rows / columns / checksums (synth.summarize) under gradsum/"""
    whole = split_prefix(g, "grad/")
    assert len(whole) >= 5
    for k, ref in whole.items():
        assert rel_l2(grads[k], ref) < tol, (k, rel_l2(grads[k], ref))
    summed = sorted({k.split("/")[1] for k in g if k.startswith("gradsum/")})
    assert len(summed) == 8
    for k in summed:
        s = summarize(grads[k].detach().float().cpu().numpy())
        for part in ("rows", "cols"):
            assert rel_l2(t(s[part]), t(g[f"gradsum/{k}/{part}"])) < tol, (k, part, rel_l2(t(s[part]), t(g[f"gradsum/{k}/{part}"])))
        assert abs(s["stats"][1] - g[f"gradsum/{k}/stats"][1]) < 2 * tol * g[f"gradsum/{k}/stats"][1], (k, "sum of squares")
