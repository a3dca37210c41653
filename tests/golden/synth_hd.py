"""Regenerable fill for the large matrices of the dh = 32 ViT fixture (vit_dh32.npz): make_golden_hd.py overwrites every weight
of 4096 elements or more in the reference model with synth.synth_weight (closed form, indexed by the key's position in the
state_dict) and stores only the small tensors; the tests rebuild the large ones here."""
import numpy as np

from synth import synth_weight

BIG = 4096


def big_weights(shapes):
    """shapes: {state_dict key: shape}, in state_dict order -> {key: array} for the keys with >= BIG elements.  A conv weight
    [E, C, P, P] is filled as the [E, C * P * P] matrix it is applied as; the scale is 1 / sqrt(fan_in)."""
    out = {}
    for c, (k, shape) in enumerate(shapes.items()):
        n = int(np.prod(shape)) if len(shape) else 1
        if n < BIG or len(shape) < 2:
            continue
        rows, cols = int(shape[0]), n // int(shape[0])
        out[k] = synth_weight((rows, cols), c, 1.7 / np.sqrt(cols)).reshape(shape)
    return out
