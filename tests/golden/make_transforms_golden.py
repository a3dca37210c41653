"""Writes tests/golden/transforms.npz: inputs, boxes, flips and expected uint8 outputs of the crop / resize / flip part of
the reference's SimMIM, supervised, finetune and eval transform lists (configs/*/train_transforms.yaml,
configs/*/val_transforms.yaml, configs/*_eval/transforms.yaml), produced by Pillow itself -- the library torchvision's
PIL path calls for them (torchvision is not installed here; its wrappers are spelled out from their published source):
    F.resized_crop(img, top, left, h, w, size) = img.crop((left, top, left + w, top + h)).resize(size[::-1], BILINEAR)
    F.hflip(img)                               = img.transpose(FLIP_LEFT_RIGHT)
    F.resize(img, [h, w])                      = img.resize((w, h), BILINEAR)
ToTensor is uint8 -> float32 / 255, channel-first; the tests apply it to the stored uint8 images with torch.

The small images are smooth patterns plus noise; the 600x500 one is made of 6x6 blocks of random colours under a diagonal
ramp (edges everywhere, but few distinct bytes), so that the compressed file stays well under the size limit.

    python tests/golden/make_transforms_golden.py
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))

# name, H, W, (top, left, h, w), (SH, SW), flip
CASES = [
    ("rect_crop_flip", 120, 160, (7, 13, 90, 121), (64, 48), 1),
    ("up_32_to_224", 32, 32, (1, 0, 30, 31), (224, 224), 0),
    ("down_600x500_to_384", 600, 500, (12, 9, 575, 480), (384, 384), 1),
    ("resize_96_to_192", 96, 96, (0, 0, 96, 96), (192, 192), 0),
]


def make_image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 120 * np.sin(xx / 7.0 + yy / 11.0), 127 + 120 * np.cos(xx / 5.0 - yy / 3.0), (xx * yy) % 256], -1)
    return np.clip(base + rng.normal(0, 20, base.shape), 0, 255).astype(np.uint8)


def make_block_image(h, w, seed, cell=6):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    blocks = rng.integers(0, 224, ((h + cell - 1) // cell, (w + cell - 1) // cell, 3)).repeat(cell, 0).repeat(cell, 1)[:h, :w]
    return (blocks + ((xx + yy) // 37 % 32)[..., None]).astype(np.uint8)


def main():
    out = {"names": np.array([c[0] for c in CASES])}
    for n, (name, H, W, (top, left, h, w), (SH, SW), flip) in enumerate(CASES):
        img = make_block_image(H, W, 100 + n) if H * W > 100000 else make_image(H, W, 100 + n)
        pil = Image.fromarray(img)
        if name.startswith("resize"):
            res = pil.resize((SW, SH), Image.BILINEAR)
        else:
            res = pil.crop((left, top, left + w, top + h)).resize((SW, SH), Image.BILINEAR)
        if flip:
            res = res.transpose(Image.FLIP_LEFT_RIGHT)
        out[f"{name}_img"] = img
        out[f"{name}_params"] = np.array([top, left, h, w, flip, SH, SW], np.int32)
        out[f"{name}_out"] = np.array(res)
        assert out[f"{name}_out"].shape == (SH, SW, 3)
    path = os.path.join(HERE, "transforms.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
