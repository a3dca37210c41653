#!/usr/bin/env python3
"""The fused transform-list kernel (vitssl_tf_resized_crop_to_tensor: crop, Pillow BILINEAR resize, flip, ToTensor in one
launch) on uint8 batches already on the device, boxes of RandomResizedCrop(scale [0.9, 1.0]) + flip drawn with a fixed seed:
time per call, achieved GB/s against the bytes the call must move -- sum over the images of h * w * 3 (its box, uint8) +
3 * S * S * 4 (its float32 output) -- and images/s.

For S = 224 the same result is also produced the only way the DINO kernels can produce it (two entry points, three
launches, uint8 `tmp` and `dst` round trips through device memory): vitssl_aug_resized_crop_u8 followed by
vitssl_aug_blur_to_tensor with the seven taps 0,0,0,1,0,0,0 (a blur that is arithmetically ToTensor).  Both are timed on the
same tensors, alternating, with HIP events around `--inner` back-to-back calls per sample; the outputs are compared.

usage: bench_transforms.py [--repeats 60] [--inner 10] [--warmup 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from data import TransformSpec, sample_transform_params  # noqa: E402
from data.transforms import pack_transform_params  # noqa: E402
from vitssl_hip import ops  # noqa: E402

SHAPES = [(256, 256, 256, 224), (256, 96, 96, 224), (64, 600, 600, 512)]      # B, H, W, S

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=60)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()
if a.repeats < 50:
    sys.exit("bench_transforms: at least 50 repeats")
if not torch.cuda.is_available():
    sys.exit("bench_transforms: no GPU visible (there is nothing to measure on a CPU)")
dev = torch.device("cuda:0")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.inner          # us per call


def stats(us):
    us = np.sort(np.asarray(us))
    return float(np.median(us)), float(us[0]), float(us[len(us) // 10]), float(us[-1 - len(us) // 10])


props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} ({getattr(props, 'gcnArchName', '?').split(':')[0]}, {props.multi_processor_count} CUs, "
      f"{props.total_memory / 2**30:.0f} GiB); {a.repeats} samples of {a.inner} back-to-back calls, {a.warmup} warm-up samples; "
      "times are us per call: median (min, p10 .. p90)")
print("every call of an arm reads and writes the same tensors, so a source set that fits the last-level cache stays in it between "
      "calls:\nGB/s is the rate over the bytes a call must move, not a measured HBM rate")
for B, H, W, S in SHAPES:
    gen = torch.Generator().manual_seed(B + H + S)
    imgs = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=gen).to(dev)
    spec = TransformSpec(kind="crop", size=(S, S), scale=(0.9, 1.0))
    prm = sample_transform_params(spec, H, W, B, gen)
    ip5 = torch.from_numpy(pack_transform_params(prm)).to(dev)
    out = torch.empty(B, 3, S, S, device=dev)
    need = int((np.asarray(prm["h"]) * np.asarray(prm["w"]) * 3).sum()) + B * 3 * S * S * 4
    fused = lambda: ops.tf_resized_crop_to_tensor(imgs, ip5, out)                                       # noqa: E731
    arms = {"fused (1 launch)": fused}
    if S == 224:
        ip11 = torch.zeros(B, ops.AUG_IP, dtype=torch.int32, device=dev)
        ip11[:, :5] = ip5
        fp = torch.zeros(B, ops.AUG_FP, device=dev)
        fp[:, 3 + 3] = 1.0
        tmp = torch.empty(B, H, S, 3, dtype=torch.uint8, device=dev)
        u8 = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
        out2 = torch.empty(B, 3, S, S, device=dev)

        def parent():
            ops.aug_resized_crop_u8(imgs, ip11, tmp, u8)
            ops.aug_blur_to_tensor(u8, fp, out2, 7)
        arms["aug_resized_crop_u8 + aug_blur_to_tensor(identity taps) (3 launches)"] = parent
    samples = {k: [] for k in arms}
    for r in range(a.warmup + a.repeats):
        for k, fn in arms.items():                       # alternating: both arms see the same clocks and neighbours
            t = timed(fn)
            if r >= a.warmup:
                samples[k].append(t)
    print(f"\nB={B} {H}x{W} -> {S}x{S}: {ops.tf_tile_rows(H, W, S, S)} output rows per tile, {need / 1e6:.1f} MB to move per call "
          f"({B * H * W * 3 / 1e6:.1f} MB of uint8 source images)")
    med = {}
    for k, us in samples.items():
        m, lo, p10, p90 = stats(us)
        med[k] = (m, p10, p90)
        print(f"  {k}: {m:.1f} us ({lo:.1f}, {p10:.1f} .. {p90:.1f})   {need / m / 1e3:.0f} GB/s of the byte floor   {B / m * 1e6:.0f} images/s")
    if S == 224:
        torch.cuda.synchronize()
        (f, f10, f90), (p, p10, p90) = med.values()
        print(f"  outputs equal: {bool(torch.equal(out, out2))};  fused is {p / f:.2f}x the two-entry-point formulation "
              f"(medians; spread p10 .. p90: fused {100 * (f90 - f10) / f:.1f} %, parent {100 * (p90 - p10) / p:.1f} % of the median; "
              f"slowest fused sample band {f90:.1f} us vs fastest parent band {p10:.1f} us)")
