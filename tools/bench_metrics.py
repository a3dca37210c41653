#!/usr/bin/env python3
"""The two metric kernels of include/vitssl_metrics.h at the workload shapes, against torch formulations of the same
quantities on the same device tensors:

  recon   n = 29 952 patches (a 256-image batch, 117 masked patches each), C = 3, P = 16: ops.recon_metrics versus a torch
          SSIM + squared error (reflect pad, grouped conv2d of x, y, x^2, y^2, xy with the 11 x 11 Gaussian, fp32)
  stats   G = 2, V = 10, B = 64, K = 65 536: ops.dino_stats versus the reference's CosineSimMetric body (norms, the
          broadcast [G, V, B, K] product, mean) plus mean / var of both tensors and the norm of the centre

Both arms of a pair are timed alternately with HIP events around `--inner` back-to-back calls per sample; results are compared
in fp64.  Bytes per call are what the algorithm must read (both inputs once).

usage: bench_metrics.py [--repeats 50] [--inner 5] [--warmup 5]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from utils.gpu_metrics import dino_values, recon_values  # noqa: E402
from vitssl_hip import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=50)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--warmup", type=int, default=5)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_metrics: no GPU visible (there is nothing to measure on a CPU)")
dev = torch.device("cuda:0")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.inner          # us per call


def compare(arms, nbytes):
    samples = {k: [] for k in arms}
    for r in range(a.warmup + a.repeats):
        for k, fn in arms.items():                       # alternating: both arms see the same clocks and neighbours
            t = timed(fn)
            if r >= a.warmup:
                samples[k].append(t)
    med = {}
    for k, us in samples.items():
        us = np.sort(np.asarray(us))
        med[k] = float(np.median(us))
        print(f"  {k}: {med[k]:.1f} us (min {us[0]:.1f}, p10 {us[len(us) // 10]:.1f} .. p90 {us[-1 - len(us) // 10]:.1f})   "
              f"{nbytes / med[k] / 1e3:.0f} GB/s of the bytes a call must read")
    return med


props = torch.cuda.get_device_properties(0)
print(f"device: {props.name} ({getattr(props, 'gcnArchName', '?').split(':')[0]}, {props.multi_processor_count} CUs); {a.repeats} samples of "
      f"{a.inner} back-to-back calls, {a.warmup} warm-up samples; times are us per call: median (min, p10 .. p90)")
gen = torch.Generator().manual_seed(1)

# ---- reconstruction metrics
n, Cc, Pp = 29952, 3, 16
pred = (0.5 + 0.5 * torch.randn(n, Cc * Pp * Pp, generator=gen)).to(dev)
target = torch.rand(n, Cc * Pp * Pp, generator=gen).to(dev)
acc = torch.zeros(4, dtype=torch.float64, device=dev)
half = (11 - 1) * 0.5
g1 = torch.exp(-0.5 * (torch.linspace(-half, half, 11) / 1.5) ** 2)
g1 = (g1 / g1.sum()).unsqueeze(0)
kernel = (g1.t() @ g1).expand(Cc, 1, -1, -1).contiguous().to(dev)
torch_out = {}


def recon_kernel():
    acc.zero_()
    ops.recon_metrics(pred, target, acc, Cc, Pp)


def recon_torch():
    x, y = pred.clamp(0, 1).view(-1, Cc, Pp, Pp), target.view(-1, Cc, Pp, Pp)
    sse = ((x - y).double() ** 2).sum()
    xp, yp = F.pad(x, [5] * 4, mode="reflect"), F.pad(y, [5] * 4, mode="reflect")
    out = F.conv2d(torch.cat([xp, yp, xp * xp, yp * yp, xp * yp]), kernel, groups=Cc)
    mx, my, exx, eyy, exy = (out[i * n:(i + 1) * n] for i in range(5))
    a1, a2 = 2 * mx * my + 1e-4, 2 * (exy - mx * my) + 9e-4
    b1, b2 = mx * mx + my * my + 1e-4, (exx - mx * mx) + (eyy - my * my) + 9e-4
    torch_out["recon"] = (sse, ((a1 * a2) / (b1 * b2)).mean((1, 2, 3), dtype=torch.float64).sum())


nbytes = 2 * pred.numel() * 4
print(f"\nrecon: n={n} C={Cc} P={Pp}, {nbytes / 1e6:.0f} MB to read per call")
med = compare({"recon_metrics kernel (2 launches)": recon_kernel, "torch conv2d SSIM + squared error (fp32)": recon_torch}, nbytes)
torch.cuda.synchronize()
k, t = recon_values(acc.cpu()), recon_values(torch.stack([*torch_out["recon"], acc[2], acc[3]]).cpu())
print(f"  kernel PSNR {k['PSNR']:.6f} SSIM {k['SSIM']:.8f};  torch fp32 PSNR {t['PSNR']:.6f} SSIM {t['SSIM']:.8f};  "
      f"torch / kernel time {list(med.values())[1] / list(med.values())[0]:.2f}x")
del pred, target

# ---- DINO statistics
G, V, B, K = 2, 10, 64, 65536
teacher = (0.3 + 1.5 * torch.randn(G, B, K, generator=gen)).to(dev)
student = (0.7 * torch.randn(V, B, K, generator=gen) - 0.2).to(dev)
center = (0.05 + 0.1 * torch.randn(K, generator=gen)).to(dev)
out = torch.empty(8, dtype=torch.float64, device=dev)


def stats_kernel():
    ops.dino_stats(teacher, student, center, out)


def stats_torch():
    tn, sn = torch.linalg.norm(teacher, dim=-1), torch.linalg.norm(student, dim=-1)
    dot = (teacher.unsqueeze(1) * student.unsqueeze(0)).sum(dim=-1)          # the [G, V, B, K] product of CosineSimMetric
    cos = (dot / (tn.unsqueeze(1) * sn.unsqueeze(0) + 1e-8)).mean()
    tf, sf = teacher.flatten(), student.flatten()
    torch_out["stats"] = {"CenterNorm": torch.linalg.norm(center), "TeacherMean": tf.mean(), "TeacherSTD": tf.std(), "TeacherVar": tf.var(),
                          "StudentMean": sf.mean(), "StudentSTD": sf.std(), "StudentVar": sf.var(), "CosineSim": cos}


nbytes = (teacher.numel() + student.numel() + center.numel()) * 4
print(f"\nstats: G={G} V={V} B={B} K={K}, {nbytes / 1e6:.0f} MB to read per call (the torch arm also writes and reads a "
      f"{G * V * B * K * 4 / 1e6:.0f} MB product)")
med = compare({"dino_stats kernel (2 launches)": stats_kernel, "torch: CosineSimMetric body + mean/std/var + norm (14 reductions)": stats_torch}, nbytes)
torch.cuda.synchronize()
k = dino_values(out.cpu(), G * V * B)
worst = max(abs(float(v) - k[name]) / abs(k[name]) for name, v in torch_out["stats"].items())
print(f"  kernel {k}\n  largest relative difference of the torch fp32 values from the kernel's: {worst:.2e};  "
      f"torch / kernel time {list(med.values())[1] / list(med.values())[0]:.2f}x")
