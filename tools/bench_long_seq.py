#!/usr/bin/env python3
"""Forward + backward of a ViT backbone at patch 8 (224 x 224 images: 784 + 1 = 785 tokens, the DINO model config of the
reference at the resolution README.md quotes), synthetic data: ms per step and the share of it spent in the attention
launches (HIP events around every attention call, ops.PROFILE).   usage: bench_long_seq.py [--model s|b|l|h] [--patch 8] [--batch 32]
(--model l / h --patch 14: ViT-L/14 and ViT-H/14 at 224 x 224, 256 + 1 = 257 tokens)"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import torch
from vit_core import ViT
from vitssl_hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("--model", choices=("s", "b", "l", "h"), default="s")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--img", type=int, default=224)
ap.add_argument("--patch", type=int, default=8)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
D, H, F, blocks = {"s": (384, 6, 1536, 12), "b": (768, 12, 3072, 12), "l": (1024, 16, 4096, 24), "h": (1280, 16, 5120, 32)}[a.model]
dev = torch.device("cuda:0")
torch.manual_seed(0)
m = ViT(num_classes=1000, num_blocks=blocks, input_shape=(3, a.img, a.img), embed_dim=D, patch_size=a.patch, num_heads=H,
        mlp_dim=F, dropout=0.0).to(dev).train()
x = torch.rand(a.batch, 3, a.img, a.img, device=dev)
y = torch.randint(0, 1000, (a.batch,), device=dev)
crit = torch.nn.CrossEntropyLoss()


def step():
    m.zero_grad(set_to_none=True)
    crit(m(x), y).backward()


for _ in range(a.warmup):
    step()
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(a.steps):
    step()
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / a.steps
ops.PROFILE = []
step()
torch.cuda.synchronize()
attn = sum(e0.elapsed_time(e1) for label, _, e0, e1, _ in ops.PROFILE if label.startswith("attn_"))
ops.PROFILE = None
T = (a.img // a.patch) ** 2 + 1
print(f"ViT-{a.model.upper()}/{a.patch} {a.img}x{a.img} ({T} tokens) batch {a.batch}: {dt * 1e3:.1f} ms per forward+backward, "
      f"{a.batch / dt:.0f} img/s, attention {attn:.1f} ms = {100 * attn / (dt * 1e3):.0f} % of the step", flush=True)
