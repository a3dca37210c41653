#!/usr/bin/env python3
"""Supervised / fine-tune step on synthetic batches: the autograd path of SupervisedTrainer against ViT.train_step in its three
backward schedules (full, input-gradient only = freeze_backbone, head only = the CLS token frozen too).

usage: python tools/bench_finetune.py [--models vit_s,vit_b] [--batch 256] [--steps 20] [--rounds 5] > profiles/finetune_ab.txt

Timing: every variant owns a model; a round times `--steps` steps of each variant in turn (device events around the window, one
synchronise at its end), and the rounds are repeated, so drifts of the machine hit all variants alike.  Reported per variant:
the median round in ms/step and img/s, and the spread (min .. max over the rounds).  The autograd variant is the step as the
trainer's default path runs it, its per-batch `int((logits.argmax(1) == labels).sum())` host read included.
Memory: torch.cuda.max_memory_allocated of three steps of each variant ALONE in the process (model, optimizer state and
workspaces included), taken before the timing models are built.
Before timing, the full-schedule train_step is compared with the autograd path on the same weights and batch (largest
relative L2 over the parameter gradients, loss difference)."""
import argparse
import gc
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd")):
    sys.path.insert(0, p)

MODELS = {"vit_s": dict(embed_dim=384, num_blocks=12, num_heads=6, mlp_dim=1536),
          "vit_b": dict(embed_dim=768, num_blocks=12, num_heads=12, mlp_dim=3072)}
VARIANTS = ["autograd", "full", "input_grad", "head"]


def build(name, variant, dev, classes, img, seed=1, dropout=0.1):
    from utils.model_builder import freeze_backbone
    from vit_core.vit import ViT
    from vitssl_hip.optim import FusedAdamW
    torch.manual_seed(seed)
    model = ViT(num_classes=classes, input_shape=(3, img, img), patch_size=16, dropout=dropout, **MODELS[name]).to(dev).train()
    if variant in ("input_grad", "head"):
        freeze_backbone(model)
    if variant == "head":
        model.patch_embedding.cls_token.requires_grad = False
    opt = FusedAdamW(model.flat_store(), lr=1e-4, weight_decay=0.05)
    if variant != "autograd":
        assert model.runtime().schedule() == variant
    return model, opt


def make_step(model, opt, variant, x, y):
    if variant != "autograd":
        return lambda: model.train_step(x, y, opt)
    crit = nn.CrossEntropyLoss()

    def step():
        opt.zero_grad(set_to_none=True)
        logits = model(x)
        loss = crit(logits, y)
        loss.backward()
        opt.step()
        int((logits.argmax(1) == y).sum())
        return loss
    return step


def window(step, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def gradient_check(name, dev, x, y, classes, img):
    a, _ = build(name, "autograd", dev, classes, img, dropout=0.0)
    b, _ = build(name, "full", dev, classes, img, dropout=0.0)
    la = nn.CrossEntropyLoss()(a(x), y)
    la.backward()

    class Rec:
        def step_flat(self, gscale=1.0):
            self.g = b.flat_store().gflat.clone()
    rec = Rec()
    lb = b.train_step(x, y, rec)
    torch.cuda.synchronize()
    st, worst = b.flat_store(), (0.0, "")
    for n, p in a.named_parameters():
        o, cnt = st.offsets[n]
        g, r = rec.g[o:o + cnt].double(), p.grad.reshape(-1).double()
        worst = max(worst, (float((g - r).norm() / (r.norm() + 1e-30)), n))
    return float(la), float(lb), worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="vit_s,vit_b")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_finetune: no GPU (nothing here can be measured on a CPU)")
    from vit_core._runtime import limit_host_threads
    limit_host_threads()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.rand(args.batch, 3, args.img, args.img, generator=g).to(dev)
    y = torch.randint(0, args.classes, (args.batch,), generator=g).to(dev)
    print(f"fine-tune step A/B on {torch.cuda.get_device_name(0)}: batch {args.batch}, {args.img}x{args.img}, {args.classes} classes, dropout 0.1, "
          f"bf16 operands; {args.rounds} interleaved rounds of {args.steps} steps after {args.warmup} warm-up steps")
    for name in args.models.split(","):
        la, lb, worst = gradient_check(name, dev, x, y, args.classes, args.img)
        print(f"\n{name}/16: full-schedule train_step against the autograd path, same weights and batch, dropout off: loss {lb:.7f} vs {la:.7f}, "
              f"largest relative L2 of a parameter gradient {worst[0]:.3g} ({worst[1]})")
        gc.collect()
        torch.cuda.empty_cache()
        peak = {}
        for v in VARIANTS:
            torch.cuda.reset_peak_memory_stats()
            model, opt = build(name, v, dev, args.classes, args.img)
            step = make_step(model, opt, v, x, y)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            peak[v] = torch.cuda.max_memory_allocated() / 2 ** 20
            del model, opt, step
            gc.collect()
            torch.cuda.empty_cache()
        steps = {}
        for v in VARIANTS:
            model, opt = build(name, v, dev, args.classes, args.img)
            steps[v] = make_step(model, opt, v, x, y)
            window(steps[v], args.warmup)
        times = {v: [] for v in VARIANTS}
        for _ in range(args.rounds):
            for v in VARIANTS:
                times[v].append(window(steps[v], args.steps))
        base = statistics.median(times["full"])
        print(f"{'variant':12s} {'ms/step':>9s} {'min':>8s} {'max':>8s} {'img/s':>9s} {'vs full':>8s} {'peak MiB alone':>15s}")
        for v in VARIANTS:
            med = statistics.median(times[v])
            print(f"{v:12s} {med:9.2f} {min(times[v]):8.2f} {max(times[v]):8.2f} {args.batch / med * 1e3:9.0f} {med / base:8.3f} {peak[v]:15.0f}")
        del steps
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
