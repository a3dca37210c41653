#!/usr/bin/env python3
"""sha256 of the losses and of the flat parameter buffer after 4 seeded steps of tiny models, with the losses themselves to 9
digits, one line per case: the three fused train_steps (ViT in its three backward schedules) and ViT through autograd, then
SimMIM again with drop path, with LayerScale, with both, and with fp8 linear operands (the other forms of the LayerNorm
backward launch), then the masked-image models' patch path: MAE fused and through autograd (nn.MSELoss, FusedAdamW.step, a
fixed keep table), SimMIM through autograd (nn.L1Loss), both again at patch 5 on 30x30 (Pd = 75: projection, head and the
gradient of the prediction run at the padded width 128) and SimMIM at patch 4 (Pd = 48: padded to 64 except for the head's
output).  Two commits that print the same lines compute the same thing bit for bit (dropout 0.1 included: its seeds
come from torch.manual_seed).

usage: python tools/step_digest.py"""
import hashlib
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd")):
    sys.path.insert(0, p)

DEV = torch.device("cuda:0")
TINY = dict(num_blocks=2, input_shape=(3, 32, 32), patch_size=8, embed_dim=128, num_heads=2, mlp_dim=256, dropout=0.1)
STEPS = 4


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def report(name, losses, store):
    torch.cuda.synchronize()
    losses = torch.stack([l.detach().float().reshape(()) for l in losses]).cpu()
    print(f"{name:18s} losses {sha(losses)}  flat {sha(store.flat)}  ({' '.join(f'{float(l):.9g}' for l in losses)})")


def images(n, size, seed):
    return torch.rand(n, 3, size, size, generator=torch.Generator().manual_seed(seed)).to(DEV)


def autograd_steps(m, opt, x, criterion, **fwd):
    losses = []
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        losses.append(criterion(*m(x, **fwd)))
        losses[-1].backward()
        opt.step()
    return losses


def simmim(name="simmim", operands="bf16", autograd=False, **extra):
    from vit_core.ssl.simmim.model import SimMIMViT
    from vitssl_hip.engine import set_linear_operands
    from vitssl_hip.optim import FusedAdamW
    torch.manual_seed(1)
    set_linear_operands(operands)          # read when the model's encoder stack is built
    try:
        cfg = dict(TINY, **extra)
        m = SimMIMViT(**cfg).to(DEV).train()
        opt, x = FusedAdamW(m.flat_store(), lr=1e-3, weight_decay=1e-2), images(8, cfg["input_shape"][1], 2)
        losses = autograd_steps(m, opt, x, nn.L1Loss()) if autograd else [m.train_step(x, opt) for _ in range(STEPS)]
        report(name, losses, m.flat_store())
    finally:
        set_linear_operands("bf16")


def mae(name="mae", autograd=False, **extra):
    from vit_core.ssl.mae import MAEViT
    from vit_core.ssl.mae.masking import draw_keep
    from vitssl_hip.optim import FusedAdamW
    torch.manual_seed(5)
    cfg = dict(TINY, dropout=0.0, decoder_embed_dim=64, decoder_blocks=1, decoder_heads=2, **extra)
    m = MAEViT(**cfg).to(DEV).train()
    opt, x = FusedAdamW(m.flat_store(), lr=1e-3, weight_decay=1e-2), images(8, cfg["input_shape"][1], 6)
    if autograd:
        keep, _ = draw_keep(8, m.num_patches, m.num_kept, generator=torch.Generator().manual_seed(7))
        losses = autograd_steps(m, opt, x, nn.MSELoss(), keep_cpu=keep)
    else:
        losses = [m.train_step(x, opt) for _ in range(STEPS)]
    report(name, losses, m.flat_store())


def dino():
    from vit_core.ssl.dino.loss import DINOLoss
    from vit_core.ssl.dino.model import DINOViT
    from vitssl_hip.optim import FusedAdamW
    torch.manual_seed(3)
    m = DINOViT(output_dim=256, **TINY).to(DEV).train()
    opt, crit = FusedAdamW(m.flat_store(), lr=1e-3, weight_decay=1e-2), DINOLoss(0.04, 0.1)
    views = [images(4, 32, 4), images(4, 32, 5), images(4, 16, 6), images(4, 16, 7)]
    report("dino", [m.train_step(views, 2, crit, opt) for _ in range(STEPS)], m.flat_store())


def vit(schedule, classes=10):
    from utils.model_builder import freeze_backbone
    from vit_core.vit import ViT
    from vitssl_hip.optim import FusedAdamW
    torch.manual_seed(8)
    m = ViT(num_classes=classes, **TINY).to(DEV).train()
    if schedule in ("input_grad", "head"):
        freeze_backbone(m)
    if schedule == "head":
        m.patch_embedding.cls_token.requires_grad = False
    opt, x = FusedAdamW(m.flat_store(), lr=1e-3, weight_decay=1e-2), images(8, 32, 9)
    y = torch.randint(0, classes, (8,), generator=torch.Generator().manual_seed(10)).to(DEV)
    if schedule != "autograd":
        assert m.runtime().schedule() == schedule
        return report(f"vit {schedule}", [m.train_step(x, y, opt) for _ in range(STEPS)], m.flat_store())
    losses = []
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        losses.append(nn.functional.cross_entropy(m(x), y))
        losses[-1].backward()
        opt.step()
    report(f"vit autograd C={classes}", losses, m.flat_store())


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("step_digest: no GPU")
    simmim()
    dino()
    for s in ("full", "input_grad", "head"):
        vit(s)
    vit("autograd", 10)
    vit("autograd", 64)
    simmim("simmim droppath", drop_path_rate=0.1)
    simmim("simmim layerscale", layer_scale_init=1e-5)
    simmim("simmim dp+ls", drop_path_rate=0.1, layer_scale_init=1e-5)
    simmim("simmim fp8", operands="fp8")
    pad = dict(input_shape=(3, 30, 30), patch_size=5)
    for case, kw in (("", {}), (" P=5", pad)):
        mae("mae" + case, **kw)
        mae("mae autograd" + case, autograd=True, **kw)
    simmim("simmim autograd", autograd=True)
    simmim("simmim P=5", **pad)
    simmim("simmim autograd P=5", autograd=True, **pad)
    simmim("simmim P=4", patch_size=4)
