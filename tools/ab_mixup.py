"""Mixup / CutMix on the GPU (csrc/mixup.hip, the MIX instantiation of csrc/classify.hip), interleaved against what it replaces
or sits beside:
  1. vitssl_mix_batch at (256, 3, 224, 224): all rows blend / all rows paste one batch-mode CutMix box / an elem-mode draw,
     against out.copy_(x) of the same tensor (the copy ceiling: blend moves 1.5x its bytes, paste the same bytes) and against
     the torch formulation (lam * x + (1 - lam) * x.flip(0); clone + slice assignment);
  2. vitssl_classify_loss_mix against vitssl_classify_loss at (256, 1000) and (256, 10), gradient and bias gradient included;
  3. one ViT-B/16 supervised fused step (batch 256, 224 x 224, 1000 classes, dropout 0.1) with and without `mix`.
Every figure is the median over ROUNDS rounds of the mean of N back-to-back calls between two HIP events; the variants
alternate inside a round.  Developer tool:  python tools/ab_mixup.py [--out profiles/mixup_ab.txt] [--skip-step]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from data import GPUMixup, MixSpec, sample_mix_params  # noqa: E402
from vitssl_hip import ops  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 7


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3          # microseconds a call


def interleaved(variants, n=20, warm=3):
    """{name: fn} -> ({name: median microseconds}, {name: (min, max)}); a warm-up pass, then the variants alternate in every round"""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            samples[k].append(timed(fn, n))
    return {k: statistics.median(v) for k, v in samples.items()}, {k: (min(v), max(v)) for k, v in samples.items()}


def hand(B, kind, lam, box=(0, 0, 0, 0)):
    full = lambda v: np.full(B, v, np.int32)      # noqa: E731
    return dict(kind=full(kind), partner=(B - 1 - np.arange(B)).astype(np.int32), y0=full(box[0]), y1=full(box[1]), x0=full(box[2]),
                x1=full(box[3]), lam=np.full(B, lam, np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true", help="leave out the ViT-B/16 step")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda med, spread, k: f"{med[k]:8.1f} us  [{spread[k][0]:.1f} .. {spread[k][1]:.1f}]"      # noqa: E731
    say(f"tools/ab_mixup.py on {torch.cuda.get_device_name(0)}: median of {ROUNDS} rounds x N calls, variants alternating")

    # ---- 1. the mix kernel
    B, C, H, W = 256, 3, 224, 224
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, C, H, W, generator=g).to(DEV)
    out = torch.empty_like(x)
    mixer = GPUMixup(MixSpec())
    box = (40, 168, 56, 200)                                                 # a CutMix box of lam ~ 0.63: 128 x 144 of 224 x 224
    tables = {"blend": mixer.to_device(hand(B, ops.MIX_BLEND, 0.3)), "paste": mixer.to_device(hand(B, ops.MIX_PASTE, 0.0, box)),
              "copy": mixer.to_device(hand(B, ops.MIX_COPY, 1.0))}
    elem = sample_mix_params(MixSpec(mode="elem"), B, H, W, torch.Generator().manual_seed(1))
    tables["elem"] = mixer.to_device(elem)
    tables = {k: type(v)(*(t.clone() for t in v)) for k, v in tables.items()}       # (the mixer's pinned block is reused per call)
    lam_t = torch.full((B, 1, 1, 1), 0.3, device=DEV)

    def torch_blend():
        torch.add(lam_t * x, (1.0 - lam_t) * x.flip(0), out=out)

    def torch_paste():
        out.copy_(x)
        out[:, :, box[0]:box[1], box[2]:box[3]] = x.flip(0)[:, :, box[0]:box[1], box[2]:box[3]]

    variants = {"copy_": lambda: out.copy_(x)}
    for k, t in tables.items():
        variants[k] = (lambda t: lambda: ops.mix_batch(x, out, t.iparams, t.lam))(t)
    variants["torch_blend"], variants["torch_paste"] = torch_blend, torch_paste
    med, spread = interleaved(variants, n=20)
    n = x.numel()
    inside = (box[1] - box[0]) * (box[3] - box[2]) / (H * W)
    n_blend, n_paste = int((elem["kind"] == 1).sum()), int((elem["kind"] == 2).sum())
    elem_bytes = 4 * C * H * W * (2 * B + n_blend)
    say()
    say(f"1. vitssl_mix_batch, x f32 {tuple(x.shape)} = {4 * n / 1e6:.1f} MB; rate = bytes the variant has to move / time")
    say(f"   out.copy_(x), the copy ceiling           {fmt(med, spread, 'copy_')}  {8 * n / med['copy_'] / 1e6:.2f} TB/s")
    say(f"   mix_batch, all rows copy                 {fmt(med, spread, 'copy')}  {8 * n / med['copy'] / 1e6:.2f} TB/s   / copy_ = {med['copy'] / med['copy_']:.3f}")
    say(f"   mix_batch, all rows blend (12 B / elem)  {fmt(med, spread, 'blend')}  {12 * n / med['blend'] / 1e6:.2f} TB/s   / copy_ = {med['blend'] / med['copy_']:.3f}")
    say(f"   mix_batch, all rows paste, box {inside:.2f}      {fmt(med, spread, 'paste')}  {8 * n / med['paste'] / 1e6:.2f} TB/s   / copy_ = {med['paste'] / med['copy_']:.3f}")
    say(f"   mix_batch, elem draw ({n_blend} blend, {n_paste} paste) {fmt(med, spread, 'elem')}  {elem_bytes / med['elem'] / 1e6:.2f} TB/s   / copy_ = {med['elem'] / med['copy_']:.3f}")
    say(f"   torch lam * x + (1 - lam) * x.flip(0)    {fmt(med, spread, 'torch_blend')}  / mix_batch blend = {med['torch_blend'] / med['blend']:.2f}")
    say(f"   torch copy_ + slice assignment           {fmt(med, spread, 'torch_paste')}  / mix_batch paste = {med['torch_paste'] / med['paste']:.2f}")
    del x, out, variants

    # ---- 2. the loss
    say()
    say("2. vitssl_classify_loss_mix against vitssl_classify_loss (dlogits and dbias written), B = 256")
    for Cn in (1000, 10):
        Bn, ld = 256, (Cn + 63) // 64 * 64
        g = torch.Generator().manual_seed(2)
        z = (2.0 * torch.randn(Bn, ld, generator=g)).to(DEV)
        y = torch.randint(0, Cn, (Bn,), generator=g).to(DEV)
        partner = torch.arange(Bn - 1, -1, -1, dtype=torch.int32, device=DEV)
        lam = torch.rand(Bn, generator=g).to(DEV)
        ones = torch.ones(Bn, device=DEV)
        loss, pred = torch.zeros(2, device=DEV), torch.zeros(Bn, dtype=torch.int64, device=DEV)
        cnt, bad = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        dl, db = torch.empty(Bn, ld, dtype=torch.bfloat16, device=DEV), torch.zeros(Cn, device=DEV)
        med, spread = interleaved({
            "one": lambda: ops.classify_loss(z, y, Cn, loss, pred, cnt, bad, dlogits=dl, dbias=db, label_smoothing=0.1),
            "mix": lambda: ops.classify_loss_mix(z, y, partner, lam, Cn, loss, pred, cnt, bad, dlogits=dl, dbias=db, label_smoothing=0.1),
            "mix1": lambda: ops.classify_loss_mix(z, y, partner, ones, Cn, loss, pred, cnt, bad, dlogits=dl, dbias=db, label_smoothing=0.1),
        }, n=50)
        say(f"   C = {Cn:4d}: classify_loss {fmt(med, spread, 'one')}   classify_loss_mix, lam ~ U(0,1) {fmt(med, spread, 'mix')}   "
            f"lam = 1 {fmt(med, spread, 'mix1')}   mix / one = {med['mix'] / med['one']:.3f}")

    # ---- 3. the step
    if not args.skip_step:
        from vit_core.vit import ViT
        from vitssl_hip.optim import FusedAdamW
        torch.manual_seed(0)
        model = ViT(num_classes=1000, num_blocks=12, input_shape=(3, 224, 224), embed_dim=768, patch_size=16, num_heads=12, mlp_dim=3072,
                    dropout=0.1).to(DEV).train()
        opt = FusedAdamW(model.flat_store(), lr=1e-4, weight_decay=0.05)
        g = torch.Generator().manual_seed(3)
        xb, yb = torch.rand(256, 3, 224, 224, generator=g).to(DEV), torch.randint(0, 1000, (256,), generator=g).to(DEV)
        params = tables["elem"]
        med, spread = interleaved({
            "plain": lambda: model.train_step(xb, yb, opt, label_smoothing=0.1),
            "mix": lambda: model.train_step(xb, yb, opt, label_smoothing=0.1, mix=params),
        }, n=5, warm=3)
        say()
        say("3. ViT-B/16 supervised fused step, batch 256, 224 x 224, 1000 classes, dropout 0.1, label_smoothing 0.1 (us a step)")
        say(f"   train_step                 {fmt(med, spread, 'plain')}")
        say(f"   train_step, mix = elem     {fmt(med, spread, 'mix')}   difference {med['mix'] - med['plain']:.1f} us = {100 * (med['mix'] / med['plain'] - 1):.2f} %")
        gen = torch.Generator().manual_seed(4)
        med, spread = interleaved({"draw": lambda: mixer.draw(256, 224, 224, gen)}, n=20)
        say(f"   GPUMixup.draw, batch mode (host draw + one pinned copy; not part of the steps above)  {fmt(med, spread, 'draw')}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
