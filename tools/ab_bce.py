"""Binary cross-entropy on the GPU (classify_bce_kernel of csrc/classify.hip), interleaved against what it sits beside:
  1. vitssl_classify_bce at (256, 1000, ld 1024) and (256, 21841, ld 21888), loss only and loss + gradient (dlogits and dbias),
     one- and two-label, against vitssl_classify_loss / _mix on the same tensors and against the torch formulation on the
     same tensors (one-hot / mixed soft targets + binary_cross_entropy_with_logits + its backward + the bf16 cast and the
     bias gradient's column sum);
  2. one ViT-B/16 supervised fused step (batch 256, 224 x 224, 1000 classes, dropout 0.1) with loss="bce" against loss="ce".
Every figure is the median over ROUNDS rounds of the mean of N back-to-back calls between two HIP events; the variants
alternate inside a round.  Developer tool:  python tools/ab_bce.py [--out profiles/bce_ab.txt] [--skip-step]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vitssl_hip import ops  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 7
EPS = 0.1


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


def torch_bce(z, y, partner, lam, Cn, grad):
    """the torch formulation on the padded logits: -> (loss, bf16 d(logits) [B, ld], bias gradient [C]) or the loss alone"""
    zc = z[:, :Cn]
    if grad:
        zc = zc.detach().requires_grad_(True)
    s = lambda lab: F.one_hot(lab, Cn).float() * (1.0 - EPS) + EPS / Cn      # noqa: E731
    t = s(y) if partner is None else lam[:, None] * s(y) + (1.0 - lam[:, None]) * s(y[partner.long()])
    loss = F.binary_cross_entropy_with_logits(zc, t)
    if not grad:
        return loss
    g, = torch.autograd.grad(loss, zc)
    out = torch.zeros(z.shape, dtype=torch.bfloat16, device=z.device)
    out[:, :Cn] = g.to(torch.bfloat16)
    return loss, out, g.sum(0)


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
    say(f"tools/ab_bce.py on {torch.cuda.get_device_name(0)}: median of {ROUNDS} rounds x N calls, variants alternating")

    # ---- 1. the loss kernel
    say()
    say(f"1. vitssl_classify_bce, B = 256, smoothing {EPS}; 'grad' = dlogits (bf16, padded) and dbias written as well")
    for Cn, ld in ((1000, 1024), (21841, 21888)):
        Bn = 256
        g = torch.Generator().manual_seed(2)
        z = (2.0 * torch.randn(Bn, ld, generator=g)).to(DEV)
        y = torch.randint(0, Cn, (Bn,), generator=g).to(DEV)
        partner = torch.arange(Bn - 1, -1, -1, dtype=torch.int32, device=DEV)
        lam = torch.rand(Bn, generator=g).to(DEV)
        loss, pred = torch.zeros(2, device=DEV), torch.zeros(Bn, dtype=torch.int64, device=DEV)
        cnt, bad = torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        dl, db = torch.empty(Bn, ld, dtype=torch.bfloat16, device=DEV), torch.zeros(Cn, device=DEV)
        out = (loss, pred, cnt, bad)
        gk = dict(dlogits=dl, dbias=db)
        # the two formulations agree before they are timed
        ops.classify_bce(z, y, Cn, *out, partner=partner, lam=lam, smoothing=EPS, **gk)
        want, wdl, _ = torch_bce(z, y, partner, lam, Cn, True)
        torch.cuda.synchronize()
        got = float(loss[0] / loss[1])
        assert abs(got - float(want)) <= 1e-5 * abs(float(want)), (got, float(want))
        assert float((dl.float() - wdl.float()).abs().max()) <= 2.0 ** -7 * float(wdl.float().abs().max())
        med, spread = interleaved({
            "bce": lambda: ops.classify_bce(z, y, Cn, *out, smoothing=EPS),
            "bce_g": lambda: ops.classify_bce(z, y, Cn, *out, smoothing=EPS, **gk),
            "bce2": lambda: ops.classify_bce(z, y, Cn, *out, partner=partner, lam=lam, smoothing=EPS),
            "bce2_g": lambda: ops.classify_bce(z, y, Cn, *out, partner=partner, lam=lam, smoothing=EPS, **gk),
            "ce": lambda: ops.classify_loss(z, y, Cn, *out, label_smoothing=EPS),
            "ce_g": lambda: ops.classify_loss(z, y, Cn, *out, label_smoothing=EPS, **gk),
            "ce2_g": lambda: ops.classify_loss_mix(z, y, partner, lam, Cn, *out, label_smoothing=EPS, **gk),
            "torch": lambda: torch_bce(z, y, None, None, Cn, False),
            "torch_g": lambda: torch_bce(z, y, None, None, Cn, True),
            "torch2_g": lambda: torch_bce(z, y, partner, lam, Cn, True),
        }, n=30)
        say(f"   C = {Cn}, ld = {ld}")
        say(f"     classify_bce, loss only              {fmt(med, spread, 'bce')}   two-label {fmt(med, spread, 'bce2')}")
        say(f"     classify_bce, grad                   {fmt(med, spread, 'bce_g')}   two-label {fmt(med, spread, 'bce2_g')}")
        say(f"     classify_loss (softmax CE), loss only {fmt(med, spread, 'ce')}   bce / ce = {med['bce'] / med['ce']:.3f}")
        say(f"     classify_loss (softmax CE), grad     {fmt(med, spread, 'ce_g')}   two-label {fmt(med, spread, 'ce2_g')}   "
            f"bce / ce = {med['bce_g'] / med['ce_g']:.3f}, two-label {med['bce2_g'] / med['ce2_g']:.3f}")
        say(f"     torch one-hot + bce_with_logits, loss only {fmt(med, spread, 'torch')}   / classify_bce = {med['torch'] / med['bce']:.2f}")
        say(f"     torch ... + backward + bf16 cast + column sum {fmt(med, spread, 'torch_g')}   two-label {fmt(med, spread, 'torch2_g')}   "
            f"/ classify_bce = {med['torch_g'] / med['bce_g']:.2f}, two-label {med['torch2_g'] / med['bce2_g']:.2f}")
        del z, dl

    # ---- 2. the step
    if not args.skip_step:
        from vit_core.vit import ViT
        from vitssl_hip.optim import FusedAdamW
        torch.manual_seed(0)
        model = ViT(num_classes=1000, num_blocks=12, input_shape=(3, 224, 224), embed_dim=768, patch_size=16, num_heads=12, mlp_dim=3072,
                    dropout=0.1).to(DEV).train()
        opt = FusedAdamW(model.flat_store(), lr=1e-4, weight_decay=0.05)
        g = torch.Generator().manual_seed(3)
        xb, yb = torch.rand(256, 3, 224, 224, generator=g).to(DEV), torch.randint(0, 1000, (256,), generator=g).to(DEV)
        med, spread = interleaved({
            "ce": lambda: model.train_step(xb, yb, opt, label_smoothing=EPS),
            "bce": lambda: model.train_step(xb, yb, opt, label_smoothing=EPS, loss="bce"),
        }, n=5, warm=3)
        say()
        say("2. ViT-B/16 supervised fused step, batch 256, 224 x 224, 1000 classes, dropout 0.1, label_smoothing 0.1 (us a step)")
        say(f"   train_step, loss = ce      {fmt(med, spread, 'ce')}")
        say(f"   train_step, loss = bce     {fmt(med, spread, 'bce')}   difference {med['bce'] - med['ce']:.1f} us = {100 * (med['bce'] / med['ce'] - 1):.2f} %")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
