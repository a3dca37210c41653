"""Segmented AdamW against the flat AdamW kernel, interleaved, on the flat stores of ViT-B/16 and ViT-L/16 (built from the real
models: 86 M and 304 M floats with their ~150 / ~300 parameters).  Per store:
  (a) vitssl_adamw over the whole buffer             (today's step)
  (b) vitssl_adamw_segments, every parameter, no clip
  (c) vitssl_grad_sumsq + vitssl_adamw_segments with the clip
  (d) frozen backbone (head and CLS token train): today's one launch per parameter against the table, without and with the clip
and, for (c) - (b), one read of the gradient at the copy rate measured here the way tools/hbm_probe.py does.
Every figure is the median over ROUNDS rounds of the mean of N back-to-back launches between two HIP events; the variants
alternate inside a round.  Developer tool:  python tools/ab_adamw.py [--out profiles/adamw_groups_ab.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import torch  # noqa: E402

from vitssl_hip import ops  # noqa: E402
from vitssl_hip.engine import FlatStore, exempt_from_weight_decay, layer_id, num_layers  # noqa: E402

DEV = torch.device("cuda:0")
MODELS = {"ViT-B/16": dict(num_blocks=12, embed_dim=768, num_heads=12, mlp_dim=3072),
          "ViT-L/16": dict(num_blocks=24, embed_dim=1024, num_heads=16, mlp_dim=4096)}
HYPER = (1e-3, 0.9, 0.999, 1e-8)
ROUNDS, N = 7, 20


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3          # microseconds a call


def interleaved(variants):
    """{name: fn} -> {name: median microseconds}; one warm-up pass, then the variants alternate in every round"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, fn in variants.items():
            samples[k].append(timed(fn))
    return {k: statistics.median(v) for k, v in samples.items()}, {k: (min(v), max(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from vit_core.vit import ViT
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/ab_adamw.py on {torch.cuda.get_device_name(0)}: median of {ROUNDS} rounds x {N} launches, variants alternating; us a step")
    for name, kw in MODELS.items():
        model = ViT(num_classes=1000, input_shape=(3, 224, 224), patch_size=16, **kw)
        store = FlatStore(model, DEV)
        n = store.numel
        layers = num_layers(store.names)
        rows = [(*store.offsets[k], 0.75 ** (layers + 1 - layer_id(k, layers)), 0.0 if exempt_from_weight_decay(k, p.dim()) else 0.05)
                for k, p in zip(store.names, store.params)]
        head = [r for k, r in zip(store.names, rows) if k.startswith("classification_head.") or k.endswith("cls_token")]
        p, g = store.flat, store.gflat
        g.normal_().mul_(0.01)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        full, part = ops.AdamWPlan(rows, n, DEV), ops.AdamWPlan(head, n, DEV)
        scratch = torch.empty_like(g)

        def per_parameter():
            for o, k, _, _ in head:
                ops.adamw(p[o:o + k], g[o:o + k], m[o:o + k], v[o:o + k], *HYPER, 0.05, 3, 1.0)

        med, spread = interleaved({
            "a": lambda: ops.adamw(p, g, m, v, *HYPER, 0.05, 3, 1.0),
            "b": lambda: ops.adamw_segments(p, g, m, v, full, *HYPER, 3, 1.0),
            "c": lambda: ops.adamw_segments(p, g, m, v, full, *HYPER, 3, 1.0, ops.grad_sumsq(g, full), 1.0),
            "d_old": per_parameter,
            "d_new": lambda: ops.adamw_segments(p, g, m, v, part, *HYPER, 3, 1.0),
            "d_clip": lambda: ops.adamw_segments(p, g, m, v, part, *HYPER, 3, 1.0, ops.grad_sumsq(g, part), 1.0),
            "copy": lambda: scratch.copy_(g),
        })
        copy_rate = 8 * n / med["copy"] / 1e6                   # TB/s, read + write
        read_us = 4 * full.elements / copy_rate / 1e6
        say()
        say(f"{name}: {n / 1e6:.2f} M floats in the store, {len(rows)} parameters ({full.elements / 1e6:.2f} M floats in segments); "
            f"head + CLS token: {len(head)} parameters, {part.elements / 1e6:.3f} M floats")
        fmt = lambda k: f"{med[k]:8.1f} us  [{spread[k][0]:.1f} .. {spread[k][1]:.1f}]"
        say(f"  (a) vitssl_adamw, whole buffer            {fmt('a')}  {28 * n / med['a'] / 1e6:.2f} TB/s")
        say(f"  (b) adamw_segments, all parameters        {fmt('b')}  {28 * full.elements / med['b'] / 1e6:.2f} TB/s   (b) / (a) = {med['b'] / med['a']:.3f}")
        say(f"  (c) grad_sumsq + adamw_segments (clip)    {fmt('c')}")
        say(f"      (c) - (b) = {med['c'] - med['b']:.1f} us; one read of g at the copy rate {copy_rate:.2f} TB/s = {read_us:.1f} us; "
            f"ratio {(med['c'] - med['b']) / read_us:.2f}")
        say(f"  (d) frozen backbone, per-parameter path   {fmt('d_old')}  ({len(head)} launches)")
        say(f"      frozen backbone, table                {fmt('d_new')}  (1 launch)   old / new = {med['d_old'] / med['d_new']:.2f}")
        say(f"      frozen backbone, table + clip         {fmt('d_clip')}  (3 launches)")
        del model, store, p, g, m, v, scratch, full, part
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
