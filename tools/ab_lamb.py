"""The fused LAMB step against the table AdamW step, interleaved, on the flat stores of ViT-B/16 and ViT-L/16 (built from the real
models: 86 M and 304 M floats with their ~150 / ~300 parameters, layer decay 0.75 and the no-weight-decay rule in the table).
Per store:
  (a) vitssl_adamw_segments, every parameter, no clip      (the step AdamW takes with the same settings; with --parent-lib the
      launch goes through that library, e.g. the parent commit's build, over the same table image)
  (b) vitssl_lamb_segments, no clip: moment pass + trust ratios + apply pass
  (c) vitssl_grad_sumsq + either step with the clip
and a copy of the gradient, for the rate of this box.  By bytes (b) moves 40 an element against (a)'s 28.
Then the fused supervised ViT-B/16 step at batch 256 (ViT.train_step, 224 x 224) with FusedAdamW and with FusedLamb, both with
layer decay, the no-weight-decay rule and the clip, so both go through the table.
Every figure is the median over ROUNDS rounds of the mean of N back-to-back calls between two HIP events; the variants alternate
inside a round.  Developer tool:  python tools/ab_lamb.py [--parent-lib PATH] [--skip-step] [--out profiles/lamb_ab.txt]"""
import argparse
import ctypes as C
import gc
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import torch  # noqa: E402

from vitssl_hip import _lib as L  # noqa: E402
from vitssl_hip import ops  # noqa: E402
from vitssl_hip.engine import FlatStore, exempt_from_weight_decay, layer_id, num_layers  # noqa: E402

DEV = torch.device("cuda:0")
MODELS = {"ViT-B/16": dict(num_blocks=12, embed_dim=768, num_heads=12, mlp_dim=3072),
          "ViT-L/16": dict(num_blocks=24, embed_dim=1024, num_heads=16, mlp_dim=4096)}
HYPER = (1e-3, 0.9, 0.999, 1e-6)
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


def parent_adamw_segments(path):
    """ops.adamw_segments through another build of the library (same ABI, same table image)"""
    lib = C.CDLL(path)
    fn = lib.vitssl_adamw_segments
    fn.restype, fn.argtypes = L.REGISTRY["optim"]["vitssl_adamw_segments"]
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731

    def call(p, g, m, v, plan, lr, b1, b2, eps, step, gscale=1.0, sumsq=None, max_norm=0.0):
        rc = fn(P(p), P(g), P(m), P(v), P(plan.table), plan.nseg, lr, b1, b2, eps, step, gscale, P(sumsq), max_norm,
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RuntimeError(f"vitssl_adamw_segments of {path} failed ({rc})")
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libvitssl_hip.so of another build: (a) launches its vitssl_adamw_segments")
    ap.add_argument("--skip-step", action="store_true", help="leave out the fused steps")
    args = ap.parse_args()
    from vit_core.vit import ViT
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    adamw_segments = parent_adamw_segments(args.parent_lib) if args.parent_lib else ops.adamw_segments
    say(f"tools/ab_lamb.py on {torch.cuda.get_device_name(0)}: median of {ROUNDS} rounds x N calls, variants alternating; us a step")
    say(f"(a) launches vitssl_adamw_segments of {'the library given with --parent-lib' if args.parent_lib else 'this build'}")
    fmt = lambda med, spread, k: f"{med[k]:9.1f} us  [{spread[k][0]:.1f} .. {spread[k][1]:.1f}]"      # noqa: E731
    for name, kw in MODELS.items():
        model = ViT(num_classes=1000, input_shape=(3, 224, 224), patch_size=16, **kw)
        store = FlatStore(model, DEV)
        n = store.numel
        layers = num_layers(store.names)
        rows = [(*store.offsets[k], 0.75 ** (layers + 1 - layer_id(k, layers)), 0.0 if exempt_from_weight_decay(k, p.dim()) else 0.05)
                for k, p in zip(store.names, store.params)]
        p, g = store.flat, store.gflat
        g.normal_().mul_(0.01)
        m, v = torch.zeros_like(p), torch.zeros_like(p)
        plan = ops.AdamWPlan(rows, n, DEV)
        scratch = torch.empty_like(g)
        med, spread = interleaved({
            "a": lambda: adamw_segments(p, g, m, v, plan, *HYPER, 3, 1.0),
            "b": lambda: ops.lamb_segments(p, g, m, v, plan, *HYPER, 3, 1.0),
            "a_clip": lambda: adamw_segments(p, g, m, v, plan, *HYPER, 3, 1.0, ops.grad_sumsq(g, plan), 1.0),
            "b_clip": lambda: ops.lamb_segments(p, g, m, v, plan, *HYPER, 3, 1.0, ops.grad_sumsq(g, plan), 1.0),
            "copy": lambda: scratch.copy_(g),
        })
        units = plan.lamb_buffers()[0].numel() // 16
        say()
        say(f"{name}: {n / 1e6:.2f} M floats in the store, {len(rows)} parameters ({plan.elements / 1e6:.2f} M floats in segments, "
            f"{units} units, workspace {units * 16 / 1e6:.2f} MB); copy rate {8 * n / med['copy'] / 1e6:.2f} TB/s (r+w)")
        say(f"  (a) adamw_segments                        {fmt(med, spread, 'a')}  {28 * plan.elements / med['a'] / 1e6:.2f} TB/s")
        say(f"  (b) lamb_segments (3 launches)            {fmt(med, spread, 'b')}  {40 * plan.elements / med['b'] / 1e6:.2f} TB/s   "
            f"(b) / (a) = {med['b'] / med['a']:.3f}  (by bytes 40 / 28 = {40 / 28:.3f}); added {med['b'] - med['a']:+.1f} us a step")
        say(f"  (c) grad_sumsq + adamw_segments (clip)    {fmt(med, spread, 'a_clip')}")
        say(f"      grad_sumsq + lamb_segments (clip)     {fmt(med, spread, 'b_clip')}   ratio {med['b_clip'] / med['a_clip']:.3f}; "
            f"added {med['b_clip'] - med['a_clip']:+.1f} us a step")
        del model, store, p, g, m, v, scratch, plan
        gc.collect()
        torch.cuda.empty_cache()

    if not args.skip_step:
        from vit_core._runtime import limit_host_threads
        from vitssl_hip.optim import FusedAdamW, FusedLamb
        limit_host_threads()
        batch = 256
        gen = torch.Generator().manual_seed(0)
        x, y = torch.rand(batch, 3, 224, 224, generator=gen).to(DEV), torch.randint(0, 10, (batch,), generator=gen).to(DEV)
        steps = {}
        for key, cls in (("adamw", FusedAdamW), ("lamb", FusedLamb)):
            torch.manual_seed(1)
            model = ViT(num_classes=10, input_shape=(3, 224, 224), patch_size=16, dropout=0.1, **MODELS["ViT-B/16"]).to(DEV).train()
            st = model.flat_store()
            layers = num_layers(st.names)
            ndim = {k: q.dim() for k, q in zip(st.names, st.params)}
            opt = cls(st, lr=1e-4, weight_decay=0.05, max_grad_norm=1.0, lr_scale=lambda k, layers=layers: 0.75 ** (layers + 1 - layer_id(k, layers)),
                      weight_decay_of=lambda k, ndim=ndim: 0.0 if exempt_from_weight_decay(k, ndim[k]) else 0.05)
            steps[key] = (lambda mo, o: lambda: mo.train_step(x, y, o))(model, opt)
        med, spread = interleaved(steps, n=8, warm=4)
        d = med["lamb"] - med["adamw"]
        say()
        say(f"fused supervised step, ViT-B/16, batch {batch}, 224 x 224, dropout 0.1, clip 1.0, layer decay 0.75, no-weight-decay rule (us a step; "
            f"FusedAdamW is this build's, its launches are the parent's)")
        say(f"  FusedAdamW {fmt(med, spread, 'adamw')}   FusedLamb {fmt(med, spread, 'lamb')}   added {d:+.1f} us a step = {100 * d / med['adamw']:+.2f} %")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
