"""Global average pooling on the GPU, measured:
  1. both kernels of include_addons/vitssl_pool.h at (B, T, D) = (256, 197, 768), (128, 197, 1024) and (32, 785, 768): time, the
     bytes the algorithm moves (the patch rows in and [B, D] out; [B, D] in and every row of g out) and their rate as a share of
     the copy rate that tools/hbm_probe.py measures in this same process.  Every call takes the next of several buffer sets that
     together pass 600 MB, so that a call does not find its operands in the 256 MiB Infinity Cache.  Reported, not gated;
  2. the ViT-B/16 fused supervised step at batch 256, global_pool="avg" against "cls", alternating in one process;
  3. with --parent-tree DIR (a built checkout of the parent commit): the headline of bench.py of this tree and of that one,
     alternating as child processes, beside the spread of the parent's own runs.  The headline runs none of the pooling code.
Figures of 1 and 2 are the median over ROUNDS rounds of the mean of N back-to-back calls between two HIP events; the variants
alternate inside a round.  Not measured here: data parallel, other batch sizes.
Developer tool:  python tools/ab_pool.py [--out profiles/pool_ab.txt] [--skip-kernels] [--skip-step] [--parent-tree DIR] [--bench-runs 3]"""
import argparse
import contextlib
import io
import itertools
import json
import os
import re
import runpy
import statistics
import subprocess
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import torch  # noqa: E402

from vitssl_hip import ops  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 7
SHAPES = [(256, 197, 768), (128, 197, 1024), (32, 785, 768)]
FOOTPRINT = 600e6          # bytes the buffer sets of one kernel pass together


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


def probe_copy_rate():
    """tools/hbm_probe.py, run here: -> (its output, the fp32 copy rate at 616 MB in TB/s, read + write)"""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        runpy.run_path(os.path.join(ROOT, "tools", "hbm_probe.py"), run_name="__main__")
    text = buf.getvalue()
    return text, float(re.search(r"copy\s+616 MB f32:\s*([0-9.]+) TB/s", text).group(1))


def rotating(make, nbytes):
    """a callable that runs the kernel on the next of enough buffer sets to pass FOOTPRINT bytes"""
    sets = [make() for _ in range(max(2, int(FOOTPRINT // nbytes) + 1))]
    it = itertools.cycle(sets)
    return lambda: next(it)()


def kernels(B, T, D):
    """name -> (callable, bytes the algorithm moves per call)"""
    def fwd():
        x, out = torch.randn(B * T, D, device=DEV), torch.empty(B, D, device=DEV)
        return lambda: ops.pool_tokens_fwd(x, out, B, T, D)

    def bwd():
        dout, g = torch.randn(B, D, device=DEV), torch.empty(B * T, D, device=DEV)
        return lambda: ops.pool_tokens_bwd(dout, g, B, T, D)
    nf, nb = 4 * D * (B * (T - 1) + B), 4 * D * (B + B * T)
    return {"pool_tokens_fwd": (rotating(fwd, nf), nf), "pool_tokens_bwd": (rotating(bwd, nb), nb)}


def headline(tree, steps, warmup):
    """images / s of `python bench.py --gpus 1` run in `tree` as a child process"""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"bench.py failed in {tree}:\n{r.stderr[-2000:]}")
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return float(out["value"]), float(out["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-kernels", action="store_true", help="leave out the copy-rate probe and the kernel table")
    ap.add_argument("--skip-step", action="store_true", help="leave out the two ViT-B/16 steps")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: also compare the bench.py headlines")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=20)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/ab_pool.py on {torch.cuda.get_device_name(0)}: median of {ROUNDS} rounds x N calls, variants alternating")
    if not args.skip_kernels:
        text, copy_rate = probe_copy_rate()
        say()
        say("0. tools/hbm_probe.py in this process")
        for ln in text.strip().splitlines():
            say("   " + ln)
        say(f"   the yardstick below: the fp32 copy at 616 MB, {copy_rate:.2f} TB/s (read + write)")
        say()
        say(f"1. kernels of include_addons/vitssl_pool.h (buffer sets rotate over more than {FOOTPRINT / 1e6:.0f} MB)")
        for B, T, D in SHAPES:
            ks = kernels(B, T, D)
            med, spread = interleaved({k: fn for k, (fn, _) in ks.items()}, n=24)
            for k, (_, nbytes) in ks.items():
                rate = nbytes / (med[k] * 1e-6) / 1e12
                say(f"   ({B:3d}, {T:3d}, {D:4d})  {k:16s} {med[k]:8.1f} us  [{spread[k][0]:.1f} .. {spread[k][1]:.1f}]   {nbytes / 1e6:7.1f} MB   "
                    f"{rate:5.2f} TB/s   {rate / copy_rate:5.2f} of the copy rate")
            del ks
            torch.cuda.empty_cache()

    if not args.skip_step:
        from vit_core.vit import ViT
        from vitssl_hip.optim import FusedAdamW
        kw = dict(num_classes=1000, num_blocks=12, input_shape=(3, 224, 224), embed_dim=768, patch_size=16, num_heads=12, mlp_dim=3072, dropout=0.1)
        models = {}
        for pool in ("cls", "avg"):
            torch.manual_seed(0)
            models[pool] = ViT(**kw, global_pool=pool).to(DEV).train()
        opts = {k: FusedAdamW(m.flat_store(), lr=1e-4, weight_decay=0.05) for k, m in models.items()}
        g = torch.Generator().manual_seed(3)
        xb, yb = torch.rand(256, 3, 224, 224, generator=g).to(DEV), torch.randint(0, 1000, (256,), generator=g).to(DEV)
        step = lambda k: (lambda: models[k].train_step(xb, yb, opts[k]))      # noqa: E731
        med, spread = interleaved({k: step(k) for k in models}, n=5, warm=3)
        say()
        say("2. fused supervised train step, ViT-B/16, batch 256, 224 x 224, dropout 0.1, fused AdamW (ms a step)")
        for k in models:
            say(f"   global_pool = {k}   {med[k] / 1e3:8.2f} ms  [{spread[k][0] / 1e3:.2f} .. {spread[k][1] / 1e3:.2f}]")
        say(f"   avg / cls = {med['avg'] / med['cls']:.4f}")
        del models, opts
        torch.cuda.empty_cache()

    if args.parent_tree:
        trees = {"parent": os.path.abspath(args.parent_tree), "this tree": ROOT}
        runs = {k: [] for k in trees}
        for _ in range(args.bench_runs):
            for k, tree in trees.items():
                runs[k].append(headline(tree, args.bench_steps, 5))
        say()
        say(f"3. bench.py --gpus 1 --steps {args.bench_steps} --warmup 5, {args.bench_runs} runs each, alternating (images / s; ms a step)")
        for k, v in runs.items():
            ips = [a for a, _ in v]
            say(f"   {k:10s} " + "  ".join(f"{a:8.1f} ({b:.2f} ms)" for a, b in v) + f"   median {statistics.median(ips):.1f}, spread {min(ips):.1f} .. {max(ips):.1f}")
        p, t = [a for a, _ in runs["parent"]], [a for a, _ in runs["this tree"]]
        say(f"   this tree / parent (medians) = {statistics.median(t) / statistics.median(p):.4f}; the parent's own runs span "
            f"{(max(p) - min(p)) / statistics.median(p) * 100:.2f} % of their median")
    say()
    say("not measured: data parallel, other batch sizes")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
