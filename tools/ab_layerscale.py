"""LayerScale (include/vitssl_layerscale.h) on the GPU, interleaved against the launches it sits beside:
  2. one supervised fused step (tools/bench_finetune.py settings: 224 x 224, 10 classes, dropout 0.1, bf16 operands) with
     layer_scale_init 1e-5 against none: ViT-B/16 at batch 256 and ViT-L/16 at batch 128;
  3. the isolated kernels at their ViT-B shapes (M = 256 x 197 = 50432 rows, D = 768): the LayerScale residual GEMM (writing the
     branch image, as a training forward does) against the plain residual GEMM (out-projection K = 768, FC2 K = 3072),
     vitssl_layernorm_bwd_ls / vitssl_grad_mask_cast_ls (with the branch image and gamma's gradient) against the plain entries.
     The forward adds one bf16 [M, D] store per launch, the backward one read of it: their bytes are printed beside the
     difference, with the time those bytes take at the copy rate given by --copy-tbs (tools/hbm_probe.py).
(1., the headline, is bench.py of this commit against the parent's, alternating: a shell loop, its figures are appended to the
same file by hand.  Data parallel is not measured.)  Every figure is the median over ROUNDS rounds of the mean of N back-to-back
calls between two HIP events; the variants alternate inside a round; [min .. max] is the spread over the rounds.
Developer tool:  python tools/ab_layerscale.py [--out profiles/layerscale_ab.txt] [--skip-step] [--skip-kernels] [--copy-tbs 4.0]"""
import argparse
import gc
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import torch  # noqa: E402

from vitssl_hip import _lib as L  # noqa: E402
from vitssl_hip import ops  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 7
MODELS = {"ViT-B/16": (dict(embed_dim=768, num_blocks=12, num_heads=12, mlp_dim=3072), 256),
          "ViT-L/16": (dict(embed_dim=1024, num_blocks=24, num_heads=16, mlp_dim=4096), 128)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true", help="leave out the fused steps")
    ap.add_argument("--skip-kernels", action="store_true", help="leave out the isolated kernels")
    ap.add_argument("--copy-tbs", type=float, default=4.0, help="copy rate of tools/hbm_probe.py in TB/s (read + write bytes a second)")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda med, spread, k: f"{med[k]:9.1f} us  [{spread[k][0]:.1f} .. {spread[k][1]:.1f}]"      # noqa: E731

    def pair(label, med, spread, a, b, extra_bytes):
        d = med[b] - med[a]
        own = spread[a][1] - spread[a][0]
        verdict = "within" if abs(d) <= own else "OUTSIDE"
        say(f"   {label:44s} plain {fmt(med, spread, a)}   ls {fmt(med, spread, b)}   difference {d:+7.1f} us ({100 * d / med[a]:+.2f} %), "
            f"{verdict} the plain launch's own spread of {own:.1f} us; extra bytes {extra_bytes / 1e6:.1f} MB = "
            f"{extra_bytes / (args.copy_tbs * 1e12) * 1e6:.1f} us at {args.copy_tbs:g} TB/s")

    say(f"tools/ab_layerscale.py on {torch.cuda.get_device_name(0)}: median of {ROUNDS} rounds x N calls, variants alternating")

    if not args.skip_step:
        from vit_core._runtime import limit_host_threads
        from vit_core.vit import ViT
        from vitssl_hip.optim import FusedAdamW
        limit_host_threads()
        say()
        say("2. supervised fused step (ViT.train_step, 224 x 224, 10 classes, dropout 0.1, bf16 operands), layer_scale_init 1e-5 against none (us a step)")
        for name, (cfg, batch) in MODELS.items():
            g = torch.Generator().manual_seed(0)
            x, y = torch.rand(batch, 3, 224, 224, generator=g).to(DEV), torch.randint(0, 10, (batch,), generator=g).to(DEV)
            steps = {}
            for key, extra in (("plain", {}), ("ls", {"layer_scale_init": 1e-5})):
                torch.manual_seed(1)
                model = ViT(num_classes=10, input_shape=(3, 224, 224), patch_size=16, dropout=0.1, **extra, **cfg).to(DEV).train()
                opt = FusedAdamW(model.flat_store(), lr=1e-4, weight_decay=0.05)
                steps[key] = (lambda m, o: lambda: m.train_step(x, y, o))(model, opt)
            med, spread = interleaved(steps, n=8, warm=4)
            d = med["ls"] - med["plain"]
            Lb, Mb, Db = cfg["num_blocks"], batch * 197, cfg["embed_dim"]
            extra_bytes = 2 * 2 * Lb * Mb * Db * 2               # two branches a block, written once and read once, bf16
            say(f"   {name}, batch {batch}: without {fmt(med, spread, 'plain')}   with {fmt(med, spread, 'ls')}   "
                f"added {d:+.1f} us a step = {100 * d / med['plain']:+.2f} %; branch images {extra_bytes / 2e9:.2f} GB kept, "
                f"{extra_bytes / 1e9:.2f} GB moved = {extra_bytes / (args.copy_tbs * 1e12) * 1e6:.0f} us at {args.copy_tbs:g} TB/s")
            del steps, model, opt
            gc.collect()
            torch.cuda.empty_cache()

    if not args.skip_kernels:
        B, T, D, F = 256, 197, 768, 3072
        M = B * T
        g = torch.Generator().manual_seed(2)
        lsg = (1e-5 * torch.ones(D)).to(DEV)
        branch = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
        dls = torch.zeros(D, device=DEV)
        image = M * D * 2
        drop = ops.make_dropout(0.1, seed=3, site=2)
        say()
        say(f"3. isolated kernels at the ViT-B shapes, M = {B} x {T} = {M} rows, dropout 0.1, gamma 1e-5, no drop path")
        res, out = torch.randn(M, D, generator=g).to(DEV), torch.empty(M, D, device=DEV)
        for label, K in (("residual GEMM, out-projection, N = K = 768", D), ("residual GEMM, FC2, N = 768, K = 3072", F)):
            A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
            W = (0.02 * torch.randn(D, K, generator=g)).to(torch.bfloat16).to(DEV)
            bias = torch.zeros(D, device=DEV)
            med, spread = interleaved({
                "plain": lambda: ops.gemm_nt(A, W, out, L.EPI_RESID, bias=bias, aux=res, drop=drop),
                "ls": lambda: ops.gemm_nt(A, W, out, L.EPI_RESID, bias=bias, aux=res, drop=drop, cols=lsg, branch=branch),
            }, n=20)
            pair(label, med, spread, "plain", "ls", image)
            del A, W
        x = torch.randn(M, D, generator=g).to(DEV)
        gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
        y16, mean, rstd = torch.empty(M, D, dtype=torch.bfloat16, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
        ops.layernorm_fwd(x, gamma, beta, y16, mean, rstd)
        dy = torch.randn(M, D, generator=g).to(torch.bfloat16).to(DEV)
        gres, gm = torch.randn(M, D, generator=g).to(DEV), torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
        dg, db, cs = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        for label, csum in (("layernorm_bwd, with gm_colsum (LayerNorm 1)", cs), ("layernorm_bwd, no gm_colsum (LayerNorm 2)", None)):
            med, spread = interleaved({
                "plain": lambda: ops.layernorm_bwd(dy, x, mean, rstd, gamma, gres, out, gm, dg, db, csum, drop),
                "ls": lambda: ops.layernorm_bwd(dy, x, mean, rstd, gamma, gres, out, gm, dg, db, csum, drop, cols=lsg, branch=branch, dls=dls),
            }, n=20)
            pair(label, med, spread, "plain", "ls", image)
        med, spread = interleaved({
            "plain": lambda: ops.grad_mask_cast(gres, gm, cs, drop),
            "ls": lambda: ops.grad_mask_cast(gres, gm, cs, drop, cols=lsg, branch=branch, dls=dls),
        }, n=20)
        pair("grad_mask_cast, with gm_colsum", med, spread, "plain", "ls", image)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
