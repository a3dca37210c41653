"""MAE on the GPU, measured:
  1. every kernel of include_ext/vitssl_mae.h at the ViT-B/16 batch-256 shapes (N = 196, K = 49, D = 768, Dd = 512, Pd = 768):
     time, the bytes the algorithm moves (computed from the shapes below) and their rate as a share of the copy rate that
     tools/hbm_probe.py measures in this same process.  Every call of a kernel takes the next of several buffer sets that
     together pass 600 MB, so that a call does not find its operands in the 256 MiB Infinity Cache;
  2. the MAEViT fused step (mask ratio 0.75, the paper's decoder: 8 blocks, width 512, 16 heads) against the SimMIMViT fused
     step of the same encoder (ViT-B/16, batch 256, 224 x 224, mask ratio 0.6), alternating in one process.  By flop count the
     MAE step is about 0.55-0.6 of the SimMIM step.
Every figure is the median over ROUNDS rounds of the mean of N back-to-back calls between two HIP events; the variants alternate
inside a round.  Developer tool:  python tools/ab_mae.py [--out profiles/mae_ab.txt] [--skip-step] [--skip-kernels]"""
import argparse
import contextlib
import io
import itertools
import os
import re
import runpy
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
import torch  # noqa: E402

from vitssl_hip import ops  # noqa: E402

DEV = torch.device("cuda:0")
ROUNDS = 7
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
B, N, K, D, DD, PD = 256, 196, 49, 768, 512, 768
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


def kernels():
    """name -> (callable, bytes the algorithm moves per call)"""
    from vit_core.ssl.mae import masking as Mk
    g = torch.Generator().manual_seed(0)
    keep, restore = Mk.draw_keep(B, N, K, generator=g)
    idx = Mk.MAEIndices(keep, restore, K)
    t = {n: torch.from_numpy(getattr(idx, n)).to(DEV) for n in idx.NAMES}
    keep_d, restore_d = t["keep"].view(B, K), t["restore"].view(B, N)
    Mm, M1, M2 = idx.Mm, B * (K + 1), B * (N + 1)
    rn = lambda *s: torch.randn(*s, device=DEV)      # noqa: E731
    em = lambda *s, dtype=F32: torch.empty(*s, dtype=dtype, device=DEV)      # noqa: E731
    pos, cls, dpos, mt = rn(N + 1, D), rn(D), rn(N + 1, DD), rn(DD)
    out = {}

    def add(name, nbytes, make):
        out[name] = (rotating(make, nbytes), nbytes)

    def tokens_fwd():
        xk, o = rn(B * K, D), em(M1, D)
        return lambda: ops.mae_tokens_fwd(xk, keep_d, pos, cls, o, B, N, K)
    add("mae_tokens_fwd", 4 * D * (B * K + M1 + N + 1) + 4 * B * K, tokens_fwd)

    def tokens_bwd():
        gg, dp, s0, s1 = rn(M1, D), em(B * K, D, dtype=BF16), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        return lambda: ops.mae_tokens_bwd(gg, dp, s0, s1, B, N, K)
    add("mae_tokens_bwd", D * (4 * M1 + 2 * B * K), tokens_bwd)

    def unshuffle_fwd():
        y, o = rn(M1, DD), em(M2, DD)
        return lambda: ops.mae_unshuffle_fwd(y, restore_d, mt, dpos, o, B, N, K)
    add("mae_unshuffle_fwd", 4 * DD * (M1 + M2 + N + 2) + 4 * B * N, unshuffle_fwd)

    def unshuffle_bwd():
        gg, dy, s0, s1 = rn(M2, DD), em(M1, DD, dtype=BF16), torch.zeros(DD, device=DEV), torch.zeros(DD, device=DEV)
        return lambda: ops.mae_unshuffle_bwd(gg, restore_d, dy, s0, s1, B, N, K)
    add("mae_unshuffle_bwd", DD * (4 * M2 + 2 * M1) + 4 * B * N, unshuffle_bwd)

    for norm in (True, False):
        def loss(norm=norm):
            pred, tgt, ls, dp = rn(Mm, PD), torch.rand(Mm, PD, device=DEV), torch.zeros(1, device=DEV), em(Mm, PD, dtype=BF16)
            return lambda: ops.mae_loss(pred, tgt, ls, dp, gscale=1.0 / Mm, norm_pix=norm)      # (normalising again: the same work)
        add("mae_loss, norm_pix" if norm else "mae_loss, raw pixels", Mm * PD * (4 + 4 + (4 if norm else 0) + 2), loss)

    def gather_bf16():
        src, o = rn(B * N, PD).to(BF16), em(B * K, PD, dtype=BF16)
        return lambda: ops.mae_gather_rows_bf16(src, t["keep_rows"], o)
    add("mae_gather_rows_bf16", 2 * 2 * B * K * PD + 4 * B * K, gather_bf16)

    def gather_f32():
        src, o = rn(M2, DD), em(Mm, DD)
        return lambda: ops.mae_gather_rows_f32(src, t["mrows"], o)
    add("mae_gather_rows_f32", 2 * 4 * Mm * DD + 4 * Mm, gather_f32)

    def scatter_f32():
        src, o = rn(Mm, DD), em(M2, DD)
        return lambda: ops.mae_scatter_rows_f32(src, t["inv"], o)
    add("mae_scatter_rows_f32", 4 * DD * (Mm + M2) + 4 * M2, scatter_f32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-step", action="store_true", help="leave out the two ViT-B/16 steps")
    ap.add_argument("--skip-kernels", action="store_true", help="leave out the copy-rate probe and the kernel table")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/ab_mae.py on {torch.cuda.get_device_name(0)}: median of {ROUNDS} rounds x N calls, variants alternating")
    if not args.skip_kernels:
        text, copy_rate = probe_copy_rate()
        say()
        say("0. tools/hbm_probe.py in this process")
        for ln in text.strip().splitlines():
            say("   " + ln)
        say(f"   the yardstick below: the fp32 copy at 616 MB, {copy_rate:.2f} TB/s (read + write)")

        say()
        say(f"1. kernels of include_ext/vitssl_mae.h at B = {B}, N = {N}, K = {K}, D = {D}, Dd = {DD}, Pd = {PD} "
            f"(buffer sets rotate over more than {FOOTPRINT / 1e6:.0f} MB)")
        ks = kernels()
        med, spread = interleaved({k: fn for k, (fn, _) in ks.items()}, n=24)
        for k, (_, nbytes) in ks.items():
            rate = nbytes / (med[k] * 1e-6) / 1e12
            say(f"   {k:24s} {med[k]:8.1f} us  [{spread[k][0]:.1f} .. {spread[k][1]:.1f}]   {nbytes / 1e6:7.1f} MB   {rate:5.2f} TB/s   "
                f"{rate / copy_rate:5.2f} of the copy rate")
        del ks
        torch.cuda.empty_cache()

    if not args.skip_step:
        from vit_core.ssl.mae import MAEViT
        from vit_core.ssl.simmim import SimMIMViT
        from vitssl_hip.optim import FusedAdamW
        torch.manual_seed(0)
        enc = dict(num_blocks=12, input_shape=(3, 224, 224), embed_dim=768, patch_size=16, num_heads=12, mlp_dim=3072)
        mae = MAEViT(**enc, mask_ratio=0.75).to(DEV).train()
        sim0 = SimMIMViT(**enc, dropout=0.0, mask_ratio=0.6).to(DEV).train()
        sim1 = SimMIMViT(**enc, dropout=0.1, mask_ratio=0.6).to(DEV).train()
        opts = {id(m): FusedAdamW(m.flat_store(), lr=1e-4, weight_decay=0.05) for m in (mae, sim0, sim1)}
        xb = torch.rand(256, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
        step = lambda m: (lambda: m.train_step(xb, opts[id(m)]))      # noqa: E731
        med, spread = interleaved({"mae": step(mae), "simmim": step(sim0), "simmim_drop": step(sim1)}, n=5, warm=3)
        fmt = lambda k: f"{med[k] / 1e3:8.2f} ms  [{spread[k][0] / 1e3:.2f} .. {spread[k][1] / 1e3:.2f}]"      # noqa: E731
        say()
        say("2. fused train step, ViT-B/16 encoder, batch 256, 224 x 224, fused AdamW (ms a step, mask draw and table upload included)")
        say(f"   MAEViT, mask ratio 0.75, decoder 8 x 512 x 16 heads, norm_pix_loss   {fmt('mae')}")
        say(f"   SimMIMViT, mask ratio 0.6, dropout 0                                 {fmt('simmim')}")
        say(f"   SimMIMViT, mask ratio 0.6, dropout 0.1 (the headline benchmark's)    {fmt('simmim_drop')}")
        say(f"   MAE / SimMIM = {med['mae'] / med['simmim']:.3f} (dropout 0), {med['mae'] / med['simmim_drop']:.3f} (dropout 0.1); "
            "the flop count expects about 0.55-0.6")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
