#!/usr/bin/env python3
"""Median time of the attention forward / backward launches at one geometry (developer tool; compare builds or
VITSSL_ATTN_STAGGER_* settings by running it in alternation), next to the reference formulation on the same tensors:
softmax(q @ k^T / 8) @ v in bf16 through torch (vit_core/attention.py:20-23 of the reference), forward and forward + backward.
The two implementations alternate round by round in one process; medians and the min - max spread of the rounds are printed.
B H N as arguments, default 256 12 196.  An optional fourth argument is the head dim (default 64): any other supported value
times the head-dim-templated kernels (ops.attn_hd_*), the reference formulation with 1 / sqrt(dh), and as a second baseline
the dh = 64 kernels at the same B, H, N, compared as rates per flop."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vit-ssl_amd"))
from vitssl_hip import ops  # noqa: E402

B, H, N = (int(v) for v in (sys.argv[1:4] if len(sys.argv) >= 4 else (256, 12, 196)))
DH = int(sys.argv[4]) if len(sys.argv) >= 5 and not sys.argv[4].startswith("--") else 64      # a mistyped head dim raises
attn_fwd, attn_bwd = ops.attn_family(DH)
dev = torch.device("cuda:0")
torch.manual_seed(0)
qkv = torch.randn(B * N, 3 * H * DH, device=dev).to(torch.bfloat16)
out = torch.empty(B * N, H * DH, dtype=torch.bfloat16, device=dev)
lse = torch.empty(B, H, N, device=dev)
dout = torch.randn(B * N, H * DH, device=dev).to(torch.bfloat16)
dqkv = torch.empty_like(qkv)
delta = torch.empty(B, H, N, device=dev)


# the reference formulation's operands: the same values as [B, H, N, 64] tensors (contiguous, as its Linear + transpose leave them)
x5 = qkv.view(B, N, 3, H, DH)
q_r, k_r, v_r = (x5[:, :, i].transpose(1, 2).contiguous().requires_grad_(True) for i in range(3))
do_r = dout.view(B, N, H, DH).transpose(1, 2).contiguous()


def ref_fwd():
    with torch.no_grad():
        return torch.matmul(torch.softmax(torch.matmul(q_r, k_r.transpose(-2, -1)) * DH ** -0.5, dim=-1), v_r)


def ref_fwd_bwd():
    o = torch.matmul(torch.softmax(torch.matmul(q_r, k_r.transpose(-2, -1)) * DH ** -0.5, dim=-1), v_r)
    torch.autograd.grad(o, (q_r, k_r, v_r), do_r)


def ours_fwd():
    attn_fwd(qkv, out, lse, B, N, H, DH)


def ours_fwd_bwd():
    attn_fwd(qkv, out, lse, B, N, H, DH)
    attn_bwd(qkv, out, dout, lse, dqkv, delta, B, N, H, DH)


def ours_bwd():
    attn_bwd(qkv, out, dout, lse, dqkv, delta, B, N, H, DH)


def time_alternating(fns, rounds=15, iters=4):
    """fns: name -> callable; every round times each of them once, in turn.  Returns name -> sorted round times (us per call)."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / iters * 1e3)
    return {k: sorted(v) for k, v in ts.items()}


def med(v):
    return v[len(v) // 2]


with_ref = "--no-ref" not in sys.argv
fns = {"fwd": ours_fwd, "bwd": ours_bwd, "fwd+bwd": ours_fwd_bwd}
if DH != 64:      # second baseline: the dh = 64 kernels on tensors of the same B, H, N (lse and delta are shared with the
    # kernels under test: both are [B, H, N] outputs / workspaces that every call rewrites, and only times are compared)
    qkv64 = torch.randn(B * N, 3 * H * 64, device=dev).to(torch.bfloat16)
    out64, dout64, dqkv64 = torch.empty(B * N, H * 64, dtype=torch.bfloat16, device=dev), torch.randn(B * N, H * 64, device=dev).to(torch.bfloat16), torch.empty_like(qkv64)
    fns["dh64 fwd"] = lambda: ops.attn_fwd(qkv64, out64, lse, B, N, H, 64)
    fns["dh64 fwd+bwd"] = lambda: (ops.attn_fwd(qkv64, out64, lse, B, N, H, 64), ops.attn_bwd(qkv64, out64, dout64, lse, dqkv64, delta, B, N, H, 64))
if with_ref:
    fns.update({"ref fwd": ref_fwd, "ref fwd+bwd": ref_fwd_bwd})
ts = time_alternating(fns)
fl = 4.0 * B * H * N * N * DH
f, b = med(ts["fwd"]), med(ts["bwd"])
print(f"B{B} H{H} N{N}" + (f" dh{DH}" if DH != 64 else "") + f": fwd {f:7.1f} us {fl / f / 1e6:6.1f} TF/s | bwd {b:7.1f} us {2.0 * fl / b / 1e6:6.1f} TF/s", flush=True)
for k, v in ts.items():
    print(f"  {k:12s} median {med(v):9.1f} us   min {v[0]:9.1f}   max {v[-1]:9.1f}", flush=True)
if with_ref:
    print(f"  reference / ours: fwd {med(ts['ref fwd']) / f:5.2f}x   fwd+bwd {med(ts['ref fwd+bwd']) / med(ts['fwd+bwd']):5.2f}x", flush=True)
if DH != 64:
    print(f"  rate per flop against the dh = 64 kernels: fwd {med(ts['dh64 fwd']) / f * DH / 64:5.2f}x   "
          f"fwd+bwd {med(ts['dh64 fwd+bwd']) / med(ts['fwd+bwd']) * DH / 64:5.2f}x", flush=True)
