"""Planted-key attention inputs, a per-row metric and a bar taken from the oracle's own bf16 emulation (no GPU code).

On `randn` inputs the softmax is diffuse: one (query, key) pair carries about 1/N of a row, and a kernel that drops the last
key of a ragged tile or mis-indexes one row per tile stays far below a whole-tensor rel-L2 bar.  Here every query i has ONE
key perm(i) whose score stands beta = ln(N) + 1 above the rest (mean softmax mass 0.57-0.70 on it for 17..2048 tokens: neither
saturated nor diffuse), perm is a permutation (every key is some query's planted key), and the error is taken per row."""
import math

import torch

from oracle import vit_oracle as O

DH = 64
TENSORS = ("out", "dq", "dk", "dv")
MARGIN = 3.0          # bar = MARGIN x the emulation's own worst row error (lse-recomputed P, hardware exp2, MFMA summation order)
LSE_BAR = 1e-4


def perm_of(name, N):
    i = torch.arange(N)
    if name == "rev":          # query 0 -> the last key of the ragged tail; the planted key crosses every tile boundary
        return N - 1 - i
    if name == "shift":
        return (i + N // 2 + 1) % N
    raise ValueError(name)


def planted(B, N, H, perm, seed):
    """-> bf16 q, k, v, dout [B,H,N,64] and the packed qkv [B*N, 3*H*64].  `perm`: "rev", "shift" or an index tensor [N]."""
    if isinstance(perm, str):
        perm = perm_of(perm, N)
    g = torch.Generator().manual_seed(seed)
    k, v, noise, dout = (torch.randn(B, H, N, DH, generator=g) for _ in range(4))
    beta = math.log(N) + 1.0
    kp = k[:, :, perm]
    q = 0.5 * noise + kp * (math.sqrt(DH) * beta / kp.square().sum(-1, keepdim=True))
    q, k, v, dout = (x.to(torch.bfloat16) for x in (q, k, v, dout))
    return q, k, v, dout, pack_qkv(q, k, v)


def randn_inputs(B, N, H, seed):
    """the inputs of the existing tests, in the same layout as planted()"""
    g = torch.Generator().manual_seed(seed)
    q, k, v, dout = (torch.randn(B, H, N, DH, generator=g).to(torch.bfloat16) for _ in range(4))
    return q, k, v, dout, pack_qkv(q, k, v)


def pack_qkv(q, k, v):
    B, H, N, dh = q.shape
    return torch.stack((q, k, v), 0).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * dh).contiguous()      # [B,N,3,H,dh]


def pack_rows(x):
    """[B,H,N,dh] -> [B*N, H*dh] (the layout of out / dout)"""
    B, H, N, dh = x.shape
    return x.transpose(1, 2).reshape(B * N, H * dh).contiguous()


def unpack_rows(x, B, N, H):
    return x.view(B, N, H, DH).transpose(1, 2)


def unpack_dqkv(dqkv, B, N, H):
    x = dqkv.view(B, N, 3, H, DH)
    return tuple(x[:, :, i].transpose(1, 2) for i in range(3))


def ref64(q, k, v, dout, drop=None):
    """plain fp64 softmax attention with autograd -> dict out, lse, dq, dk, dv.  drop = (b, h, i, j): that score is -inf
    (negative controls only)."""
    q, k, v = (x.double().clone().requires_grad_(True) for x in (q, k, v))
    s = (q @ k.transpose(-2, -1)) / math.sqrt(q.shape[-1])
    if drop is not None:
        m = torch.zeros_like(s, dtype=torch.bool)
        m[drop] = True
        s = s.masked_fill(m, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    out = torch.softmax(s, dim=-1) @ v
    (out * dout.double()).sum().backward()
    return {"out": out.detach(), "lse": lse.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def emu(q, k, v, dout):
    """the oracle's model of the kernels' rounding points (bf16 P, delta from the stored bf16 O, bf16 dS), outputs rounded
    to bf16 as the kernels store them"""
    q, k, v = (x.float().clone().requires_grad_(True) for x in (q, k, v))
    with O.flash_delta():
        o, _ = O.sdpa(q, k, v, emu="bf16")
        (o * dout.float()).sum().backward()
    res = {"out": o.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}
    return {n: x.to(torch.bfloat16).double() for n, x in res.items()}


def row_err(got, ref):
    """[B,H,N,dh] x 2 -> [B,H,N]: |got_row - ref_row| / max(|ref_row|, median over the (b, h) item's rows of |ref_row|).
    The median floor keeps near-saturated rows of dq (tiny |ref_row|) from asking the kernel to beat the conditioning of
    the flash formulation itself."""
    got, ref = got.double().cpu(), ref.double().cpu()
    nrm = ref.norm(dim=-1)
    floor = nrm.median(dim=-1, keepdim=True).values
    return (got - ref).norm(dim=-1) / torch.maximum(nrm, floor)


def bars(ref, em):
    """per tensor: MARGIN x the worst row error of the emulation in this case -> (bars, the emulation's worst row errors)"""
    worst = {n: float(row_err(em[n], ref[n]).max()) for n in TENSORS}
    return {n: MARGIN * w for n, w in worst.items()}, worst


def failures(got, ref, bar, tensors=TENSORS):
    """-> {tensor: (worst row error, (b, h, row))} of the tensors with a NaN or a row above their bar"""
    bad = {}
    for n in tensors:
        e = row_err(got[n], ref[n])
        e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
        if float(e.max()) > bar[n]:
            b, h, r = (int(x) for x in (e == e.max()).nonzero()[0])
            bad[n] = (float(e.max()), (b, h, r))
    return bad
