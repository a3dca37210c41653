"""Attention inputs, references and checkers with the head dim as a parameter (no GPU code): what tests/_attn_planted.py is for
dh = 64, for the head-dim-templated kernels (csrc/attention_hd.hip).

Planted-key inputs: every query i has ONE key perm(i) whose score stands beta = ln(N) + 1 above the rest, perm is a
permutation, and the error is taken per row (row_err, bars, failures: the definitions of _attn_planted.py, which do not
depend on the head dim and are re-used as they are).  The whole-tensor bars are those of
tests/test_gpu_ops.py::test_attention_fwd_bwd.  The case lists of the GPU tests live here so that the CPU tests can run the
oracle's bf16 emulation through exactly the checks the kernels get."""
import functools
import math

import torch

from _attn_planted import LSE_BAR, MARGIN, TENSORS, failures, pack_qkv, pack_rows, perm_of, ref64, row_err   # noqa: F401
from _util import max_abs, rel_l2
from oracle import vit_oracle as O

B, H = 2, 3

# ---- the cases of tests/test_gpu_attention_hd.py
WHOLE_DHS = [8, 16, 32, 48, 80, 96, 128]
WHOLE_NS = [5, 197]
# streamed tiles are 64 rows and every kernel's workgroup tile is 128 rows: one below, on and one above each; 197 = three full
# streamed tiles and a ragged tail of 5
ROW_NS = [1, 63, 64, 65, 127, 128, 129, 197]
ROW_LONG = [(80, 300), (32, 257)]     # more than one workgroup per item AND three or more streamed tiles, per row as well
ROW_DHS = [8, 32, 80, 128]            # 32 and 128: no pad columns; 8 (in 32) and 80 (in 96): pad columns
PERMS = ["rev", "shift"]
CROSS_NS = [37, 197, 300]             # dh = 64 against the dh = 64 kernels
POISON = (80, 300)
LARGE = [(32, 45), (128, 45)]
BOUNDS = [(8, 1), (80, 129), (128, 65), (32, 257)]


def padded(dh):
    """the width the kernels are instantiated for"""
    return 32 * ((dh + 31) // 32)


# ------------------------------------------------------------------------------------------------ inputs
def planted(Bn, N, Hn, dh, perm, seed):
    """-> bf16 q, k, v, dout [B,H,N,dh] and the packed qkv [B*N, 3*H*dh].  `perm`: "rev", "shift" or an index tensor [N]."""
    if isinstance(perm, str):
        perm = perm_of(perm, N)
    g = torch.Generator().manual_seed(seed)
    k, v, noise, dout = (torch.randn(Bn, Hn, N, dh, generator=g) for _ in range(4))
    beta = math.log(N) + 1.0
    kp = k[:, :, perm]
    q = 0.5 * noise + kp * (math.sqrt(dh) * beta / kp.square().sum(-1, keepdim=True))
    q, k, v, dout = (x.to(torch.bfloat16) for x in (q, k, v, dout))
    return q, k, v, dout, pack_qkv(q, k, v)


def randn_inputs(Bn, N, Hn, dh, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v, dout = (torch.randn(Bn, Hn, N, dh, generator=g) for _ in range(4))
    q, k, v = ((x * scale).to(torch.bfloat16) for x in (q, k, v))
    dout = dout.to(torch.bfloat16)
    return q, k, v, dout, pack_qkv(q, k, v)


def unpack_rows(x, Bn, N, Hn, dh):
    return x.view(Bn, N, Hn, dh).transpose(1, 2)


def unpack_dqkv(dqkv, Bn, N, Hn, dh):
    x = dqkv.view(Bn, N, 3, Hn, dh)
    return tuple(x[:, :, i].transpose(1, 2) for i in range(3))


# ------------------------------------------------------------------------------------------------ references
def oracle32(q, k, v, dout):
    """the fp32 oracle (oracle.sdpa, no emulation) with autograd -> out, probs, lse, dq, dk, dv"""
    q, k, v = (x.float().clone().requires_grad_(True) for x in (q, k, v))
    o, p = O.sdpa(q, k, v, None)
    s = (q @ k.transpose(-2, -1)) / math.sqrt(q.shape[-1])
    (o * dout.float()).sum().backward()
    return {"out": o.detach(), "probs": p.detach(), "lse": torch.logsumexp(s, dim=-1).detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


def emu(q, k, v, dout, full=False):
    """the oracle's model of the kernels' rounding points (bf16 P into P.V, delta from the stored bf16 O, bf16 dS): oracle.sdpa(emu="bf16")
    under flash_delta(), outputs rounded to bf16 as the kernels store them.  full: probs and lse (fp32) as well."""
    q, k, v = (x.float().clone().requires_grad_(True) for x in (q, k, v))
    with O.flash_delta():
        o, p = O.sdpa(q, k, v, emu="bf16")
        (o * dout.float()).sum().backward()
    res = {n: x.to(torch.bfloat16).double() for n, x in (("out", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad))}
    if full:
        s = (q.detach() @ k.detach().transpose(-2, -1)) / math.sqrt(q.shape[-1])
        res["probs"], res["lse"] = p.detach(), torch.logsumexp(s, dim=-1)
    return res


def bars(ref, em, tensors=TENSORS):
    """per tensor: MARGIN x the worst row error of the emulation in this case -> (bars, the emulation's worst row errors)"""
    worst = {n: float(row_err(em[n], ref[n]).max()) for n in tensors}
    return {n: MARGIN * w for n, w in worst.items()}, worst


def row_tensors(N):
    """With one token the softmax is the constant 1: dq and dk are identically zero, a relative row error has no denominator, and
    they are held to single_token_bound instead."""
    return ("out", "dv") if N == 1 else TENSORS


def single_token_bound(q, k, v, dout):
    """N = 1: dS = P (dP - delta) with P = 1 and dP = <dO, v> = delta in exact arithmetic (O = v exactly).  The two are fp32 sums
    of the same dh products in different orders, each within dh * 2^-24 * sum |dO_d v_d| of the exact value, so
    |dS| <= 2 dh 2^-24 sum |dO_d v_d| (x 1.01 for its bf16 rounding), and |dq row| = |dS| |k row| / sqrt(dh), |dk row| likewise
    with q.  -> bounds [B,H,1] on the row norms of dq and dk."""
    dh = q.shape[-1]
    ds = 1.01 * 2.0 * dh * 2.0 ** -24 * (dout.double() * v.double()).abs().sum(-1)
    return ds * k.double().norm(dim=-1) / math.sqrt(dh), ds * q.double().norm(dim=-1) / math.sqrt(dh)


def check_rows(got, case, what=""):
    """the per-row assertions of the GPU test on `got` (dict out, lse, dq, dk, dv; CPU tensors) -> the worst row errors"""
    (q, k, v, dout), ref, em, bar, emu_worst = case
    N = q.shape[-2]
    tensors = row_tensors(N)
    for n in ("out", "lse", "dq", "dk", "dv"):
        assert not torch.isnan(got[n].float()).any(), f"{what} {n}: NaN left"
    lse_err = float((got["lse"].double() - ref["lse"]).abs().max())
    worst = {n: float(row_err(got[n], ref[n]).max()) for n in tensors}
    print(f"{what}: max row error (got / emulation) " + "  ".join(f"{n} {worst[n]:.2e} / {emu_worst[n]:.2e}" for n in tensors)
          + f"  lse {lse_err:.2e}")
    assert lse_err < LSE_BAR, f"{what} lse: max abs error {lse_err:.3e}"
    bad = failures(got, ref, bar, tensors=tensors)
    assert not bad, what + " " + "; ".join(f"{n}: row error {e:.3e} > {bar[n]:.3e} at (b, h, row) = {at}" for n, (e, at) in bad.items())
    if N == 1:
        bq, bk = single_token_bound(q, k, v, dout)
        assert bool((got["dq"].double().norm(dim=-1) <= bq).all()) and bool((got["dk"].double().norm(dim=-1) <= bk).all()), \
            f"{what}: dq / dk of a single token must vanish up to fp32 summation order"
    return worst


@functools.lru_cache(maxsize=None)
def planted_case(dh, N, perm, Bn=B, Hn=H):
    """inputs, fp64 reference, emulation, bars and the emulation's worst row errors; computed once, shared by the tests"""
    q, k, v, dout, _ = planted(Bn, N, Hn, dh, perm, seed=1000 * dh + 10 * N + PERMS.index(perm))
    ref = ref64(q, k, v, dout)
    em = emu(q, k, v, dout)
    bar, worst = bars(ref, em, row_tensors(N))
    return (q, k, v, dout), ref, em, bar, worst


@functools.lru_cache(maxsize=None)
def randn_case(dh, N, scale=1.0, Bn=B, Hn=H):
    """Gaussian inputs of seed 1000 dh + N and their fp32-oracle results, computed once"""
    q, k, v, dout, qkv = randn_inputs(Bn, N, Hn, dh, seed=1000 * dh + N, scale=scale)
    return (q, k, v, dout, qkv), oracle32(q, k, v, dout)


def check_whole(got, ref, what="", inputs=None):
    """the whole-tensor bars of test_gpu_ops.py::test_attention_fwd_bwd on `got` (dict with out, lse, dq, dk, dv and, if present,
    probs), against the fp32 oracle.  With one token dq and dk are identically zero (row_tensors): they are held to
    single_token_bound of `inputs` = (q, k, v, dout) instead of a relative bar."""
    figs = {}
    single = got["lse"].shape[-1] == 1
    grads = ("dv",) if single else ("dq", "dk", "dv")
    if "probs" in got:
        figs["probs rel"], figs["probs abs"] = rel_l2(got["probs"], ref["probs"]), max_abs(got["probs"], ref["probs"])
    figs["lse abs"] = max_abs(got["lse"], ref["lse"])
    refo = ref["out"].to(torch.bfloat16).float()
    figs["out excess"] = float(((got["out"].float() - refo).abs() - (4e-3 + 2.0 ** -7 * refo.abs())).max())
    for n in grads:
        figs[n + " rel"] = rel_l2(got[n], ref[n])
    print(f"{what}: " + "  ".join(f"{n} {x:.2e}" for n, x in figs.items()))
    for n in ("out", "lse", "dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all(), f"{what} {n}: not finite"
    if "probs" in got:
        assert figs["probs rel"] < 1e-3 and figs["probs abs"] < 2e-4, what
    assert figs["lse abs"] < 1e-4, what
    close_bf16(got["out"], refo, atol=4e-3, what=what + " attn out")
    for n in grads:
        assert figs[n + " rel"] < 2e-2, (what, n)
    if single:
        bq, bk = single_token_bound(*inputs)
        assert bool((got["dq"].double().norm(dim=-1) <= bq).all()) and bool((got["dk"].double().norm(dim=-1) <= bk).all()), \
            f"{what}: dq / dk of a single token must vanish up to fp32 summation order"
    return figs


def close_bf16(got, ref, atol, what=""):
    """close_bf16 of tests/test_gpu_ops.py (atol + one bf16 ulp of the reference), importable without a GPU"""
    g, r = got.float().cpu(), ref.float().cpu()
    tol = atol + 2.0 ** -7 * r.abs()
    bad = (g - r).abs() > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, worst {float((g - r).abs().max()):.3e}"


# ------------------------------------------------------------------------------------------------ negative controls
ITEM = (1, 1)
MUTATIONS = ["drop_pair", "key_off_by_one", "stale_delta", "scale_eighth", "pad_nonzero"]


def _bf(x):
    return x.to(torch.bfloat16).float()


def flash(q, k, v, dout, mutation=None, i=None, j=None):
    """The flash-style forward / backward with the kernels' rounding points, outputs rounded to bf16.  `mutation` plants one
    fault in item ITEM (row i, j = its planted key):
      drop_pair       score (i, j) = -inf in the forward and the backward
      key_off_by_one  row i reads k[j + 1] where it should read k[j] (scores and dQ)
      stale_delta     the backward takes delta of row i from row i + 1
      scale_eighth    the item's scores (and dS) are scaled by 1/8 where 1/sqrt(dh) is due
      pad_nonzero     the contraction of the item's scores runs over one column >= dh that is not zero: what lies behind a head's
                      slice of a qkv row is the next head's (or k's / v's) first column
    (i + 1, j + 1 wrap around at N)."""
    q, k, v, do = (x.float() for x in (q, k, v, dout))
    N, dh = q.shape[-2], q.shape[-1]
    b, h = ITEM
    sc = torch.full((q.shape[0], q.shape[1], 1, 1), 1.0 / math.sqrt(dh))
    if mutation == "scale_eighth":
        sc[b, h] = 0.125
    s = (q @ k.transpose(-2, -1)) * sc
    if mutation == "pad_nonzero":
        hn = (h + 1) % q.shape[1]
        s[b, h] = s[b, h] + torch.outer(q[b, hn, :, 0], k[b, hn, :, 0]) * sc[b, h]
    if mutation == "drop_pair":
        s[b, h, i, j] = float("-inf")
    if mutation == "key_off_by_one":
        s[b, h, i, j] = (q[b, h, i] * k[b, h, (j + 1) % N]).sum() * sc[b, h, 0, 0]
    lse = torch.logsumexp(s, dim=-1)
    o = _bf(torch.exp(s - lse[..., None])) @ v
    p = torch.exp(s - lse[..., None])
    dv = _bf(p).transpose(-2, -1) @ do
    dp = do @ v.transpose(-2, -1)
    delta = (do * _bf(o)).sum(-1)
    if mutation == "stale_delta":
        d = delta.clone()
        d[b, h, i] = delta[b, h, (i + 1) % N]
        delta = d
    ds = _bf(p * (dp - delta[..., None]))
    dq = (ds @ k) * sc
    if mutation == "key_off_by_one":
        k1 = k[b, h].clone()
        k1[j] = k[b, h, (j + 1) % N]
        dq[b, h, i] = (ds[b, h, i] @ k1) * sc[b, h, 0, 0]
    dk = (ds.transpose(-2, -1) @ q) * sc
    return {n: x.to(torch.bfloat16).double() for n, x in (("out", o), ("dq", dq), ("dk", dk), ("dv", dv))}
