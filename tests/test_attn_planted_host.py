"""The per-row checker of tests/_attn_planted.py is not vacuous (CPU only).

The oracle's bf16 emulation passes it, and a flash-style pipeline with ONE localised fault -- what a wrong tail mask, a key
read one index off, or a stale row of `delta` / `lse` does in a kernel -- fails it on at least one of out, dq, dv (the rows the
forward, the dQ kernel and the dK/dV kernel each write), at every fixed position and for both permutations.  On `randn`
inputs the same dropped pair stays under the whole-tensor bar of the existing tests: that is why this file exists."""
import functools
import math

import pytest
import torch

import _attn_planted as P
from _util import rel_l2

B, H = 2, 2
ITEM = (1, 1)                        # the (b, h) item the faults are planted in
LENGTHS = [17, 129, 257, 785]
PERMS = ["rev", "shift"]
MUTATIONS = ["drop_pair", "key_off_by_one", "stale_delta", "stale_lse"]


def _bf(x):
    return x.to(torch.bfloat16).float()


def flash(q, k, v, dout, mutation=None, i=None, j=None):
    """The flash-style forward / backward with the rounding points of oracle.sdpa(emu="bf16") under flash_delta() (bf16 P, delta
    from the stored bf16 O, bf16 dS, P recomputed from lse), outputs rounded to bf16.  `mutation` plants one fault in row i of
    item ITEM (j = its planted key):
      drop_pair       score (i, j) = -inf in the forward and the backward
      key_off_by_one  row i reads k[j + 1] where it should read k[j] (scores and dQ)
      stale_delta     the backward takes delta of row i from row i + 1
      stale_lse       the backward takes lse of row i from row i + 1
    (i + 1, j + 1 wrap around at N)."""
    q, k, v, do = (x.float() for x in (q, k, v, dout))
    N = q.shape[-2]
    b, h = ITEM
    sc = 1.0 / math.sqrt(q.shape[-1])
    s = (q @ k.transpose(-2, -1)) * sc
    if mutation == "drop_pair":
        s[b, h, i, j] = float("-inf")
    if mutation == "key_off_by_one":
        s[b, h, i, j] = (q[b, h, i] * k[b, h, (j + 1) % N]).sum() * sc
    lse = torch.logsumexp(s, dim=-1)
    o = _bf(torch.exp(s - lse[..., None])) @ v
    lse_b = lse.clone()
    if mutation == "stale_lse":
        lse_b[b, h, i] = lse[b, h, (i + 1) % N]
    p = torch.exp(s - lse_b[..., None])
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
        dq[b, h, i] = (ds[b, h, i] @ k1) * sc
    dk = (ds.transpose(-2, -1) @ q) * sc
    return {n: x.to(torch.bfloat16).double() for n, x in (("out", o), ("dq", dq), ("dk", dk), ("dv", dv))}


def positions(N):
    """the fixed query rows {0, 15, 16, 63, 64, N-1}, as far as the case has them"""
    return sorted({i for i in (0, 15, 16, 63, 64, N - 1) if i < N})


MIN_DLSE, MIN_DDELTA = 0.05, 0.5


def stale_rows_differ(N, ref, dout):
    """A stale row of lse / delta is a fault only if the neighbour's value differs: lse by >= 0.05 (row i of P off by 5 %),
    delta by >= 0.5 (a tenth of its spread over the rows, ~|O row| ~ 5), at every fixed position.  Judged on the fp64
    reference alone."""
    b, h = ITEM
    lse = ref["lse"][b, h]
    delta = (dout.double() * ref["out"]).sum(-1)[b, h]
    return all(abs(float(lse[i] - lse[(i + 1) % N])) >= MIN_DLSE and abs(float(delta[i] - delta[(i + 1) % N])) >= MIN_DDELTA
               for i in positions(N))


@functools.lru_cache(maxsize=None)
def case(N, perm):
    """Inputs of seed N, N + 1000, ...: the first draw on which the stale-row faults are faults (about one neighbour pair in
    forty is closer than that by chance).  No length, permutation, position or mutation is left out."""
    for seed in range(N, N + 20000, 1000):
        q, k, v, dout, _ = P.planted(B, N, H, perm, seed=seed)
        ref = P.ref64(q, k, v, dout)
        if stale_rows_differ(N, ref, dout):
            break
    else:
        raise AssertionError("no draw with distinct neighbouring lse / delta rows")
    em = P.emu(q, k, v, dout)
    bar, worst = P.bars(ref, em)
    return (q, k, v, dout), ref, em, bar, worst


@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("N", LENGTHS)
def test_planted_inputs_are_neither_saturated_nor_diffuse(N, perm):
    (q, k, v, dout), ref, _, _, _ = case(N, perm)
    pm = P.perm_of(perm, N)
    assert sorted(pm.tolist()) == list(range(N))
    s = (q.double() @ k.double().transpose(-2, -1)) / 8.0
    mass = torch.softmax(s, dim=-1)[..., torch.arange(N), pm].mean()
    print(f"N={N} {perm}: mean mass on the planted key {float(mass):.3f}")
    assert 0.5 < float(mass) < 0.8


@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("N", LENGTHS)
def test_emulation_passes_the_checker(N, perm):
    inputs, ref, em, bar, worst = case(N, perm)
    print(f"N={N} {perm}: emulation's worst row error " + "  ".join(f"{n} {worst[n]:.2e}" for n in P.TENSORS))
    assert all(0 < worst[n] < 5e-2 for n in P.TENSORS), worst        # a bar of 3 x this still means something
    assert P.failures(em, ref, bar) == {}
    fl = flash(*inputs)                                              # the carrier of the faults below, without one
    assert P.failures(fl, ref, bar) == {}


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("perm", PERMS)
@pytest.mark.parametrize("N", LENGTHS)
def test_one_local_fault_fails_the_checker(N, perm, mutation):
    inputs, ref, _, bar, _ = case(N, perm)
    pm = P.perm_of(perm, N)
    for i in positions(N):
        j = int(pm[i])
        bad = P.failures(flash(*inputs, mutation=mutation, i=i, j=j), ref, bar, tensors=("out", "dq", "dv"))
        assert bad, f"{mutation} at row {i}, key {j} passes the checker"
        for n, (err, (b, h, r)) in bad.items():                      # and it is found where it was planted
            assert (b, h) == ITEM and r == (j if n == "dv" else i), (mutation, i, j, n, err, (b, h, r))


@pytest.mark.parametrize("N,BH", [(197, (2, 2)), (785, (2, 2)), (2048, (1, 1))])
def test_dropped_pair_hides_under_the_tensor_bar_on_randn(N, BH):
    """Regression note: one (query, key) pair removed from item (0, 0) of Gaussian inputs moves out, dq, dk and dv of that item
    by far less than the rel-L2 < 2e-2 that test_attention_fwd_bwd, _check_bwd_items and test_attention_long_fwd_bwd ask."""
    q, k, v, dout, _ = P.randn_inputs(BH[0], N, BH[1], seed=N)
    ref = P.ref64(q, k, v, dout)
    mut = P.ref64(q, k, v, dout, drop=(0, 0, 0, N - 1))
    errs = {n: rel_l2(mut[n][0, 0], ref[n][0, 0]) for n in P.TENSORS}
    print(f"N={N}: " + "  ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert all(0 < e < 2e-2 for e in errs.values()), errs
