"""Each kernel of include_ext/vitssl_mae.h alone, against torch on the same tensors.

Forwards: every output element is ONE fp32 add, so the results are compared as bits.  Backwards: the bf16 results are the one
round-to-nearest-even of an fp32 value (bits of `.to(torch.bfloat16)`); the column sums run on integer-valued inputs, |v| <= 8,
where fp32 sums are exact in any order, and are compared as bits with an int64 reference (the idiom of tests/_gemm_exact.py): a
dropped, repeated or misrouted row is an integer difference.  A column sum gives one slot row to each run of 32 rows (the
chunk, MAE_SUM_ROWS in csrc/mae.hip; at most 512 runs, longer ones beyond 16384 rows): the shapes cross both.
Loss: against fp64 torch."""
import numpy as np
import pytest
import torch

import _mae_ref as Ref
from vit_core.ssl.mae import masking as Mk

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
CHUNK, MAX_SPLITS = 32, 512

# (B, N, K, D); the fifth has B * (N - K) = 1025 masked rows and 1075 rows of g (34 runs of 32), the last 16548 rows of g
# (more than 512 * 32: runs of 33 rows)
SHAPES = [(1, 4, 1, 64), (3, 9, 2, 64), (2, 196, 49, 192), (5, 16, 15, 128), (25, 42, 1, 64)]
SUM_SHAPES = SHAPES + [(84, 196, 49, 64)]


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def tables(B, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    keep, restore = Mk.draw_keep(B, N, K, generator=g)
    return keep, restore, keep.to(I32).to(DEV), restore.to(I32).to(DEV)


def ints(shape, seed, hi=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-hi, hi + 1, shape, generator=g).to(F32)


@pytest.mark.parametrize("B,N,K,D", SHAPES, ids=str)
def test_forwards_are_bit_equal(B, N, K, D):
    from vitssl_hip import ops
    torch.manual_seed(B * 1000 + N)
    keep, restore, keep_d, restore_d = tables(B, N, K, 1)
    xk, pos, cls = torch.randn(B * K, D, device=DEV), torch.randn(N + 1, D, device=DEV), torch.randn(D, device=DEV)
    out = torch.full((B * (K + 1), D), float("nan"), device=DEV)
    ops.mae_tokens_fwd(xk, keep_d, pos, cls, out, B, N, K)
    want = torch.cat([(cls + pos[0]).expand(B, 1, D), xk.view(B, K, D) + pos[1 + keep.to(DEV)]], dim=1)
    assert torch.equal(bits(out), bits(want.reshape(B * (K + 1), D)))

    y, mt, dpos = torch.randn(B * (K + 1), D, device=DEV), torch.randn(D, device=DEV), torch.randn(N + 1, D, device=DEV)
    out = torch.full((B * (N + 1), D), float("nan"), device=DEV)
    ops.mae_unshuffle_fwd(y, restore_d, mt, dpos, out, B, N, K)
    y3 = y.view(B, K + 1, D)
    full = torch.cat([y3[:, 1:], mt.expand(B, N - K, D)], dim=1)                 # the paper's un-shuffle: gather with ids_restore
    full = torch.gather(full, 1, restore.to(DEV)[:, :, None].expand(B, N, D))
    want = torch.cat([y3[:, :1], full], dim=1) + dpos
    assert torch.equal(bits(out), bits(want.reshape(B * (N + 1), D)))


# every shape into zeroed slots; two of them again into slots that already hold something (the "+=" of the header)
@pytest.mark.parametrize("B,N,K,D,nonzero", [s + (False,) for s in SUM_SHAPES] + [SHAPES[1] + (True,), SHAPES[4] + (True,)], ids=str)
def test_backwards_bf16_rows_and_exact_column_sums(B, N, K, D, nonzero):
    from vitssl_hip import ops
    keep, restore, keep_d, restore_d = tables(B, N, K, 2)
    assert 8 * B * (N + 1) + 64 < (1 << 24)                                      # the sums are exact in fp32
    # token assembly
    g = ints((B * (K + 1), D), 3)
    s0 = [ints((D,), 4 + i, 64) if nonzero else torch.zeros(D) for i in range(2)]
    dproj = torch.full((B * K, D), float("nan"), dtype=BF16, device=DEV)
    dbias, dcls = s0[0].to(DEV), s0[1].to(DEV)
    # rounding is visible: the bf16 rows are checked on non-integer values too
    frac = g + torch.rand(g.shape, generator=torch.Generator().manual_seed(9)) if not nonzero else g
    if not nonzero:
        d2 = torch.full_like(dproj, float("nan"))
        ops.mae_tokens_bwd(frac.to(DEV), d2, torch.zeros(D, device=DEV), torch.zeros(D, device=DEV), B, N, K)
        assert torch.equal(bits(d2), bits(frac.view(B, K + 1, D)[:, 1:].reshape(B * K, D).to(BF16).to(DEV)))
    ops.mae_tokens_bwd(g.to(DEV), dproj, dbias, dcls, B, N, K)
    g3 = g.view(B, K + 1, D)
    assert torch.equal(bits(dproj), bits(g3[:, 1:].reshape(B * K, D).to(BF16).to(DEV)))
    want_bias = g3[:, 1:].to(torch.int64).sum((0, 1)) + s0[0].to(torch.int64)
    want_cls = g3[:, 0].to(torch.int64).sum(0) + s0[1].to(torch.int64)
    assert torch.equal(bits(dbias.cpu()), bits(want_bias.to(F32))) and torch.equal(bits(dcls.cpu()), bits(want_cls.to(F32)))
    # un-shuffle
    g = ints((B * (N + 1), D), 5)
    dy = torch.full((B * (K + 1), D), float("nan"), dtype=BF16, device=DEV)
    dbias, dmt = s0[0].to(DEV), s0[1].to(DEV)
    ops.mae_unshuffle_bwd(g.to(DEV), restore_d, dy, dbias, dmt, B, N, K)
    g3 = g.view(B, N + 1, D)
    rows = torch.cat([g3[:, :1], torch.gather(g3[:, 1:], 1, keep[:, :, None].expand(B, K, D))], dim=1)      # (b, 0), then g[b, 1 + keep[b, j]]
    assert torch.equal(bits(dy), bits(rows.reshape(B * (K + 1), D).to(BF16).to(DEV)))
    masked = (restore >= K)
    want_bias = rows.to(torch.int64).sum((0, 1)) + s0[0].to(torch.int64)
    want_mt = g3[:, 1:][masked].to(torch.int64).sum(0) + s0[1].to(torch.int64)
    assert int(masked.sum()) == B * (N - K)
    assert torch.equal(bits(dbias.cpu()), bits(want_bias.to(F32))) and torch.equal(bits(dmt.cpu()), bits(want_mt.to(F32)))


def test_the_sum_shapes_cross_the_chunk_and_the_split_cap():
    rows = lambda B, N, K: (B * (K + 1), B * (N + 1))       # noqa: E731
    assert 25 * (42 - 1) == 1025 and rows(25, 42, 1)[1] == 1075 > CHUNK * 33
    assert rows(84, 196, 49)[1] > CHUNK * MAX_SPLITS and rows(1, 4, 1)[0] < CHUNK


@pytest.mark.parametrize("B,N,K,D", SHAPES[:4], ids=str)
def test_rows_by_index(B, N, K, D):
    from vitssl_hip import ops
    keep, restore, _, _ = tables(B, N, K, 6)
    idx = Mk.MAEIndices(keep, restore, K)
    src = torch.randn(B * N, D, device=DEV)
    kr = torch.from_numpy(idx.keep_rows).to(DEV)
    out = torch.full((B * K, D), float("nan"), dtype=BF16, device=DEV)
    ops.mae_gather_rows_bf16(src.to(BF16), kr, out)
    assert torch.equal(bits(out), bits(src.to(BF16)[kr.long()]))
    tok = torch.randn(B * (N + 1), D, device=DEV)
    mrows, inv = torch.from_numpy(idx.mrows).to(DEV), torch.from_numpy(idx.inv).to(DEV)
    sel = torch.full((idx.Mm, D), float("nan"), device=DEV)
    ops.mae_gather_rows_f32(tok, mrows, sel)
    assert torch.equal(bits(sel), bits(tok[mrows.long()]))
    back = torch.full((B * (N + 1), D), float("nan"), device=DEV)
    ops.mae_scatter_rows_f32(sel, inv, back)
    want = torch.zeros_like(tok)
    want[mrows.long()] = tok[mrows.long()]
    assert torch.equal(bits(back), bits(want))


# ---- loss -------------------------------------------------------------------------------------------------------------------------
def ulp_bf16(x):
    """spacing of bf16 at |x| (8 significant bits; subnormals do not occur here)"""
    return torch.where(x == 0, torch.zeros_like(x), torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-38))) - 7))


@pytest.mark.parametrize("norm_pix", [True, False], ids=["norm_pix", "raw"])
@pytest.mark.parametrize("Mm,Pd,ld,Pdp", [(1, 2, 2, 64), (7, 192, 192, 192), (33, 588, 592, 640), (130, 768, 768, 768), (3, 9, 12, 64), (2, 4100, 4100, 4160)],
                         ids=str)
def test_loss_against_fp64(Mm, Pd, ld, Pdp, norm_pix):
    from vitssl_hip import ops
    g = torch.Generator().manual_seed(Mm * 7 + Pd)
    pred = torch.randn(Mm, Pd, generator=g)
    raw = torch.rand(Mm, Pd, generator=g) * 255.0 if Pd != 192 else torch.rand(Mm, Pd, generator=g)
    if Mm > 2:
        raw[1] = 0.75                                                            # a constant row: var = 0
    gscale = 1.0 / Mm
    wide = torch.full((Mm, ld), float("nan"))
    wide[:, :Pd] = pred
    # fp64 reference
    t64 = Ref.normalise(raw.double()) if norm_pix else raw.double()
    d64 = pred.double() - t64
    want_loss = float((d64 ** 2).mean(dim=-1).sum())
    want_dp = (2.0 * d64 * gscale / Pd)
    runs = []
    for _ in range(2):
        pd_, tgt = wide.to(DEV)[:, :Pd], raw.to(DEV)
        loss = torch.zeros(1, device=DEV)
        dp = torch.full((Mm, Pdp), float("nan"), dtype=BF16, device=DEV)
        ops.mae_loss(pd_, tgt, loss, dp, gscale=gscale, norm_pix=norm_pix)
        runs.append((loss.cpu(), dp.cpu(), tgt.cpu()))
    (loss, dp, tgt), again = runs
    for a, b in zip(runs[0], again):
        assert torch.equal(bits(a) if a.dtype != BF16 else a.view(torch.int16), bits(b) if b.dtype != BF16 else b.view(torch.int16))
    assert torch.isfinite(tgt).all() and torch.isfinite(dp.float()).all() and torch.isfinite(loss).all()
    # targets: within 1 fp32 ulp of the rounded fp64 value (raw: untouched)
    t32 = t64.float()
    if norm_pix:
        lo, hi = torch.nextafter(t32, torch.full_like(t32, -float("inf"))), torch.nextafter(t32, torch.full_like(t32, float("inf")))
        assert bool(((tgt >= lo) & (tgt <= hi)).all()), float((tgt - t32).abs().max())
        if Mm > 2:
            assert not tgt[1].any()
    else:
        assert torch.equal(bits(tgt), bits(raw))
    print(f"loss {float(loss)} fp64 {want_loss} rel {abs(float(loss) - want_loss) / want_loss:.3e}")
    assert abs(float(loss) - want_loss) <= 1e-6 * want_loss
    # gradient: within 1 bf16 ulp of the rounded fp64 value; pad columns exactly zero
    ref = want_dp.float().to(BF16).float()
    got = dp[:, :Pd].float()
    err = (got - ref).abs()
    assert bool((err <= torch.maximum(ulp_bf16(ref), ulp_bf16(got))).all()), float(err.max())
    assert not dp[:, Pd:].view(torch.int16).any()
    # loss only (no gradient): the same loss bits
    loss2 = torch.zeros(1, device=DEV)
    ops.mae_loss(wide.to(DEV)[:, :Pd], raw.to(DEV), loss2, None, norm_pix=norm_pix)
    assert torch.equal(bits(loss2.cpu()), bits(loss))


def test_loss_accumulates_and_refuses_one_column_normalisation():
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    pred, tgt = torch.randn(5, 64, device=DEV), torch.randn(5, 64, device=DEV)
    a, b = torch.zeros(1, device=DEV), torch.full((1,), 3.0, device=DEV)
    ops.mae_loss(pred, tgt.clone(), a, None, norm_pix=False)
    ops.mae_loss(pred, tgt.clone(), b, None, norm_pix=False)
    assert abs(float(b) - 3.0 - float(a)) < 1e-5 * float(a)
    with pytest.raises(L.VitsslError, match="norm_pix"):
        ops.mae_loss(torch.randn(4, 1, device=DEV), torch.randn(4, 1, device=DEV), a, None, norm_pix=True)
    ops.mae_loss(torch.randn(4, 1, device=DEV), torch.randn(4, 1, device=DEV), a, None, norm_pix=False)
    assert np.isfinite(float(a))
