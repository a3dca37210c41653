"""fp64 restatement of what include/vitssl_bce.h promises (timm's BinaryCrossEntropy with ignore_index), the seeded inputs of its
tests and the checker the GPU tests hold the kernel to.  NumPy only in the restatement: the CPU test holds it against torch's
own binary_cross_entropy_with_logits in fp64 on explicit dense targets, and shows that the checker refuses wrong gradients."""
import math

import numpy as np

import _classify_ref as R
import _mixup_ref as M

IGNORE = R.IGNORE
SHAPES = R.SHAPES                                                            # (B, C, ld)
COUNTERS0, BAD0 = (5, 9), 3                                                  # what the accumulated outputs hold before the call


def dbias0(C, sum_classes=False):
    """What the bias gradient is accumulated onto: 2^-6 (the start of tests/test_gpu_classify.py) on the scale of this loss's
    gradient, whose elements carry the 1 / C of the mean over the classes -- 7.6e-6 / n_valid at C = 65536, where the fp32
    addition onto 2^-6 itself (half an ulp, 9e-10) would be 1e-4 of the addend and the bar of 1e-5 would measure that rounding,
    not the kernel.  C is rounded up to a power of two, so that the start is an fp32 number and taking it off again is exact."""
    return 2.0 ** -6 if sum_classes else 2.0 ** (-6 - math.ceil(math.log2(C)))


def _ordinary(z, tie, B):
    """B == 1: _classify_ref.make_case puts the one row's tie at 80, where a sigmoid loss is either about 0 or about 80 per
    class; logits of ordinary size keep the tie and give a loss a relative bar means something against."""
    if B == 1:
        z[0, list(tie)] = np.float32(1.5)
    return z


def make_case(B, C, ld, seed=1234, all_ignored=False):
    """_classify_ref.make_case: NaN behind column C, a tied row, a +-80 row, every third row ignored -> (z, y, tie)"""
    z, y, tie = R.make_case(B, C, ld, seed=seed, all_ignored=all_ignored)
    return _ordinary(z, tie, B), y, tie


def make_mix_case(B, C, ld, rot=0, seed=1234, all_ignored=False):
    """_mixup_ref.make_loss_case: the same logits with partner / lam tables -> (z, y, partner, lam, tie)"""
    z, y, partner, lam, tie = M.make_loss_case(B, C, ld, rot=rot, seed=seed, all_ignored=all_ignored)
    return _ordinary(z, tie, B), y, partner, lam, tie


def row_states(y, partner, lam, B, C, ignore_index=IGNORE):
    """-> (valid, bad, a, b, l): the rows of vitssl_classify_loss (no tables: b = a, l = 1) or of vitssl_classify_loss_mix"""
    y = np.asarray(y)
    if partner is None:
        bad = (y != ignore_index) & ((y < 0) | (y >= C))
        return (y != ignore_index) & ~bad, bad, y, y, np.ones(B)
    valid, bad, a, b = M.row_states(y, partner, lam, B, C, ignore_index)
    return valid, bad, a, b, np.asarray(lam, dtype=np.float32).astype(np.float64)


def targets(y, partner, lam, C, eps, threshold=None, ignore_index=IGNORE):
    """-> (t fp64 [B, C], soft fp64 [B, C], valid [B], bad [B]); rows that are not valid hold zeros.  soft is
    l s(a) + (1 - l) s(b) with s(y) = (1 - eps) onehot(y) + eps / C, t is soft or (soft > threshold)."""
    B = len(y)
    valid, bad, a, b, l = row_states(y, partner, lam, B, C, ignore_index)
    rows = np.arange(B)

    def s(lab):
        out = np.full((B, C), eps / C)
        out[rows, np.where(valid, lab, 0)] += 1.0 - eps
        return out

    l = np.where(valid, l, 1.0)[:, None]
    soft = l * s(a) + (1.0 - l) * s(b)
    soft[~valid] = 0.0
    t = soft if threshold is None else (soft > threshold).astype(np.float64)
    t[~valid] = 0.0
    return t, soft, valid, bad


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def reference(z, y, C, eps, partner=None, lam=None, threshold=None, sum_classes=False, ignore_index=IGNORE, upstream=1.0):
    """-> dict(loss_sum, n_valid, n_bad, loss (nan when n_valid == 0), grad [B, C], dbias [C], pred [B], correct, valid [B],
    t [B, C], soft [B, C]), all fp64 / exact."""
    z = np.asarray(z)[:, :C].astype(np.float64)
    t, soft, valid, bad = targets(y, partner, lam, C, eps, threshold, ignore_index)
    n = int(valid.sum())
    div = 1.0 if sum_classes else float(C)
    with np.errstate(invalid="ignore"):
        e = np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z)))
        d = np.where(t == 1.0, -sigmoid(-z), sigmoid(z) - t)
    row = e.sum(1) / div
    loss_sum = float(row[valid].sum())
    grad = d.copy()
    grad[~valid] = 0.0
    if n:
        grad *= upstream / (n * div)
    with np.errstate(invalid="ignore"):
        pred = z.argmax(1)
    return dict(loss_sum=loss_sum, n_valid=n, n_bad=int(bad.sum()), loss=loss_sum / n if n else float("nan"), grad=grad,
                dbias=grad.sum(0), pred=pred, correct=int((pred[valid] == np.asarray(y)[valid]).sum()), valid=valid, t=t, soft=soft)


# ---------------------------------------------------------------------------------------------- the checker
def check_loss(ref, loss_out, t32, what=""):
    """The loss bar of tests/test_gpu_classify.py: |kernel - fp64| / |fp64| <= max(4 x the same distance of torch's fp32 CPU
    result `t32`, 1e-6); both distances are printed.  loss_out: the two floats the kernel wrote."""
    assert float(loss_out[1]) == ref["n_valid"]
    if ref["n_valid"] == 0:
        assert float(loss_out[0]) == 0.0 and math.isnan(float(loss_out[0]) / float(loss_out[1]) if float(loss_out[1]) else float("nan"))
        return
    mine = float(loss_out[0]) / float(loss_out[1])
    d_torch, d_mine = abs(t32 - ref["loss"]) / abs(ref["loss"]), abs(mine - ref["loss"]) / abs(ref["loss"])
    print(f"bce loss {what}: fp64 {ref['loss']:.12g}  torch fp32 cpu rel {d_torch:.3g}  kernel rel {d_mine:.3g}")
    assert d_mine <= max(4 * d_torch, 1e-6), (d_mine, d_torch)


def check_grad(ref, g, C):
    """g: the bf16 dlogits as fp64 [B, ld_out].  Every element within max(2^-8 |ref|, 2^-126) of the bf16-rounded fp64 value (one
    bf16 ulp; the floor because sigmoid(-80) / (n C) lies below bf16's smallest normal); padding and ignored rows exactly 0."""
    import torch
    want = torch.from_numpy(ref["grad"]).to(torch.bfloat16).double().numpy()
    assert not np.isnan(g).any()
    err, bar = np.abs(g[:, :C] - want), np.maximum(2.0 ** -8 * np.abs(ref["grad"]), 2.0 ** -126)
    assert (err <= bar).all(), f"gradient: {int((err > bar).sum())} elements over the bar, first at {np.argwhere(err > bar)[0]}"
    assert not g[:, C:].any()
    assert not g[~ref["valid"]].any()


def check_dbias(ref, dbias, start):
    db = np.asarray(dbias, dtype=np.float64) - start                         # accumulated onto what was there (dbias0)
    if ref["n_valid"]:
        assert np.linalg.norm(db - ref["dbias"]) <= 1e-5 * np.linalg.norm(ref["dbias"])
    else:
        assert not db.any()
