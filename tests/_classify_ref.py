"""fp64 restatement of what include/vitssl_classify.h promises, and the seeded inputs of its tests.  NumPy only: the CPU test
holds it against torch's own F.cross_entropy in fp64, the GPU tests hold the kernel against it."""
import numpy as np

IGNORE = -100
SHAPES = [(1, 2, 64), (33, 10, 64), (7, 1000, 1024), (5, 1027, 1088), (3, 65536, 65536)]      # (B, C, ld)


def make_case(B, C, ld, seed=1234, all_ignored=False):
    """logits f32 [B, ld] ~ N(0, 4) in the C valid columns and NaN behind them (a read of the padding poisons the result),
    labels i64 [B].  Row 0 carries an exact tie of its two largest values; the last row (B >= 3) is of magnitude +-80;
    every third row from row 1 on is ignored.  B == 1: the one row is the tie, at 80."""
    g = np.random.default_rng(seed + 7919 * B + C)
    z = np.full((B, ld), np.nan, dtype=np.float32)
    z[:, :C] = (2.0 * g.standard_normal((B, C))).astype(np.float32)
    j1, j2 = sorted(g.choice(C, size=2, replace=False).tolist())
    top = np.float32(80.0) if B == 1 else np.float32(z[0, :C].max() + 1.0)
    z[0, j1] = z[0, j2] = top
    if B >= 3:
        z[B - 1, :C] = np.where(g.random(C) < 0.5, -80.0, 80.0).astype(np.float32)
        z[B - 1, g.integers(C)] = 80.0
    y = g.integers(0, C, size=B).astype(np.int64)
    y[1::3] = IGNORE
    if all_ignored:
        y[:] = IGNORE
    return z, y, (j1, j2)


def reference(z, y, C, eps, ignore_index=IGNORE, upstream=1.0):
    """-> dict(loss_sum, n_valid, loss (nan when n_valid == 0), grad [B, C], dbias [C], pred [B], correct), all fp64 / exact.
    Rows whose label is ignore_index or outside [0, C) contribute nothing.  1 - p[y] is summed from the other columns."""
    z = np.asarray(z)[:, :C].astype(np.float64)
    y = np.asarray(y)
    B = z.shape[0]
    valid = (y != ignore_index) & (y >= 0) & (y < C)
    n = int(valid.sum())
    rows = np.arange(B)
    yy = np.where(valid, y, 0)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1)
    lse = m[:, 0] + np.log(s)
    row = (1.0 - eps) * (lse - z[rows, yy]) + eps * (lse - z.mean(1))
    loss_sum = float(row[valid].sum())
    others = e.copy()
    others[rows, yy] = 0.0
    grad = e / s[:, None] - eps / C
    grad[rows, yy] = eps * (1.0 - 1.0 / C) - others.sum(1) / s
    grad[~valid] = 0.0
    if n:
        grad *= upstream / n
    pred = z.argmax(1)
    return dict(loss_sum=loss_sum, n_valid=n, loss=loss_sum / n if n else float("nan"), grad=grad, dbias=grad.sum(0), pred=pred,
                correct=int((pred[valid] == y[valid]).sum()))
