"""fp64 restatements of what include/vitssl_mixup.h promises -- the mix kernel and the loss against two-label targets -- and
the seeded inputs of their tests.  NumPy only: the CPU test holds the loss against torch's own F.cross_entropy with
probability targets in fp64, the GPU tests hold the kernels against both."""
import numpy as np

import _classify_ref as R

IGNORE = R.IGNORE
COPY, BLEND, PASTE = 0, 1, 2
LAMS = np.array([0.0, 2.0 ** -20, 0.3, 0.5, 1.0 - 2.0 ** -20, 1.0], dtype=np.float32)
LOSS_SHAPES = R.SHAPES[:4]                                                   # (B, C, ld)
MIX_SHAPES = [(1, 3, 8, 8), (5, 3, 32, 32), (4, 1, 7, 30), (3, 4, 9, 5), (2, 3, 224, 224)]      # (B, C, H, W)


# ---------------------------------------------------------------------------------------------- the mix kernel
def sanitise(iparams, B, H, W):
    """The table as the kernel reads it: unknown kinds copy, a partner outside the batch is the row itself, boxes are clamped."""
    ip = np.asarray(iparams, dtype=np.int64).copy()
    ip[:, 0] = np.where((ip[:, 0] == BLEND) | (ip[:, 0] == PASTE), ip[:, 0], COPY)
    ip[:, 1] = np.where((ip[:, 1] < 0) | (ip[:, 1] >= B), np.arange(B), ip[:, 1])
    ip[:, 2], ip[:, 3] = np.maximum(ip[:, 2], 0), np.minimum(ip[:, 3], H)
    ip[:, 4], ip[:, 5] = np.maximum(ip[:, 4], 0), np.minimum(ip[:, 5], W)
    return ip


def mix_reference(x, iparams, lam):
    """-> (out fp64 [B,C,H,W], bound fp64 [B,C,H,W]).  Copy and paste rows are exact (bound 0: compare the bits); a blend row
    is lam a + (1 - lam) b in fp64 from the float32 lam, with the bound 2^-22 max(|a|, |b|) of its three fp32 roundings."""
    x = np.asarray(x)
    B, _, H, W = x.shape
    ip = sanitise(iparams, B, H, W)
    out = x.astype(np.float64)
    bound = np.zeros(x.shape)
    for i, (kind, p, y0, y1, x0, x1) in enumerate(ip.tolist()):
        a, b = x[i].astype(np.float64), x[p].astype(np.float64)
        if kind == BLEND:
            l = float(np.float32(lam[i]))
            out[i] = l * a + (1.0 - l) * b
            bound[i] = 2.0 ** -22 * np.maximum(np.abs(a), np.abs(b))
        elif kind == PASTE and y1 > y0 and x1 > x0:
            out[i, :, y0:y1, x0:x1] = b[:, y0:y1, x0:x1]
    return out, bound


def boxes(H, W):
    """(y0, y1, x0, x1) of the cases a paste must survive: empty, one pixel, the full image, touching each of the four edges,
    x0 % 4 in {1, 2, 3}, x1 - x0 < 4 (where the image is wide enough to tell them apart)."""
    h2, w2 = max(H // 2, 1), max(W // 2, 1)
    out = [(2, 2, 1, 3), (H - 1, H, W - 1, W), (0, H, 0, W), (0, h2, 1, W - 1), (h2, H, 1, W - 1), (1, H - 1, 0, w2),
           (1, H - 1, w2, W)]
    for x0 in (1, 2, 3):
        out.append((1, H, x0, W))
        out.append((0, H - 1, x0, min(x0 + 3, W)))
    out.append((0, 1, W - 2, W))
    return [(max(a, 0), max(b, 0), max(c, 0), max(d, 0)) for a, b, c, d in out]


def mix_tables(B, H, W, seed=0):
    """A list of (iparams int32 [B,6], lam f32 [B]): every batch mixes the three kinds (B >= 3; a smaller batch takes turns),
    the partner of row i is B-1-i (the middle row of an odd batch is its own partner), and the paste rows walk through
    `boxes` until each has been pasted once."""
    g = np.random.default_rng(1000 + seed + 31 * B + H * W)
    bx = boxes(H, W)
    tables, nb, t = [], 0, 0
    while nb < len(bx):
        ip = np.zeros((B, 6), np.int32)
        ip[:, 1] = B - 1 - np.arange(B)
        ip[:, 0] = (np.arange(B) + t) % 3
        for i in range(B):
            if ip[i, 0] == PASTE:
                ip[i, 2:] = bx[nb % len(bx)]
                nb += 1
            else:                                                            # the box columns of other kinds are not read
                ip[i, 2:] = g.integers(-5, 50, 4)
        lam = g.choice(LAMS[:5], B).astype(np.float32)                       # never a blend with lam == 1
        tables.append((ip, lam))
        t += 1
    return tables


def mix_input(B, C, H, W, seed=0):
    g = np.random.default_rng(77 + seed + B * C * H * W)
    return (g.standard_normal((B, C, H, W)) * np.exp(2.0 * g.standard_normal((B, C, H, 1)))).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the loss
def row_states(y, partner, lam, B, C, ignore_index=IGNORE):
    """-> (valid, bad, a, b): the rule of vitssl_classify_loss_mix.  Nothing is indexed through a bad partner."""
    y, partner = np.asarray(y), np.asarray(partner)
    lam = np.asarray(lam, dtype=np.float32)
    pok = (partner >= 0) & (partner < B)
    a = y
    b = np.where(pok, y[np.where(pok, partner, 0)], ignore_index)
    out = lambda l: (l != ignore_index) & ((l < 0) | (l >= C))
    with np.errstate(invalid="ignore"):
        lam_ok = (lam >= 0) & (lam <= 1)
    bad = ~pok | ~lam_ok | out(a) | out(b)
    valid = ~bad & (a != ignore_index) & (b != ignore_index)
    return valid, bad, a, b


def loss_reference(z, y, partner, lam, C, eps, ignore_index=IGNORE, upstream=1.0):
    """-> dict(loss_sum, n_valid, n_bad, loss, grad [B, C], dbias [C], pred [B], correct, valid [B]) in fp64.  A row with
    a == b, lam == 1 or lam == 0 is the one-label row of tests/_classify_ref.reference, statement for statement; in a
    two-label row 1 - t[y] - p[y] is summed from the other columns for both labels."""
    z = np.asarray(z)[:, :C].astype(np.float64)
    B = z.shape[0]
    valid, bad, a, b = row_states(y, partner, lam, B, C, ignore_index)
    l = np.asarray(lam, dtype=np.float32).astype(np.float64)
    n = int(valid.sum())
    rows = np.arange(B)
    one = valid & ((a == b) | (l == 1.0) | (l == 0.0))
    two = valid & ~one
    ya = np.where(valid, np.where(one & (l == 0.0) & (a != b), b, a), 0)     # the one label of a one-label row, a of a two-label one
    yb = np.where(two, b, 0)
    wa, wb = np.where(two, l, 1.0), np.where(two, 1.0 - l, 0.0)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1)
    lse = m[:, 0] + np.log(s)
    row = (1.0 - eps) * (wa * (lse - z[rows, ya]) + wb * (lse - z[rows, yb])) + eps * (lse - z.mean(1))
    loss_sum = float(row[valid].sum())
    others = e.copy()
    others[rows, ya] = 0.0
    others[two, yb[two]] = 0.0
    so = others.sum(1)
    grad = e / s[:, None] - eps / C
    k = eps * (1.0 - 1.0 / C)
    grad[rows, ya] = np.where(two, (wb * (1.0 - eps) + k) - (so + e[rows, yb]) / s, k - so / s)
    grad[two, yb[two]] = ((wa * (1.0 - eps) + k) - (so + e[rows, ya]) / s)[two]
    grad[~valid] = 0.0
    if n:
        grad *= upstream / n
    pred = z.argmax(1)
    return dict(loss_sum=loss_sum, n_valid=n, n_bad=int(bad.sum()), loss=loss_sum / n if n else float("nan"), grad=grad,
                dbias=grad.sum(0), pred=pred, correct=int((pred[valid] == np.asarray(y)[valid]).sum()), valid=valid)


def soft_targets(y, partner, lam, C):
    """lam onehot(a) + (1 - lam) onehot(b) of the valid rows, fp64 [n_valid, C], and the mask of those rows."""
    B = len(y)
    valid, _, a, b = row_states(y, partner, lam, B, C)
    l = np.asarray(lam, dtype=np.float32).astype(np.float64)[valid]
    t = np.zeros((int(valid.sum()), C))
    r = np.arange(t.shape[0])
    np.add.at(t, (r, a[valid]), l)
    np.add.at(t, (r, b[valid]), 1.0 - l)
    return t, valid


def make_loss_case(B, C, ld, rot=0, seed=1234, all_ignored=False):
    """The logits and labels of _classify_ref.make_case (the tie row, the +-80 row, NaN padding, every third row's own label
    ignored) with partner int32 [B] and lam f32 [B]: partners are drawn freely in [0, B) -- so some partner labels are
    ignored -- lam walks through LAMS from `rot`, and (B >= 3) the tie row mixes the labels of its two largest logits, row 2
    is its own partner (a == b), row 3 mixes with the ignored row 1 and the last row mixes with row 0."""
    z, y, tie = R.make_case(B, C, ld, seed=seed, all_ignored=all_ignored)
    g = np.random.default_rng(seed + 13 * B + C + 1)
    partner = g.integers(0, B, B).astype(np.int32)
    lam = LAMS[(np.arange(B) + rot + 2) % len(LAMS)].copy()                     # rot = 0: the tie row at 0.3
    if B >= 3 and not all_ignored:                                           # rows 0 and 2 are never ignored (1, 4, 7, ... are)
        partner[0], y[0], y[2] = 2, tie[0], tie[1]                           # the tie row: a two-label row on its two largest logits
        partner[2] = 2                                                       # a == b
        partner[B - 1] = 0                                                   # the +-80 row, mixed with a valid label
        if B >= 5:
            partner[3] = 1                                                   # a valid row whose partner's label is ignored
    return z, y, partner, lam, tie
