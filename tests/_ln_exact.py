"""LayerNorm family (csrc/layernorm.hip): host-only case builders, references and fp32 restatements (no GPU code).

Part 1, exact backward cases.  The backward takes `mean` and `rstd` as inputs, so a case can be planted in which every intermediate
of the kernel's formula is an integer or a dyadic fraction far below 2^24: any summation order, any FMA contraction and any slot
layout give the same bits, and every output element, column sums included, is compared for equality.  Per row
    xh in {+-1} with some octets replaced by {2, -2, 0 x 6}, shuffled: sum xh = 0, sum xh^2 = cols
    rstd = 2^-k (k in 0..2), mean an integer in -8..8, x = mean + xh / rstd: the true statistics of the row at eps = 0
    gamma in {+-0.5, +-1, +-2};  dy * gamma = b + m1 + m2 * xh with b even, antisymmetric over pairs of columns of equal xh
    (sum b = sum b xh = 0) and m1, m2 even in +-{2, 4}: dy is an integer, |dy| <= 32, and sum dy gamma = cols m1,
    sum dy gamma xh = cols m2, so the input gradient is b * rstd, a multiple of 0.5 with |.| <= 4
    g_res integers in -3..3: g_out = b rstd + g_res has at most four significant bits and so has every product of it with the
    dropout scale 2 (p = 0.5), a row scale from {0, 0.5, 1, 2}, a LayerScale gamma from {+-0.25, +-1, +-2} and a power-of-two
    qscale: the bf16 and e4m3 images are exact, not rounded.
The kernel forms wave_sum(s) * (1.0f / cols); that is the planned integer only where fl(fl(1 / cols) * cols * k) == k, which
`check_width` asserts for |k| <= 256 (true for every width the tests use; false for 28, 52, 56, ...).
`expected` is the reference: fp64 autograd through torch.nn.functional.layer_norm(eps = 0) for g_out, dgamma, dbeta, plain fp64
arithmetic for the rest; it asserts that every value is representable in its output type.  `restate` is the kernel's formula in
fp32 NumPy with the launch's block / slot-row layout, a column order and optional FMA-style products, and the planted faults of
FAULTS: tests/test_ln_exact_host.py proves on the CPU that the restatement gives the reference bits and that every fault moves them.

Part 2, real-valued rows (`family_rows`) with per-row error bounds derived from the standard any-order summation bound
gamma_n = n u / (1 - n u), u = 2^-24, propagated through the two-pass forward and the backward formula (`fwd_bounds`, `bwd_ref`),
and three wrong restatements of the forward (`fwd_restate`) that the bounds must reject."""
import numpy as np
import torch

from _gemm_exact import BF16, F32, FP8, bf16_rne, to_f32_exact, to_fp8
from test_dropout_stream import keep_mask

F64 = torch.float64
U = 2.0 ** -24                       # unit roundoff of fp32
LN_THREADS_ROWS = 4                  # rows (PAIR: row pairs) in flight per block: one per wave
WIDTHS = (4, 8, 64, 256, 260, 384, 512, 516, 768, 772, 1024, 1028, 1280, 2048)
FULL_WIDTHS = (64, 384, 772, 1280)   # the full form x option matrix runs here
FORMS = ("ln", "ln_fp8", "ln_rows", "ln_ls", "gmc", "gmc_fp8", "gmc_rows", "gmc_ls")
DROP_P, DROP_SEED, DROP_SITE = 0.5, 4242, 5
QSCALE, AMAX0 = 2.0, 0.25


def gamma_n(n):
    return n * U / (1.0 - n * U)


def check_width(cols, kmax=256):
    """the kernel's `sum * (1.0f / cols)` returns the planned integer k for every |k| <= kmax"""
    inv = np.float32(1.0) / np.float32(cols)
    k = np.arange(-kmax, kmax + 1, dtype=np.float32)
    got = (k * np.float32(cols)) * inv
    assert np.array_equal(got, k), f"width {cols}: fl(fl(1/cols) * cols * k) != k for k = {k[got != k][:4]}: no exact case at this width"


# =============================================================================================== part 1: the planted cases
class Case:
    """one planted backward problem with every optional operand; `opts` decide which of them a launch receives"""


def _pick(table, shape, g):
    t = torch.tensor(table, dtype=F64)
    return t[torch.randint(0, len(table), shape, generator=g)]


def build_case(rows, cols, seed=0):
    assert cols % 4 == 0 and cols >= 4
    check_width(cols)
    g = torch.Generator().manual_seed(1000 * cols + rows + seed)
    c = Case()
    c.rows, c.cols = rows, cols
    # ---- xh: balanced +-1, some octets {2, -2, 0 x 6}; shuffled per row
    n_oct = cols // 32 if cols >= 16 else 0
    base = [2.0, -2.0] * n_oct + [0.0] * (6 * n_oct)
    rest = cols - 8 * n_oct
    base += [1.0] * (rest // 2) + [-1.0] * (rest // 2)
    base = torch.tensor(base, dtype=F64)
    xh = torch.stack([base[torch.randperm(cols, generator=g)] for _ in range(rows)])
    assert bool((xh.sum(1) == 0).all()) and bool(((xh * xh).sum(1) == cols).all())
    # ---- statistics: every row differs from both neighbours in mean and in rstd
    k = torch.zeros(rows, dtype=torch.int64)
    mean = torch.zeros(rows, dtype=F64)
    for r in range(rows):
        k[r] = (int(k[r - 1]) + 1 + int(torch.randint(0, 2, (1,), generator=g))) % 3 if r else int(torch.randint(0, 3, (1,), generator=g))
        m = int(torch.randint(-8, 9, (1,), generator=g))
        while r and m == int(mean[r - 1]):
            m = int(torch.randint(-8, 9, (1,), generator=g))
        mean[r] = m
    rstd = 2.0 ** (-k.double())
    x = mean[:, None] + xh / rstd[:, None]
    gamma = _pick([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], (cols,), g)
    # ---- dy * gamma = b + m1 + m2 xh
    b = torch.zeros(rows, cols, dtype=F64)
    for r in range(rows):
        for v in (-2.0, -1.0, 0.0, 1.0, 2.0):
            idx = (xh[r] == v).nonzero().flatten()
            n2 = idx.numel() // 2
            if n2 == 0:
                continue
            val = _pick([-4.0, -2.0, 2.0, 4.0, 0.0], (n2,), g)
            b[r, idx[:n2]] = val
            b[r, idx[n2:2 * n2]] = -val
    m1 = _pick([-4.0, -2.0, 2.0, 4.0], (rows,), g)
    m2 = _pick([-4.0, -2.0, 2.0, 4.0], (rows,), g)
    for r in range(1, rows, 2):                      # a pair's two rows differ in m1 and in m2
        if m1[r] == m1[r - 1]:
            m1[r] = -m1[r]
        if m2[r] == m2[r - 1]:
            m2[r] = -m2[r]
    w = b + m1[:, None] + m2[:, None] * xh
    assert bool((b.sum(1) == 0).all()) and bool(((b * xh).sum(1) == 0).all())
    assert bool((w.sum(1) == cols * m1).all()) and bool(((w * xh).sum(1) == cols * m2).all())
    dy = w / gamma
    assert bool((dy == dy.round()).all()) and float(dy.abs().max()) <= 32
    c.xh, c.b, c.m1, c.m2 = xh, b, m1, m2
    c.x, c.mean, c.rstd, c.gamma = to_f32_exact(x), to_f32_exact(mean), to_f32_exact(rstd), to_f32_exact(gamma)
    c.dy = bf16_rne(dy)
    assert torch.equal(c.dy.double(), dy)
    c.g_res = torch.randint(-3, 4, (rows, cols), generator=g).to(F32)
    c.g = to_f32_exact(b * rstd[:, None] + c.g_res.double())          # input of the mask + cast forms: the LayerNorm form's g_out
    c.init = {n: torch.randint(-5, 6, (cols,), generator=g).to(F32) for n in ("dgamma", "dbeta", "cs", "dls")}
    c.keep = torch.from_numpy(keep_mask(rows, cols, DROP_P, DROP_SEED, DROP_SITE).astype(np.float64))
    assert 65536.0 / (65536 - round(DROP_P * 65536)) == 2.0
    # ---- row scales: one group per row (seven rows per group where 7 divides the count), zero and non-zero entries
    c.rpg = 7 if rows % 7 == 0 else 1
    groups = rows // c.rpg
    c.rowscale = torch.tensor([2.0, 0.0, 0.5, 1.0], dtype=F32)[(torch.arange(groups) + seed) % 4]
    c.lsgamma = to_f32_exact(_pick([0.25, -0.25, 1.0, -1.0, 2.0, -2.0], (cols,), g))
    c.branch = torch.randint(-4, 5, (rows, cols), generator=g).to(BF16)
    return c


def options(form, which="all"):
    """the option sets of a form: dicts over drop, cs, res (LayerNorm forms), gm, and for the LayerScale forms rows, dls.
    which = "all": everything on; "matrix": each option with and without, plus the gm = None launches."""
    ln, ls, q8 = form.startswith("ln"), form.endswith("_ls"), form.endswith("_fp8")
    full = dict(drop=True, cs=True, gm=True)
    if ln:
        full["res"] = True
    if ls:
        full.update(rows=True, dls=True)
    if which == "all":
        return [full]
    out = [full]
    for key in full:
        if key == "gm":
            continue
        out.append(dict(full, **{key: False}))
    out.append({k: (k == "gm") for k in full})                       # everything optional off
    if form == "ln":
        out.append(dict(full, gm=False, cs=False))                   # gm = None: no operand, no column sum of it
    if q8:
        out.append(dict(full, gm=False))                             # the e4m3 image alone
    return out


def opt_id(o):
    return "+".join(k for k, v in o.items() if v) or "bare"


def _row_scale(c):
    return c.rowscale.double().repeat_interleave(c.rpg)


def expected(c, form, o):
    """-> dict of the outputs the launch must produce, each in its output type and exactly representable there"""
    ln, ls, q8, rws = form.startswith("ln"), form.endswith("_ls"), form.endswith("_fp8"), form.endswith("_rows")
    out = {}
    if ln:
        x = c.x.double().requires_grad_(True)
        ga = c.gamma.double().requires_grad_(True)
        be = torch.zeros(c.cols, dtype=F64, requires_grad=True)
        y = torch.nn.functional.layer_norm(x, (c.cols,), ga, be, eps=0.0)
        (y * c.dy.double()).sum().backward()
        planned = c.b * c.rstd.double()[:, None]
        # torch's fp64 layer_norm carries its own rounding (1e-16, visible where the planted value is 0): the reference is the
        # autograd result on the grid of halves the construction lives on, and that is the planted closed form
        assert float((x.grad - planned).abs().max()) < 1e-9, "the planted input gradient is not the autograd result"
        assert torch.equal((x.grad * 2).round() / 2, planned)
        base = planned + (c.g_res.double() if o["res"] else 0.0)
        out["g_out"] = to_f32_exact(base)
        dgam, dbet = ga.grad.round(), be.grad.round()
        assert float((ga.grad - dgam).abs().max()) < 1e-9 and float((be.grad - dbet).abs().max()) < 1e-9
        assert torch.equal(dgam, (c.dy.double() * c.xh).sum(0)) and torch.equal(dbet, c.dy.double().sum(0))
        out["dgamma"] = to_f32_exact(c.init["dgamma"].double() + dgam)
        out["dbeta"] = to_f32_exact(c.init["dbeta"].double() + dbet)
    else:
        base = c.g.double()
    sc = _row_scale(c)[:, None] if (rws or (ls and o["rows"])) else torch.ones(c.rows, 1, dtype=F64)
    op = base * (c.keep * 2.0 if o["drop"] else 1.0) * sc
    if ls:
        op = op * c.lsgamma.double()
    if o["gm"]:
        out["gm"] = bf16_rne(op)
        assert torch.equal(out["gm"].double(), op)
    if q8:
        out["gm8"] = to_fp8(to_f32_exact(op * QSCALE))
        out["amax"] = to_f32_exact(torch.maximum(op.abs().max(), torch.tensor(AMAX0, dtype=F64)).reshape(1))
    if o["cs"]:
        out["cs"] = to_f32_exact(c.init["cs"].double() + op.sum(0))
    if ls and o["dls"]:
        out["dls"] = to_f32_exact(c.init["dls"].double() + (sc * base * c.branch.double()).sum(0))
    return out


# ----------------------------------------------------------------------------------------------- the launch's geometry
def launch_plan(form, rows, cols, cus):
    """launch_ln_bwd restated: -> (pair, grid).  `cus` = the CUs the library may occupy (vitssl_persistent_cus)."""
    pair = form in ("ln", "ln_rows", "ln_ls") and cols == 384 and rows % 2 == 0
    krows, kcols = (rows // 2, 768) if pair else (rows, cols)
    grid = min((krows + 3) // 4, cus * (2 if kcols <= 512 else 1))
    return pair, max(grid, 1)


def sweeps(form, rows, cols, cus):
    """rows a wave visits at most"""
    pair, grid = launch_plan(form, rows, cols, cus)
    krows = rows // 2 if pair else rows
    return -(-krows // (4 * grid))


FAULTS = ("neigh_stats", "pair_swap", "m1_other", "slot_dropped", "stride_768", "drop_pair_row", "scale_g_out", "dls_scaled")


def fault_applies(fault, c, form, o, pair, grid):
    """the case has enough rows (and the form the operands) to express the fault"""
    ln, ls, rws = form.startswith("ln"), form.endswith("_ls"), form.endswith("_rows")
    scaled = rws or (ls and o["rows"])
    any_sum = ln or o["cs"] or (ls and o["dls"])
    if fault == "neigh_stats":
        return ln and c.rows >= 2
    if fault in ("pair_swap", "m1_other"):
        return pair
    if fault == "slot_dropped":
        return any_sum and grid >= 2
    if fault == "stride_768":
        return any_sum and grid >= 2 and c.cols == 384
    if fault == "drop_pair_row":
        # (rows 0 and 1 read mask rows 0 and 0: with row scales, row 1 is scaled by 0 and the first row to show it is row 2)
        return pair and o["drop"] and o["gm"] and c.rows >= (4 if scaled else 2)
    if fault == "scale_g_out":
        return ln and scaled
    if fault == "dls_scaled":
        return ls and o["dls"] and o["rows"]
    raise ValueError(fault)


def _seq_sum(a, order, b=None, fma=False):
    """sum over the columns `order` of a (or of a * b), one fp32 add at a time, all rows at once; fma: the product unrounded"""
    acc = np.zeros(a.shape[0], np.float32)
    for j in order:
        if b is None:
            acc = acc + a[:, j]
        elif fma:
            acc = (acc.astype(np.float64) + a[:, j].astype(np.float64) * b[:, j].astype(np.float64)).astype(np.float32)
        else:
            acc = acc + a[:, j] * b[:, j]
    return acc


def restate(c, form, o, cus=256, order=None, fma=False, fault=None):
    """ln_bwd_kernel + reduce_parts_kernel in fp32 NumPy: same outputs as `expected`, as numpy arrays (gm, gm8 as fp32 values)"""
    f = np.float32
    ln, ls, q8, rws = form.startswith("ln"), form.endswith("_ls"), form.endswith("_fp8"), form.endswith("_rows")
    rows, cols = c.rows, c.cols
    pair, grid = launch_plan(form, rows, cols, cus)
    order = np.arange(cols) if order is None else order
    ridx = np.arange(rows)
    sc = (c.rowscale.numpy().repeat(c.rpg) if (rws or (ls and o["rows"])) else np.ones(rows, f))[:, None]
    out = {}
    sums = {}
    if ln:
        mu, rs = c.mean.numpy(), c.rstd.numpy()
        if fault == "neigh_stats":
            nb = np.where(ridx + 1 < rows, ridx + 1, ridx - 1)
            mu, rs = mu[nb], rs[nb]
        if fault == "pair_swap":
            mu, rs = mu[ridx ^ 1], rs[ridx ^ 1]
        mu, rs = mu[:, None], rs[:, None]
        d = c.dy.float().numpy()
        xh = (c.x.numpy() - mu) * rs
        dyg = d * c.gamma.numpy()[None, :]
        inv = f(1.0) / f(cols)
        m1 = _seq_sum(dyg, order) * inv
        m2 = _seq_sum(dyg, order, xh, fma) * inv
        if fault == "m1_other":
            m1 = m1[ridx ^ 1]
        if fma:
            t = (dyg.astype(np.float64) - m1[:, None] - xh.astype(np.float64) * m2[:, None]).astype(f)
        else:
            t = dyg - m1[:, None] - xh * m2[:, None]
        dx = t * rs
        if o["res"]:
            dx = dx + c.g_res.numpy()
        out["g_out"] = dx * sc if fault == "scale_g_out" else dx
        sums["dgamma"], sums["dbeta"] = d * xh, d
    else:
        dx = c.g.numpy()
    if o["gm"] or q8:
        op = dx
        if o["drop"]:
            keep = c.keep.numpy().astype(f)
            if fault == "drop_pair_row":
                keep = keep[ridx // 2]
            op = op * keep * f(2.0)
        op = op * sc
        if ls:
            op = op * c.lsgamma.numpy()[None, :]
            if o["dls"]:
                u = c.branch.float().numpy()
                term = sc * (dx * sc if fault == "dls_scaled" else dx) * u
                sums["dls"] = np.where(sc == 0, f(0), term)
        if o["gm"]:
            out["gm"] = op
        if q8:
            out["gm8"] = op * f(QSCALE)
            out["amax"] = np.array([max(f(AMAX0), np.abs(op).max())], f)
        if o["cs"]:
            sums["cs"] = op
    # ---- slot rows: block b holds the rows (PAIR: pairs) 4 b + wave + k * 4 grid; then the fixed-order reduce
    per = 2 if pair else 1
    krows = rows // per
    for name, terms in sums.items():
        stride = 768 if fault == "stride_768" else cols
        ws = np.zeros(grid * max(stride, cols) + cols, f)
        for blk in range(grid):
            slot = np.zeros(cols, f)
            for wave in range(LN_THREADS_ROWS):
                acc = np.zeros(cols, f)
                for kr in range(4 * blk + wave, krows, 4 * grid):
                    for h in range(per):
                        acc = acc + terms[per * kr + h]
                slot = slot + acc
            ws[blk * stride: blk * stride + cols] = slot
        nparts = grid - 1 if fault == "slot_dropped" else grid
        tot = np.zeros(cols, f)
        for p in range(nparts):
            tot = tot + ws[p * cols: (p + 1) * cols]
        out[name] = c.init[name].numpy() + tot
    return out


def same_bits(want, got):
    """`expected` against `restate`: -> the names of the outputs that differ (+0 and -0 equal)"""
    bad = []
    for k, w in want.items():
        w = w.float().numpy()
        if not np.array_equal(w, got[k].astype(np.float32)):
            bad.append(k)
    return bad


# =============================================================================================== part 2: real-valued rows
FAMILIES = "abcdefg"


def family_rows(rows, cols, seed):
    """-> x fp32 [rows, cols], fam int [rows] (index into FAMILIES), kconst [rows] (the constant of a family-d row, else 0).
    Row r is of family r mod 7: neighbours always differ."""
    check_width(cols)                                          # mean == k of a constant row rests on it
    g = torch.Generator().manual_seed(seed)
    fam = torch.arange(rows) % 7
    z = torch.randn(rows, cols, generator=g)
    x = z.clone()
    x[fam == 1] = 256.0 + z[fam == 1]
    x[fam == 2] = -4096.0 + 4.0 * z[fam == 2]
    kconst = torch.zeros(rows)
    kd = torch.tensor([3.0, -7.0, 100.0, -256.0, 1.0, 0.0])
    nd = int((fam == 3).sum())
    kconst[fam == 3] = kd[torch.arange(nd) % len(kd)]
    x[fam == 3] = kconst[fam == 3][:, None].expand(-1, cols)
    x[fam == 4] = 1e-4 * z[fam == 4]
    x[fam == 5] = 1e4 * z[fam == 5]
    gr = (fam == 6).nonzero().flatten()
    col = torch.randint(0, cols, (gr.numel(),), generator=g)
    col[::2] = cols - 1                                        # the last column included
    sign = torch.where(torch.arange(gr.numel()) % 4 < 2, 1.0, -1.0)
    x[gr, col] = 1e4 * sign
    return x.float(), fam, kconst


def affine(cols, seed):
    """gamma of mixed sign and magnitude with exact zeros, a non-zero beta"""
    g = torch.Generator().manual_seed(seed)
    gamma = (torch.randn(cols, generator=g) * torch.tensor([0.05, 1.0, 3.0])[torch.arange(cols) % 3]).clamp(-4, 4)
    gamma[::7] = 0.0
    beta = torch.randn(cols, generator=g) * 0.5 + 0.25
    beta[beta == 0] = 0.125
    return gamma.float(), beta.float()


def fwd_ref(x, gamma, beta, eps):
    """fp64 two-pass LayerNorm of fp32 inputs -> mean, rstd, y (all fp64)"""
    x = x.double()
    mean = x.mean(1)
    c = x - mean[:, None]
    var = (c * c).mean(1)
    rstd = (var + float(np.float32(eps))).rsqrt()
    return mean, rstd, c * rstd[:, None] * gamma.double() + beta.double()


def fwd_bounds(x, gamma, beta, eps):
    """Per-row bounds on the fp32 two-pass forward with sums taken in ANY order, from the row's own magnitudes.
        mean:  fl(sum x) is within gamma_n sum|x| of the sum; the factor fl(1 / n) and the product add 2 u:
               E_mu = gamma_{n+2} sum|x| / n
        var:   d_i = fl(x_i - mean^) = c_i + delta + r_i with c the true centred row, delta = mean - mean^ (|delta| <= E_mu) common
               to the row and |r_i| <= u (|c_i| + E_mu).  sum c_i = 0, so sum d^2 - sum c^2 = 2 sum c_i r_i + sum (delta + r_i)^2:
               dS <= 2 u sum |c_i| (|c_i| + E_mu) + n (E_mu + u (max|c| + E_mu))^2.
               The squares and their sum (all positive) add gamma_{n+1} S, the factor 1 / n and the add of eps 3 u more:
               dv = dS / n + gamma_{n+4} (S + dS) / n + u eps,  rho = dv / (var + eps)
        rstd:  |1 / sqrt(v (1 +- rho)) - 1 / sqrt(v)| / (1 / sqrt(v)) <= 1 / sqrt(1 - rho) - 1, plus 2 ulp of the hardware rsqrt
        y:     t_i = d_i rstd^: |t^ - t| <= |t| (E_rs + 2 u) + (E_mu + u (|c_i| + E_mu)) rstd (1 + E_rs); times gamma and plus beta,
               one rounding each: E_y = |gamma| dt (1 + 2 u) + 2 u (|gamma t| + |beta|).  Against the bf16 image of the reference
               the project's rule 2^-7 |ref| + atol applies with atol = E_y (1 + 2^-8).
    -> E_mu [rows], E_rs [rows] (relative), atol_y [rows, cols] as fp64 tensors"""
    n = x.shape[1]
    xd = x.double()
    mean, rstd, _ = fwd_ref(x, gamma, beta, eps)
    c = xd - mean[:, None]
    e_mu = gamma_n(n + 2) * xd.abs().sum(1) / n
    S = (c * c).sum(1)
    cmax = c.abs().amax(1)
    dS = 2 * U * (c.abs() * (c.abs() + e_mu[:, None])).sum(1) + n * (e_mu + U * (cmax + e_mu)) ** 2
    v = S / n + float(np.float32(eps))
    dv = dS / n + gamma_n(n + 4) * (S + dS) / n + U * float(np.float32(eps))
    rho = (dv / v).clamp(max=0.5)
    e_rs = 1.0 / (1.0 - rho).sqrt() - 1.0 + 2.0 ** -22
    t = c * rstd[:, None]
    dt = t.abs() * (e_rs[:, None] + 2 * U) + (e_mu[:, None] + U * (c.abs() + e_mu[:, None])) * rstd[:, None] * (1 + e_rs[:, None])
    ga, be = gamma.double().abs(), beta.double().abs()
    e_y = ga * dt * (1 + 2 * U) + 2 * U * (ga * t.abs() + be)
    return e_mu, e_rs, e_y * (1 + 2.0 ** -8)


def fwd_ratios(x, gamma, beta, eps, mean, rstd, y, fam):
    """the checks of part 3 on one launch's outputs (CPU tensors): -> {(family, output): largest error / bound}; family d is
    asserted bit-exact here.  `y` may be None (the fp8 form without a bf16 image)."""
    rm, rr, ry = fwd_ref(x, gamma, beta, eps)
    e_mu, e_rs, a_y = fwd_bounds(x, gamma, beta, eps)
    out = {}
    isd = fam == 3
    # ---- family d: bit-exact
    kc = x[isd, 0]
    assert torch.equal(mean[isd], kc), "constant rows: mean != k"
    want = torch.rsqrt(torch.tensor(eps, dtype=F32))
    ulp = float(np.spacing(np.float32(want)))
    assert bool(((rstd[isd].double() - float(want)).abs() <= 2 * ulp).all()), "constant rows: rstd != rsqrt(eps) within 2 ulp"
    if y is not None:
        assert torch.equal(y[isd], beta.to(BF16)[None, :].expand(int(isd.sum()), -1)), "constant rows: y != bf16(beta)"
    # ---- the other families, per row
    qm = (mean.double() - rm).abs() / e_mu.clamp_min(1e-300)
    qr = ((rstd.double() - rr).abs() / rr) / e_rs
    if y is not None:
        ref_b = ry.float().to(BF16).double()
        qy = ((y.double() - ref_b).abs() / (2.0 ** -7 * ref_b.abs() + a_y)).amax(1)
    for i, name in enumerate(FAMILIES):
        sel = fam == i
        if name == "d" or not bool(sel.any()):
            continue
        out[(name, "mean")] = float(qm[sel].max())
        out[(name, "rstd")] = float(qr[sel].max())
        if y is not None:
            q = qy[sel]
            out[(name, "y")] = float("inf") if bool(torch.isnan(q).any()) else float(q.max())
        for k in ("mean", "rstd"):
            if out[(name, k)] != out[(name, k)]:
                out[(name, k)] = float("inf")
    return out


def fp8_excluded(x, gamma, beta, mean, rstd, y8):
    """The e4m3 image against the value the kernel rounds: o = (x - mean) rstd gamma + beta with the launch's OWN mean and rstd
    (checked against fp64 on their own), which fp32 evaluates within E_o = 4 u (|(x - mean) rstd gamma| + |beta|) (three
    roundings of the product, one of the sum; 6 u here covers the fp64 -> fp32 step of this check).  Where e4m3(o - E_o) and
    e4m3(o + E_o) are the same byte, y8 must be that byte; elsewhere o is within its bound of an e4m3 rounding boundary and the
    element is left out.  -> (mismatches among the checked elements, largest left-out share of a row).  y8 = None: only the share."""
    t = (x.double() - mean.double()[:, None]) * rstd.double()[:, None] * gamma.double()
    o = t + beta.double()
    e = 6 * U * (t.abs() + beta.double().abs()) + 1e-45
    lo = (o - e).float().clamp(-448, 448).to(FP8).float()
    hi = (o + e).float().clamp(-448, 448).to(FP8).float()
    sure = lo == hi
    share = float((~sure).double().mean(1).max())
    if y8 is None:
        return 0, share
    bad = sure & (y8.float() != lo)
    return int(bad.sum()), share


def fwd_restate(x, gamma, beta, eps, wrong=None):
    """ln_fwd_kernel in fp32 NumPy (sequential sums) -> mean, rstd, y (bf16 tensor).  wrong: "one_pass" (E[x^2] - mean^2),
    "prev_row" (the previous row's statistics), "no_eps"."""
    f = np.float32
    xn = x.numpy()
    n = xn.shape[1]
    inv = f(1.0) / f(n)
    mu = np.cumsum(xn, axis=1, dtype=f)[:, -1] * inv
    if wrong == "one_pass":
        var = np.cumsum(xn * xn, axis=1, dtype=f)[:, -1] * inv - mu * mu
    else:
        d = xn - mu[:, None]
        var = np.cumsum(d * d, axis=1, dtype=f)[:, -1] * inv
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = (f(1.0) / np.sqrt(var + (f(0) if wrong == "no_eps" else f(eps)), dtype=f)).astype(f)
        if wrong == "prev_row":
            mu, rs = np.roll(mu, 1), np.roll(rs, 1)
        y = (xn - mu[:, None]) * rs[:, None] * gamma.numpy()[None, :] + beta.numpy()[None, :]
    return torch.from_numpy(mu), torch.from_numpy(rs), torch.from_numpy(y.astype(f)).to(BF16)


def bwd_ref(x, mean, rstd, gamma, dy, g_res):
    """The backward formula in fp64 on the kernel's own inputs (fp32 mean / rstd, bf16 dy), and bounds for fp32 sums in any order:
    gamma_n times the sum of the absolute values of the terms added, n = cols for a row's two means, n = rows for a column.
        m1 = sum(dy g) / n, m2 = sum(dy g xh) / n with xh = fl(fl(x - mean) rstd) (2 u) and one rounding per product, the factor
        fl(1 / n) and its product: dm1 = gamma_{n+3} sum|dy g| / n, dm2 = gamma_{n+6} sum|dy g xh| / n
        g_out_i: rstd (dm1 + |xh_i| dm2 + 8 u (|dy g| + |m1| + |xh m2|)_i) + u (|g_res_i| + |g_out_i|)
        dgamma_c: gamma_{rows+3} sum_r |dy xh|;  dbeta_c: gamma_rows sum_r |dy|;
        gm_colsum_c (no dropout: the sum of the fp32 g_out): gamma_rows sum_r |g_out| + (1 + gamma_rows) sum_r E(g_out)
    -> refs (g_out, dgamma, dbeta, cs) and bounds in the same order"""
    n, rows = x.shape[1], x.shape[0]
    xd, d = x.double(), dy.double()
    rs = rstd.double()[:, None]
    xh = (xd - mean.double()[:, None]) * rs
    dyg = d * gamma.double()
    m1 = dyg.mean(1, keepdim=True)
    m2 = (dyg * xh).mean(1, keepdim=True)
    g_out = (dyg - m1 - xh * m2) * rs + g_res.double()
    dm1 = gamma_n(n + 3) * dyg.abs().sum(1, keepdim=True) / n
    dm2 = gamma_n(n + 6) * (dyg * xh).abs().sum(1, keepdim=True) / n
    e_g = rs * (dm1 + xh.abs() * dm2 + 8 * U *(dyg.abs() + m1.abs() + (xh * m2).abs())) + U * (g_res.double().abs() + g_out.abs())
    refs = (g_out, (d * xh).sum(0), d.sum(0), g_out.sum(0))
    bounds = (e_g, gamma_n(rows + 3) * (d * xh).abs().sum(0), gamma_n(rows) * d.abs().sum(0) + 1e-300,
              gamma_n(rows) * g_out.abs().sum(0) + (1 + gamma_n(rows)) * e_g.sum(0))
    return refs, bounds


# =============================================================================================== the case lists both test files use
SMALL_ROWS = (1, 2, 3, 5, 6)         # idle waves and blocks in the LDS reduce; at 384 columns the even counts take PAIR
SWEEP_CUS = 8                        # the CUs the reserve leaves to the library
NARROW_FORMS = ("ln", "ln_ls", "ln_fp8")   # what runs at the widths outside FULL_WIDTHS, all options on
FWD_WIDTHS = (64, 260, 384, 772, 1280, 2048)
FWD_ROWS = 67                        # backward on SWEEP_CUS CUs: 64 rows per trip up to 512 columns, 32 above: a ragged later trip at every width
FWD_LONG = 2 * 16384 + 7             # past twice the forward grid cap of 4 x 4096 rows: every wave takes a second and third row
FWD_LONG_WIDTHS = (64, 772)


def sweep_rows(cols):
    """row counts at which, on SWEEP_CUS CUs, every wave sweeps 3 to 4 rows and the last trip is ragged"""
    return (202, 203) if cols == 384 else ((197,) if cols <= 512 else (101,))


def sweep_cases():
    """(form, cols, rows, options) of the reduced-grid launches"""
    out = []
    for cols in WIDTHS:
        for rows in sweep_rows(cols):
            for form in (FORMS if cols in FULL_WIDTHS else NARROW_FORMS):
                for o in options(form, "matrix" if cols in FULL_WIDTHS else "all"):
                    out.append((form, cols, rows, o))
    return out


def case_id(case):
    form, cols, rows, o = case
    return f"{form}-{cols}x{rows}-{opt_id(o)}"


_CASES = {}


def cached_case(rows, cols):
    if (rows, cols) not in _CASES:
        _CASES[(rows, cols)] = build_case(rows, cols)
    return _CASES[(rows, cols)]
