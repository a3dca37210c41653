"""The drop-path entry points of include/vitssl_droppath.h on the GPU, op by op.

  * vitssl_droppath_table against the NumPy restatement (tests/_droppath_ref.py), bit for bit;
  * vitssl_gemm_bf16_nt_rows on the small-integer operands of tests/_gemm_exact.py (every value an exact integer, so the result is
    compared as bits with an integer reference), rows of dropped samples against `aux` as bits (signed zeros included), a table of
    ones against the plain launch as bits, and a rate of 0.1 against a float64 reference;
  * vitssl_layernorm_bwd_rows / vitssl_grad_mask_cast_rows against the plain entries: g_out, dgamma, dbeta the same bits,
    gm = bf16(scale * the plain fp32 operand) element for element, gm_colsum at the bar of the column-sum op tests (1e-4, rel-L2,
    against the float64 sum).

Shapes: (B, T) = (16, 17): M = 272, sample edges inside the 16-row MFMA groups and a sample across the 256-row tile edge; (3, 197):
M = 591, odd (the 384-column LayerNorm backward then takes one row per wave, the other two take the two-rows-per-wave path);
(1, 64): one sample.  Seeds are chosen on the CPU so that every case has a kept and a dropped sample (asserted); with one sample that
is two seeds, one of each kind.

WIDTHS: the two backward bodies once more at every edge of the launch's column-count ladder (256 / 260, 512 / 516, 1024 / 1028 and
2048: V = 1, 2, 2, 3, 4, 8, 8) with (B, T) = (3, 5): M = 15, odd, four workgroups of which the last has three live waves; and
384 columns with M = 10 (five row pairs) and M = 15 (no pairs)."""
import itertools

import numpy as np
import pytest
import torch

import _droppath_ref as DP
import _gemm_exact as X

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(16, 17), (3, 197), (1, 64)]
WIDTHS = [(3, 5, c) for c in (256, 260, 512, 516, 1024, 1028, 2048)] + [(2, 5, 384), (3, 5, 384)]
SITE = DP.site(1, 0)


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from vitssl_hip import _lib
    return _lib


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def scales_for(B, rate, start=1):
    """[(seed, f32 [B] scales)]: one seed with a kept and a dropped sample; for B == 1 two seeds, a kept and a dropped one"""
    found = {}
    for seed in range(start, start + 10000):
        s = DP.path_scales(B, rate, seed, SITE)
        kept, dropped = bool((s != 0).any()), bool((s == 0).any())
        if B > 1 and kept and dropped:
            return [(seed, s)]
        if B == 1:
            found.setdefault("kept" if kept else "dropped", (seed, s))
            if len(found) == 2:
                return [found["kept"], found["dropped"]]
    raise AssertionError("no seed found")


def device_scales(ops, B, rate, seed):
    out = torch.full((1, B), float("nan"), device=DEV)
    ops.droppath_table([(rate, SITE)], B, seed, out)
    return out[0]


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("seed", [3, 0x1234567890ABCDEF])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_table_equals_the_restatement(ops, B, seed):
    pairs = [(rate, DP.site(blk, br)) for rate in (0.0, 0.1, 0.5) for blk in (0, 1) for br in (0, 1)]
    out = torch.full((len(pairs), B), float("nan"), device=DEV)
    ops.droppath_table(pairs, B, seed, out)
    want = np.stack([DP.path_scales(B, r, seed, s) for r, s in pairs])
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    assert (want[:4] == 1).all()                                             # a rate of 0: a row of ones


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_table_keeps_the_expected_share(ops, rate):
    B = 4096
    out = torch.empty(2, B, device=DEV)
    ops.droppath_table([(rate, DP.site(0, 0)), (rate, DP.site(0, 1))], B, 99, out)
    got = out.cpu().numpy()
    assert np.array_equal(got[0], DP.path_scales(B, rate, 99, DP.site(0, 0)))
    for row in got:
        assert abs(float((row != 0).mean()) - (1 - DP.r_eff(rate))) < 4 * (rate * (1 - rate) / B) ** 0.5
    assert not np.array_equal(got[0], got[1])                                # the two branches draw independently


# ------------------------------------------------------------------------------------------------ the residual GEMM
def exact_cases(axes, extra):
    """SHAPES x N x K x the named axes (value, id) as one list of cases, then `extra`.  The last case of each exact test is
    N % 8 == 4 on the 8-wave tiles (16 x 5 = 80 tiles of 256 x 256): the accumulator-layout stores of the first main loop under
    the row-scale forms of the residual epilogue, which the smaller cases do not reach."""
    cases = [(B, T, N, K) + tuple(v for v, _ in combo) + ("-".join(str(x) for x in (B, T, N, K) + tuple(i for _, i in combo)),)
             for B, T in SHAPES for N in (64, 192, 384) for K in (64, 192) for combo in itertools.product(*axes)]
    return [pytest.param(*c[:-1], id=c[-1]) for c in cases + [extra]]


DROPS = [(0.0, "nodrop"), (0.5, "drop0.5")]


@pytest.mark.parametrize("B,T,N,K,p", exact_cases([DROPS], (20, 195, 1028, 64, 0.5, "20-195-1028-64-drop0.5")))
def test_gemm_rows_exact(ops, L, B, T, N, K, p):
    """path rate 0.5 (scale exactly 2), element dropout off and at 0.5 (scale exactly 2): every value is an integer below 2^24"""
    M = B * T
    A, Bm, bias = X.operands(M, N, K, seed=M + N + K, hi=3, scale=4.0)
    acc = X.ref_nt(A, Bm) + bias.double()
    res = X.int_values((M, N), -100, 100, seed=M)
    res[::7, ::5] = -0.0                                                     # a dropped row keeps the residual's bits, signed zeros too
    drop = ops.make_dropout(p, seed=5, site=11)
    keep = ops.dropout_mask(M, N, drop, DEV).cpu().double()
    Ad, Bd, biasd, resd = A.to(DEV), Bm.to(DEV), bias.to(DEV), res.to(DEV)
    for seed, s in scales_for(B, 0.5, start=N + K):
        assert B == 1 or ((s == 0).any() and (s != 0).any())
        assert set(np.unique(s)) <= {np.float32(0), np.float32(2)}
        sd = device_scales(ops, B, 0.5, seed)
        assert np.array_equal(sd.cpu().numpy(), s)
        out = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm_nt(Ad, Bd, out, L.EPI_RESID, bias=biasd, aux=resd, drop=drop, rows=(sd, T))
        rows = torch.from_numpy(s).double().repeat_interleave(T).view(M, 1)
        want = res.double() + rows * acc * keep * (2.0 if p else 1.0)
        X.check_exact(out, X.to_f32_exact(want), f"EPI_RESID rows B={B} T={T} p={p} seed={seed}")
        dropped = (rows[:, 0] == 0)
        assert B > 1 or bool(dropped.all()) == bool(s[0] == 0)
        assert torch.equal(bits(out)[dropped], bits(res)[dropped]), "a dropped sample's rows must equal aux bit for bit"
    assert B > 1 or len(scales_for(B, 0.5, start=N + K)) == 2                # one sample: a kept and a dropped seed were both run


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,N,K", [(16, 17, 192, 192), (3, 197, 384, 64), (1, 64, 64, 192), (40, 197, 768, 64)], ids=str)
def test_gemm_rows_rate_tenth_and_table_of_ones(ops, L, B, T, N, K, p):
    """Rate 0.1 against float64: the kernel forms fma(keep ? acc + bias : 0, scale[row] * 1 / (1 - p), aux), i.e. at most one rounding of
    the product of the two scales (relative 2^-24, so below one ulp of the product term) and one of the fma (half an ulp of the
    result): |error| <= ulp(product) + ulp(result), the "2 ulp of fp32" of one rounded product and one rounded add.
    A table of ones: the bits of the plain launch, on real-valued operands.  (40, 197) x 768: 93 tiles of 256 x 256, enough for the
    persistent ping-pong kernel with line-shaped epilogue accesses that the training shapes run; the smaller cases take the
    small-tile kernel."""
    M = B * T
    g = torch.Generator().manual_seed(M + N)
    A, Bm = torch.randn(M, K, generator=g).to(BF16), torch.randn(N, K, generator=g).to(BF16)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    drop = ops.make_dropout(p, seed=7, site=2)
    keep = ops.dropout_mask(M, N, drop, DEV).cpu().double()
    Ad, Bd, biasd, resd = A.to(DEV), Bm.to(DEV), bias.to(DEV), res.to(DEV)
    plain = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm_nt(Ad, Bd, plain, L.EPI_RESID, bias=biasd, aux=resd, drop=drop)
    ones = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm_nt(Ad, Bd, ones, L.EPI_RESID, bias=biasd, aux=resd, drop=drop, rows=(torch.ones(B, device=DEV), T))
    assert torch.equal(bits(ones), bits(plain)), "a table of ones must give the bits of the plain launch"
    # the accumulator itself, to fp32 rounding: recovered from the plain launch with a zero residual and no dropout
    accd = torch.empty(M, N, device=DEV)
    ops.gemm_nt(Ad, Bd, accd, L.EPI_RESID, bias=biasd, aux=torch.zeros(M, N, device=DEV))
    acc = accd.cpu().double()
    dscale = 65536.0 / (65536 - int(p * 65536 + 0.5)) if p else 1.0
    dscale = float(np.float32(dscale))
    for seed, s in scales_for(B, 0.1, start=K):
        sd = device_scales(ops, B, 0.1, seed)
        assert np.array_equal(sd.cpu().numpy(), s)
        out = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm_nt(Ad, Bd, out, L.EPI_RESID, bias=biasd, aux=resd, drop=drop, rows=(sd, T))
        rows = torch.from_numpy(s).double().repeat_interleave(T).view(M, 1)
        prod = rows * dscale * acc * keep
        want = res.double() + prod
        ulp = lambda v: torch.from_numpy(np.spacing(v.abs().float().numpy()).astype(np.float64))      # noqa: E731
        err = (out.cpu().double() - want).abs()
        worst = float((err / (ulp(prod) + ulp(want))).max())
        print(f"B={B} T={T} N={N} K={K} p={p} seed={seed}: worst error {worst:.3f} of the bound")
        assert worst <= 1.0
        dropped = (rows[:, 0] == 0)
        assert torch.equal(bits(out)[dropped], bits(res)[dropped])


def test_gemm_rows_refuses_other_epilogues_and_wrong_groups(ops, L):
    A, Bm = torch.zeros(64, 64, dtype=BF16, device=DEV), torch.zeros(64, 64, dtype=BF16, device=DEV)
    s = torch.ones(4, device=DEV)
    with pytest.raises(L.VitsslError, match="EPI_RESID"):
        ops.gemm_nt(A, Bm, torch.empty(64, 64, device=DEV), L.EPI_F32, rows=(s, 16))
    with pytest.raises(L.VitsslError):
        ops.gemm_nt(A, Bm, torch.empty(64, 64, device=DEV), L.EPI_RESID, aux=torch.zeros(64, 64, device=DEV), rows=(s, 15))
    import ctypes as C
    g = L.Gemm()
    g.A, g.B, g.out0, g.aux = A.data_ptr(), Bm.data_ptr(), torch.empty(64, 64, device=DEV).data_ptr(), torch.zeros(64, 64, device=DEV).data_ptr()
    g.M, g.N, g.K = 64, 64, 64
    r = L.RowScale(s.data_ptr(), 4, 16)
    for epi in (L.EPI_BF16, L.EPI_F32, L.EPI_GELU, L.EPI_DGELU, L.EPI_EMBED):
        g.epilogue = epi
        assert L.lib().vitssl_gemm_bf16_nt_rows(C.byref(g), C.byref(r), None) == -1
    g.epilogue = L.EPI_RESID
    r.groups = 5
    assert L.lib().vitssl_gemm_bf16_nt_rows(C.byref(g), C.byref(r), None) == -1 and b"must equal M" in L.lib().vitssl_last_error()


# ------------------------------------------------------------------------------------------------ the masked gradient operand
def _operand(g_out, keep, p, s, T):
    """bf16(scale[row // T] * (keep * g_out / (1 - p))): the plain entry's fp32 operand, one more fp32 multiply, one bf16 rounding"""
    o = g_out.cpu().float()
    if p:
        dscale = torch.tensor(np.float32(65536.0) / np.float32(65536 - int(p * 65536 + 0.5)))
        o = torch.where(keep.cpu() != 0, o * dscale, torch.zeros(()))
    rows = torch.from_numpy(s).repeat_interleave(T).view(-1, 1)
    o = o * rows
    return o.to(BF16), o.double().sum(0)


@pytest.mark.parametrize("cs", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cols", [64, 384, 768])
@pytest.mark.parametrize("B,T", SHAPES, ids=str)
def test_layernorm_bwd_rows(ops, B, T, cols, p, cs):
    from _util import rel_l2
    M = B * T
    g = torch.Generator().manual_seed(M + cols)
    x = torch.randn(M, cols, generator=g).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(cols, generator=g)).to(DEV), torch.zeros(cols, device=DEV)
    dy = torch.randn(M, cols, generator=g).to(BF16).to(DEV)
    g_res = torch.randn(M, cols, generator=g).to(DEV)
    y, mean, rstd = torch.empty(M, cols, dtype=BF16, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x, gamma, beta, y, mean, rstd)
    drop = ops.make_dropout(p, seed=21, site=4)
    keep = ops.dropout_mask(M, cols, drop, DEV)

    def run(rows):
        g_out, gm = torch.full((M, cols), float("nan"), device=DEV), torch.full((M, cols), float("nan"), dtype=BF16, device=DEV)
        dg, db, csum = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV) if cs else None
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, g_res, g_out, gm, dg, db, csum, drop, rows=rows)
        return g_out, gm, dg, db, csum

    plain = run(None)
    for seed, s in scales_for(B, 0.3, start=cols):
        assert B == 1 or ((s == 0).any() and (s != 0).any())
        got = run((torch.from_numpy(s).to(DEV), T))
        for name, a, b in zip(("g_out", "dgamma", "dbeta"), (got[0], got[2], got[3]), (plain[0], plain[2], plain[3])):
            assert torch.equal(bits(a), bits(b)), f"{name} must not see the row scales"
        want, wsum = _operand(plain[0], keep, p, s, T)
        X.check_exact(got[1], want, f"gm rows B={B} T={T} cols={cols} p={p}")
        if cs:
            assert rel_l2(got[4], wsum) < 1e-4
    # a table of ones: the plain entry's bits, column sums included
    ones = run((torch.ones(B, device=DEV), T))
    for a, b in zip(ones, plain):
        assert a is None or torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("cs", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cols", [64, 384, 768])
@pytest.mark.parametrize("B,T", SHAPES, ids=str)
def test_grad_mask_cast_rows(ops, B, T, cols, p, cs):
    from _util import rel_l2
    M = B * T
    g = torch.randn(M, cols, generator=torch.Generator().manual_seed(M + cols + 1)).to(DEV)
    drop = ops.make_dropout(p, seed=22, site=8)
    keep = ops.dropout_mask(M, cols, drop, DEV)

    def run(rows):
        gm = torch.full((M, cols), float("nan"), dtype=BF16, device=DEV)
        csum = torch.zeros(cols, device=DEV) if cs else None
        ops.grad_mask_cast(g, gm, csum, drop, rows=rows)
        return gm, csum

    plain = run(None)
    for seed, s in scales_for(B, 0.3, start=cols):
        gm, csum = run((torch.from_numpy(s).to(DEV), T))
        want, wsum = _operand(g, keep, p, s, T)
        X.check_exact(gm, want, f"grad_mask_cast rows B={B} T={T} cols={cols} p={p}")
        if cs:
            assert rel_l2(csum, wsum) < 1e-4
    ones = run((torch.ones(B, device=DEV), T))
    for a, b in zip(ones, plain):
        assert a is None or torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("cs", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,cols", WIDTHS, ids=str)
def test_layernorm_bwd_rows_widths(ops, B, T, cols, p, cs):
    test_layernorm_bwd_rows(ops, B, T, cols, p, cs)


@pytest.mark.parametrize("cs", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,cols", WIDTHS, ids=str)
def test_grad_mask_cast_rows_widths(ops, B, T, cols, p, cs):
    test_grad_mask_cast_rows(ops, B, T, cols, p, cs)
