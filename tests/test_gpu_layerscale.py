"""The LayerScale entry points of include/vitssl_layerscale.h on the GPU, op by op.

  * vitssl_gemm_bf16_nt_ls on the small-integer operands of tests/_gemm_exact.py with gamma from {-2, -1, -0.5, 0.25, 1, 3} (every
    value an exact multiple of 1/4 below 2^24): out0 and the bf16 image of the branch compared as bits with the integer reference,
    dropped rows against `aux` as bits, a gamma of ones against the _rows / plain launch as bits (real-valued operands too), and
    random gammas at two scales against float64;
  * vitssl_layernorm_bwd_ls / vitssl_grad_mask_cast_ls against the plain entries: g_out, dgamma, dbeta the same bits,
    gm = bf16(gamma * the _rows fp32 operand) element for element, gm_colsum and dls against float64 sums of the device's own
    read-back operands at the column-sum bar of the project (1e-4, rel-L2), dls the same bits in two runs, a gamma of ones the
    _rows bits.

Shapes as in tests/test_gpu_droppath.py: (B, T) = (16, 17): M = 272, sample edges inside the 16-row MFMA groups and a sample across
the 256-row tile edge; (3, 197): M = 591, odd (the 384-column LayerNorm backward then takes one row per wave, the other two the
two-rows-per-wave path); (1, 64): one sample.  The two backward bodies run once more at its WIDTHS: every edge of the launch's
column-count ladder at M = 15, and 384 columns with and without row pairs."""
import ctypes as C

import numpy as np
import pytest
import torch

import _gemm_exact as X
from _util import rel_l2
from test_gpu_droppath import DROPS, SHAPES, WIDTHS, bits, exact_cases, scales_for

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
GAMMAS = torch.tensor([-2.0, -1.0, -0.5, 0.25, 1.0, 3.0])


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from vitssl_hip import _lib
    return _lib


def exact_gamma(N, seed):
    return GAMMAS[torch.randint(0, len(GAMMAS), (N,), generator=torch.Generator().manual_seed(seed))]


def row_tables(B, rate, start, with_rows):
    """[(f32 [B] scales or None)]: no table, or the seeds of scales_for (a kept and a dropped sample)"""
    return [s for _, s in scales_for(B, rate, start=start)] if with_rows else [None]


# ------------------------------------------------------------------------------------------------ the residual GEMM
@pytest.mark.parametrize("B,T,N,K,p,with_rows", exact_cases([DROPS, [(False, "norows"), (True, "rows0.5")]],
                                                            (20, 195, 1028, 64, 0.5, True, "20-195-1028-64-drop0.5-rows0.5")))
def test_gemm_ls_exact(ops, L, B, T, N, K, p, with_rows):
    """row scale in {0, 2}, dropout scale 2, gamma a multiple of 1/4 up to 3: every value is a multiple of 1/4 below 2^24 / 4"""
    M = B * T
    A, Bm, bias = X.operands(M, N, K, seed=M + N + K, hi=3, scale=48.0)
    acc = X.ref_nt(A, Bm) + bias.double()
    res = X.int_values((M, N), -100, 100, seed=M)
    res[::7, ::5] = -0.0
    gamma = exact_gamma(N, N + K)
    drop = ops.make_dropout(p, seed=5, site=11)
    keep = ops.dropout_mask(M, N, drop, DEV).cpu().double()
    Ad, Bd, biasd, resd, gd = A.to(DEV), Bm.to(DEV), bias.to(DEV), res.to(DEV), gamma.to(DEV)
    u = acc * keep * (2.0 if p else 1.0)
    for s in row_tables(B, 0.5, N + K, with_rows):
        rows_arg = None if s is None else (torch.from_numpy(s).to(DEV), T)
        out = torch.full((M, N), float("nan"), device=DEV)
        br = torch.full((M, N), float("nan"), dtype=BF16, device=DEV)
        ops.gemm_nt(Ad, Bd, out, L.EPI_RESID, bias=biasd, aux=resd, drop=drop, rows=rows_arg, cols=gd, branch=br)
        rows = torch.ones(M, 1, dtype=torch.float64) if s is None else torch.from_numpy(s).double().repeat_interleave(T).view(M, 1)
        want = res.double() + rows * gamma.double().view(1, N) * u
        X.check_exact(out, X.to_f32_exact(want), f"EPI_RESID ls B={B} T={T} p={p} rows={with_rows}")
        X.check_exact(br, X.bf16_rne(u), f"branch image B={B} T={T} p={p} rows={with_rows}")       # independent of rs and gamma
        dropped = rows[:, 0] == 0
        assert torch.equal(bits(out)[dropped], bits(res)[dropped]), "a dropped sample's rows must equal aux bit for bit"
        # without the branch pointer: the same out0
        out2 = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm_nt(Ad, Bd, out2, L.EPI_RESID, bias=biasd, aux=resd, drop=drop, rows=rows_arg, cols=gd)
        assert torch.equal(bits(out2), bits(out))


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,N,K", [(16, 17, 192, 192), (3, 197, 384, 64), (1, 64, 64, 192), (40, 197, 768, 64)], ids=str)
def test_gemm_ls_real_operands(ops, L, B, T, N, K, p):
    """A gamma of ones: the bits of the _rows launch and of the plain launch, on real-valued operands ((40, 197) x 768: the
    persistent ping-pong kernel with line-shaped epilogue accesses; the smaller cases take the small-tile kernel).
    Random gamma at two scales (1e-5 and O(1) with mixed signs), row rate 0.1, against float64.  The kernel forms
    fma(keep ? acc + bias : 0, (rs * dropscale) * gamma, aux): two roundings of the scale product (each relative 2^-24, so each
    below one ulp of the product term) and one of the fma (half an ulp of the result): |error| <= 2 ulp(product) + ulp(result),
    derived as in test_gemm_rows_rate_tenth_and_table_of_ones with one more rounded product."""
    M = B * T
    g = torch.Generator().manual_seed(M + N)
    A, Bm = torch.randn(M, K, generator=g).to(BF16), torch.randn(N, K, generator=g).to(BF16)
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    drop = ops.make_dropout(p, seed=7, site=2)
    keep = ops.dropout_mask(M, N, drop, DEV).cpu().double()
    Ad, Bd, biasd, resd = A.to(DEV), Bm.to(DEV), bias.to(DEV), res.to(DEV)
    ones = torch.ones(N, device=DEV)

    def run(rows=None, cols=None, branch=None):
        out = torch.full((M, N), float("nan"), device=DEV)
        ops.gemm_nt(Ad, Bd, out, L.EPI_RESID, bias=biasd, aux=resd, drop=drop, rows=rows, cols=cols, branch=branch)
        return out

    assert torch.equal(bits(run(cols=ones)), bits(run())), "a gamma of ones must give the bits of the plain launch"
    accd = torch.empty(M, N, device=DEV)
    ops.gemm_nt(Ad, Bd, accd, L.EPI_RESID, bias=biasd, aux=torch.zeros(M, N, device=DEV))
    acc = accd.cpu().double()
    dscale = float(np.float32(65536.0 / (65536 - int(p * 65536 + 0.5)))) if p else 1.0
    ulp = lambda v: torch.from_numpy(np.spacing(v.abs().float().numpy()).astype(np.float64))      # noqa: E731
    for _, s in scales_for(B, 0.1, start=K):
        sd = torch.from_numpy(s).to(DEV)
        assert torch.equal(bits(run(rows=(sd, T), cols=ones)), bits(run(rows=(sd, T)))), "a gamma of ones must give the _rows bits"
        rows = torch.from_numpy(s).double().repeat_interleave(T).view(M, 1)
        for scale in (1e-5, 1.0):
            gg = torch.Generator().manual_seed(N + int(scale))
            gamma = (scale * (0.5 + torch.rand(N, generator=gg)) * torch.where(torch.rand(N, generator=gg) < 0.5, -1.0, 1.0)).float()
            br = torch.full((M, N), float("nan"), dtype=BF16, device=DEV)
            out = run(rows=(sd, T), cols=gamma.to(DEV), branch=br)
            prod = rows * dscale * gamma.double().view(1, N) * acc * keep
            want = res.double() + prod
            err = (out.cpu().double() - want).abs()
            worst = float((err / (2 * ulp(prod) + ulp(want))).max())
            print(f"B={B} T={T} N={N} K={K} p={p} gamma~{scale:g}: worst error {worst:.3f} of the bound")
            assert worst <= 1.0
            dropped = rows[:, 0] == 0
            assert torch.equal(bits(out)[dropped], bits(res)[dropped])
            # the branch image: bf16 of the device's own fp32 (acc + bias) times the fp32 dropout scale, masked
            want_u = torch.where(keep != 0, (accd.cpu() * np.float32(dscale)).double(), torch.zeros((), dtype=torch.float64)).float().to(BF16)
            X.check_exact(br, want_u, f"branch image B={B} T={T} N={N} p={p}")


def test_gemm_ls_refusals(ops, L):
    A, Bm = torch.zeros(64, 64, dtype=BF16, device=DEV), torch.zeros(64, 64, dtype=BF16, device=DEV)
    gam, s = torch.ones(64, device=DEV), torch.ones(4, device=DEV)
    out, aux = torch.empty(64, 64, device=DEV), torch.zeros(64, 64, device=DEV)
    with pytest.raises(L.VitsslError, match="EPI_RESID"):
        ops.gemm_nt(A, Bm, out, L.EPI_F32, cols=gam)
    with pytest.raises(L.VitsslError):
        ops.gemm_nt(A, Bm, out, L.EPI_RESID, aux=aux, cols=torch.ones(60, device=DEV))
    with pytest.raises(L.VitsslError):
        ops.gemm_nt(A, Bm, out, L.EPI_RESID, aux=aux, cols=gam, rows=(s, 15))
    with pytest.raises(L.VitsslError, match="cols="):
        ops.gemm_nt(A, Bm, out, L.EPI_RESID, aux=aux, branch=torch.empty(64, 64, dtype=BF16, device=DEV))
    g = L.Gemm()
    g.A, g.B, g.out0, g.aux = A.data_ptr(), Bm.data_ptr(), out.data_ptr(), aux.data_ptr()
    g.M, g.N, g.K = 64, 64, 64
    c, r = L.ColScale(gam.data_ptr(), 64), L.RowScale(s.data_ptr(), 4, 16)
    fn = L.lib().vitssl_gemm_bf16_nt_ls
    for epi in (L.EPI_BF16, L.EPI_F32, L.EPI_GELU, L.EPI_DGELU, L.EPI_EMBED):
        g.epilogue = epi
        assert fn(C.byref(g), C.byref(c), None, None, None) == -1 and b"EPI_RESID" in L.lib().vitssl_last_error()
    g.epilogue = L.EPI_RESID
    assert fn(C.byref(g), None, None, None, None) == -1
    c.cols = 60
    assert fn(C.byref(g), C.byref(c), None, None, None) == -1 and b"must equal N" in L.lib().vitssl_last_error()
    c.cols = 64
    r.groups = 5
    assert fn(C.byref(g), C.byref(c), C.byref(r), None, None) == -1 and b"must equal M" in L.lib().vitssl_last_error()


# ------------------------------------------------------------------------------------------------ the masked gradient operand
def _rows_operand(g_out, keep, p, s, T):
    """fp32 rs * (keep * g_out / (1 - p)): the _rows entry's operand before its bf16 rounding"""
    o = g_out.cpu().float()
    if p:
        dscale = torch.tensor(np.float32(65536.0) / np.float32(65536 - int(p * 65536 + 0.5)))
        o = torch.where(keep.cpu() != 0, o * dscale, torch.zeros(()))
    if s is not None:
        o = o * torch.from_numpy(s).repeat_interleave(T).view(-1, 1)
    return o


def _check_ls(got_gm, got_cs, got_dls, g_out, branch, keep, p, s, T, gamma, what):
    M = g_out.shape[0]
    o = _rows_operand(g_out, keep, p, s, T) * gamma.cpu().view(1, -1)        # one more fp32 multiply
    X.check_exact(got_gm, o.to(BF16), what)
    if got_cs is not None:
        assert rel_l2(got_cs, o.double().sum(0)) < 1e-4, what
    rows = torch.ones(M, 1, dtype=torch.float64) if s is None else torch.from_numpy(s).double().repeat_interleave(T).view(M, 1)
    want = (rows * g_out.cpu().double() * branch.cpu().double()).sum(0)
    fig = rel_l2(got_dls, want)
    print(f"{what}: dls rel-L2 {fig:.3g}")
    assert fig < 1e-4, what


@pytest.mark.parametrize("with_rows", [False, True], ids=["norows", "rows0.3"])
@pytest.mark.parametrize("cs", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cols", [64, 384, 768])
@pytest.mark.parametrize("B,T", SHAPES, ids=str)
def test_layernorm_bwd_ls(ops, B, T, cols, p, cs, with_rows):
    M = B * T
    g = torch.Generator().manual_seed(M + cols)
    x = torch.randn(M, cols, generator=g).to(DEV)
    gamma, beta = (1 + 0.1 * torch.randn(cols, generator=g)).to(DEV), torch.zeros(cols, device=DEV)
    dy = torch.randn(M, cols, generator=g).to(BF16).to(DEV)
    g_res = torch.randn(M, cols, generator=g).to(DEV)
    branch = torch.randn(M, cols, generator=g).to(BF16).to(DEV)
    lsg = ((0.5 + torch.rand(cols, generator=g)) * torch.where(torch.rand(cols, generator=g) < 0.5, -1.0, 1.0)).to(DEV)
    y, mean, rstd = torch.empty(M, cols, dtype=BF16, device=DEV), torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    ops.layernorm_fwd(x, gamma, beta, y, mean, rstd)
    drop = ops.make_dropout(p, seed=21, site=4)
    keep = ops.dropout_mask(M, cols, drop, DEV)

    def run(rows, lscale=None, want_dls=True):
        g_out, gm = torch.full((M, cols), float("nan"), device=DEV), torch.full((M, cols), float("nan"), dtype=BF16, device=DEV)
        dg, db, csum = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV) if cs else None
        dls = torch.zeros(cols, device=DEV) if lscale is not None and want_dls else None
        kw = {} if lscale is None else dict(cols=lscale, branch=branch if want_dls else None, dls=dls)
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, g_res, g_out, gm, dg, db, csum, drop, rows=rows, **kw)
        return g_out, gm, dg, db, csum, dls

    plain = run(None)
    for s in row_tables(B, 0.3, cols, with_rows):
        assert s is None or B == 1 or ((s == 0).any() and (s != 0).any())        # a kept and a dropped sample
        rows_arg = None if s is None else (torch.from_numpy(s).to(DEV), T)
        got = run(rows_arg, lsg)
        for name, a, b in zip(("g_out", "dgamma", "dbeta"), (got[0], got[2], got[3]), (plain[0], plain[2], plain[3])):
            assert torch.equal(bits(a), bits(b)), f"{name} must not see the scales"
        _check_ls(got[1], got[4], got[5], plain[0], branch, keep, p, s, T, lsg, f"layernorm_bwd_ls B={B} T={T} cols={cols} p={p}")
        again = run(rows_arg, lsg)
        assert torch.equal(bits(again[5]), bits(got[5])), "dls must be the same bits in two runs"
        nodls = run(rows_arg, lsg, want_dls=False)                           # no gradient of gamma wanted: the same operand
        assert torch.equal(bits(nodls[1]), bits(got[1]))
        # a gamma of ones: the _rows (or plain) bits, column sums included
        base = run(rows_arg)
        ones = run(rows_arg, torch.ones(cols, device=DEV))
        for a, b in zip(ones[:5], base[:5]):
            assert a is None or torch.equal(bits(a), bits(b))
    # dls accumulates into its target as gm_colsum does
    if cs:
        rows_arg = None
        g_out, gm = torch.empty(M, cols, device=DEV), torch.empty(M, cols, dtype=BF16, device=DEV)
        dg, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        csum, dls = torch.full((cols,), 3.0, device=DEV), torch.full((cols,), 5.0, device=DEV)
        ops.layernorm_bwd(dy, x, mean, rstd, gamma, g_res, g_out, gm, dg, db, csum, drop, cols=lsg, branch=branch, dls=dls)
        first = run(None, lsg)
        assert rel_l2(dls - 5.0, first[5]) < 1e-5 and rel_l2(csum - 3.0, first[4]) < 1e-5


@pytest.mark.parametrize("with_rows", [False, True], ids=["norows", "rows0.3"])
@pytest.mark.parametrize("cs", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("cols", [64, 384, 768])
@pytest.mark.parametrize("B,T", SHAPES, ids=str)
def test_grad_mask_cast_ls(ops, B, T, cols, p, cs, with_rows):
    M = B * T
    gen = torch.Generator().manual_seed(M + cols + 1)
    g = torch.randn(M, cols, generator=gen).to(DEV)
    branch = torch.randn(M, cols, generator=gen).to(BF16).to(DEV)
    lsg = ((0.5 + torch.rand(cols, generator=gen)) * torch.where(torch.rand(cols, generator=gen) < 0.5, -1.0, 1.0)).to(DEV)
    drop = ops.make_dropout(p, seed=22, site=8)
    keep = ops.dropout_mask(M, cols, drop, DEV)

    def run(rows, lscale=None):
        gm = torch.full((M, cols), float("nan"), dtype=BF16, device=DEV)
        csum = torch.zeros(cols, device=DEV) if cs else None
        dls = torch.zeros(cols, device=DEV) if lscale is not None else None
        kw = {} if lscale is None else dict(cols=lscale, branch=branch, dls=dls)
        ops.grad_mask_cast(g, gm, csum, drop, rows=rows, **kw)
        return gm, csum, dls

    for s in row_tables(B, 0.3, cols, with_rows):
        rows_arg = None if s is None else (torch.from_numpy(s).to(DEV), T)
        gm, csum, dls = run(rows_arg, lsg)
        _check_ls(gm, csum, dls, g, branch, keep, p, s, T, lsg, f"grad_mask_cast_ls B={B} T={T} cols={cols} p={p}")
        assert torch.equal(bits(run(rows_arg, lsg)[2]), bits(dls)), "dls must be the same bits in two runs"
        base, ones = run(rows_arg), run(rows_arg, torch.ones(cols, device=DEV))
        for a, b in zip(ones[:2], base[:2]):
            assert a is None or torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("with_rows", [False, True], ids=["norows", "rows0.3"])
@pytest.mark.parametrize("cs", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,cols", WIDTHS, ids=str)
def test_layernorm_bwd_ls_widths(ops, B, T, cols, p, cs, with_rows):
    test_layernorm_bwd_ls(ops, B, T, cols, p, cs, with_rows)


@pytest.mark.parametrize("with_rows", [False, True], ids=["norows", "rows0.3"])
@pytest.mark.parametrize("cs", [True, False], ids=["colsum", "nocolsum"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,cols", WIDTHS, ids=str)
def test_grad_mask_cast_ls_widths(ops, B, T, cols, p, cs, with_rows):
    test_grad_mask_cast_ls(ops, B, T, cols, p, cs, with_rows)


def test_backward_entries_refuse_bad_arguments(ops, L):
    M, cols = 64, 64
    g, gm = torch.zeros(M, cols, device=DEV), torch.empty(M, cols, dtype=BF16, device=DEV)
    lsg, br, dls = torch.ones(cols, device=DEV), torch.zeros(M, cols, dtype=BF16, device=DEV), torch.zeros(cols, device=DEV)
    with pytest.raises(L.VitsslError, match="together"):
        ops.grad_mask_cast(g, gm, cols=lsg, branch=br)
    with pytest.raises(L.VitsslError):
        ops.grad_mask_cast(g, gm, cols=torch.ones(60, device=DEV), branch=br, dls=dls)
    with pytest.raises(L.VitsslError, match="cols="):
        ops.grad_mask_cast(g, gm, branch=br, dls=dls)
    c = L.ColScale(lsg.data_ptr(), 60)
    ws = torch.empty(int(L.lib().vitssl_layerscale_workspace_floats(M, cols)), device=DEV)
    rc = L.lib().vitssl_grad_mask_cast_ls(g.data_ptr(), gm.data_ptr(), None, ops.NO_DROP, None, C.byref(c), br.data_ptr(), dls.data_ptr(),
                                         M, cols, ws.data_ptr(), ws.numel(), None)
    assert rc == -1 and b"column scales hold" in L.lib().vitssl_last_error()
    c.cols = cols
    rc = L.lib().vitssl_grad_mask_cast_ls(g.data_ptr(), gm.data_ptr(), None, ops.NO_DROP, None, C.byref(c), br.data_ptr(), None,
                                         M, cols, ws.data_ptr(), ws.numel(), None)
    assert rc == -1 and b"together" in L.lib().vitssl_last_error()
