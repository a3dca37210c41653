"""The entry points of include/vitssl_layerscale.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_droppath_bounds.py: every input, table, gamma, the branch image, every output and an EXACT-size workspace are carved
from a 0xFF-poisoned arena.  Per case: no guard byte changes; no NaN poison reaches a result (every output element is written,
every workspace slot is written before it is read, the guards around gamma and the table of scales are never read into a
result); a zero-filled and a 0xFF-filled workspace give the same bits; one float short of the documented workspace is refused
before anything is launched; inputs are only read."""
import ctypes as C

import pytest
import torch

from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)
from test_gpu_droppath_bounds import P, S, _ln_case, mixed_scales, same_bits

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
gpu = pytest.mark.gpu


def signed_gamma(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.5 + torch.rand(n, generator=g)) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


@gpu
@pytest.mark.parametrize("with_rows", [False, True], ids=["norows", "rows"])
@pytest.mark.parametrize("p", [0.0, 0.5], ids=["nodrop", "drop0.5"])
@pytest.mark.parametrize("B,T,N,K", [(16, 17, 192, 64), (3, 197, 260, 128), (1, 1, 4, 64), (1, 64, 64, 64), (30, 197, 768, 64)], ids=str)
def test_gemm_ls_on_the_arena(B, T, N, K, p, with_rows):
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    M = B * T
    g = torch.Generator().manual_seed(M + N)
    a = Arena(DEV, mib=128)
    A = a.put("A", torch.randn(M, K, generator=g).to(BF16))
    Bm = a.put("B", torch.randn(N, K, generator=g).to(BF16))
    bias, res = a.put("bias", torch.randn(N, generator=g)), a.put("aux", torch.randn(M, N, generator=g))
    gam = a.put("gamma", signed_gamma(N, N))
    s = mixed_scales(B) if with_rows else torch.ones(B)
    sc = a.put("scale", s)
    out, br = a.empty("out0", (M, N), F32), a.empty("branch", (M, N), BF16)
    gm = L.Gemm()
    gm.A, gm.B, gm.M, gm.N, gm.K, gm.epilogue = A.data_ptr(), Bm.data_ptr(), M, N, K, L.EPI_RESID
    gm.bias, gm.aux, gm.out0 = bias.data_ptr(), res.data_ptr(), out.data_ptr()
    gm.drop = ops.make_dropout(p, seed=3, site=5)
    r, c = L.RowScale(sc.data_ptr(), B, T), L.ColScale(gam.data_ptr(), N)
    before = [t.clone() for t in (A, Bm, bias, res, sc, gam)]
    L.call("vitssl_gemm_bf16_nt_ls", C.byref(gm), C.byref(c), C.byref(r) if with_rows else None, P(br), S())
    torch.cuda.synchronize()
    a.check()
    assert not torch.isnan(out).any() and not torch.isnan(br.float()).any()
    # without the branch pointer nothing is written there
    Arena.fill(br)
    first = out.clone()
    Arena.fill(out)
    L.call("vitssl_gemm_bf16_nt_ls", C.byref(gm), C.byref(c), C.byref(r) if with_rows else None, None, S())
    torch.cuda.synchronize()
    a.check()
    assert Arena.untouched(br) and same_bits(out, first)
    plain = torch.empty(M, N, device=DEV)
    ops.gemm_nt(A.clone(), Bm.clone(), plain, L.EPI_RESID, bias=bias.clone(), aux=torch.zeros(M, N, device=DEV), drop=gm.drop)
    rows = s.repeat_interleave(T).view(M, 1).to(DEV)
    want = res.double() + rows.double() * gam.double().view(1, N) * plain.double()
    assert float((out.double() - want).abs().max()) <= 2e-6 * float(want.abs().max())
    dropped = rows[:, 0] == 0
    assert same_bits(out[dropped], res[dropped])
    for t, b in zip((A, Bm, bias, res, sc, gam), before):
        assert same_bits(t, b)


def _run_backward(a, launch, need, outs, sums, sizing):
    """refusal one float short, then a 0xFF- and a zero-filled workspace: the results of both"""
    from vitssl_hip import _lib as L
    ws = a.empty("workspace", (need,), F32)
    assert launch(ws, need - 1) == -1 and sizing in L.lib().vitssl_last_error()
    torch.cuda.synchronize()
    assert Arena.untouched(ws) and all(Arena.untouched(t) for t in outs)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill)
        for t in outs:
            Arena.fill(t)
        for t in sums:
            Arena.fill(t, 0)
        assert launch(ws, need) == 0, L.lib().vitssl_last_error()
        torch.cuda.synchronize()
        a.check()
        got = [t.cpu().clone() for t in list(outs) + list(sums)]
        assert not any(torch.isnan(t.float()).any() for t in got)
        results.append(got)
    for u, v in zip(*results):
        assert same_bits(u, v), "bits depend on what the workspace held"
    return results[0]


@gpu
@pytest.mark.parametrize("with_rows", [False, True], ids=["norows", "rows"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,cols", [(16, 17, 384), (3, 197, 384), (3, 197, 768), (1, 64, 64), (1, 1, 4), (5, 33, 260), (5, 33, 1024),
                                      (2, 40, 2048), (600, 7, 384)], ids=str)
def test_layernorm_bwd_ls_on_the_arena(B, T, cols, p, with_rows):
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    M = B * T
    a = Arena(DEV, mib=128)
    x, gamma, dy, g_res, mean, rstd = _ln_case(a, M, cols, M + cols)
    s = mixed_scales(B, 0.3) if with_rows else torch.ones(B)
    sc, gam = a.put("scale", s), a.put("lsgamma", signed_gamma(cols, cols))
    br = a.put("branch", torch.randn(M, cols, generator=torch.Generator().manual_seed(M)).to(BF16))
    g_out, gm = a.empty("g_out", (M, cols), F32), a.empty("gm", (M, cols), BF16)
    dg, db, cs, dls = (a.empty(n, (cols,), F32) for n in ("dgamma", "dbeta", "gm_colsum", "dls"))
    need = int(L.lib().vitssl_layerscale_workspace_floats(M, cols))
    assert need >= int(L.lib().vitssl_sum_workspace_floats(M, cols))
    drop = ops.make_dropout(p, seed=9, site=1)
    r, c = L.RowScale(sc.data_ptr(), B, T), L.ColScale(gam.data_ptr(), cols)
    before = [t.clone() for t in (x, gamma, dy, g_res, mean, rstd, sc, gam, br)]

    def launch(ws, n):
        return L.lib().vitssl_layernorm_bwd_ls(P(dy), P(x), P(mean), P(rstd), P(gamma), P(g_res), P(g_out), P(gm), P(dg), P(db), P(cs), drop,
                                               C.byref(r) if with_rows else None, C.byref(c), P(br), P(dls), M, cols, P(ws), n, S())

    got = _run_backward(a, launch, need, (g_out, gm), (dg, db, cs, dls), b"vitssl_layerscale_workspace_floats")
    po, pm = torch.empty(M, cols, device=DEV), torch.empty(M, cols, dtype=BF16, device=DEV)
    pg, pb = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
    ops.layernorm_bwd(dy.clone(), x.clone(), mean.clone(), rstd.clone(), gamma.clone(), g_res.clone(), po, pm, pg, pb, None, drop)
    assert same_bits(got[0], po) and same_bits(got[2], pg) and same_bits(got[3], pb)
    rows = s.repeat_interleave(T).view(M, 1)
    dropped = rows[:, 0] == 0
    assert bool((got[1][dropped].float() == 0).all())
    want = pm.cpu().float() * rows * gam.cpu().view(1, cols)
    assert float((got[1].float() - want).abs().max()) <= 2.0 ** -6 * float(want.abs().max()) + 1e-30
    wls = (rows.double() * po.cpu().double() * br.cpu().double()).sum(0)
    assert float((got[5].double() - wls).norm()) <= 1e-4 * float(wls.norm()) + 1e-30
    for t, b in zip((x, gamma, dy, g_res, mean, rstd, sc, gam, br), before):
        assert same_bits(t, b)


@gpu
@pytest.mark.parametrize("with_rows", [False, True], ids=["norows", "rows"])
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,cols", [(16, 17, 384), (3, 197, 768), (1, 64, 64), (1, 1, 4), (5, 33, 260), (5, 33, 1024), (2, 40, 2048)], ids=str)
def test_grad_mask_cast_ls_on_the_arena(B, T, cols, p, with_rows):
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    M = B * T
    a = Arena(DEV, mib=64)
    g = a.put("g", torch.randn(M, cols, generator=torch.Generator().manual_seed(M)))
    s = mixed_scales(B, 0.3) if with_rows else torch.ones(B)
    sc, gam = a.put("scale", s), a.put("lsgamma", signed_gamma(cols, cols))
    br = a.put("branch", torch.randn(M, cols, generator=torch.Generator().manual_seed(M + 1)).to(BF16))
    gm, cs, dls = a.empty("gm", (M, cols), BF16), a.empty("gm_colsum", (cols,), F32), a.empty("dls", (cols,), F32)
    need = int(L.lib().vitssl_layerscale_workspace_floats(M, cols))
    drop = ops.make_dropout(p, seed=10, site=2)
    r, c = L.RowScale(sc.data_ptr(), B, T), L.ColScale(gam.data_ptr(), cols)

    def launch(ws, n):
        return L.lib().vitssl_grad_mask_cast_ls(P(g), P(gm), P(cs), drop, C.byref(r) if with_rows else None, C.byref(c), P(br), P(dls), M, cols,
                                                P(ws), n, S())

    got = _run_backward(a, launch, need, (gm,), (cs, dls), b"vitssl_layerscale_workspace_floats")
    pm = torch.empty(M, cols, dtype=BF16, device=DEV)
    ops.grad_mask_cast(g.clone(), pm, None, drop)
    rows = s.repeat_interleave(T).view(M, 1)
    want = pm.cpu().float() * rows * gam.cpu().view(1, cols)
    assert bool((got[0][rows[:, 0] == 0].float() == 0).all())
    assert float((got[0].float() - want).abs().max()) <= 2.0 ** -6 * float(want.abs().max()) + 1e-30
    assert float((got[1].double() - want.double().sum(0)).norm()) <= 1e-2 * float(want.double().sum(0).norm()) + 1e-30
    wls = (rows.double() * g.cpu().double() * br.cpu().double()).sum(0)
    assert float((got[2].double() - wls).norm()) <= 1e-4 * float(wls.norm()) + 1e-30
    assert same_bits(g, torch.randn(M, cols, generator=torch.Generator().manual_seed(M)))


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_gemm_ls_on_the_arena)
def test_gemm_ls_on_the_arena_off_stream(B, T, N, K, p, with_rows, mode, offstream):
    offstream(mode, test_gemm_ls_on_the_arena, B, T, N, K, p, with_rows)


@twin_of(test_layernorm_bwd_ls_on_the_arena)
def test_layernorm_bwd_ls_on_the_arena_off_stream(B, T, cols, p, with_rows, mode, offstream):
    offstream(mode, test_layernorm_bwd_ls_on_the_arena, B, T, cols, p, with_rows)


@twin_of(test_grad_mask_cast_ls_on_the_arena)
def test_grad_mask_cast_ls_on_the_arena_off_stream(B, T, cols, p, with_rows, mode, offstream):
    offstream(mode, test_grad_mask_cast_ls_on_the_arena, B, T, cols, p, with_rows)
