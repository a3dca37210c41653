"""The four entry points of include/vitssl_droppath.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_mixup_bounds.py: every input, table, output and an EXACT-size workspace are carved from a 0xFF-poisoned arena.  Per
case: no guard byte changes; no NaN poison reaches a result (every output element is written, every workspace slot is written
before it is read, the guards around the table of scales are never read into a result); a zero-filled and a 0xFF-filled workspace
give the same bits; one float short of the documented workspace is refused before anything is launched; inputs are only read."""
import ctypes as C

import numpy as np
import pytest
import torch

import _droppath_ref as DP
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)

DEV = torch.device("cuda:0")
F32, BF16 = torch.float32, torch.bfloat16
gpu = pytest.mark.gpu


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    return torch.equal(a.cpu().reshape(-1).view(torch.uint8), b.cpu().reshape(-1).view(torch.uint8))


def mixed_scales(B, rate=0.5):
    for seed in range(1, 1000):
        s = DP.path_scales(B, rate, seed, DP.site(0, 1))
        if B == 1 or ((s == 0).any() and (s != 0).any()):
            return torch.from_numpy(s)
    raise AssertionError("no seed found")


@gpu
@pytest.mark.parametrize("sites,B", [(1, 1), (6, 5), (128, 257)], ids=str)
def test_table_on_the_arena(sites, B):
    from vitssl_hip import _lib as L
    a = Arena(DEV, mib=8)
    out = a.empty("scale", (sites, B), F32)
    rates = (C.c_float * sites)(*[0.5 * (j % 3) / 2 for j in range(sites)])
    ids = (C.c_uint32 * sites)(*[DP.site(j // 2, j % 2) for j in range(sites)])
    L.call("vitssl_droppath_table", P(out), rates, ids, sites, B, C.c_uint64(77), S())
    torch.cuda.synchronize()
    a.check()
    want = np.stack([DP.path_scales(B, rates[j], 77, ids[j]) for j in range(sites)])
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))


@gpu
@pytest.mark.parametrize("p", [0.0, 0.5], ids=["nodrop", "drop0.5"])
@pytest.mark.parametrize("B,T,N,K", [(16, 17, 192, 64), (3, 197, 260, 128), (1, 1, 4, 64), (30, 197, 768, 64)], ids=str)
def test_gemm_rows_on_the_arena(B, T, N, K, p):
    """the guards around the [B] table are NaN: a read outside it that reached a result would show in `out`"""
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    M = B * T
    g = torch.Generator().manual_seed(M + N)
    a = Arena(DEV, mib=128)
    A = a.put("A", torch.randn(M, K, generator=g).to(BF16))
    Bm = a.put("B", torch.randn(N, K, generator=g).to(BF16))
    bias, res = a.put("bias", torch.randn(N, generator=g)), a.put("aux", torch.randn(M, N, generator=g))
    s = mixed_scales(B)
    sc = a.put("scale", s)
    out = a.empty("out0", (M, N), F32)
    gm = L.Gemm()
    gm.A, gm.B, gm.M, gm.N, gm.K, gm.epilogue = A.data_ptr(), Bm.data_ptr(), M, N, K, L.EPI_RESID
    gm.bias, gm.aux, gm.out0 = bias.data_ptr(), res.data_ptr(), out.data_ptr()
    gm.drop = ops.make_dropout(p, seed=3, site=5)
    r = L.RowScale(sc.data_ptr(), B, T)
    before = [t.clone() for t in (A, Bm, bias, res, sc)]
    L.call("vitssl_gemm_bf16_nt_rows", C.byref(gm), C.byref(r), S())
    torch.cuda.synchronize()
    a.check()
    assert not torch.isnan(out).any()
    # against the plain launch on ordinary tensors: kept rows scale the branch, dropped rows are the residual's bits
    plain = torch.empty(M, N, device=DEV)
    ops.gemm_nt(A.clone(), Bm.clone(), plain, L.EPI_RESID, bias=bias.clone(), aux=torch.zeros(M, N, device=DEV), drop=gm.drop)
    rows = s.repeat_interleave(T).view(M, 1).to(DEV)
    want = res.double() + rows.double() * plain.double()
    assert float((out.double() - want).abs().max()) <= 2e-6 * float(want.abs().max())
    dropped = (rows[:, 0] == 0)
    assert same_bits(out[dropped], res[dropped])
    for t, b in zip((A, Bm, bias, res, sc), before):
        assert same_bits(t, b)


def _ln_case(a, M, cols, seed):
    from vitssl_hip import ops
    g = torch.Generator().manual_seed(seed)
    x = a.put("x", torch.randn(M, cols, generator=g))
    gamma = a.put("gamma", 1 + 0.1 * torch.randn(cols, generator=g))
    dy = a.put("dy", torch.randn(M, cols, generator=g).to(BF16))
    g_res = a.put("g_res", torch.randn(M, cols, generator=g))
    mean, rstd = a.empty("mean", (M,), F32), a.empty("rstd", (M,), F32)
    ops.layernorm_fwd(x, gamma, torch.zeros(cols, device=DEV), torch.empty(M, cols, dtype=BF16, device=DEV), mean, rstd)
    return x, gamma, dy, g_res, mean, rstd


@gpu
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,cols", [(16, 17, 384), (3, 197, 384), (3, 197, 768), (1, 1, 4), (5, 33, 260), (2, 40, 2048), (600, 7, 384)], ids=str)
def test_layernorm_bwd_rows_on_the_arena(B, T, cols, p):
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    M = B * T
    a = Arena(DEV, mib=128)
    x, gamma, dy, g_res, mean, rstd = _ln_case(a, M, cols, M + cols)
    s = mixed_scales(B, 0.3)
    sc = a.put("scale", s)
    g_out, gm = a.empty("g_out", (M, cols), F32), a.empty("gm", (M, cols), BF16)
    dg, db, cs = a.empty("dgamma", (cols,), F32), a.empty("dbeta", (cols,), F32), a.empty("gm_colsum", (cols,), F32)
    need = int(L.lib().vitssl_sum_workspace_floats(M, cols))
    ws = a.empty("workspace", (need,), F32)
    drop = ops.make_dropout(p, seed=9, site=1)
    r = L.RowScale(sc.data_ptr(), B, T)

    def launch(n):
        return L.lib().vitssl_layernorm_bwd_rows(P(dy), P(x), P(mean), P(rstd), P(gamma), P(g_res), P(g_out), P(gm), P(dg), P(db), P(cs), drop,
                                                 C.byref(r), M, cols, P(ws), n, S())

    assert launch(need - 1) == -1 and b"vitssl_sum_workspace_floats" in L.lib().vitssl_last_error()      # one float short: refused
    torch.cuda.synchronize()
    assert Arena.untouched(ws) and Arena.untouched(g_out) and Arena.untouched(gm)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill)
        for t in (g_out, gm):
            Arena.fill(t)
        for t in (dg, db, cs):
            Arena.fill(t, 0)
        assert launch(need) == 0, L.lib().vitssl_last_error()
        torch.cuda.synchronize()
        a.check()
        got = [t.cpu().clone() for t in (g_out, gm, dg, db, cs)]
        assert not any(torch.isnan(t.float()).any() for t in got)
        results.append(got)
    for u, v in zip(*results):
        assert same_bits(u, v), "bits depend on what the workspace held"
    # against the plain entry on ordinary tensors
    po, pm = torch.empty(M, cols, device=DEV), torch.empty(M, cols, dtype=BF16, device=DEV)
    pg, pb = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
    ops.layernorm_bwd(dy.clone(), x.clone(), mean.clone(), rstd.clone(), gamma.clone(), g_res.clone(), po, pm, pg, pb, None, drop)
    assert same_bits(results[0][0], po) and same_bits(results[0][2], pg) and same_bits(results[0][3], pb)
    rows = s.repeat_interleave(T).view(M, 1)
    dropped = rows[:, 0] == 0
    assert bool((results[0][1][dropped].float() == 0).all())                 # a dropped sample contributes exact zeros
    want = (pm.cpu().float() * rows)
    assert float((results[0][1].float() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max()) + 1e-30


@gpu
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("B,T,cols", [(16, 17, 384), (3, 197, 768), (1, 1, 4), (5, 33, 260), (2, 40, 2048)], ids=str)
def test_grad_mask_cast_rows_on_the_arena(B, T, cols, p):
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    M = B * T
    a = Arena(DEV, mib=64)
    g = a.put("g", torch.randn(M, cols, generator=torch.Generator().manual_seed(M)))
    s = mixed_scales(B, 0.3)
    sc = a.put("scale", s)
    gm, cs = a.empty("gm", (M, cols), BF16), a.empty("gm_colsum", (cols,), F32)
    need = int(L.lib().vitssl_sum_workspace_floats(M, cols))
    ws = a.empty("workspace", (need,), F32)
    drop = ops.make_dropout(p, seed=10, site=2)
    r = L.RowScale(sc.data_ptr(), B, T)

    def launch(n):
        return L.lib().vitssl_grad_mask_cast_rows(P(g), P(gm), P(cs), drop, C.byref(r), M, cols, P(ws), n, S())

    assert launch(need - 1) == -1 and b"vitssl_sum_workspace_floats" in L.lib().vitssl_last_error()
    torch.cuda.synchronize()
    assert Arena.untouched(ws) and Arena.untouched(gm)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill)
        Arena.fill(gm)
        Arena.fill(cs, 0)
        assert launch(need) == 0, L.lib().vitssl_last_error()
        torch.cuda.synchronize()
        a.check()
        got = [gm.cpu().clone(), cs.cpu().clone()]
        assert not any(torch.isnan(t.float()).any() for t in got)
        results.append(got)
    for u, v in zip(*results):
        assert same_bits(u, v)
    pm = torch.empty(M, cols, dtype=BF16, device=DEV)
    ops.grad_mask_cast(g.clone(), pm, None, drop)
    rows = s.repeat_interleave(T).view(M, 1)
    want = pm.cpu().float() * rows
    assert bool((results[0][0][rows[:, 0] == 0].float() == 0).all())
    assert float((results[0][0].float() - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max()) + 1e-30
    assert float((results[0][1].double() - want.double().sum(0)).norm()) <= 1e-2 * float(want.double().sum(0).norm()) + 1e-30
    assert same_bits(g, torch.randn(M, cols, generator=torch.Generator().manual_seed(M)))


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_table_on_the_arena)
def test_table_on_the_arena_off_stream(sites, B, mode, offstream):
    offstream(mode, test_table_on_the_arena, sites, B)


@twin_of(test_gemm_rows_on_the_arena)
def test_gemm_rows_on_the_arena_off_stream(B, T, N, K, p, mode, offstream):
    offstream(mode, test_gemm_rows_on_the_arena, B, T, N, K, p)


@twin_of(test_layernorm_bwd_rows_on_the_arena)
def test_layernorm_bwd_rows_on_the_arena_off_stream(B, T, cols, p, mode, offstream):
    offstream(mode, test_layernorm_bwd_rows_on_the_arena, B, T, cols, p)


@twin_of(test_grad_mask_cast_rows_on_the_arena)
def test_grad_mask_cast_rows_on_the_arena_off_stream(B, T, cols, p, mode, offstream):
    offstream(mode, test_grad_mask_cast_rows_on_the_arena, B, T, cols, p)
