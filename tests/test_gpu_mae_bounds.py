"""Every entry point of include_ext/vitssl_mae.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_bce_bounds.py: every input, table, output and an EXACT-size workspace are carved from a 0xFF-poisoned arena.  Per
entry point: no guard byte changes; no NaN poison reaches a result (every output element and every workspace slot is written
before it is read, pad columns of the prediction -- NaN -- are never read); a zero-filled and a 0xFF-filled workspace give the
same bits; the inputs are only read; one float short of the documented workspace is refused.  And each argument refusal of the
header (null operand, non-positive size, K outside [1, N-1], misaligned pointer) returns -1 with a message and writes nothing."""
import ctypes as C

import pytest
import torch

from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)
from vit_core.ssl.mae import masking as Mk

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32


def P(t, off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + off)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def lib():
    from vitssl_hip import _lib as L
    return L.lib()


def clean(t):
    return not torch.isnan(t.float()).any()


def refused(rc):
    assert rc == -1 and lib().vitssl_last_error(), rc
    torch.cuda.synchronize()


def case(B, N, K, D, seed=0):
    g = torch.Generator().manual_seed(seed)
    keep, restore = Mk.draw_keep(B, N, K, generator=g)
    return keep, restore, Mk.MAEIndices(keep, restore, K), g


@pytest.mark.parametrize("B,N,K,D", [(1, 4, 1, 64), (3, 9, 2, 64), (5, 16, 15, 128), (2, 196, 49, 192)], ids=str)
def test_token_kernels_on_the_arena(B, N, K, D):
    l = lib()
    keep, restore, idx, g = case(B, N, K, D)
    a = Arena(DEV, mib=32)
    rnd = lambda *shape: torch.randn(*shape, generator=g)      # noqa: E731
    xk, pos, cls = a.put("xk", rnd(B * K, D)), a.put("pos", rnd(N + 1, D)), a.put("cls", rnd(D))
    keep_d, restore_d = a.put("keep", keep.to(I32)), a.put("restore", restore.to(I32))
    y, mt, dpos = a.put("y", rnd(B * (K + 1), D)), a.put("mask_token", rnd(D)), a.put("dpos", rnd(N + 1, D))
    g1, g2 = a.put("g1", rnd(B * (K + 1), D)), a.put("g2", rnd(B * (N + 1), D))
    out1, out2 = a.empty("out1", (B * (K + 1), D), F32), a.empty("out2", (B * (N + 1), D), F32)
    dproj, dy = a.empty("dproj", (B * K, D), BF16), a.empty("dy", (B * (K + 1), D), BF16)
    sums = [a.zeros(n, (D,), F32) for n in ("dbias1", "dcls", "dbias2", "dmask_token")]
    need1, need2 = int(l.vitssl_sum_workspace_floats(B * (K + 1), D)), int(l.vitssl_sum_workspace_floats(B * (N + 1), D))
    ws1, ws2 = a.empty("ws1", (need1,), F32), a.empty("ws2", (need2,), F32)
    inputs = [xk, pos, cls, keep_d, restore_d, y, mt, dpos, g1, g2]
    before = [t.clone() for t in inputs]

    tb = lambda ws, n: l.vitssl_mae_tokens_bwd(P(g1), P(dproj), P(sums[0]), P(sums[1]), B, N, K, D, P(ws), n, S())                # noqa: E731
    ub = lambda ws, n: l.vitssl_mae_unshuffle_bwd(P(g2), P(restore_d), P(dy), P(sums[2]), P(sums[3]), B, N, K, D, P(ws), n, S())   # noqa: E731
    refused(tb(ws1, need1 - 1))                                 # one float short: refused before anything is launched
    assert b"vitssl_sum_workspace_floats" in l.vitssl_last_error()
    refused(ub(ws2, need2 - 1))
    refused(tb(None, need1))
    assert Arena.untouched(ws1) and Arena.untouched(ws2) and Arena.untouched(dproj) and Arena.untouched(dy) and not any(s.any() for s in sums)

    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws1, fill), Arena.fill(ws2, fill)
        for t in (out1, out2, dproj, dy):
            Arena.fill(t)
        for s in sums:
            Arena.fill(s, 0)
        assert l.vitssl_mae_tokens_fwd(P(xk), P(keep_d), P(pos), P(cls), P(out1), B, N, K, D, S()) == 0, l.vitssl_last_error()
        assert l.vitssl_mae_unshuffle_fwd(P(y), P(restore_d), P(mt), P(dpos), P(out2), B, N, K, D, S()) == 0, l.vitssl_last_error()
        assert tb(ws1, need1) == 0, l.vitssl_last_error()
        assert ub(ws2, need2) == 0, l.vitssl_last_error()
        torch.cuda.synchronize()
        a.check()
        got = [t.cpu().clone() for t in (out1, out2, dproj, dy, *sums)]
        assert all(clean(t) for t in got)
        results.append(got)
    for x, z in zip(*results):
        assert torch.equal(x.view(torch.uint8), z.view(torch.uint8)), "bits depend on what the workspace held"
    for t, b in zip(inputs, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
    # the values (the kernels alone are held to torch bit for bit in tests/test_gpu_mae_kernels.py)
    out1_, out2_, dproj_, dy_, dbias1, dcls, dbias2, dmt = results[0]
    g13, g23 = g1.cpu().view(B, K + 1, D), g2.cpu().view(B, N + 1, D)
    assert torch.equal(out1_.view(B, K + 1, D)[:, 1:], xk.cpu().view(B, K, D) + pos.cpu()[1 + keep])
    assert torch.equal(dproj_, g13[:, 1:].reshape(B * K, D).to(BF16))
    assert torch.allclose(dcls, g13[:, 0].sum(0), atol=1e-4) and torch.allclose(dbias1, g13[:, 1:].sum((0, 1)), atol=1e-3)
    assert torch.allclose(dmt, g23[:, 1:][restore >= K].sum(0), atol=1e-3)
    assert torch.allclose(dbias2 + dmt, g23.sum((0, 1)), atol=2e-3)

    # ---- refusals: -1, a message, nothing written
    for t in (out1, out2, dproj, dy, ws1, ws2):
        Arena.fill(t)
    tf = lambda **k: l.vitssl_mae_tokens_fwd(P(k.get("xk", xk), k.get("off", 0)), P(k.get("keep", keep_d)), P(pos), P(k.get("cls", cls)),   # noqa: E731
                                             P(k.get("out", out1)), k.get("B", B), k.get("N", N), k.get("K", K), k.get("D", D), S())
    uf = lambda **k: l.vitssl_mae_unshuffle_fwd(P(k.get("y", y), k.get("off", 0)), P(k.get("restore", restore_d)), P(mt), P(dpos),          # noqa: E731
                                                P(k.get("out", out2)), k.get("B", B), k.get("N", N), k.get("K", K), k.get("D", D), S())
    for bad in (dict(xk=None), dict(keep=None), dict(cls=None), dict(out=None), dict(B=0), dict(N=0), dict(D=0), dict(D=-4), dict(D=D + 2),
                dict(K=0), dict(K=N), dict(K=N + 3), dict(off=4)):
        refused(tf(**bad))
    for bad in (dict(y=None), dict(restore=None), dict(out=None), dict(B=-1), dict(D=0), dict(K=0), dict(K=N), dict(off=8)):
        refused(uf(**bad))
    refused(l.vitssl_mae_tokens_bwd(P(g1), P(dproj), P(None), P(sums[1]), B, N, K, D, P(ws1), need1, S()))
    refused(l.vitssl_mae_tokens_bwd(P(g1), P(dproj), P(sums[0]), P(sums[1]), B, N, N, D, P(ws1), need1, S()))
    refused(l.vitssl_mae_tokens_bwd(P(g1), P(dproj), P(sums[0]), P(sums[1]), 0, N, K, D, P(ws1), need1, S()))
    refused(l.vitssl_mae_tokens_bwd(P(g1, 4), P(dproj), P(sums[0]), P(sums[1]), B, N, K, D, P(ws1), need1, S()))
    refused(l.vitssl_mae_tokens_bwd(P(g1), P(dproj, 2), P(sums[0]), P(sums[1]), B, N, K, D, P(ws1), need1, S()))
    refused(l.vitssl_mae_unshuffle_bwd(P(g2), P(None), P(dy), P(sums[2]), P(sums[3]), B, N, K, D, P(ws2), need2, S()))
    refused(l.vitssl_mae_unshuffle_bwd(P(g2), P(restore_d), P(dy), P(sums[2]), P(sums[3]), B, N, 0, D, P(ws2), need2, S()))
    refused(l.vitssl_mae_unshuffle_bwd(P(g2), P(restore_d), P(dy), P(sums[2]), P(sums[3]), B, N, K, 0, P(ws2), need2, S()))
    refused(l.vitssl_mae_unshuffle_bwd(P(g2, 4), P(restore_d), P(dy), P(sums[2]), P(sums[3]), B, N, K, D, P(ws2), need2, S()))
    refused(l.vitssl_mae_unshuffle_bwd(P(g2), P(restore_d), P(dy, 4), P(sums[2]), P(sums[3]), B, N, K, D, P(ws2), need2, S()))
    assert all(Arena.untouched(t) for t in (out1, out2, dproj, dy, ws1, ws2))
    for s, v in zip(sums, results[0][4:]):
        assert torch.equal(s.cpu(), v)
    a.check()


@pytest.mark.parametrize("norm_pix", [1, 0], ids=["norm_pix", "raw"])
@pytest.mark.parametrize("Mm,Pd,ld,Pdp", [(1, 2, 2, 64), (33, 588, 592, 640), (130, 768, 768, 768), (5, 9, 12, 64), (3, 4100, 4100, 4160)], ids=str)
def test_loss_on_the_arena(Mm, Pd, ld, Pdp, norm_pix):
    l = lib()
    g = torch.Generator().manual_seed(Pd)
    a = Arena(DEV, mib=32)
    wide = torch.full((Mm, ld), float("nan"))                   # pad columns of the prediction: never read
    wide[:, :Pd] = torch.randn(Mm, Pd, generator=g)
    raw = torch.rand(Mm, Pd, generator=g)
    pred, tgt = a.put("pred", wide), a.empty("target", (Mm, Pd), F32)
    loss, dp = a.zeros("loss", (1,), F32), a.empty("dpred", (Mm, Pdp), BF16)
    need = int(l.vitssl_sum_workspace_floats(Mm, Pd))
    ws = a.empty("workspace", (need,), F32)
    run = lambda **k: l.vitssl_mae_loss(P(k.get("pred", pred), k.get("off", 0)), k.get("ld", ld), P(k.get("tgt", tgt)), P(k.get("loss", loss)),      # noqa: E731
                                        P(k.get("dp", dp), k.get("dpoff", 0)), k.get("Mm", Mm), k.get("Pd", Pd), k.get("Pdp", Pdp), norm_pix, 1.0 / Mm,
                                        P(k.get("ws", ws)), k.get("need", need), S())
    tgt.copy_(raw)
    refused(run(need=need - 1))
    assert b"vitssl_sum_workspace_floats" in l.vitssl_last_error()
    assert Arena.untouched(ws) and Arena.untouched(dp) and not loss.any() and torch.equal(tgt.cpu(), raw)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill), Arena.fill(dp), Arena.fill(loss, 0)
        tgt.copy_(raw)
        assert run() == 0, l.vitssl_last_error()
        torch.cuda.synchronize()
        a.check()
        got = [loss.cpu().clone(), dp.cpu().clone(), tgt.cpu().clone()]
        assert all(clean(t) for t in got) and not got[1][:, Pd:].view(torch.int16).any()
        results.append(got)
    for x, z in zip(*results):
        assert torch.equal(x.view(torch.uint8), z.view(torch.uint8)), "bits depend on what the workspace held"
    assert torch.equal(pred.cpu().view(torch.int32), wide.view(torch.int32))
    if not norm_pix:
        assert torch.equal(results[0][2], raw)
    want = float(((wide[:, :Pd].double() - results[0][2].double()) ** 2).mean(-1).sum())      # against the targets it left
    assert abs(float(results[0][0]) - want) < 1e-5 * want
    # refusals
    Arena.fill(dp), Arena.fill(ws), Arena.fill(loss, 0)
    tgt.copy_(raw)
    bads = [dict(pred=None), dict(tgt=None), dict(loss=None), dict(ws=None), dict(Mm=0), dict(Pd=0), dict(Pd=-1), dict(ld=Pd - 1), dict(Pdp=Pd - 1 if Pd > 4 else 2),
            dict(Pdp=Pdp + 2), dict(dpoff=2)]
    if Pd % 4 == 0 and ld % 4 == 0:
        bads.append(dict(off=4))                                # it vectorises there: a misaligned pointer is refused
    for bad in bads:
        refused(run(**bad))
    if norm_pix:
        refused(run(Pd=1, ld=ld))                               # the unbiased variance of one value
        assert b"norm_pix" in l.vitssl_last_error()
    assert Arena.untouched(dp) and Arena.untouched(ws) and not loss.any() and torch.equal(tgt.cpu(), raw)
    a.check()


@pytest.mark.parametrize("B,N,K,D", [(1, 4, 1, 64), (3, 9, 2, 64), (2, 196, 49, 192)], ids=str)
def test_rows_by_index_on_the_arena(B, N, K, D):
    l = lib()
    keep, restore, idx, g = case(B, N, K, D, seed=3)
    a = Arena(DEV, mib=32)
    patches = a.put("patches", torch.randn(B * N, D, generator=g).to(BF16))
    tokens = a.put("tokens", torch.randn(B * (N + 1), D, generator=g))
    kr, mrows, inv = (a.put(n, torch.from_numpy(getattr(idx, n))) for n in ("keep_rows", "mrows", "inv"))
    kept, sel, back = a.empty("kept", (B * K, D), BF16), a.empty("sel", (idx.Mm, D), F32), a.empty("back", (B * (N + 1), D), F32)
    gb = lambda **k: l.vitssl_mae_gather_rows_bf16(P(k.get("src", patches), k.get("off", 0)), P(k.get("idx", kr)), P(k.get("out", kept)),      # noqa: E731
                                                   k.get("n", B * K), k.get("cols", D), S())
    gf = lambda **k: l.vitssl_mae_gather_rows_f32(P(k.get("src", tokens)), P(k.get("idx", mrows)), P(k.get("out", sel), k.get("off", 0)),      # noqa: E731
                                                  k.get("n", idx.Mm), k.get("cols", D), S())
    sc = lambda **k: l.vitssl_mae_scatter_rows_f32(P(k.get("src", sel)), P(k.get("idx", inv)), P(k.get("out", back), k.get("off", 0)),         # noqa: E731
                                                   k.get("n", B * (N + 1)), k.get("cols", D), S())
    for f in (gb, gf, sc):
        for bad in (dict(src=None), dict(idx=None), dict(out=None), dict(n=0), dict(n=-2), dict(cols=0), dict(cols=D + 2), dict(off=4)):
            refused(f(**bad))
    refused(gb(cols=D + 4))                                     # bf16 rows move as 8 elements
    assert Arena.untouched(kept) and Arena.untouched(sel) and Arena.untouched(back)
    assert gb() == 0 and gf() == 0, l.vitssl_last_error()
    assert sc() == 0, l.vitssl_last_error()
    torch.cuda.synchronize()
    a.check()
    assert clean(kept) and clean(sel) and clean(back)
    assert torch.equal(kept.cpu(), patches.cpu()[torch.from_numpy(idx.keep_rows).long()])
    m = torch.from_numpy(idx.mrows).long()
    assert torch.equal(sel.cpu(), tokens.cpu()[m])
    want = torch.zeros(B * (N + 1), D)
    want[m] = tokens.cpu()[m]
    assert torch.equal(back.cpu(), want)


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_token_kernels_on_the_arena)
def test_token_kernels_on_the_arena_off_stream(B, N, K, D, mode, offstream):
    offstream(mode, test_token_kernels_on_the_arena, B, N, K, D)


@twin_of(test_loss_on_the_arena)
def test_loss_on_the_arena_off_stream(Mm, Pd, ld, Pdp, norm_pix, mode, offstream):
    offstream(mode, test_loss_on_the_arena, Mm, Pd, ld, Pdp, norm_pix)


@twin_of(test_rows_by_index_on_the_arena)
def test_rows_by_index_on_the_arena_off_stream(B, N, K, D, mode, offstream):
    offstream(mode, test_rows_by_index_on_the_arena, B, N, K, D)
