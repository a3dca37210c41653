"""vitssl_mix_batch and vitssl_classify_loss_mix on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_classify_bounds.py: every input, table, output and an EXACT-size workspace are carved from a 0xFF-poisoned
arena.  Per case: no guard byte changes; no NaN poison reaches a result (every output element and every workspace slot is
written before it is read, the padding columns of the logits -- NaN -- are never read); a zero-filled and a 0xFF-filled
workspace give the same bits; the result equals the restatement; the inputs are only read."""
import ctypes as C

import numpy as np
import pytest
import torch

import _mixup_ref as M
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)
from test_gpu_classify_mix import check_mix
from test_gpu_mixup import check

DEV = torch.device("cuda:0")
F32, BF16, I64, I32 = torch.float32, torch.bfloat16, torch.int64, torch.int32
gpu = pytest.mark.gpu


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@gpu
@pytest.mark.parametrize("B,Cn,H,W", [(5, 3, 32, 32), (3, 4, 9, 5), (4, 1, 7, 30)], ids=str)
def test_mix_batch_on_the_arena(B, Cn, H, W):
    from vitssl_hip import _lib as L
    x = M.mix_input(B, Cn, H, W)
    a = Arena(DEV, mib=16)
    xd = a.put("x", torch.from_numpy(x))
    out = a.empty("out", (B, Cn, H, W), F32)
    ipd, lamd = a.empty("iparams", (B, 6), I32), a.empty("lam", (B,), F32)
    tables = M.mix_tables(B, H, W)[:4]
    wild = tables[0][0].copy()                                               # a table nobody sanitised: the kernel clamps it
    wild[:, 1] = [-1, B, 2 ** 31 - 1, -(2 ** 31), 0][:B]
    wild[:, 2:] = [-(2 ** 31), 2 ** 31 - 1, -7, 2 ** 31 - 1]
    wild[:, 0] = [2, 2, 1, 9, 2][:B]
    for ip, lam in tables + [(wild, tables[0][1])]:
        ipd.copy_(torch.from_numpy(ip))
        lamd.copy_(torch.from_numpy(lam))
        Arena.fill(out)
        L.call("vitssl_mix_batch", P(xd), P(out), P(ipd), P(lamd), B, Cn, H, W, S())
        torch.cuda.synchronize()
        a.check()
        check(x, ip, lam, out.cpu().numpy())
    assert torch.equal(xd.cpu().view(torch.int32), torch.from_numpy(x).view(torch.int32))


@gpu
@pytest.mark.parametrize("grad", [True, False], ids=["dlogits", "null"])
@pytest.mark.parametrize("B,Cn", [(1, 2), (33, 10)], ids=str)
def test_classify_loss_mix_on_the_arena(B, Cn, grad):
    from vitssl_hip import _lib as L
    z, y, partner, lam, _ = M.make_loss_case(B, Cn, 64, rot=2)
    if B > 8:
        partner[5], partner[8], lam[6] = -1, 2 ** 31 - 1, np.nan             # bad rows: nothing is read through them
    a = Arena(DEV, mib=16)
    zd, yd = a.put("logits", torch.from_numpy(z)), a.put("labels", torch.from_numpy(y))
    pd, ld_ = a.put("partner", torch.from_numpy(partner)), a.put("lam", torch.from_numpy(lam))
    loss, pred = a.empty("loss_out", (2,), F32), a.empty("pred", (B,), I64)
    counters, bad = a.zeros("counters", (2,), I64), a.zeros("bad_labels", (1,), I32)
    dl = a.empty("dlogits", (B, 64), BF16) if grad else None
    db = a.zeros("dbias", (Cn,), F32) if grad else None
    need = int(L.lib().vitssl_classify_loss_mix_workspace_floats(B, Cn))
    ws = a.empty("workspace", (need,), F32)

    def launch(ws_floats):
        return L.lib().vitssl_classify_loss_mix(P(zd), P(yd), P(pd), P(ld_), B, Cn, 64, 0.1, M.IGNORE, 1.0, P(loss), P(dl), 64, P(db), P(pred),
                                                P(counters), P(bad), P(ws), ws_floats, S())

    assert launch(need - 1) == -1                                            # one float short: refused before anything is launched
    assert b"vitssl_classify_loss_mix_workspace_floats" in L.lib().vitssl_last_error()
    torch.cuda.synchronize()
    assert Arena.untouched(ws) and Arena.untouched(loss) and Arena.untouched(pred)
    ref = M.loss_reference(z, y, partner, lam, Cn, 0.1)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill)
        for t in (loss, pred) + ((dl,) if grad else ()):
            Arena.fill(t)
        for t in (counters, bad) + ((db,) if grad else ()):
            Arena.fill(t, 0)
        counters += torch.tensor([5, 9], device=DEV)
        assert launch(need) == 0, L.lib().vitssl_last_error()
        torch.cuda.synchronize()
        a.check()
        got = dict(loss=loss.cpu().clone(), pred=pred.cpu().clone(), counters=counters.cpu().clone(), bad=bad.cpu().clone())
        if grad:
            got.update(dlogits=dl.cpu().clone(), dbias=db.cpu().clone())
            assert not torch.isnan(got["dlogits"].float()).any() and not torch.isnan(got["dbias"]).any()
        assert not torch.isnan(got["loss"]).any() and got["bad"].tolist() == [ref["n_bad"]]
        results.append(got)
    for k in results[0]:
        assert torch.equal(results[0][k].view(torch.uint8), results[1][k].view(torch.uint8)), f"{k}: bits depend on what the workspace held"
    check_mix(ref, results[0], z, y, partner, lam, Cn, 0.1, grad=grad, dbias0=0.0, bad0=0)
    assert torch.equal(zd.cpu().view(torch.int32), torch.from_numpy(z).view(torch.int32)) and torch.equal(yd.cpu(), torch.from_numpy(y))
    assert torch.equal(pd.cpu(), torch.from_numpy(partner)) and torch.equal(ld_.cpu().view(torch.int32), torch.from_numpy(lam).view(torch.int32))


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_mix_batch_on_the_arena)
def test_mix_batch_on_the_arena_off_stream(B, Cn, H, W, mode, offstream):
    offstream(mode, test_mix_batch_on_the_arena, B, Cn, H, W)


@twin_of(test_classify_loss_mix_on_the_arena)
def test_classify_loss_mix_on_the_arena_off_stream(B, Cn, grad, mode, offstream):
    offstream(mode, test_classify_loss_mix_on_the_arena, B, Cn, grad)
