"""vitssl_classify_bce on guarded-arena tensors (tests/_arena.py), in the manner of tests/test_gpu_classify_bounds.py and
tests/test_gpu_mixup_bounds.py: every input, table, output and an EXACT-size workspace are carved from a 0xFF-poisoned arena.
Per case: one float short of the documented workspace is refused before anything is launched; no guard byte changes; no NaN
poison reaches a result (every output element and every workspace slot is written before it is read, the padding columns of
the logits -- NaN -- are never read); a zero-filled and a 0xFF-filled workspace give the same bits; the result equals the
restatement; the inputs are only read."""
import ctypes as C

import numpy as np
import pytest
import torch

import _bce_ref as Bc
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)
from test_gpu_bce import check

DEV = torch.device("cuda:0")
F32, BF16, I64, I32 = torch.float32, torch.bfloat16, torch.int64, torch.int32
gpu = pytest.mark.gpu


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@gpu
@pytest.mark.parametrize("grad", [True, False], ids=["dlogits", "null"])
@pytest.mark.parametrize("two", [False, True], ids=["one-label", "two-label"])
@pytest.mark.parametrize("B,Cn,ld,ld_out", [(1, 2, 64, 64), (33, 10, 64, 128), (5, 1027, 1088, 1088)], ids=str)
def test_classify_bce_on_the_arena(B, Cn, ld, ld_out, two, grad):
    from vitssl_hip import _lib as L
    z, y, partner, lam, _ = Bc.make_mix_case(B, Cn, ld, rot=2)
    if B > 8:
        partner[5], partner[8], lam[6] = -1, 2 ** 31 - 1, np.nan             # bad rows: nothing is read through them
        y[9] = 2 ** 40
    a = Arena(DEV, mib=16)
    zd, yd = a.put("logits", torch.from_numpy(z)), a.put("labels", torch.from_numpy(y))
    pd = a.put("partner", torch.from_numpy(partner)) if two else None
    ld_ = a.put("lam", torch.from_numpy(lam)) if two else None
    loss, pred = a.empty("loss_out", (2,), F32), a.empty("pred", (B,), I64)
    counters, bad = a.zeros("counters", (2,), I64), a.zeros("bad_labels", (1,), I32)
    dl = a.empty("dlogits", (B, ld_out), BF16) if grad else None
    db = a.zeros("dbias", (Cn,), F32) if grad else None
    need = int(L.lib().vitssl_classify_bce_workspace_floats(B, Cn))
    assert need == (2 * B + 3) // 4 * 4 + B * ((Cn + 3) // 4 * 4)            # the documented size
    ws = a.empty("workspace", (need,), F32)

    def launch(ws_floats):
        return L.lib().vitssl_classify_bce(P(zd), P(yd), P(pd), P(ld_), B, Cn, ld, 0.1, -1.0, 0, Bc.IGNORE, 1.0, P(loss), P(dl), ld_out, P(db),
                                           P(pred), P(counters), P(bad), P(ws), ws_floats, S())

    assert launch(need - 1) == -1                                            # one float short: refused before anything is launched
    assert b"vitssl_classify_bce_workspace_floats" in L.lib().vitssl_last_error()
    torch.cuda.synchronize()
    assert Arena.untouched(ws) and Arena.untouched(loss) and Arena.untouched(pred)
    ref = Bc.reference(z, y, Cn, 0.1, partner if two else None, lam if two else None)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill)
        for t in (loss, pred) + ((dl,) if grad else ()):
            Arena.fill(t)
        for t in (counters, bad) + ((db,) if grad else ()):
            Arena.fill(t, 0)
        counters += torch.tensor(Bc.COUNTERS0, device=DEV)
        bad += Bc.BAD0
        if grad:
            db += Bc.dbias0(Cn)
        assert launch(need) == 0, L.lib().vitssl_last_error()
        torch.cuda.synchronize()
        a.check()
        got = dict(loss=loss.cpu().clone(), pred=pred.cpu().clone(), counters=counters.cpu().clone(), bad=bad.cpu().clone())
        if grad:
            got.update(dlogits=dl.cpu().clone(), dbias=db.cpu().clone())
            assert not torch.isnan(got["dlogits"].float()).any() and not torch.isnan(got["dbias"]).any()
        assert not torch.isnan(got["loss"]).any()
        results.append(got)
    for k in results[0]:
        assert torch.equal(results[0][k].view(torch.uint8), results[1][k].view(torch.uint8)), f"{k}: bits depend on what the workspace held"
    check(ref, results[0], z, Cn, grad=grad, what=f"arena (B,C)=({B},{Cn})")
    assert torch.equal(zd.cpu().view(torch.int32), torch.from_numpy(z).view(torch.int32)) and torch.equal(yd.cpu(), torch.from_numpy(y))
    if two:
        assert torch.equal(pd.cpu(), torch.from_numpy(partner)) and torch.equal(ld_.cpu().view(torch.int32), torch.from_numpy(lam).view(torch.int32))


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_classify_bce_on_the_arena)
def test_classify_bce_on_the_arena_off_stream(B, Cn, ld, ld_out, two, grad, mode, offstream):
    offstream(mode, test_classify_bce_on_the_arena, B, Cn, ld, ld_out, two, grad)
