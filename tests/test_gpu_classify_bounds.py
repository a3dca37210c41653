"""vitssl_classify_loss on guarded-arena tensors (tests/_arena.py), in the manner of tests/test_gpu_metrics_bounds.py: logits,
labels, every output and an EXACT-size workspace are carved from a 0xFF-poisoned arena.  Per case: no guard byte changes; no
NaN poison reaches a result (every workspace slot is written before it is read, the padding columns of the logits -- NaN --
are never read); a zero-filled and a 0xFF-filled workspace give the same bits; the result equals the fp64 restatement."""
import ctypes as C

import pytest
import torch

import _classify_ref as R
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)
from test_gpu_classify import check_against

DEV = torch.device("cuda:0")
F32, BF16, I64, I32 = torch.float32, torch.bfloat16, torch.int64, torch.int32
gpu = pytest.mark.gpu


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@gpu
@pytest.mark.parametrize("grad", [True, False], ids=["dlogits", "null"])
@pytest.mark.parametrize("B,Cn", [(1, 2), (33, 10)], ids=str)
def test_classify_loss_on_the_arena(B, Cn, grad):
    from vitssl_hip import _lib as L
    z, y, _ = R.make_case(B, Cn, 64)
    a = Arena(DEV, mib=16)
    zd, yd = a.put("logits", torch.from_numpy(z)), a.put("labels", torch.from_numpy(y))
    loss, pred = a.empty("loss_out", (2,), F32), a.empty("pred", (B,), I64)
    counters, bad = a.zeros("counters", (2,), I64), a.zeros("bad_labels", (1,), I32)
    dl = a.empty("dlogits", (B, 64), BF16) if grad else None
    db = a.zeros("dbias", (Cn,), F32) if grad else None
    need = int(L.lib().vitssl_classify_loss_workspace_floats(B, Cn))
    ws = a.empty("workspace", (need,), F32)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill)
        for t in (loss, pred) + ((dl,) if grad else ()):
            Arena.fill(t)
        for t in (counters, bad) + ((db,) if grad else ()):
            Arena.fill(t, 0)
        counters += torch.tensor([5, 9], device=DEV)
        L.call("vitssl_classify_loss", P(zd), P(yd), B, Cn, 64, 0.1, R.IGNORE, 1.0, P(loss), P(dl), 64, P(db), P(pred), P(counters), P(bad),
               P(ws), need, S())
        torch.cuda.synchronize()
        a.check()
        got = dict(loss=loss.cpu().clone(), pred=pred.cpu().clone(), counters=counters.cpu().clone(), bad=bad.cpu().clone())
        if grad:
            got.update(dlogits=dl.cpu().clone(), dbias=db.cpu().clone())
            assert not torch.isnan(got["dlogits"].float()).any() and not torch.isnan(got["dbias"]).any()
        assert not torch.isnan(got["loss"]).any() and got["bad"].tolist() == [0]
        results.append(got)
    for k in results[0]:
        assert torch.equal(results[0][k].view(torch.uint8), results[1][k].view(torch.uint8)), f"{k}: bits depend on what the workspace held"
    check_against(R.reference(z, y, Cn, 0.1), results[0], z, y, Cn, 0.1, grad=grad)
    assert torch.equal(zd.cpu().view(torch.int32), torch.from_numpy(z).view(torch.int32)) and torch.equal(yd.cpu(), torch.from_numpy(y))


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_classify_loss_on_the_arena)
def test_classify_loss_on_the_arena_off_stream(B, Cn, grad, mode, offstream):
    offstream(mode, test_classify_loss_on_the_arena, B, Cn, grad)
