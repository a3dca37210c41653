"""The two launching entry points of include/vitssl_metrics.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_abi_bounds.py: inputs, accumulator / output and an EXACT-size workspace are carved from a 0xFF-poisoned arena.
Per case: no guard byte changes; no NaN poison reaches a result (every workspace slot is written before it is read, no input
is read past its end); a zero-filled and a 0xFF-filled workspace give the same bits; the result equals the fp64 restatement
(bars of tests/test_gpu_metrics.py)."""
import ctypes as C

import pytest
import torch

import _metrics_ref as R
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)
from test_gpu_metrics import DINO_TOL, RECON_BAR, close, dino_inputs

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
gpu = pytest.mark.gpu


def P(t):
    return C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@gpu
@pytest.mark.parametrize("Pp,Cc,n", [(6, 1, 1), (8, 3, 5), (16, 3, 67), (7, 3, 5)], ids=str)
def test_recon_metrics_on_the_arena(Pp, Cc, n):
    from vitssl_hip import _lib as L
    pred, target = R.recon_inputs(8 if Pp == 7 else Pp, Cc, n)
    pred, target = pred[:, :Cc * Pp * Pp].contiguous(), target[:, :Cc * Pp * Pp].contiguous()
    a = Arena(DEV, mib=16)
    p, t = a.put("pred", pred), a.put("target", target)
    acc = a.zeros("acc", (4,), F64)
    need = int(L.lib().vitssl_recon_metrics_workspace_floats(n, Cc, Pp))
    ws = a.empty("workspace", (need,), F32)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill)
        Arena.fill(acc, 0)
        L.call("vitssl_recon_metrics", P(p), P(t), P(acc), n, Cc, Pp, P(ws), need, S())
        torch.cuda.synchronize()
        a.check()
        assert not torch.isnan(acc).any()
        results.append(acc.cpu().clone())
    assert torch.equal(results[0], results[1]), "bits depend on what the workspace held before the call"
    want = R.recon_sums(pred, target, Cc, Pp)
    got = results[0].tolist()
    assert close(got[0], want[0], RECON_BAR) and close(got[1], want[1], RECON_BAR) and got[2:] == [n * Cc * Pp * Pp, n]
    assert torch.equal(p.cpu(), pred) and torch.equal(t.cpu(), target)      # inputs are inputs


@gpu
@pytest.mark.parametrize("G,V,B,K", [(2, 2, 1, 4), (1, 3, 5, 1000), (3, 16, 2, 8200)], ids=str)
def test_dino_stats_on_the_arena(G, V, B, K):
    from utils.gpu_metrics import dino_values
    from vitssl_hip import _lib as L
    teacher, student, center = dino_inputs(G, V, B, K, "random")
    a = Arena(DEV, mib=32)
    t, s, c = a.put("teacher", teacher), a.put("student", student), a.put("center", center)
    out = a.empty("out", (8,), F64)
    need = int(L.lib().vitssl_dino_stats_workspace_floats(G, V, B, K))
    ws = a.empty("workspace", (need,), F32)
    results = []
    for fill in (0xFF, 0x00):
        Arena.fill(ws, fill)
        Arena.fill(out)
        L.call("vitssl_dino_stats", P(t), P(s), P(c), P(out), G, V, B, K, P(ws), need, S())
        torch.cuda.synchronize()
        a.check()
        assert not torch.isnan(out).any()
        results.append(out.cpu().clone())
    assert torch.equal(results[0], results[1]), "bits depend on what the workspace held before the call"
    got, want = dino_values(results[0], G * V * B), R.dino_metrics(teacher, student, center)
    for name, tol in DINO_TOL.items():
        assert close(got[name], want[name], tol), name
    assert torch.equal(t.cpu(), teacher) and torch.equal(s.cpu(), student)


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_recon_metrics_on_the_arena)
def test_recon_metrics_on_the_arena_off_stream(Pp, Cc, n, mode, offstream):
    offstream(mode, test_recon_metrics_on_the_arena, Pp, Cc, n)


@twin_of(test_dino_stats_on_the_arena)
def test_dino_stats_on_the_arena_off_stream(G, V, B, K, mode, offstream):
    offstream(mode, test_dino_stats_on_the_arena, G, V, B, K)
