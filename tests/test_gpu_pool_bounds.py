"""Both entry points of include_addons/vitssl_pool.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_mae_bounds.py: inputs and outputs are carved from a 0xFF-poisoned arena.  No guard byte changes; no NaN poison
reaches a result (every output element is written, the CLS rows of the forward's input -- NaN -- are never read); the inputs are
only read; and each argument refusal of the header (null pointer, B < 1, T < 2, D < 4 or no multiple of 4, misaligned pointer)
returns -1 with a message and writes nothing.

tests/_offstream.py lists the headers of include/ and include_ext/; the twin below runs with include_addons/ added to that
list, so that the two entry points of this file are wrapped (gated, captured) like every other."""
import ctypes as C
import glob
import os

import pytest
import torch

import _offstream as OS
import _pool_ref as PR
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = torch.float32
ADDONS = os.path.join(OS.ROOT, "include_addons", "*.h")


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


@pytest.mark.parametrize("B,T,D", [(1, 2, 4), (3, 3, 64), (5, 17, 100), (2, 197, 192), (40, 10, 3328)], ids=str)
def test_pool_kernels_on_the_arena(B, T, D):
    """(40, 10, 3328): 2080 work items, more than the 2048 workgroups of the capped grid; D = 100: a chunk that ends inside a
    lane group; D = 4: one lane."""
    l = lib()
    g = torch.Generator().manual_seed(T)
    a = Arena(DEV, mib=64)
    xh = torch.randn(B * T, D, generator=g)
    doh = torch.randn(B, D, generator=g)
    xp = xh.clone()
    xp.view(B, T, D)[:, 0] = float("nan")                       # the CLS rows: never read
    x, dout = a.put("x", xp), a.put("dout", doh)
    out, gg = a.empty("out", (B, D), F32), a.empty("g", (B * T, D), F32)
    before = [x.clone(), dout.clone()]
    f = lambda **k: l.vitssl_pool_tokens_fwd(P(k.get("x", x), k.get("off", 0)), P(k.get("out", out), k.get("ooff", 0)), k.get("B", B),      # noqa: E731
                                             k.get("T", T), k.get("D", D), S())
    b = lambda **k: l.vitssl_pool_tokens_bwd(P(k.get("dout", dout), k.get("off", 0)), P(k.get("g", gg), k.get("ooff", 0)), k.get("B", B),   # noqa: E731
                                             k.get("T", T), k.get("D", D), S())
    assert f() == 0, l.vitssl_last_error()
    assert b() == 0, l.vitssl_last_error()
    torch.cuda.synchronize()
    a.check()
    assert clean(out) and clean(gg)
    for t, was in zip((x, dout), before):
        assert torch.equal(t.view(torch.uint8), was.view(torch.uint8))
    # the values (held to the restatement bit for bit on more shapes in tests/test_gpu_pool_kernels.py)
    ref = xh.view(B, T, D)[:, 1:].double().mean(1)
    mag = xh.view(B, T, D)[:, 1:].double().abs().mean(1)
    assert bool(((out.cpu().double() - ref).abs() <= (T + 2) * 2.0 ** -24 * mag).all())
    assert torch.equal(gg.cpu().view(torch.int32), PR.pool_bwd(doh, B, T).view(torch.int32))

    # ---- refusals: -1, a message, nothing written
    Arena.fill(out), Arena.fill(gg)
    for bad in (dict(x=None), dict(out=None), dict(B=0), dict(B=-1), dict(T=1), dict(T=0), dict(T=-3), dict(D=0), dict(D=2), dict(D=-4),
                dict(D=D + 2), dict(D=D + 1), dict(off=4), dict(off=8), dict(ooff=4)):
        refused(f(**bad))
    for bad in (dict(dout=None), dict(g=None), dict(B=0), dict(T=1), dict(T=-1), dict(D=0), dict(D=3), dict(D=D + 2), dict(off=4),
                dict(ooff=8), dict(ooff=12)):
        refused(b(**bad))
    assert Arena.untouched(out) and Arena.untouched(gg)
    for t, was in zip((x, dout), before):
        assert torch.equal(t.view(torch.uint8), was.view(torch.uint8))
    a.check()


# ============================================================================================ off the default stream (tests/_offstream.py)
@pytest.fixture
def addon_headers(monkeypatch):
    listed = OS.headers
    monkeypatch.setattr(OS, "headers", lambda: sorted(listed() + glob.glob(ADDONS)))
    assert {"vitssl_pool_tokens_fwd", "vitssl_pool_tokens_bwd"} <= OS.launching()


@twin_of(test_pool_kernels_on_the_arena)
def test_pool_kernels_on_the_arena_off_stream(B, T, D, mode, offstream, addon_headers):
    offstream(mode, test_pool_kernels_on_the_arena, B, T, D)
