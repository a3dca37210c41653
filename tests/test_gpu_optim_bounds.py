"""Both launching entry points of include/vitssl_optim.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_attention_hd_bounds.py: p, g, m, v, the table image, the EXACT-size workspace and the one-float results are carved
from a 0xFF-poisoned arena.  Per case: no guard byte changes; the floats between the segments (NaN poison in all four buffers)
stay what they were; g and the table are unchanged; no poison reaches a result; the results hold the bar of the torch recipe."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import _optim_cases as K
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)

DEV = torch.device("cuda:0")
F32 = torch.float32
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COVERED = {"vitssl_grad_sumsq", "vitssl_adamw_segments"}        # the entry points test_on_the_arena launches

# the common layout, and one whose last segment ends with the store at a partial 16-byte group behind whole units
LAYOUTS = {"common": K.COMMON, "ragged_end": [((5,), True), ((64,), False), ((2, 1024 + 3), True)]}


def P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_every_launching_function_has_a_case():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vitssl_optim.h")).read(), flags=re.S)
    launching = {m.group(1) for m in re.finditer(r"\bint\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*void\s*\*\s*stream[^)]*)\)\s*;", txt)}
    assert launching == COVERED


@gpu
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_on_the_arena(name):
    from vitssl_hip import _lib as L
    lay = K.Layout(LAYOUTS[name])
    n = lay.rows[-1][0] + lay.rows[-1][1]                          # the store ends with its last parameter: no pad behind it
    params, grads = K.make_case(lay, seed=7)
    ref = K.torch_reference(lay, params, grads[:2], torch.float64)
    bar, _ = K.bar_from(K.torch_reference(lay, params, grads[:2], torch.float32), ref)
    l = L.lib()
    nseg = len(lay.rows)
    rows = (L.OptimSegment * nseg)(*[L.OptimSegment(*r) for r in lay.rows])
    image = torch.zeros(int(l.vitssl_optim_table_bytes(nseg)), dtype=torch.uint8)
    L.call("vitssl_optim_table_build", rows, nseg, n, P(image), image.numel())

    a = Arena(DEV, mib=64)
    nan = float("nan")
    p = a.put("p", lay.scatter(params, nan)[:n])
    m = a.put("m", lay.scatter([torch.zeros_like(x) for x in params], nan)[:n])
    v = a.put("v", lay.scatter([torch.zeros_like(x) for x in params], nan)[:n])
    table = a.put("table", image)
    ws = a.empty("workspace", (int(l.vitssl_grad_sumsq_workspace_bytes(nseg)),), torch.uint8)          # exactly the sizing function's bytes
    ss = a.empty("sumsq", (1,), F32)
    mask = lay.mask[:n]
    between = {what: t.cpu().view(torch.int32)[~mask] for what, t in (("p", p), ("m", m), ("v", v))}
    for k in range(2):
        g_host = lay.scatter(grads[k], nan)[:n]
        g = a.put(f"g{k}", g_host)
        Arena.fill(ws)
        L.call("vitssl_grad_sumsq", P(g), P(table), nseg, P(ss), P(ws), ws.numel(), S())
        L.call("vitssl_adamw_segments", P(p), P(g), P(m), P(v), P(table), nseg, K.LR, *K.BETAS, K.EPS, k + 1, 1.0, P(ss), K.MAX_NORM, S())
        torch.cuda.synchronize()
        a.check()
        assert torch.equal(g.cpu().view(torch.int32), g_host.view(torch.int32)), "inputs are inputs"
        assert torch.equal(table.cpu(), image)
        assert not torch.isnan(ss).any() and not torch.isnan(ws.view(torch.float64)).any(), "every partial is written"
        rp, rm, rv, rnorm = ref[k]
        assert abs(math.sqrt(float(ss)) - float(rnorm)) <= 2e-6 * float(rnorm)
        for what, t, r in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
            tc = t.cpu()
            assert torch.equal(tc.view(torch.int32)[~mask], between[what]), f"{what}: written between the segments"
            assert not torch.isnan(tc[mask]).any(), f"{what}: poison read"
            pad = torch.zeros(lay.numel - n)
            err = max(float((x.double() - y).abs().max()) for x, y in zip(lay.gather(torch.cat([tc, pad])), r))
            assert err < bar, f"{what}: {err:.3e} from torch float64, bar {bar:.3e}"


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_on_the_arena)
def test_on_the_arena_off_stream(name, mode, offstream):
    offstream(mode, test_on_the_arena, name)
