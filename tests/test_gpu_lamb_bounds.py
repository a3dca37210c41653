"""The launching entry point of include/vitssl_lamb.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_optim_bounds.py: p, g, m, v, the table image, the EXACT-size workspace, the EXACT-size trust and the one-float
sum of squares are carved from a 0xFF-poisoned arena.  Per case: no guard byte changes; the floats between the segments (NaN
poison in all four buffers) stay what they were; g and the table are unchanged; every slot and every ratio is written; the
results hold the bar of the float64 restatement.  Then every VITSSL_ERR_ARG case of the header, and the bound prototypes."""
import ctypes as C
import os
import re

import pytest
import torch

import _lamb_ref as R
import _optim_cases as K
from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)

DEV = torch.device("cuda:0")
F32 = torch.float32
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COVERED = {"vitssl_lamb_segments"}        # the entry points test_on_the_arena launches

# the common layout, and one whose last segment ends with the store at a partial 16-byte group behind whole units
LAYOUTS = {"common": K.COMMON, "ragged_end": [((5,), True), ((64,), False), ((2, 1024 + 3), True)]}


def P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_every_launching_function_has_a_case():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vitssl_lamb.h")).read(), flags=re.S)
    launching = {m.group(1) for m in re.finditer(r"\bint\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*void\s*\*\s*stream[^)]*)\)\s*;", txt)}
    assert launching == COVERED


def test_prototypes_match_the_header():
    from vitssl_hip import _lib as L
    from _abi_mirror import mismatches
    declared = L.declarations("lamb")
    assert set(declared) == set(L.REGISTRY["lamb"]) == {"vitssl_lamb_workspace_bytes", "vitssl_lamb_segments"}
    for name, bound in L.REGISTRY["lamb"].items():
        assert not mismatches(name, declared[name], bound, L.STRUCTS), mismatches(name, declared[name], bound, L.STRUCTS)
    assert L.REGISTRY["lamb"]["vitssl_lamb_workspace_bytes"] == (C.c_int64, [C.POINTER(L.OptimSegment), C.c_int])      # the table is typed
    raw = C.CDLL(L.LIB_PATH)
    for name in L.REGISTRY["lamb"]:
        assert hasattr(raw, name), f"{name} declared in include/vitssl_lamb.h but not exported"


def test_workspace_sizing_is_sixteen_bytes_a_unit():
    from vitssl_hip import _lib as L
    l = L.lib()
    rows = [(0, 1, 1.0, 0.0), (64, 1024, 1.0, 0.0), (2048, 1025, 1.0, 0.0), (4096, 5 * 1024 + 3, 1.0, 0.0)]
    arr = (L.OptimSegment * 4)(*[L.OptimSegment(*r) for r in rows])
    assert l.vitssl_lamb_workspace_bytes(arr, 4) == 16 * (1 + 1 + 2 + 6)
    assert l.vitssl_lamb_workspace_bytes(arr, 1) == 16
    for nseg in (0, -1, (1 << 20) + 1):
        assert l.vitssl_lamb_workspace_bytes(arr, nseg) == 0
    assert l.vitssl_lamb_workspace_bytes(None, 4) == 0
    bad = (L.OptimSegment * 1)(L.OptimSegment(0, 0, 1.0, 0.0))
    assert l.vitssl_lamb_workspace_bytes(bad, 1) == 0


@gpu
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_on_the_arena(name):
    from vitssl_hip import _lib as L
    lay = K.Layout(LAYOUTS[name])
    n = lay.rows[-1][0] + lay.rows[-1][1]                          # the store ends with its last parameter: no pad behind it
    params, grads = K.make_case(lay, seed=7)
    rows2 = R.rows_of(lay)
    ref = R.run(params, grads[:2], rows2, torch.float64, always_adapt=True)
    bar, _ = R.bar_from(R.run(params, grads[:2], rows2, torch.float32, always_adapt=True), ref)
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
    sws = a.empty("sumsq workspace", (int(l.vitssl_grad_sumsq_workspace_bytes(nseg)),), torch.uint8)
    ss = a.empty("sumsq", (1,), F32)
    ws = a.empty("workspace", (int(l.vitssl_lamb_workspace_bytes(rows, nseg)),), torch.uint8)        # exactly the sizing function's bytes
    trust = a.empty("trust", (nseg,), F32)                                                            # exactly nseg floats
    assert ws.numel() == 16 * sum((r[1] + 1023) // 1024 for r in lay.rows)
    mask = lay.mask[:n]
    between = {what: t.cpu().view(torch.int32)[~mask] for what, t in (("p", p), ("m", m), ("v", v))}
    for k in range(2):
        g_host = lay.scatter(grads[k], nan)[:n]
        g = a.put(f"g{k}", g_host)
        Arena.fill(ws)
        Arena.fill(trust)
        L.call("vitssl_grad_sumsq", P(g), P(table), nseg, P(ss), P(sws), sws.numel(), S())
        L.call("vitssl_lamb_segments", P(p), P(g), P(m), P(v), P(table), nseg, R.LR, *R.BETAS, R.EPS, k + 1, 1.0, P(ss), R.MAX_NORM,
               L.LAMB_ALWAYS_ADAPT, P(trust), P(ws), ws.numel(), S())
        torch.cuda.synchronize()
        a.check()
        assert torch.equal(g.cpu().view(torch.int32), g_host.view(torch.int32)), "inputs are inputs"
        assert torch.equal(table.cpu(), image)
        assert not torch.isnan(ws.view(torch.float64)).any(), "every slot is written"
        assert not torch.isnan(trust).any(), "every ratio is written"
        rp, rm, rv, rtrust, _ = ref[k]
        rel = float(((trust.cpu().double() - torch.tensor(rtrust, dtype=torch.float64)).abs() / torch.tensor(rtrust, dtype=torch.float64)).max())
        assert rel < bar, f"trust: {rel:.3e} (relative) from the float64 restatement, bar {bar:.3e}"
        for what, t, r in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
            tc = t.cpu()
            assert torch.equal(tc.view(torch.int32)[~mask], between[what]), f"{what}: written between the segments"
            assert not torch.isnan(tc[mask]).any(), f"{what}: poison read"
            pad = torch.zeros(lay.numel - n)
            err = max(float((x.double() - y).abs().max()) for x, y in zip(lay.gather(torch.cat([tc, pad])), r))
            assert err < bar, f"{what}: {err:.3e} from the float64 restatement, bar {bar:.3e}"


@gpu
def test_too_few_slots_is_a_loud_no_op():
    """a workspace that passes the entry's check (16 bytes a segment) but is below the sizing function's answer: nothing is
    written but NaN ratios"""
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    n = 4096
    plan = ops.AdamWPlan([(0, 2048 + 5, 1.0, 0.1), (3072, 7, 1.0, 0.1)], n, DEV)                     # 3 + 1 units
    a = Arena(DEV, mib=16)
    p, g = a.put("p", torch.ones(n)), a.put("g", torch.ones(n))
    m, v = a.zeros("m", (n,), F32), a.zeros("v", (n,), F32)
    ws = a.empty("workspace", (16 * 3,), torch.uint8)
    trust = a.zeros("trust", (2,), F32)
    L.call("vitssl_lamb_segments", P(p), P(g), P(m), P(v), P(plan.table), 2, 1e-3, 0.9, 0.999, 1e-6, 1, 1.0, P(None), 0.0, 0, P(trust),
           P(ws), ws.numel(), S())
    torch.cuda.synchronize()
    a.check()
    assert bool(torch.isnan(trust).all()) and Arena.untouched(ws)
    assert bool((p == 1).all()) and not m.any() and not v.any()


@gpu
def test_refusals_launch_nothing():
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    n = 256
    z = lambda: torch.zeros(n, device=DEV)           # noqa: E731
    p, g, m, v = z(), z() + 1.0, z(), z()
    plan = ops.AdamWPlan([(0, 100, 1.0, 0.1), (128, 3, 1.0, 0.1)], n, DEV)
    ws, trust = plan.lamb_buffers()
    assert ws.numel() == 32 and tuple(trust.shape) == (2,)
    trust.fill_(7.0)
    ws.zero_()
    good = dict(p=P(p), g=P(g), m=P(m), v=P(v), table=P(plan.table), nseg=2, step=1, sumsq=P(None), max_norm=0.0, flags=0, trust=P(trust),
                ws=P(ws), ws_bytes=ws.numel())

    def launch(**change):
        a = dict(good, **change)
        L.call("vitssl_lamb_segments", a["p"], a["g"], a["m"], a["v"], a["table"], a["nseg"], 1e-3, 0.9, 0.999, 1e-6, a["step"], 1.0,
               a["sumsq"], a["max_norm"], a["flags"], a["trust"], a["ws"], a["ws_bytes"], S())

    off = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)        # noqa: E731
    cases = [("NULL", dict(p=P(None))), ("NULL", dict(g=P(None))), ("NULL", dict(m=P(None))), ("NULL", dict(v=P(None))),
             ("table is NULL", dict(table=P(None))), ("trust is NULL", dict(trust=P(None))),
             ("nseg", dict(nseg=0)), ("nseg", dict(nseg=-1)), ("nseg", dict(nseg=(1 << 20) + 1, ws_bytes=1 << 30)),
             ("step", dict(step=0)),
             ("max_norm", dict(sumsq=P(plan.sumsq), max_norm=0.0)), ("max_norm", dict(sumsq=P(plan.sumsq), max_norm=-1.0)),
             ("vitssl_lamb_workspace_bytes", dict(ws_bytes=31)), ("vitssl_lamb_workspace_bytes", dict(ws=P(None))),
             ("8-byte aligned", dict(ws=off(ws, 4), ws_bytes=40)),
             ("16-byte", dict(p=off(p, 4))), ("16-byte", dict(g=off(g, 8))), ("16-byte", dict(m=off(m, 4))), ("16-byte", dict(v=off(v, 12))),
             ("unknown bits", dict(flags=4)), ("unknown bits", dict(flags=-1))]
    for match, change in cases:
        with pytest.raises(L.VitsslError, match=match) as e:
            launch(**change)
        assert "vitssl_lamb_segments failed (-" in str(e.value) and "lamb_segments:" in str(e.value)
    for bad in (0.0, -1.0):
        with pytest.raises(L.VitsslError, match="max_norm"):
            ops.lamb_segments(p, g, m, v, plan, 1e-3, 0.9, 0.999, 1e-6, 1, 1.0, plan.sumsq, bad)
    with pytest.raises(L.VitsslError, match="trust"):
        ops.lamb_segments(p, g, m, v, plan, 1e-3, 0.9, 0.999, 1e-6, 1, trust=torch.zeros(3, device=DEV))
    with pytest.raises(L.VitsslError, match="flat buffer"):
        ops.lamb_segments(p[:128], g, m, v, plan, 1e-3, 0.9, 0.999, 1e-6, 1)
    torch.cuda.synchronize()
    assert not p.any() and not m.any() and not v.any() and not ws.any(), "a refused call launched"
    assert bool((trust == 7.0).all()), "a refused call launched"
    launch()                                                   # the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert m[:100].any() and p[:100].any() and not p[100:128].any() and bool((trust != 7.0).all())


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_on_the_arena)
def test_on_the_arena_off_stream(name, mode, offstream):
    offstream(mode, test_on_the_arena, name)
