"""The segmented AdamW step and the gradient's sum of squares (include/vitssl_optim.h) through ops.AdamWPlan / ops.grad_sumsq /
ops.adamw_segments: bit identity with vitssl_adamw, parity with torch.optim.AdamW (one group per tensor) plus clip_grad_norm_
in float64, the norm against float64, the clip's edges, and the refusals."""
import ctypes as C
import math

import pytest
import torch

import _optim_cases as K

DEV = torch.device("cuda:0")
F32 = torch.float32
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops
    return ops


@pytest.fixture(scope="module")
def common():
    """the common layout, its case and the torch references (computed once, never modified)"""
    lay = K.Layout()
    params, grads = K.make_case(lay)
    ref32 = K.torch_reference(lay, params, grads, torch.float32)
    ref64 = K.torch_reference(lay, params, grads, torch.float64)
    return lay, params, grads, ref32, ref64


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def flat_state(lay, params):
    """p, m, v on the device: the trainable slices hold params / zeros, every other float the sentinel pattern"""
    sent = torch.tensor([K.SENTINEL], dtype=torch.int32).view(F32).item()
    p = lay.scatter(params, sent)
    m = lay.scatter([torch.zeros_like(x) for x in params], sent)
    return p.to(DEV), m.to(DEV), m.clone().to(DEV)


def flat_grad(lay, g):
    return lay.scatter(g, float("nan")).to(DEV)


# ---- 1. bit identity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1001, 4099])
def test_one_segment_is_bit_identical_to_adamw(ops, n):
    torch.manual_seed(n)
    p0, grads = torch.randn(n), [torch.randn(n) * 0.1 for _ in range(3)]
    a = [p0.clone().to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [t.clone() for t in a]
    plan = ops.AdamWPlan([(0, n, 1.0, 0.05)], n, DEV)
    for k, g in enumerate(grads):
        gd = g.to(DEV)
        ops.adamw(a[0], gd, a[1], a[2], 1e-3, 0.9, 0.999, 1e-8, 0.05, k + 1, 0.5)
        ops.adamw_segments(b[0], gd, b[1], b[2], plan, 1e-3, 0.9, 0.999, 1e-8, k + 1, 0.5)
    for name, x, y in zip("pmv", a, b):
        assert torch.equal(bits(x), bits(y)), f"{name}: bits differ from vitssl_adamw"


# ---- 2. parity with torch over the common layout ----------------------------------------------------------------------------------
def test_common_layout_matches_torch_float64(ops, common):
    lay, params, grads, ref32, ref64 = common
    bar, dist = K.bar_from(ref32, ref64)
    print(f"float32-vs-float64 distance of the torch recipe {dist:.3e}, bar {bar:.3e}")
    p, m, v = flat_state(lay, params)
    plan = ops.AdamWPlan(lay.rows, lay.numel, DEV)
    outside = ~lay.mask
    start = [bits(t) for t in (p, m, v)]
    worst = 0.0
    for k, g in enumerate(grads):
        gd = flat_grad(lay, g)
        g_before = bits(gd)
        ss = ops.grad_sumsq(gd, plan)
        ops.adamw_segments(p, gd, m, v, plan, K.LR, *K.BETAS, K.EPS, k + 1, 1.0, ss, K.MAX_NORM)
        torch.cuda.synchronize()
        assert torch.equal(bits(gd), g_before), "g is an input"
        rp, rm, rv, rnorm = ref64[k]
        for name, t, s0, ref in (("p", p, start[0], rp), ("m", m, start[1], rm), ("v", v, start[2], rv)):
            tc = t.cpu()
            assert torch.equal(bits(tc)[outside], s0[outside]), f"step {k + 1}: {name} was written outside the segments"
            assert not torch.isnan(tc[lay.mask]).any(), f"step {k + 1}: NaN reached a trainable element of {name}"
            err = max(float((x.double() - r).abs().max()) for x, r in zip(lay.gather(tc), ref))
            worst = max(worst, err)
            print(f"step {k + 1} {name}: max abs error {err:.3e}")
            assert err < bar, f"step {k + 1}: {name} is {err:.3e} from torch float64, bar {bar:.3e}"
        norm = math.sqrt(float(ss))
        assert abs(norm - float(rnorm)) <= 2e-6 * float(rnorm)
        assert (float(rnorm) > K.MAX_NORM) == (k % 2 == 1), "the recipe alternates an idle and an active clip"
    print(f"worst error {worst:.3e}")


# ---- 3. the norm ------------------------------------------------------------------------------------------------------------------
def _norm_cases(common):
    lay, _, grads, _, _ = common
    yield "common", lay, [x.double() / K.GRAD_SCALES[0] for x in grads[0]]            # global norm 1
    big = K.Layout([((2 ** 20 + 3,), True)])
    yield "2^20+3", big, [torch.randn(2 ** 20 + 3, generator=torch.Generator().manual_seed(3), dtype=torch.float64)]


@pytest.mark.parametrize("scale", [1e-4, 1.0, 30.0])
def test_grad_sumsq_matches_float64(ops, common, scale):
    for name, lay, g64 in _norm_cases(common):
        g = [(x * scale).float() for x in g64]
        want = math.sqrt(sum(float((x.double() ** 2).sum()) for x in g))
        gd = flat_grad(lay, g)
        plan = ops.AdamWPlan(lay.rows, lay.numel, DEV)
        out = torch.full((1,), float("nan"), device=DEV)
        ops.grad_sumsq(gd, plan, out)
        got = math.sqrt(float(out))
        print(f"{name} scale {scale}: norm {got:.9e}, float64 {want:.9e}, relative {abs(got - want) / want:.2e}")
        assert abs(got - want) <= 2e-6 * want, f"{name}: {got} against {want}"
        out2 = torch.full((1,), float("nan"), device=DEV)
        ops.grad_sumsq(gd, plan, out2)
        assert torch.equal(bits(out), bits(out2)), "two runs, two results"


# ---- 4. the clip's edges ----------------------------------------------------------------------------------------------------------
def test_idle_clip_is_bit_identical_to_no_clip(ops, common):
    lay, params, grads, _, _ = common
    plan = ops.AdamWPlan(lay.rows, lay.numel, DEV)
    gd = flat_grad(lay, grads[0])                         # global norm 0.01 < MAX_NORM: the coefficient is exactly 1
    a, b = flat_state(lay, params), flat_state(lay, params)
    ss = ops.grad_sumsq(gd, plan)
    assert K.MAX_NORM / (math.sqrt(float(ss)) + 1e-6) > 1.0
    ops.adamw_segments(*a[:1], gd, *a[1:], plan, K.LR, *K.BETAS, K.EPS, 1, 1.0, ss, K.MAX_NORM)
    ops.adamw_segments(*b[:1], gd, *b[1:], plan, K.LR, *K.BETAS, K.EPS, 1, 1.0)
    for name, x, y in zip("pmv", a, b):
        assert torch.equal(bits(x), bits(y)), f"{name}: an idle clip changed bits"


def test_zero_gradient(ops, common):
    lay, params, _, _, _ = common
    plan = ops.AdamWPlan(lay.rows, lay.numel, DEV)
    gd = flat_grad(lay, [torch.zeros_like(x) for x in params])
    p, m, v = flat_state(lay, params)
    ss = ops.grad_sumsq(gd, plan)
    ops.adamw_segments(p, gd, m, v, plan, K.LR, *K.BETAS, K.EPS, 1, 1.0, ss, K.MAX_NORM)
    assert float(ss) == 0.0
    mask = lay.mask.to(DEV)
    assert bool((m[mask] == 0).all()) and bool((v[mask] == 0).all())
    assert bool(torch.isfinite(p[mask]).all())


def test_gscale_folds_the_average(ops, common):
    lay, params, grads, _, _ = common
    plan = ops.AdamWPlan(lay.rows, lay.numel, DEV)
    summed = [x * 2.0 for x in grads[1]]                  # two ranks' sum of a gradient of norm 3: the clip is active
    a, b = flat_state(lay, params), flat_state(lay, params)
    ga, gb = flat_grad(lay, summed), flat_grad(lay, grads[1])
    ops.adamw_segments(a[0], ga, a[1], a[2], plan, K.LR, *K.BETAS, K.EPS, 1, 0.5, ops.grad_sumsq(ga, plan), K.MAX_NORM)
    ssb = torch.empty(1, device=DEV)
    ops.adamw_segments(b[0], gb, b[1], b[2], plan, K.LR, *K.BETAS, K.EPS, 1, 1.0, ops.grad_sumsq(gb, plan, ssb), K.MAX_NORM)
    mask = lay.mask.to(DEV)
    for x, y in zip(a, b):
        assert float((x[mask] - y[mask]).abs().max()) < 1e-7


# ---- 5. refusals before any launch ------------------------------------------------------------------------------------------------
def test_refusals(ops):
    from vitssl_hip import _lib as L
    n = 256
    z = lambda: torch.zeros(n, device=DEV)
    p, g, m, v = z(), z(), z(), z()
    plan = ops.AdamWPlan([(0, 100, 1.0, 0.0), (128, 3, 1.0, 0.0)], n, DEV)
    P = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    hyper = (1e-3, 0.9, 0.999, 1e-8, 1, 1.0)
    ws = plan.workspace
    with pytest.raises(L.VitsslError, match="table is NULL"):
        L.call("vitssl_adamw_segments", P(p), P(g), P(m), P(v), P(None), 2, *hyper, P(None), 0.0, S)
    with pytest.raises(L.VitsslError, match="table is NULL"):
        L.call("vitssl_grad_sumsq", P(g), P(None), 2, P(plan.sumsq), P(ws), ws.numel(), S)
    for nseg in (0, -1):
        with pytest.raises(L.VitsslError, match="nseg"):
            L.call("vitssl_adamw_segments", P(p), P(g), P(m), P(v), P(plan.table), nseg, *hyper, P(None), 0.0, S)
        with pytest.raises(L.VitsslError, match="nseg"):
            L.call("vitssl_grad_sumsq", P(g), P(plan.table), nseg, P(plan.sumsq), P(ws), ws.numel(), S)
    with pytest.raises(L.VitsslError, match="nseg"):
        ops.AdamWPlan([], n, DEV)
    with pytest.raises(L.VitsslError, match="multiple of 4"):
        ops.AdamWPlan([(0, 100, 1.0, 0.0), (130, 3, 1.0, 0.0)], n, DEV)
    with pytest.raises(L.VitsslError, match="before the end"):
        ops.AdamWPlan([(0, 100, 1.0, 0.0), (64, 3, 1.0, 0.0)], n, DEV)
    with pytest.raises(L.VitsslError, match="behind the store"):
        ops.AdamWPlan([(0, 100, 1.0, 0.0), (128, 129, 1.0, 0.0)], n, DEV)
    with pytest.raises(L.VitsslError, match="vitssl_grad_sumsq_workspace_bytes"):
        ops.grad_sumsq(g, plan, workspace=ws[:ws.numel() - 8])
    for bad in (0.0, -1.0):
        with pytest.raises(L.VitsslError, match="max_norm"):
            ops.adamw_segments(p, g, m, v, plan, *hyper, plan.sumsq, bad)
    torch.cuda.synchronize()
    for t in (p, m, v):
        assert not t.any(), "a refused call launched"
