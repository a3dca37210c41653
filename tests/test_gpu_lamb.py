"""The segmented LAMB step (include/vitssl_lamb.h) through ops.AdamWPlan / ops.grad_sumsq / ops.lamb_segments: parity with the
float64 restatement (tests/_lamb_ref.py) over a layout with every unit edge and a segment that wraps the grid, the edge rules of
the trust ratio, determinism and store hygiene, and a sanity check against ops.adamw_segments."""
import functools

import pytest
import torch

import _lamb_ref as R
import _optim_cases as K

DEV = torch.device("cuda:0")
F32 = torch.float32
pytestmark = pytest.mark.gpu

# the common layout (n = 1, 3, 4, 65, 4097, 128 x 64, one frozen hole), then the unit edges (one whole unit, one float more,
# three units and a partial 16-byte group), then 2048 * 1024 + 1029 floats: more units than the grid has workgroups, so the
# grid stride wraps inside ONE segment that owns more slots than there are workgroups.  Two-dimensional shapes: the layout
# decays those (wd 0.05), so their trust ratios are computed, not 1.
PARITY = K.COMMON + [((1, 1024), True), ((1, 1025), True), ((1, 3 * 1024 + 5), True), ((1, 2048 * 1024 + 1029), True)]


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops
    return ops


@functools.lru_cache(maxsize=None)
def parity_case():
    lay = K.Layout(PARITY)
    params, grads = K.make_case(lay, seed=11)
    return lay, params, grads


@functools.lru_cache(maxsize=None)
def parity_reference(gscale, always_adapt, trust_clip):
    """the float64 run and the bar of this layout (computed once per setting, never modified)"""
    lay, params, grads = parity_case()
    kw = dict(gscale=gscale, always_adapt=always_adapt, trust_clip=trust_clip)
    run64 = R.run(params, grads, R.rows_of(lay), torch.float64, **kw)
    bar, dist = R.bar_from(R.run(params, grads, R.rows_of(lay), torch.float32, **kw), run64)
    return run64, bar, dist


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


def lamb_steps(ops, lay, params, grads, gscale=1.0, clip=True, **kw):
    """the steps of `grads` on the device; yields (k, p, m, v, trust, gd) after each"""
    p, m, v = flat_state(lay, params)
    plan = ops.AdamWPlan(lay.rows, lay.numel, DEV)
    for k, g in enumerate(grads):
        gd = flat_grad(lay, g)
        ss = ops.grad_sumsq(gd, plan) if clip else None
        trust = ops.lamb_segments(p, gd, m, v, plan, R.LR, *R.BETAS, R.EPS, k + 1, gscale, ss, R.MAX_NORM if clip else 0.0, **kw)
        yield k, p, m, v, trust, gd


# ---- 1. parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale,always_adapt,trust_clip", [(1.0, False, False), (0.5, False, False), (1.0, True, False)])
def test_matches_the_float64_restatement(ops, gscale, always_adapt, trust_clip):
    lay, params, grads = parity_case()
    run64, bar, dist = parity_reference(gscale, always_adapt, trust_clip)
    print(f"float32-vs-float64 distance of the restatement {dist:.3e}, bar {bar:.3e}")
    outside = ~lay.mask
    start = torch.full((int(outside.sum()),), K.SENTINEL, dtype=torch.int32)
    active = 0
    for k, p, m, v, trust, gd in lamb_steps(ops, lay, params, grads, gscale, always_adapt=always_adapt, trust_clip=trust_clip):
        rp, rm, rv, rtrust, rnorm = run64[k]
        active += rnorm > R.MAX_NORM
        for name, t, ref in (("p", p, rp), ("m", m, rm), ("v", v, rv)):
            tc = t.cpu()
            assert torch.equal(bits(tc)[outside], start), f"step {k + 1}: {name} was written outside the segments"
            assert not torch.isnan(tc[lay.mask]).any(), f"step {k + 1}: NaN reached a trainable element of {name}"
            err = max(float((x.double() - r).abs().max()) for x, r in zip(lay.gather(tc), ref))
            print(f"step {k + 1} {name}: max abs error {err:.3e}")
            assert err < bar, f"step {k + 1}: {name} is {err:.3e} from the float64 restatement, bar {bar:.3e}"
        got = trust.cpu().double()
        want = torch.tensor(rtrust, dtype=torch.float64)
        rel = float(((got - want).abs() / want).max())
        print(f"step {k + 1} trust: max relative error {rel:.3e}, ratios {float(want.min()):.4g} .. {float(want.max()):.4g}")
        assert rel < bar, f"step {k + 1}: trust ratios {rel:.3e} (relative) from the float64 restatement, bar {bar:.3e}"
        if not always_adapt:
            assert all(t == 1.0 for t, (_, w) in zip(got.tolist(), R.rows_of(lay)) if w == 0.0)
        if trust_clip:
            assert float(got.max()) <= 1.0
    assert 0 < active < len(grads), "the recipe alternates an idle and an active clip"
    assert any(t != 1.0 for t in run64[-1][3]), "no trust ratio was computed"


# ---- 2. edge rules ----------------------------------------------------------------------------------------------------------------
def one_step(ops, tensors, rows, grads, **kw):
    """one unclipped device step over tensors laid out 64-float aligned; returns (new tensors, trust list)"""
    lay = K.Layout([(tuple(t.shape), True) for t in tensors])
    lay.rows = [(o, n, s, w) for (o, n, _, _), (s, w) in zip(lay.rows, rows)]
    for k, p, m, v, trust, gd in lamb_steps(ops, lay, tensors, [grads], clip=False, **kw):
        return lay.gather(p.cpu()), trust.cpu().tolist()


def test_zero_parameter_with_decay_gets_trust_one(ops):
    new, trust = one_step(ops, [torch.zeros(5)], [(1.0, 0.1)], [torch.ones(5)])
    ref = R.LambRef([torch.zeros(5)], [(1.0, 0.1)], torch.float64)
    ref.step([torch.ones(5)])
    assert trust == [1.0] and float((new[0].double() - ref.p[0]).abs().max()) < K.BAR_FLOOR and bool((new[0] != 0).all())


def test_zero_update_gets_trust_one(ops):
    tensors, rows, grads = [torch.zeros(5), torch.ones(3)], [(1.0, 0.1), (1.0, 0.1)], [torch.zeros(5), torch.ones(3)]
    new, trust = one_step(ops, tensors, rows, grads)
    ref = R.LambRef(tensors, rows, torch.float64)
    want = ref.step(grads)
    assert trust[0] == 1.0 and not new[0].any()
    assert want[1] != 1.0 and abs(trust[1] - want[1]) < K.BAR_FLOOR * want[1]


def test_trust_clip_caps_at_one(ops):
    big, small, grad = torch.full((8,), 10.0), torch.full((8,), 0.01), torch.ones(8)
    rows = [(1.0, 0.01), (1.0, 0.01)]
    want = R.LambRef([big, small], rows, torch.float64).step([grad, grad])
    _, free = one_step(ops, [big, small], rows, [grad, grad])
    _, capped = one_step(ops, [big, small], rows, [grad, grad], trust_clip=True)
    assert want[0] > 1.0 > want[1]
    assert all(abs(a - b) < K.BAR_FLOOR * b for a, b in zip(free, want))
    assert capped[0] == 1.0 and capped[1] == free[1]


def test_always_adapt_adapts_tensors_without_decay(ops):
    p, grad = torch.full((8,), 10.0), torch.ones(8)
    _, plain = one_step(ops, [p], [(1.0, 0.0)], [grad])
    _, adapted = one_step(ops, [p], [(1.0, 0.0)], [grad], always_adapt=True)
    assert plain == [1.0]
    assert abs(adapted[0] - 10.0 * (1.0 + R.EPS)) < K.BAR_FLOOR * 10.0


# ---- 3. determinism and store hygiene ---------------------------------------------------------------------------------------------
def test_two_runs_same_bits_and_nothing_else_touched(ops):
    lay, params, grads = parity_case()
    outside = ~lay.mask
    runs = []
    for _ in range(2):
        for k, p, m, v, trust, gd in lamb_steps(ops, lay, params, grads[:2]):
            g_host = lay.scatter(grads[k], float("nan"))
            assert torch.equal(bits(gd), g_host.view(torch.int32)), "g keeps its bits (NaN between the segments included)"
        runs.append([bits(t) for t in (p, m, v, trust)])
    for name, a, b in zip(("p", "m", "v", "trust"), *runs):
        assert torch.equal(a, b), f"{name}: two runs from the same start, two results"
    for name, a in zip("pmv", runs[0]):
        assert bool((a[outside] == K.SENTINEL).all()), f"{name}: a float outside the segments lost the sentinel"


# ---- 4. sanity across kernels -----------------------------------------------------------------------------------------------------
def test_without_decay_it_stays_within_the_bar_of_adamw_segments(ops):
    """every wd == 0 and no always_adapt: trust is 1 and the step is AdamW's with wd 0 (the order of the expression differs:
    not a bit-equality check)"""
    lay = K.Layout()
    lay.rows = [(o, n, s, 0.0) for o, n, s, _ in lay.rows]
    params, grads = K.make_case(lay)
    rows = R.rows_of(lay)
    bar, _ = R.bar_from(R.run(params, grads, rows, torch.float32), R.run(params, grads, rows, torch.float64))
    p2, m2, v2 = flat_state(lay, params)
    plan = ops.AdamWPlan(lay.rows, lay.numel, DEV)
    mask = lay.mask.to(DEV)
    for k, p, m, v, trust, gd in lamb_steps(ops, lay, params, grads):
        ops.adamw_segments(p2, gd, m2, v2, plan, R.LR, *R.BETAS, R.EPS, k + 1, 1.0, ops.grad_sumsq(gd, plan), R.MAX_NORM)
        assert bool((trust == 1.0).all())
        for name, a, b in (("p", p, p2), ("m", m, m2), ("v", v, v2)):
            err = float((a[mask].double() - b[mask].double()).abs().max())
            assert err < bar, f"step {k + 1}: {name} is {err:.3e} from adamw_segments, bar {bar:.3e}"
