"""The two kernels of include_addons/vitssl_pool.h alone, against tests/_pool_ref.py on the same tensors.

Forward on integers in [-8, 8]: every partial sum stays below 2^24 in magnitude, so the fp32 accumulation is exact in ANY order
and the result is the one rounding of r * (integer sum): all bits equal the restatement (tests/test_pool_host.py shows that this
comparison tells a mean over the CLS row, a division by T and a dropped last token from the right one).
Forward on randn, per element against an fp64 mean:  |got - ref| <= (T + 2) * 2^-24 * mean_t |x[b, t, c]|.  An n-term fp32 sum
in any order is off by at most (n - 1) u * sum |x_i| to first order, u = 2^-24; the fp32 scale r and the product round once each
(2 u more), and sum |x_i| / n is the mean of the magnitudes with n = T - 1: (n + 1) u mean|x| <= (T + 2) u mean|x|, the slack
covering the second-order terms.  Derived, not measured.
Backward: one fp32 product per element, all bits equal the restatement; the CLS rows are +0.
Both: the same bits on a second run, image b of a batch equals a launch on that image alone, the inputs are only read, and a
NaN-poisoned CLS row reaches no result of the forward.
The shapes cross the 16 token parts of a workgroup (T - 1 < 16, = 16, a multiple, not a multiple; the four-deep unrolled sweep
needs T > 49), the 64-column chunk (D = 64, two chunks, a chunk of 192 = 3 full ones, 12 chunks) and several images."""
import pytest
import torch

import _pool_ref as PR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = torch.float32
SHAPES = [(1, 2, 64), (3, 3, 64), (2, 5, 192), (5, 17, 128), (2, 65, 64), (1, 197, 768), (2, 257, 384), (1, 2048, 64)]


def bits(t):
    return t.contiguous().view(torch.int32)


def ints(shape, seed, hi=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-hi, hi + 1, shape, generator=g).to(F32)


def fwd(x, B, T, D):
    from vitssl_hip import ops
    out = torch.full((B, D), float("nan"), device=DEV)
    ops.pool_tokens_fwd(x, out, B, T, D)
    return out


def bwd(dout, B, T, D):
    from vitssl_hip import ops
    g = torch.full((B * T, D), float("nan"), device=DEV)
    ops.pool_tokens_bwd(dout, g, B, T, D)
    return g


@pytest.mark.parametrize("B,T,D", SHAPES, ids=str)
def test_forward_on_integers_is_bit_equal(B, T, D):
    assert 8 * T < (1 << 24)                                                    # every partial sum is exact in fp32
    x = ints((B * T, D), T)
    want = PR.pool_fwd(x, B, T)
    xd = x.to(DEV)
    xd.view(B, T, D)[:, 0] = float("nan")                                       # the CLS rows are never read
    before = xd.clone()
    out = fwd(xd, B, T, D)
    assert not torch.isnan(out).any(), "the CLS row was read (or an element was not written)"
    assert torch.equal(bits(out.cpu()), bits(want))
    assert torch.equal(bits(fwd(xd, B, T, D)), bits(out)), "a second run gives other bits"
    assert torch.equal(bits(xd), bits(before)), "the input was written"


@pytest.mark.parametrize("B,T,D", SHAPES, ids=str)
def test_forward_on_randn_within_the_fp32_sum_bound(B, T, D):
    g = torch.Generator().manual_seed(1000 + T)
    x = torch.randn(B * T, D, generator=g)
    xd = x.to(DEV)
    xd.view(B, T, D)[:, 0] = float("nan")
    out = fwd(xd, B, T, D)
    assert not torch.isnan(out).any()
    x64 = x.view(B, T, D)[:, 1:].double()
    ref, mag = x64.mean(1), x64.abs().mean(1)
    err, bound = (out.cpu().double() - ref).abs(), (T + 2) * 2.0 ** -24 * mag
    print(f"pool fwd ({B}, {T}, {D}): worst |got - ref| / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert torch.equal(bits(fwd(xd, B, T, D)), bits(out)), "a second run gives other bits"
    for b in range(B):                                                          # the order depends on (T, D) alone
        alone = fwd(xd[b * T:(b + 1) * T].clone(), 1, T, D)
        assert torch.equal(bits(alone[0]), bits(out[b])), f"image {b} of the batch differs from a launch on it alone"


@pytest.mark.parametrize("B,T,D", SHAPES, ids=str)
def test_backward_is_bit_equal(B, T, D):
    g = torch.Generator().manual_seed(2000 + T)
    dout = torch.randn(B, D, generator=g)
    dout[0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0])
    want = PR.pool_bwd(dout, B, T)
    dd = dout.to(DEV)
    before = dd.clone()
    got = bwd(dd, B, T, D)
    assert not torch.isnan(got).any(), "an element of g was not written"
    assert torch.equal(bits(got.cpu()), bits(want))
    assert not bits(got).view(B, T, D)[:, 0].any(), "a CLS row is not +0"
    assert torch.equal(bits(bwd(dd, B, T, D)), bits(got)), "a second run gives other bits"
    assert torch.equal(bits(dd), bits(before)), "the input was written"
    for b in range(B):
        alone = bwd(dd[b:b + 1].clone(), 1, T, D)
        assert torch.equal(bits(alone), bits(got[b * T:(b + 1) * T])), f"image {b} of the batch differs from a launch on it alone"


def test_the_wrappers_check_shape_and_dtype():
    from vitssl_hip import _lib as L
    from vitssl_hip import ops
    B, T, D = 2, 5, 64
    x, out = torch.zeros(B * T, D, device=DEV), torch.zeros(B, D, device=DEV)
    for bad in (lambda: ops.pool_tokens_fwd(x, out, B, T + 1, D), lambda: ops.pool_tokens_fwd(x.bfloat16(), out, B, T, D),
                lambda: ops.pool_tokens_fwd(x, out[:, :32], B, T, 32), lambda: ops.pool_tokens_bwd(out, x, B + 1, T, D),
                lambda: ops.pool_tokens_bwd(out.double(), x, B, T, D), lambda: ops.pool_tokens_fwd(x.cpu(), out, B, T, D),
                lambda: ops.pool_tokens_fwd(x[:B], out, B, 1, D)):                # T = 1: no patch token, refused by the entry point
        with pytest.raises(L.VitsslError):
            bad()
