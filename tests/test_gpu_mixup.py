"""The mix kernel (include/vitssl_mixup.h, vitssl_mix_batch) against its restatement (tests/_mixup_ref.py).

Copy and paste rows are compared as bits.  Blend rows: |out - ref64| <= 2^-22 max(|a|, |b|) per element, the reference taken in
fp64 from the float32 lam.  The bound is derived: out = fmaf(lam, a, (1 - lam) * b) has three roundings -- 1 - lam, the
product, the fma's result -- each at most 2^-24 relative to a quantity no larger than max(|a|, |b|) (lam and 1 - lam lie in
[0, 1]), so 3 x 2^-24 < 2^-22.  One wrong pixel is off by the difference of two images, about 0.1 of their scale."""
import numpy as np
import pytest
import torch

import _mixup_ref as M

DEV = torch.device("cuda:0")
F32, I32 = torch.float32, torch.int32
gpu = pytest.mark.gpu


def run(x, ip, lam, out=None):
    from vitssl_hip import ops
    xd = x if torch.is_tensor(x) else torch.from_numpy(x).to(DEV)
    out = torch.full(tuple(xd.shape), float("nan"), dtype=F32, device=DEV) if out is None else out
    ops.mix_batch(xd, out, torch.from_numpy(np.ascontiguousarray(ip, dtype=np.int32)).to(DEV), torch.from_numpy(np.asarray(lam, np.float32)).to(DEV))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(x, ip, lam, got):
    ref, bound = M.mix_reference(x, ip, lam)
    assert not np.isnan(got).any()                                           # out started as NaN: every element was written
    exact = bound == 0
    assert np.array_equal(got[exact].view(np.int32), ref[exact].astype(np.float32).view(np.int32))      # copy / paste: the bits
    err = np.abs(got.astype(np.float64) - ref)
    assert (err <= bound).all(), f"blend: worst error / bound {np.max(err[~exact] / np.maximum(bound[~exact], 1e-300)):.3g}"
    return float(np.max(err[~exact] / np.maximum(bound[~exact], 1e-300))) if (~exact).any() else 0.0


@gpu
@pytest.mark.parametrize("B,C,H,W", M.MIX_SHAPES, ids=str)
def test_mix_kernel_against_the_restatement(B, C, H, W):
    x = M.mix_input(B, C, H, W)
    xd = torch.from_numpy(x).to(DEV)
    worst = 0.0
    for n, (ip, lam) in enumerate(M.mix_tables(B, H, W)):
        got = run(xd, ip, lam)
        worst = max(worst, check(x, ip, lam, got))
        if n < 2:
            assert np.array_equal(run(xd, ip, lam).view(np.int32), got.view(np.int32)), "two runs differ"
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                        # the input is only read
    print(f"mix_batch {(B, C, H, W)}: worst blend error / (2^-22 max(|a|,|b|)) = {worst:.3g}")


@gpu
@pytest.mark.parametrize("B,C,H,W", [(5, 3, 32, 32), (3, 4, 9, 5)], ids=str)
def test_mix_kernel_nonfinite_inputs_are_copied_and_pasted_as_bits(B, C, H, W):
    x = M.mix_input(B, C, H, W)
    x[0, 0, 0, 0], x[B - 1, C - 1, H - 1, W - 1], x[1, 0, 1, 1] = np.inf, -np.inf, -0.0
    x.view(np.int32)[B - 1, 0, 2, 2] = 0x7FC12345                            # a NaN with a payload
    ip = np.zeros((B, 6), np.int32)
    ip[:, 1] = B - 1 - np.arange(B)
    ip[:, 0] = [0, 2, 0, 2, 2][:B] if B == 5 else [2, 0, 2]
    ip[:, 2:] = (0, H, 0, W)
    ip[1, 2:] = (1, H, 1, 3) if B == 5 else ip[1, 2:]
    got = run(x, ip, np.full(B, 0.5, np.float32))
    want = x.copy()
    for i, (kind, p, y0, y1, x0, x1) in enumerate(ip.tolist()):
        if kind == 2:
            want[i, :, y0:y1, x0:x1] = x[p, :, y0:y1, x0:x1]
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


@gpu
@pytest.mark.parametrize("B,C,H,W", [(5, 3, 32, 32), (4, 1, 7, 30)], ids=str)
def test_mix_kernel_bad_tables_have_defined_behaviour(B, C, H, W):
    """The tables are device memory: a partner of -1 or B acts as the row itself, a box beyond the image is clamped, kind 7
    (and any other) is a copy."""
    x = M.mix_input(B, C, H, W)
    ip = np.array([[M.PASTE, -1, 0, H, 0, W], [M.PASTE, B, -3, H + 9, -2, W + 5], [7, 0, 0, H, 0, W], [M.BLEND, B, 0, 0, 0, 0],
                   [M.PASTE, 0, -(2 ** 31), 2 ** 31 - 1, -(2 ** 31), 2 ** 31 - 1]][:B], np.int32)
    ip[1, 1] = 2 if B > 2 else 0                                             # the clamped box pastes all of row 2
    lam = np.full(B, 0.25, np.float32)
    got = run(x, ip, lam)
    check(x, ip, lam, got)
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[1], x[2]) and np.array_equal(got[2], x[2])
    blend_self = np.float32(0.25) * x[3].astype(np.float64) + np.float64(np.float32(0.75)) * x[3]
    assert (np.abs(got[3] - blend_self) <= 2.0 ** -22 * np.abs(x[3])).all()
    if B > 4:
        assert np.array_equal(got[4], x[0])
    for kind in (-1, 3, 2 ** 31 - 1, -(2 ** 31)):                            # every other kind copies too
        ip2 = ip.copy()
        ip2[:, 0] = kind
        assert np.array_equal(run(x, ip2, lam).view(np.int32), x.view(np.int32))


@gpu
def test_mix_kernel_refuses_overlapping_buffers_before_any_launch():
    from vitssl_hip import VitsslError, ops
    B, C, H, W = 4, 3, 8, 8
    n = B * C * H * W
    buf = torch.zeros(2 * n, dtype=F32, device=DEV)
    x = buf[:n].view(B, C, H, W)
    x.copy_(torch.from_numpy(M.mix_input(B, C, H, W)))
    ip = torch.zeros(B, 6, dtype=I32, device=DEV)
    ip[:, 0] = 1
    lam = torch.full((B,), 0.5, device=DEV)
    before = buf.clone()
    for out in (x, buf[4:n + 4].view(B, C, H, W), buf[n - 4:2 * n - 4].view(B, C, H, W)):
        with pytest.raises(VitsslError, match="overlaps"):
            ops.mix_batch(x, out, ip, lam)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                          # nothing ran
    ops.mix_batch(x, buf[n:].view(B, C, H, W), torch.zeros_like(ip), lam)    # adjacent is fine (all copy)
    torch.cuda.synchronize()
    assert torch.equal(buf[:n], before[:n]) and torch.equal(buf[n:], before[:n])


@gpu
def test_gpu_mixup_object_draws_and_applies():
    from data import GPUMixup, MixSpec, sample_mix_params
    B, C, H, W = 6, 3, 32, 32
    x = M.mix_input(B, C, H, W)
    xd = torch.from_numpy(x).to(DEV)
    for mode in ("batch", "elem"):
        mx = GPUMixup(MixSpec(mode=mode))
        for seed in (1, 2, 3):
            p = sample_mix_params(mx.spec, B, H, W, torch.Generator().manual_seed(seed))
            params = mx.draw(B, H, W, torch.Generator().manual_seed(seed))
            ip = np.stack([p[k] for k in ("kind", "partner", "y0", "y1", "x0", "x1")], 1)
            assert np.array_equal(params.iparams.cpu().numpy(), ip) and np.array_equal(params.lam.cpu().numpy(), p["lam"])
            assert np.array_equal(params.partner.cpu().numpy(), p["partner"]) and params.partner.dtype == I32 and params.lam.dtype == F32
            out = mx.apply(xd, params)
            torch.cuda.synchronize()
            check(x, ip, p["lam"], out.cpu().numpy())
