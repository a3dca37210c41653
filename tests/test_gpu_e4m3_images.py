"""Every e4m3 byte that the quantiser, the attention kernels and the weight-image kernels write, judged per element
(tests/_e4m3.py; the checker's own tests are tests/test_e4m3_host.py).

  quantiser   all 2^16 bf16 patterns (NaN, infinities, bf16 subnormals included) byte for byte against the NumPy restatement of
              the format, four scales, every tail length, a call long enough for a second grid-stride pass, the running maximum
              planted where each part of the kernel reads it, non-finite inputs
  attention   dh = 64, (B, H) = (2, 3): the bf16 output is the non-fp8 entry point's, every image byte is inside the admissible
              pair of its bf16 neighbour, at lengths on both sides of every kernel's tile edges; backward at a scale that keeps all
              gradients in range and at one 2^5 larger (saturation and e4m3 subnormals in one image); persistent kernels with 3-4
              items per workgroup; a NaN in V
  weights     all four vectorisation combinations of (R % 4, C % 4), ragged and exact tiles, each destination alone and both; the
              maximum planted on, one fp32 step above and below the exponent rule's boundary, at the exponent clamp and near
              FLT_MAX; an infinity, a NaN; sources changed in place between runs of one plan.

The rule for non-finite values: NaN -> NaN (the quantisers keep its sign, 0x7F | sign; a computed NaN of
an epilogue is a NaN byte of either sign), +-inf and overflow -> +-448, recorded maxima ignore NaN.
Outputs start as 0x7F bytes / NaN: an element a kernel does not write is a NaN nobody asked for."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _e4m3 as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FP8, BF16 = torch.float8_e4m3fn, torch.bfloat16
BF16_MAX_BITS = 0x7F7F                       # largest finite bf16
SCALES = [None, 2.0 ** 17, 2.0 ** -9, 3.0]


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops
    return ops


def _fill8(*shape):
    return torch.full(shape, 0x7F, dtype=torch.uint8, device=DEV).view(FP8)


def _nan16(*shape):
    return torch.full(shape, math.nan, dtype=BF16, device=DEV)


def _bits16(values):
    return torch.tensor([v - (1 << 16) if v >= 0x8000 else v for v in values], dtype=torch.int16).view(BF16)


def _all_bf16():
    return torch.arange(1 << 16, dtype=torch.int32).to(torch.int16).view(BF16)


def _u8(t8):
    return t8.cpu().view(torch.uint8).numpy()


def _scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV)


def _same_bytes(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {int(bad[0])}: got 0x{got[bad[0]]:02X}, want 0x{want[bad[0]]:02X}"


# ----------------------------------------------------------------------------- quantiser
# tails: NaN, an infinity, a value just beyond 448 and a bf16 subnormal, both signs, rotated so that every tail length holds a
# different selection and lengths >= 4 hold all four kinds
TAIL = [0x7FC0, 0x7F80, 0x43E1, 0x0001, 0xFFC1, 0xFF80, 0x8040]   # 0x43E1 = 450: the bf16 value next to 448 (449.0 is not one)


@pytest.mark.parametrize("scale", SCALES)
def test_quantiser_all_bf16_patterns(ops, scale):
    table = _all_bf16()
    for r in range(8):
        tail = _bits16([TAIL[(r + j) % len(TAIL)] for j in range(r)])
        x = torch.cat([table, tail])
        y = _fill8(x.numel() + 64)                           # 64 guard bytes behind the image
        ops.quantize_fp8(x.to(DEV), y[: x.numel()], scale=_scalar(scale))
        got = _u8(y)
        _same_bytes(got[: x.numel()], E.quantize_ref(x.float(), scale), f"quantize_fp8 scale {scale}, n = 65536 + {r}")
        assert (got[x.numel():] == 0x7F).all(), f"n = 65536 + {r}: bytes written behind the image"


def test_quantiser_second_grid_stride_pass(ops):
    """n = 8 (256 x 32 x 256) + 8 x 1000 + 5: every lane of the capped grid has taken one 8-element group when 1000 of them take a
    second one, and five elements are left to the scalar tail.  The pattern's period (65 560) does not divide the grid's stride, so
    a lane's second group differs from its first."""
    n = 8 * (256 * 32 * 256) + 8 * 1000 + 5
    period = torch.cat([_all_bf16(), _all_bf16()[:24]])
    reps = -(-n // period.numel())
    x = period.to(DEV).repeat(reps)[:n].contiguous()
    y = _fill8(n + 64)
    scale = _scalar(2.0 ** -9)
    ops.quantize_fp8(x, y[:n], scale=scale)
    want = torch.from_numpy(E.quantize_ref(period.float(), 2.0 ** -9)).to(DEV).repeat(reps)[:n]
    got = y.view(torch.uint8)
    bad = torch.nonzero(got[:n] != want)
    assert bad.numel() == 0, f"{bad.numel()} bytes differ, first at {int(bad[0])} (second pass starts at {8 * 256 * 32 * 256})"
    assert bool((got[n:] == 0x7F).all())


def test_quantiser_running_maximum_positions(ops):
    """max |x| is found wherever it sits: the first element, the last element of the scalar tail, a group of the second grid-stride
    pass, the first element of a later workgroup; a prior maximum below it is replaced, one above it is kept.  Equality as bits."""
    n = 8 * (256 * 32 * 256) + 8 * 1000 + 5
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(1 << 16, generator=g) * 50).to(BF16).to(DEV).repeat(-(-n // (1 << 16)))[:n].contiguous()
    big = _bits16([BF16_MAX_BITS, BF16_MAX_BITS | 0x8000]).to(DEV)
    big_bits = BF16_MAX_BITS << 16
    above = torch.tensor([3.4e38], dtype=torch.float32)
    y = _fill8(n)
    for k, pos in enumerate([0, n - 1, 8 * (256 * 32 * 256) + 8 * 500 + 3, 8 * 256 * 5]):
        old = x[pos].clone()
        x[pos] = big[k & 1]
        for prior, want_bits in ((1.0, big_bits), (0.0, big_bits), (3.4e38, int(above.view(torch.int32)))):
            amax = _scalar(prior)
            ops.quantize_fp8(x, y, amax=amax)
            assert int(amax.cpu().view(torch.int32)) == want_bits, (pos, prior, float(amax))
        x[pos] = old
    amax = _scalar(0.0)
    ops.quantize_fp8(x, y, amax=amax)
    assert float(amax) == float(x.float().abs().max())          # and without the planted value: the tensor's own


def test_quantiser_maximum_of_non_finite_inputs(ops):
    """An infinity makes the recorded maximum +inf; a NaN is ignored (the maximum of the other elements), in the 8-element groups
    and in the scalar tail alike.  `EncoderStack._rescale` leaves a scale alone where the maximum is not finite."""
    g = torch.Generator().manual_seed(4)
    n = 4096 + 3
    base = (torch.randn(n, generator=g) * 7).to(BF16)
    top = float(base.float().abs().max())
    for pos in (17, n - 1):
        for bits, want in ((0x7F80, math.inf), (0xFF80, math.inf), (0x7FC0, top), (0xFFC0, top)):
            x = base.clone()
            x[pos] = _bits16([bits])[0]
            y, amax = _fill8(n), _scalar(0.0)
            ops.quantize_fp8(x.to(DEV), y, amax=amax)
            assert float(amax) == want, (pos, hex(bits), float(amax))
            _same_bytes(_u8(y), E.quantize_ref(x.float()), f"non-finite 0x{bits:04X} at {pos}")


# ----------------------------------------------------------------------------- attention
B_, H_, DH = 2, 3, 64
FWD_N = [1, 37, 64, 65, 128, 129, 197, 224]
BWD_N = FWD_N + [225, 256]
TWO_BYTE_MAX = 1.0 / 8          # twice the constructed 1 / 16: a degenerate input cannot hide behind the alternative byte


def _qkv(B, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * N, 3 * H * DH, generator=g).to(BF16).to(DEV)


def _dout(B, N, H, seed):
    """Gaussian x 1e-3; the odd feature columns 2^-18 .. 2^-21 of that.  dV = P^T dO keeps a column's magnitude, so one image holds
    gradients 2^21 apart: at the larger of the two scales the even columns saturate while the odd ones land in the e4m3 subnormals."""
    g = torch.Generator().manual_seed(seed)
    d = torch.arange(H * DH)
    col = torch.where(d % 2 == 1, torch.exp2(-(18.0 + (d // 2) % 4)), torch.ones(()))
    return (torch.randn(B * N, H * DH, generator=g) * 1e-3 * col).to(BF16).to(DEV)


def _fwd_case(ops, B, N, H, seed=0, qkv=None):
    qkv = _qkv(B, N, H, seed) if qkv is None else qkv
    out0, out = _nan16(B * N, H * DH), _nan16(B * N, H * DH)
    out8 = _fill8(B * N, H * DH)
    lse = torch.empty(B, H, N, device=DEV)
    ops.attn_fwd(qkv, out0, lse, B, N, H, DH)
    ops.attn_fwd(qkv, out, lse, B, N, H, DH, out_fp8=out8)
    assert torch.equal(out.view(torch.int16), out0.view(torch.int16)), "bf16 output differs from the non-fp8 entry point's"
    return qkv, out, out8, lse


@pytest.mark.parametrize("N", FWD_N)
def test_attention_forward_image(ops, N):
    _, out, out8, _ = _fwd_case(ops, B_, N, H_, seed=N)
    st = E.check_image(out8, out, 1.0, f"attn_fwd_fp8 N = {N}")
    print(f"attn_fwd_fp8 N={N}: {st}")
    assert st["nan"] == 0 and st["two_byte"] <= TWO_BYTE_MAX, st


def _bwd_case(ops, B, N, H, seed):
    """-> per scale (in range, 2^5 larger): coverage of the image; asserts everything the issue lists"""
    qkv = _qkv(B, N, H, seed)
    out = torch.empty(B * N, H * DH, dtype=BF16, device=DEV)
    lse = torch.empty(B, H, N, device=DEV)
    ops.attn_fwd(qkv, out, lse, B, N, H, DH)
    dout = _dout(B, N, H, seed + 1000)
    delta = torch.empty(B, H, N, device=DEV)
    d0 = _nan16(B * N, 3 * H * DH)
    ops.attn_bwd(qkv, out, dout, lse, d0, delta, B, N, H, DH)
    top = d0.float().abs().max()
    assert math.isfinite(float(top)) and float(top) > 0
    from oracle import vit_oracle as O
    k = O.fp8_scale_exp(float(top))                     # largest power of two that keeps max |dqkv| at or below 448
    stats = []
    for s in (2.0 ** k, 2.0 ** (k + 5)):
        what = f"attn_bwd_fp8 N = {N} scale 2^{int(math.log2(s))}"
        d1, d8 = _nan16(B * N, 3 * H * DH), _fill8(B * N, 3 * H * DH)
        scale, amax = _scalar(s), _scalar(0.0)
        ops.attn_bwd(qkv, out, dout, lse, d1, delta, B, N, H, DH, dqkv_fp8=d8, scale=scale, amax=amax)
        assert torch.equal(d1.view(torch.int16), d0.view(torch.int16)), f"{what}: bf16 gradients differ from the non-fp8 entry point's"
        st = E.check_image(d8, d1, s, what)
        print(f"{what}: {st}")
        # rounding to bf16 is monotone: the bf16 image of the fp32 maximum is the maximum of the bf16 image
        assert torch.equal(amax.to(BF16).view(torch.int16), top.to(BF16).view(torch.int16).reshape(1)), (what, float(amax), float(top))
        d8n, amaxn = _fill8(B * N, 3 * H * DH), _scalar(0.0)
        ops.attn_bwd(qkv, out, dout, lse, None, delta, B, N, H, DH, dqkv_fp8=d8n, scale=scale, amax=amaxn)
        assert torch.equal(d8n.view(torch.uint8), d8.view(torch.uint8)), f"{what}: image without the bf16 output differs"
        assert torch.equal(amaxn.view(torch.int32), amax.view(torch.int32)), f"{what}: maximum without the bf16 output differs"
        assert st["nan"] == 0 and st["two_byte"] <= TWO_BYTE_MAX, (what, st)
        stats.append(st)
    assert stats[0]["saturated"] <= stats[1]["saturated"] and stats[1]["saturated"] >= 100, stats
    assert stats[1]["subnormal"] >= 100, stats
    return stats


@pytest.mark.parametrize("N", BWD_N)
def test_attention_backward_image(ops, N):
    _bwd_case(ops, B_, N, H_, seed=N)


@pytest.fixture
def reserve():
    """set(n) -> vitssl_set_reserved_cus(n); the count in force before the test is restored afterwards, also on failure."""
    from vitssl_hip import _lib as L
    lib = L.lib()
    old = lib.vitssl_get_reserved_cus()

    def set_(n):
        L.call("vitssl_set_reserved_cus", C.c_int(n))
        assert lib.vitssl_get_reserved_cus() == n
    yield set_
    torch.cuda.synchronize()
    L.call("vitssl_set_reserved_cus", C.c_int(old))
    assert lib.vitssl_get_reserved_cus() == old


def test_attention_images_swept_items(ops, reserve):
    """27 items on 8 workgroups: the persistent forward and backward sweep 3-4 items each, every image byte judged"""
    from vitssl_hip import _lib as L
    B, N, H = 9, 197, 3
    reserve(torch.cuda.get_device_properties(0).multi_processor_count - 8)
    _, out, out8, _ = _fwd_case(ops, B, N, H, seed=7)
    assert L.lib().vitssl_debug_last_attn_fwd_grid() == 8
    st = E.check_image(out8, out, 1.0, "attn_fwd_fp8, 27 items on 8 workgroups")
    assert st["two_byte"] <= TWO_BYTE_MAX, st
    _bwd_case(ops, B, N, H, seed=8)


@pytest.mark.parametrize("N", [37, 197])
def test_attention_forward_image_keeps_nan(ops, N):
    """one NaN in a V row: every query of that (image, head) gets a NaN in that feature; NaN in bf16 <=> NaN byte in the image"""
    B, H = B_, H_
    qkv = _qkv(B, N, H, seed=50 + N)
    b, tok, h, d = 1, N // 3, 2, 21
    qkv[b * N + tok, 2 * H * DH + h * DH + d] = math.nan
    _, out, out8, _ = _fwd_case(ops, B, N, H, qkv=qkv)
    nan16 = torch.isnan(out).cpu().numpy()
    want = np.zeros_like(nan16)
    want[b * N:(b + 1) * N, h * DH + d] = True
    assert np.array_equal(nan16, want), "the NaN of V reached other elements of the bf16 output (or missed some)"
    got = _u8(out8).copy()
    nan8 = (got & 0x7F) == 0x7F
    assert np.array_equal(nan8, nan16), f"{int(nan16.sum())} NaN in bf16, {int(nan8.sum())} NaN bytes, {int((nan8 & nan16).sum())} in common"
    # the sign of a computed NaN is not part of the contract: give the checker the sign the bf16 image carries
    sign = (out.cpu().view(torch.int16).numpy() < 0)
    got[nan16] = np.where(sign[nan16], 0xFF, 0x7F)
    st = E.check_image(got, out, 1.0, f"attn_fwd_fp8 N = {N} with a NaN in V")
    assert st["nan"] == N


# ----------------------------------------------------------------------------- weight images
W_SHAPES = [(6, 7), (7, 8), (8, 7), (8, 8), (65, 129), (129, 65), (64, 64)]
STEP_UP, STEP_DOWN = 1, -1


def _fp32_step(v, steps):
    return float((torch.tensor([v], dtype=torch.float32).view(torch.int32) + steps).view(torch.float32))


def _w_sources(top, seed):
    """per shape one source with max |w| = top exactly (the last element of the first one: the amax kernel's scalar tail), the
    others Gaussian at a quarter of it, cut off at 0.99 top"""
    g = torch.Generator().manual_seed(seed)
    srcs = []
    for i, s in enumerate(W_SHAPES):
        w = (torch.randn(*s, generator=g) * (top / 4)).clamp(-0.99 * top, 0.99 * top)
        pos = (s[0] - 1, s[1] - 1) if i % 2 == 0 else (s[0] // 2, 0)
        w[pos] = top if i % 3 else -top
        srcs.append(w)
    return srcs


def _w_jobs(srcs):
    """every source three times: only dst, only dst_t, both"""
    jobs = []
    for w in srcs:
        for has_d, has_t in ((True, False), (False, True), (True, True)):
            jobs.append((w.to(DEV), _fill8(*w.shape) if has_d else None, _fill8(w.shape[1], w.shape[0]) if has_t else None))
    return jobs


def _w_check(plan, jobs, what, k_want=None):
    from oracle import vit_oracle as O
    alpha = plan.alpha.cpu()
    for i, (w, d, t) in enumerate(jobs):
        wc = w.cpu()
        finite_max = float(wc[~torch.isnan(wc)].abs().max())
        k = O.fp8_scale_exp(finite_max) if k_want is None else k_want
        tag = f"{what}: job {i} {tuple(wc.shape)}"
        assert float(alpha[i]) == 2.0 ** -k, (tag, float(alpha[i]), k)
        want = E.quantize_ref(wc, 2.0 ** k)
        if d is not None:
            _same_bytes(_u8(d).ravel(), want.ravel(), tag + " dst")
        if t is not None:
            _same_bytes(_u8(t).ravel(), np.ascontiguousarray(want.T).ravel(), tag + " dst_t")
    return alpha


W_TOPS = {"on the boundary": 448.0 * 2.0 ** -11, "one step above": _fp32_step(448.0 * 2.0 ** -11, STEP_UP),
          "one step below": _fp32_step(448.0 * 2.0 ** -11, STEP_DOWN), "exponent clamp": 1e-40, "near FLT_MAX": 3.2e38}
W_EXP = {"on the boundary": 11, "one step above": 10, "one step below": 11, "exponent clamp": 120, "near FLT_MAX": -120}


@pytest.mark.parametrize("case", list(W_TOPS))
def test_weight_images_planted_maximum(ops, case):
    from oracle import vit_oracle as O
    top = W_TOPS[case]
    assert O.fp8_scale_exp(top) == W_EXP[case]
    jobs = _w_jobs(_w_sources(top, seed=len(case)))
    plan = ops.Fp8WeightPlan()
    plan.run(jobs)
    _w_check(plan, jobs, case, k_want=W_EXP[case])


@pytest.mark.parametrize("kind", ["inf", "nan"])
def test_weight_images_non_finite(ops, kind):
    """An infinity: the maximum is +inf, the exponent rule answers 0 (alpha = 1), the infinity saturates to +-448.  A NaN: the
    maximum ignores it (the exponent is that of the other elements), its byte is a NaN byte."""
    srcs = _w_sources(0.3, seed=9)
    for i, w in enumerate(srcs):
        w[min(3, w.shape[0] - 1), 2] = {"inf": (-1) ** i * math.inf, "nan": math.nan}[kind]
    jobs = _w_jobs(srcs)
    plan = ops.Fp8WeightPlan()
    plan.run(jobs)
    _w_check(plan, jobs, kind, k_want={"inf": 0, "nan": 10}[kind])      # 0.3 = 0.6 x 2^-1: k = 9 + 1
    for w, d, t in jobs:
        r, byte = min(3, w.shape[0] - 1), {"inf": None, "nan": 0x7F}[kind]
        for img, at in ((d, (r, 2)), (t, (2, r))):
            if img is not None:
                got = int(_u8(img)[at])
                assert got == byte if byte is not None else got in (0x7E, 0xFE), (kind, tuple(w.shape), hex(got))


def test_weight_images_follow_sources_changed_in_place(ops):
    """one plan, three runs: the sources x 2^-3 (a smaller maximum than the run before: nothing may be left of the old one), then
    x 2^5"""
    jobs = _w_jobs(_w_sources(1.7, seed=10))
    plan = ops.Fp8WeightPlan()
    plan.run(jobs)
    a0 = _w_check(plan, jobs, "first run").clone()
    for factor in (2.0 ** -3, 2.0 ** 5):
        for w in {id(j[0]): j[0] for j in jobs}.values():
            w.mul_(factor)
        for _, d, t in jobs:
            for img in (d, t):
                if img is not None:
                    img.view(torch.uint8).fill_(0x7F)
        plan.run(jobs)
        a1 = _w_check(plan, jobs, f"after x {factor}")
        assert torch.equal(a1, a0 * factor)
        a0 = a1.clone()
