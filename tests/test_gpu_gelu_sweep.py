"""EPI_GELU on every finite bf16 pre-activation: the ping-pong kernel's table against the arithmetic it is filled from.

tests/_gelu_sweep.py plants a chosen bf16 pattern at every element of the pre-activation (K = 64, A a cyclic identity, B the
patterns), so u is exact and the two bf16 outputs are judged per element against a float64 reference at
2^-8 |s ref| + c s max(|u|, 1), c = 4 c_ref (c_ref from the float32 restatement of gelu_both_scaled, test_gelu_sweep_host.py).
Launches (csrc/gemm_nt.hip, launch_nt), each with the arrangements table / arith / mixed:

  pp     M = N = 2048, K = 64   64 tiles of 256 x 256, N % 8 == 0: ping-pong kernel, results by table for 2^-14 <= |u| < 16
  small  M = 64, N = 2048       fewer than 64 tiles: gemm_nt_kernel, arithmetic only
  odd    M = 64, N = 2052       N % 8 == 4: gemm_nt_kernel, stores in the accumulator layout
  fp8    M = 64, K = 128, N = 65536, B8 = 0, u planted through the fp32 bias along the columns: ping-pong kernel; the table serves
         the launch that writes g' and the e4m3 image only, the launch with out1 and out_amax is arithmetic

1 the EPI_BF16 image of the same operands is the planted one (a denormal may come back as a signed zero); the references are
  gathered from that image
2 both outputs meet the bar at p = 0, 0.5, 0.3; dropped elements are +0
3 p = 0: every pattern has ONE pair of result bits over all its occurrences in all nine launches -- the "bit-identical" claim of
  the table's comment; a neighbouring or mis-packed entry fails here outright
4 p = 0.5 (s = 2): keep x 2 x (p = 0 result), bit for bit, wherever the p = 0 result is a normal bf16 in [2^-125, 2^126).  (One
  binade above the smallest normal: u = +-0x00ff gives the fp32 value 2^-126 - 2^-134, which ties up to the NORMAL bf16 2^-126,
  while twice it is the bf16 number 2^-125 - 2^-133 itself; from 2^-125 on the fp32 value behind the bf16 result is normal and
  doubling commutes with the rounding.)
5 fp8 operands: the table launch and the arithmetic launch write the same out0 bits and e4m3 bytes; the e4m3 image meets
  2^-4 |s ref| + 2^-10 / out_scale + c s max(|u|, 1), saturates at +-448 / out_scale; out_amax to 2^-8 relative

Outputs start as NaN (a 7.0 sentinel would pass as gelu(7)): an element the kernel does not write misses every check.
Each test prints the smallest c its launch needed; run with -s to see them."""
import functools
import math
import os

import pytest
import torch

import _gelu_sweep as S
import _gemm_exact as X

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32, FP8 = S.BF16, S.F32, S.FP8
KERNELS = {"pp": (2048, 2048), "small": (64, 2048), "odd": (64, 2052)}
ARRS = ["table", "arith", "mixed"]
PS = [0.0, 0.5, 0.3]
FP8_SHAPE = (64, 128, 65536)      # M, K, N
OUT_SCALE = 64.0                  # e4m3 saturates from s gelu(u) = 7 on: inside the table's range as well
SEEDS = {"table": 11, "arith": 12, "mixed": 13}

kernels = pytest.mark.parametrize("kern", list(KERNELS))
arrs = pytest.mark.parametrize("arr", ARRS)


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from vitssl_hip import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def _release_images():
    """the cached images of this file (a few hundred MB on the host) go when its last test has run"""
    yield
    for f in (_case, _preact, _gelu, _fp8_case):
        f.cache_clear()


def _c_gpu():
    return S.C_GPU_FACTOR * S.c_ref()


def _nan(shape, dtype=BF16):
    t = torch.full(shape, math.nan, dtype=BF16, device=DEV)
    return t if dtype == BF16 else t.to(dtype)


def _drop(ops, p):
    return ops.make_dropout(p, seed=5, site=11)


def _knob(name):
    return int(os.environ.get(name, "0") or 0)


@functools.lru_cache(maxsize=None)
def _case(kern, arr):
    """operands and the planted image of a launch, made once and shared by all tests (left unchanged)"""
    M, N = KERNELS[kern]
    A, B, planted = S.plant(M, N, S.arrange(arr, N * S.K_PLANT, seed=SEEDS[arr] + N))
    return {"A": A.to(DEV), "B": B.to(DEV), "planted": planted}


@functools.lru_cache(maxsize=None)
def _preact(kern, arr):
    """the EPI_BF16 image of the case's operands as patterns: the u of every reference"""
    from vitssl_hip import _lib, ops
    c = _case(kern, arr)
    out = _nan(KERNELS[kern])
    ops.gemm_nt(c["A"], c["B"], out, _lib.EPI_BF16)
    return S.bits_of(out)


@functools.lru_cache(maxsize=None)
def _gelu(kern, arr, p):
    """-> (out0 = s gelu' bits, out1 = s gelu bits, keep or None) of one EPI_GELU launch, on the CPU"""
    from vitssl_hip import _lib, ops
    c = _case(kern, arr)
    M, N = KERNELS[kern]
    drop = _drop(ops, p)
    gp, a = _nan((M, N)), _nan((M, N))
    ops.gemm_nt(c["A"], c["B"], gp, _lib.EPI_GELU, out1=a, drop=drop)
    keep = ops.dropout_mask(M, N, drop, DEV).cpu().bool() if p else None
    return S.bits_of(gp), S.bits_of(a), keep


def _check_planted(got, planted, what):
    """item 1: normal patterns come back as planted, denormal ones as planted or as a signed zero"""
    normal = ((planted >> 7) & 0xFF) != 0
    bad = (got != planted) & (normal | ((got & 0x7FFF) != 0))
    if bool(bad.any()):
        r, col = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} pre-activations are not the planted pattern; first at (row {r}, col {col}): "
                             f"planted 0x{int(planted[r, col]):04x}, got 0x{int(got[r, col]):04x}")


def _check_outputs(gp_bits, a_bits, u_bits, keep, p, what):
    """item 2 for one launch -> the smallest c it needed"""
    s = S.drop_scale(p)
    u = S.VALUES[u_bits.long()]
    g, d = S.reference()
    k = keep.double() if keep is not None else 1.0
    # p > 0: s u overflows bf16 for |u| >= 2^126, in the reference as well
    mask = None if p == 0 else ((u_bits >> 7) & 0xFF) < 253
    need = 0.0
    for name, bits, ref in (("out1 = s gelu(u)", a_bits, g), ("out0 = s gelu'(u)", gp_bits, d)):
        got, want = S.VALUES[bits.long()], s * k * ref[u_bits.long()]
        n = S.needed_c(got, want, u, s, mask=mask)
        print(f"{what} {name}: smallest c that passes {n:.4e} (bar {_c_gpu():.4e}, c_ref {S.c_ref():.4e})")
        need = max(need, n)
        S.check_bar(got, want, u_bits, s, _c_gpu(), f"{what} {name}", mask=mask)
        if keep is not None:
            assert bool((bits[~keep] == 0).all()), f"{what} {name}: a dropped element is not +0"
    return need


def _check_same_bits(a, b, u_bits, what, names, cap=6):
    bad = a != b
    if bool(bad.any()):
        lines = [f"pattern 0x{int(u_bits[r, c]):04x} at (row {r}, col {c}): {names[0]} 0x{int(a[r, c]):x}, {names[1]} 0x{int(b[r, c]):x}"
                 for r, c in bad.nonzero()[:cap].tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in {len(torch.unique(u_bits[bad]))} patterns; " + "; ".join(lines))


# ----------------------------------------------------------------------------- bf16 operands
def test_launch_paths(ops, L):
    """the shapes select the kernels the case names promise: the ping-pong launch records its grid, the other two leave it alone"""
    if _knob("VITSSL_NT_TILE"):
        return                                                   # a forced tile: the other tests still hold, the path is the knob's
    G = torch.cuda.get_device_properties(0).multi_processor_count - L.lib().vitssl_get_reserved_cus()
    M, N = KERNELS["pp"]
    kind, rows = X.nt_tile_rows(M, N, G)
    assert kind == "big" and N % 8 == 0
    pp_grid = min(math.ceil(M / rows) * math.ceil(N / 256), G)
    _gelu.__wrapped__("pp", "table", 0.0)
    assert L.lib().vitssl_debug_last_nt_grid() == pp_grid, (L.lib().vitssl_debug_last_nt_grid(), pp_grid)
    for kern in ("small", "odd"):
        M, N = KERNELS[kern]
        assert X.nt_tile_rows(M, N, G)[0] == "small"
        _gelu.__wrapped__(kern, "table", 0.0)
        if math.ceil(N / 256) != pp_grid:                        # (the grid a ping-pong launch of this shape would have recorded)
            assert L.lib().vitssl_debug_last_nt_grid() == pp_grid, f"{kern}: the ping-pong kernel ran"
    assert KERNELS["odd"][1] % 8 == 4


@arrs
@kernels
def test_preactivation_is_planted(kern, arr):
    planted = _case(kern, arr)["planted"]
    _check_planted(_preact(kern, arr), planted, f"{kern} {arr} EPI_BF16")
    inside = S.IN_TABLE[planted.long()]
    assert {"table": bool(inside.all()), "arith": not bool(inside.all()), "mixed": bool(inside.any()) and not bool(inside.all())}[arr]


@pytest.mark.parametrize("p", PS, ids=lambda p: f"p{p}")
@arrs
@kernels
def test_gelu_accuracy(kern, arr, p):
    gp, a, keep = _gelu(kern, arr, p)
    assert p == 0 or abs(float(keep.double().mean()) - (1 - p)) < 0.02
    need = _check_outputs(gp, a, _preact(kern, arr), keep, p, f"EPI_GELU {kern} {arr} p={p}")
    assert need <= _c_gpu()


def test_gelu_is_one_function_of_u():
    tables = {}
    for kern in KERNELS:
        for arr in ARRS:
            gp, a, _ = _gelu(kern, arr, 0.0)
            tables[f"{kern}/{arr}"] = S.per_pattern(_case(kern, arr)["planted"], (gp.long() << 16) | a.long())
    n = S.check_one_function(tables, "EPI_GELU p=0, (out0 bits << 16) | out1 bits by pattern")
    assert n == len(S.FINITE), n


@arrs
@kernels
def test_half_dropout_doubles_exactly(kern, arr):
    gp0, a0, _ = _gelu(kern, arr, 0.0)
    gp5, a5, keep = _gelu(kern, arr, 0.5)
    assert S.drop_scale(0.5) == 2.0 and 0.48 < float(keep.double().mean()) < 0.52
    u_bits = _case(kern, arr)["planted"]
    for name, b0, b5 in (("out1", a0, a5), ("out0", gp0, gp5)):
        e = (b0 >> 7) & 0xFF
        doubles = keep & (e >= 2) & (e < 253)
        assert bool(doubles.any())
        want = torch.where(doubles, b0 + 128, b5)                      # one more in the exponent field
        want = torch.where(keep, want, torch.zeros_like(want))
        _check_same_bits(b5, want, u_bits, f"EPI_GELU {kern} {arr} {name}: p = 0.5 against keep x 2 x (p = 0)", ("p = 0.5", "expected"))


# ----------------------------------------------------------------------------- fp8 operands
def _scalar(v):
    return torch.tensor([v], device=DEV)


@functools.lru_cache(maxsize=None)
def _fp8_case(arr):
    M, K, N = FP8_SHAPE
    pats = S.arrange(arr, N, seed=SEEDS[arr])
    bias = S.VALUES[pats.long()].float()
    assert torch.equal(S.bits_of(bias.to(BF16)), pats)
    A8 = torch.ones(M, K).to(FP8).to(DEV)
    B8 = torch.zeros(N, K).to(FP8).to(DEV)
    return {"A8": A8, "B8": B8, "bias": bias.to(DEV), "planted": pats.view(1, N).expand(M, N).contiguous()}


@pytest.mark.parametrize("p", [0.0, 0.5], ids=lambda p: f"p{p}")
@arrs
def test_fp8_table_and_arithmetic(ops, L, arr, p):
    M, K, N = FP8_SHAPE
    c = _fp8_case(arr)
    what = f"fp8 EPI_GELU {arr} p={p}"
    pre = _nan((M, N))
    ops.gemm_fp8_nt(c["A8"], c["B8"], pre, L.EPI_BF16, bias=c["bias"])
    u_bits = S.bits_of(pre)
    _check_planted(u_bits, c["planted"], f"fp8 {arr} EPI_BF16")

    drop, s, qs = _drop(ops, p), S.drop_scale(p), _scalar(OUT_SCALE)
    keep = ops.dropout_mask(M, N, drop, DEV).cpu().bool() if p else None
    gp_t, q_t = _nan((M, N)), _nan((M, N), FP8)
    ops.gemm_fp8_nt(c["A8"], c["B8"], gp_t, L.EPI_GELU, bias=c["bias"], out_fp8=q_t, out_scale=qs, drop=drop)       # table
    G = torch.cuda.get_device_properties(0).multi_processor_count - L.lib().vitssl_get_reserved_cus()
    assert L.lib().vitssl_debug_last_nt_grid() == min(math.ceil(N / 256), G)
    gp_a, a_a, q_a, amax = _nan((M, N)), _nan((M, N)), _nan((M, N), FP8), torch.zeros(1, device=DEV)
    ops.gemm_fp8_nt(c["A8"], c["B8"], gp_a, L.EPI_GELU, bias=c["bias"], out1=a_a, out_fp8=q_a, out_scale=qs, out_amax=amax, drop=drop)
    gp_t, gp_a, a_a = S.bits_of(gp_t), S.bits_of(gp_a), S.bits_of(a_a)
    q_t, q_a = q_t.cpu().view(torch.uint8).to(torch.int32), q_a.cpu().view(torch.uint8).to(torch.int32)
    _check_same_bits(gp_t, gp_a, u_bits, f"{what}: out0", ("table launch", "arithmetic launch"))
    _check_same_bits(q_t, q_a, u_bits, f"{what}: e4m3 image", ("table launch", "arithmetic launch"))

    need = _check_outputs(gp_a, a_a, u_bits, keep, p, what)
    u = S.VALUES[u_bits.long()]
    sref = s * (keep.double() if keep is not None else 1.0) * S.reference()[0][u_bits.long()]
    assert not bool(((q_t & 0x7F) == 0x7F).any()), f"{what}: nan bytes in the e4m3 image"
    deq = q_t.to(torch.uint8).view(FP8).float().double() / OUT_SCALE
    want = sref.clamp(-448.0 / OUT_SCALE, 448.0 / OUT_SCALE)
    n8 = S.needed_c(deq, want, u, s, rel=S.REL_E4M3, extra=S.ABS_E4M3 / OUT_SCALE)
    print(f"{what} e4m3 image: smallest c that passes {n8:.4e}")
    S.check_bar(deq, want, u_bits, s, _c_gpu(), f"{what} e4m3 image / out_scale", rel=S.REL_E4M3, extra=S.ABS_E4M3 / OUT_SCALE)
    # saturation as the suite's quantiser: past the midpoint of 448 and the 512 that e4m3 does not have, the byte is +-448
    sat = (sref * OUT_SCALE).abs() > 481.0
    want8 = S.q8((sref * OUT_SCALE).float()).view(torch.uint8).to(torch.int32)
    assert bool(sat.any()) and bool(((want8[sat] & 0x7F) == 0x7E).all())
    _check_same_bits(torch.where(sat, q_t, want8), want8, u_bits, f"{what}: saturated e4m3 bytes", ("kernel", "quantiser"))
    if keep is not None:
        assert bool((q_t[~keep] == 0).all()), f"{what}: a dropped e4m3 byte is not +0"
    # the fp32 maximum: s u overflows fp32 at p = 0.5 for the largest kept |u| of `arith` and `mixed`, in the reference as well
    want_max = sref.abs().max().float()
    got_max = float(amax)
    print(f"{what} out_amax: got {got_max:.9g}, want {float(want_max):.9g}")
    if math.isinf(float(want_max)):
        assert math.isinf(got_max) and got_max > 0
    else:
        assert abs(got_max - float(want_max)) <= 2.0 ** -8 * float(want_max), (got_max, float(want_max))
    assert need <= _c_gpu() and n8 <= _c_gpu()
