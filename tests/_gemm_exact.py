"""Small-integer GEMM operands, an integer reference and a bit-for-bit checker (no GPU code).

With operands from {+-lo..+-hi} every product is an exact integer and every partial sum stays below 2^24, so fp32 accumulation is
exact IN ANY ORDER: the MFMA's own, split-K atomics, slab / slot reduces, helper workgroups and the fixed-order column sums must
all give the same bits as an integer matmul.  A dropped, duplicated or misaddressed row, column, K-tile, split, slab or bias is
then an integer difference at a known (row, col), which no whole-matrix tolerance hides.  Two regimes:
  small  hi = 1, K <= 128: |acc + bias| <= 136 < 256, every bf16 output is representable, nothing rounds anywhere
  round  hi = 3, larger K: |acc| passes 256 and a bf16 store must be the ONE round-to-nearest-even of the exact fp32 value.
The generators assert the exactness bound themselves: a case that violates it is a mistake in the test, not a skip."""
import torch

BF16, F32, FP8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
EXACT = 1 << 24          # integers of magnitude below 2^24 are exact in fp32
BIAS_MAX = 8
TILE = 256               # output tile edge of the GEMM kernels (the checker reports the tiles of the bad blocks)


def regime_hi(regime, K):
    if regime == "small":
        assert K <= 128, f"the `small` regime needs K <= 128 (|acc + bias| < 256), got K = {K}"
        return 1
    assert regime == "round", regime
    return 3


def _ints(shape, lo, hi, g):
    """integers from {+-lo..+-hi}: no zeros, so every single product matters"""
    mag = torch.randint(lo, hi + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).to(F32)


def operands(M, N, K, seed, lo=1, hi=3, colsum=False, scale=1.0):
    """-> bf16 A[M,K], B[N,K] from {+-lo..+-hi} and an integer-valued fp32 bias[N] in [-8, 8].  `scale`: the factor the
    accumulator is multiplied by (fp8 alpha x alpha2, a power of two), part of the bound."""
    assert 1 <= lo <= hi <= 3, "e4m3 and bf16 hold the integers up to 3 exactly; the bound below is written for them"
    bound = scale * K * hi * hi + BIAS_MAX
    assert bound < EXACT, f"K * hi^2 + 8 = {bound} >= 2^24: fp32 accumulation is no longer exact"
    if colsum:
        assert M * bound < EXACT, f"M * (K * hi^2 + 8) = {M * bound} >= 2^24: the column sums are no longer exact"
    g = torch.Generator().manual_seed(seed)
    A, B = _ints((M, K), lo, hi, g), _ints((N, K), lo, hi, g)
    bias = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (N,), generator=g).to(F32)
    return A.to(BF16), B.to(BF16), bias


def operands_tn(M, N1, N2, seed, lo=1, hi=3, c0_max=64, calls=2, scale=1.0):
    """-> bf16 A[M,N1], B[M,N2] and an integer fp32 C0[N1,N2]; exact for `calls` accumulating calls."""
    assert 1 <= lo <= hi <= 3
    bound = calls * scale * M * hi * hi + c0_max
    assert bound < EXACT, f"M * hi^2 + |C0| = {bound} >= 2^24: fp32 accumulation is no longer exact"
    g = torch.Generator().manual_seed(seed)
    A, B = _ints((M, N1), lo, hi, g), _ints((M, N2), lo, hi, g)
    C0 = torch.randint(-c0_max, c0_max + 1, (N1, N2), generator=g).to(F32)
    return A.to(BF16), B.to(BF16), C0


def to_fp8(x):
    """the same integers as e4m3 bytes (integers up to 3 are exact in e4m3)"""
    y = x.float().to(FP8)
    assert torch.equal(y.float(), x.float())
    return y


def int_values(shape, lo, hi, seed):
    """integer-valued fp32 tensor in [lo, hi] (residuals, position tables, mask tokens, gradients)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(F32)


def dgelu_aux(M, N, seed):
    """bf16 g' values from {0, +-0.5, +-1, +-2}: acc * aux is exact in fp32"""
    g = torch.Generator().manual_seed(seed)
    table = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
    return table[torch.randint(0, 7, (M, N), generator=g)].to(BF16)


def ref_nt(A, B, fp32=False):
    """A @ B^T as an exact integer-valued fp64 (or, for the largest cases, fp32: exact too under the bound) matrix"""
    if fp32:
        return (A.float() @ B.float().t()).double()
    return A.double() @ B.double().t()


def ref_tn(A, B, fp32=False):
    if fp32:
        return (A.float().t() @ B.float()).double()
    return A.double().t() @ B.double()


def to_f32_exact(x64):
    """fp64 -> fp32; asserts that nothing was rounded (the bound of the generators holds for this value)"""
    y = x64.float()
    assert torch.equal(y.double(), x64), "reference value is not representable in fp32: the case violates the exactness bound"
    return y


def bf16_rne(x64):
    """the single round-to-nearest-even bf16 image of an exact value"""
    return to_f32_exact(x64).to(BF16)


def _bits(x):
    x = x.detach().cpu().contiguous()
    if x.dtype == BF16:
        return x.view(torch.int16).to(torch.int32) & 0xFFFF, 0x7FFF
    if x.dtype == F32:
        return x.view(torch.int32), 0x7FFFFFFF
    if x.dtype == FP8:
        return x.view(torch.uint8).to(torch.int32), 0x7F
    raise TypeError(x.dtype)


def check_exact(got, want, what, block=(16, 16), cap=8):
    """Every element of `got` equals `want` bit for bit (+0 and -0 taken as equal: a dropped element is an exact +0 in the
    kernels, `x * 0` keeps the sign of x).  No sampling, no allowed share of misses.  On a mismatch the AssertionError names the
    count, the first bad (row, col, got, want), the distinct bad blocks with the 256 x 256 tiles they fall in, and whether the
    difference is constant over the bad region (constant: a bias or one product; not constant: a K-tile or an address)."""
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.detach().cpu(), want.detach().cpu()
    if g.dim() == 1:
        g, w = g.unsqueeze(0), w.unsqueeze(0)
    gb, absmask = _bits(g)
    wb, _ = _bits(w)
    bad = (gb != wb) & ~(((gb & absmask) == 0) & ((wb & absmask) == 0))
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    r0, c0 = (int(v) for v in idx[0])
    blocks = torch.unique(torch.stack((idx[:, 0] // block[0], idx[:, 1] // block[1]), 1), dim=0)
    tiles = torch.unique(torch.stack((idx[:, 0] // TILE, idx[:, 1] // TILE), 1), dim=0)
    diff = (g.double() - w.double())[bad]
    finite = bool(torch.isfinite(diff).all())
    if finite and float(diff.min()) == float(diff.max()):
        kind = f"constant difference {float(diff[0]):g} over the bad region (a bias or one product?)"
    elif finite:
        kind = f"differences from {float(diff.min()):g} to {float(diff.max()):g} (a K-tile or an address?)"
    else:
        kind = "non-finite values in the bad region"

    def listing(t):
        s = ", ".join(f"({int(a)}, {int(b)})" for a, b in t[:cap])
        return s + (f", ... {len(t) - cap} more" if len(t) > cap else "")
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at (row {r0}, col {c0}): got {float(g[r0, c0]):g}, "
        f"want {float(w[r0, c0]):g}; {len(blocks)} bad {block[0]}x{block[1]} block(s) (block row, block col): {listing(blocks)}; "
        f"in {len(tiles)} {TILE}x{TILE} tile(s) (tile row, tile col): {listing(tiles)}; {kind}")


# ---- the host-side split plans of csrc/gemm_tn.hip, restated: the GPU tests assert through them (and the library's own workspace
# ---- answers) that a shape takes the combination path its comment names
def _cdiv(a, b):
    return -(-a // b)


def tn_plan(M, N1, N2, G, km=64):
    """vitssl_gemm_bf16_tn with G usable CUs -> (tiles, splits, chunks_per_split); splits == 1 is the direct mode"""
    tiles = _cdiv(N1, TILE) * _cdiv(N2, TILE)
    total = _cdiv(M, km)
    sp = max(1, min(G // tiles, total))
    cps = _cdiv(total, sp)
    return tiles, _cdiv(total, cps), cps


def tn_batch_plan(M, T, G, km=64, forced=0, use_rem=True):
    """vitssl_gemm_bf16_tn_batch over T tiles with G usable CUs -> (splits, chunks_per_split, rem_chunks); rem_chunks > 0 is the
    helper-workgroup plan.  `forced` / `use_rem`: the VITSSL_TN_BATCH_SPLITS / VITSSL_TN_BATCH_REM knobs."""
    total = _cdiv(M, km)
    c_kt, c_unit, c_part, c_rem = 1.46, 9.0, 0.15, 2.2
    best, best_s = 1e30, 1
    for sp in range(1, min(total, 64) + 1):
        cps = _cdiv(total, sp)
        if _cdiv(total, cps) != sp:
            continue
        units = T * sp
        cost = _cdiv(units, G) * (cps * c_kt + c_unit) + (units * c_part if sp > 1 else 0.0)
        if cost < best:
            best, best_s = cost, sp
    if 0 < forced <= total:
        best_s = forced
    cps = _cdiv(total, best_s)
    S = _cdiv(total, cps)
    rem = 0
    R = G - T * S
    if use_rem and T * S <= G and R >= 8:
        nr = float(_cdiv(T, R))
        L = (nr * (total * c_rem + c_unit) - c_unit) / (c_kt + nr * S * c_rem)
        Li = int(L + 0.999)
        r = total - S * Li
        t_main, t_rem, t_old = Li * c_kt + c_unit, nr * (r * c_rem + c_unit), cps * c_kt + c_unit
        tax = T * c_part * (2.0 if S == 1 else 1.0)
        if r >= 4 and Li >= 4 and max(t_main, t_rem) + tax < 0.95 * t_old:
            cps, rem = Li, r
    return S, cps, rem


def tn_batch_workspace(M, T, G, **kw):
    S, _, rem = tn_batch_plan(M, T, G, **kw)
    return (S + (rem > 0)) * T * TILE * TILE if (S > 1 or rem > 0) else 0


def nt_tile_rows(M, N, G):
    """launch_nt's choice for bf16 operands with G usable CUs and no VITSSL_NT_TILE -> ("small", 256) or ("big", 256 / 224 / 192)"""
    if _cdiv(M, 256) * _cdiv(N, 256) < 64:
        return "small", 256
    tn = _cdiv(N, 256)
    c256 = float(_cdiv(_cdiv(M, 256) * tn, G))
    c224 = 0.90 * _cdiv(_cdiv(M, 224) * tn, G)
    c192 = 0.78 * _cdiv(_cdiv(M, 192) * tn, G)
    if c192 < 0.9 * c256 and c192 <= c224:
        return "big", 192
    if c224 < 0.95 * c256:
        return "big", 224
    return "big", 256
