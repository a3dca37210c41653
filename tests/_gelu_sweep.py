"""All 65536 bf16 inputs of the GELU epilogue: pattern sets, planted operands, a float64 reference and checkers (no GPU code).

EPI_GELU (csrc/nt_epilogue.h, nt_epilogue) rounds u = acc + bias to bf16 and writes out1 = s gelu(u), out0 = s gelu'(u) as bf16 (s = the
dropout scale), with fp8 operands also e4m3(s gelu(u) out_scale).  The ping-pong kernel reads the results from a table in LDS where
its comment says it does,

    2^-14 <= |u| < 16:  18 binades x 128 mantissas x 2 signs = 4608 inputs, bf16 exponent field in [127 - 14, 127 + 4),

(TABLE below is derived from that sentence, not from the kernel's constants: if the table's range changes, test_gelu_sweep_host.py
fails on purpose and the sets here are revisited) and redoes a 4-element-per-lane group of a wave arithmetically (common.h,
gelu_both_scaled) when any of its lanes is outside.  A wave's group is 16 rows x 16 columns of the output, aligned to 16.

Planting: with K = 64, A[m, k] = (k == m % 64) and B[n, k] any finite bf16 pattern, acc[m, n] = B[n, m % 64] exactly (one product
by 1.0, 63 by +0), so without a bias the pre-activation is a chosen bit pattern at every element.  Three arrangements of the
N x 64 slots of B: `table` (TABLE only: every group takes the lookup), `arith` (all of FINITE: nearly every group is redone) and
`mixed` (TABLE with outsiders at density 1 / 256: (1 - 1/256)^256 = 37 % of the groups stay on the lookup, so a wave flips between
the two forms from group to group).

Bar for a bf16 output: |got - s ref| <= 2^-8 |s ref| + c s max(|u|, 1).  2^-8 is the half-ulp of ONE round-to-nearest-even to bf16
(u is exact here, so nothing else is rounded to bf16); the absolute term is what fp32 `1 + erf` cannot resolve -- the 1.5e-7 of
the Abramowitz-Stegun polynomial, the fp32 rounding at 1.0, flushed denormals -- times |u|.  c comes from the NumPy float32
restatement of gelu_both_scaled below (c_ref = the smallest c at which the restatement passes on FINITE), the GPU gets
C_GPU_FACTOR x c_ref for its approximate v_rcp_f32 / __expf; it is never taken from a kernel's output."""
import functools
import math

import numpy as np
import torch

BF16, F32, FP8 = torch.bfloat16, torch.float32, torch.float8_e4m3fn
K_PLANT = 64
GROUP = 16                                   # a wave's 4-element group covers GROUP x GROUP outputs
E_LO, E_HI = 127 - 14, 127 + 4               # the table's exponent fields: 2^-14 <= |u| < 16
DENSITY = 1.0 / 256                          # outsiders in `mixed`
REL_BF16 = 2.0 ** -8                         # half an ulp of 8 significant bits
REL_E4M3 = 2.0 ** -4                         # half an ulp of 4 significant bits
ABS_E4M3 = 2.0 ** -10                        # half the smallest e4m3 subnormal step (2^-9)
C_REF_MAX = 2.5e-7                           # (1.5e-7 + 2 x 2^-24) / 2 = 1.35e-7 for Phi = (1 + erf) / 2, with room for the fmas
C_GPU_FACTOR = 4.0

ALL = torch.arange(65536, dtype=torch.int32)
_EXP = (ALL >> 7) & 0xFF
# -0 is left out: it cannot come out of an MFMA accumulation that starts at +0 ((+0) + (-0) = +0 in round-to-nearest), and a bias of
# -0 added to that +0 gives +0 as well.  (A flushed negative denormal may still show up as -0 in the pre-activation image; the
# reference is gathered from the image the kernel returns, so it is covered, just not planted.)
FINITE = ALL[(_EXP != 255) & (ALL != 0x8000)]
IN_TABLE = (_EXP >= E_LO) & (_EXP < E_HI)    # bool[65536], by pattern
TABLE = ALL[IN_TABLE]
OUTSIDE = FINITE[~IN_TABLE[FINITE.long()]]
# the outsiders next to every boundary of the range test, both signs; `mixed` always holds them
EDGES = torch.tensor([0x0000, 0x0001, 0x007F, 0x0080, (E_LO << 7) - 1, E_HI << 7, 0x7F7F,
                      0x8001, 0x807F, 0x8080, 0x8000 | ((E_LO << 7) - 1), 0x8000 | (E_HI << 7), 0xFF7F], dtype=torch.int32)


def to_bf16(bits):
    """int patterns 0..65535 -> the bf16 tensor with those bits"""
    b = bits.to(torch.int32)
    return (((b + 0x8000) & 0xFFFF) - 0x8000).to(torch.int16).view(BF16)


def bits_of(x):
    """bf16 tensor -> int32 patterns 0..65535 (on the CPU)"""
    assert x.dtype == BF16, x.dtype
    return x.detach().cpu().contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


VALUES = to_bf16(ALL).double()               # the value of every pattern (inf / nan where the pattern says so)


def drop_scale(p):
    """the survivor scale the kernels use: an fp32 quotient over the rate rounded to 1 / 65536 (common.h)"""
    thr = int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))
    return 1.0 if thr == 0 else float(np.float32(65536.0) / np.float32(65536 - thr))


# ------------------------------------------------------------------------------------------------- arrangements
def _fill(pool, slots, g):
    """every pattern of `pool` at least once, the rest drawn from it, randomly permuted"""
    assert slots >= len(pool), f"{slots} slots cannot hold {len(pool)} patterns once each"
    extra = pool[torch.randint(0, len(pool), (slots - len(pool),), generator=g)]
    both = torch.cat([pool, extra])
    return both[torch.randperm(slots, generator=g)]


def arrange(kind, slots, seed):
    """-> int32[slots] bf16 patterns.  table: TABLE, each at least once.  arith: FINITE, each at least once.  mixed: a TABLE
    background, each slot replaced by an outsider independently with probability 1 / 256; the outsiders are EDGES first, then a
    random sample of OUTSIDE without repeats (all 60671 of them cannot fit at that density: `arith` is where each one appears)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "table":
        return _fill(TABLE, slots, g)
    if kind == "arith":
        return _fill(FINITE, slots, g)
    assert kind == "mixed", kind
    out = _fill(TABLE, slots, g)
    where = (torch.rand(slots, generator=g) < DENSITY).nonzero().view(-1)
    assert len(EDGES) <= len(where) <= len(OUTSIDE), f"{len(where)} outsider slots of {slots}: the image is too small for the edges"
    rest = OUTSIDE[~torch.isin(OUTSIDE, EDGES)]
    pool = torch.cat([EDGES, rest[torch.randperm(len(rest), generator=g)]])[:len(where)]
    out[where] = pool[torch.randperm(len(where), generator=g)]
    return out


def plant(M, N, patterns):
    """-> bf16 A[M, 64], B[N, 64] and the int32 image u_bits[M, N] = pattern of B[n, m % 64] that A @ B^T is, exactly"""
    assert patterns.numel() == N * K_PLANT, (patterns.numel(), N)
    assert bool(((patterns >> 7) & 0xFF != 255).all()), "only finite patterns can be planted (0 x inf is nan)"
    b_bits = patterns.view(N, K_PLANT)
    rows = torch.arange(M) % K_PLANT
    A = torch.zeros(M, K_PLANT)
    A[torch.arange(M), rows] = 1.0
    return A.to(BF16), to_bf16(b_bits), b_bits.t()[rows].contiguous()


def groups_in_range(u_bits):
    """-> (groups whose 16 x 16 elements all lie in the table's range, all groups) of an image whose sides are multiples of 16"""
    M, N = u_bits.shape
    assert M % GROUP == 0 and N % GROUP == 0, (M, N)
    ok = IN_TABLE[u_bits.long()].view(M // GROUP, GROUP, N // GROUP, GROUP).permute(0, 2, 1, 3).reshape(M // GROUP, N // GROUP, -1)
    return int(ok.all(-1).sum()), (M // GROUP) * (N // GROUP)


# ------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def reference():
    """-> float64 (gelu, gelu') of every pattern, indexed by pattern.  Phi = erfc(-u / sqrt 2) / 2 keeps the negative tail that
    1 + erf cancels away."""
    u = VALUES
    cdf = 0.5 * torch.special.erfc(-u / math.sqrt(2.0))
    return u * cdf, cdf + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in fp64, the sum is rounded there and once more to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gelu_both_scaled_f32(x, s=1.0):
    """common.h gelu_both_scaled restated in NumPy float32, operation by operation (the division and the exponential are
    correctly rounded here and approximate on the GPU) -> (y, dy) as float32"""
    f = np.float32
    x = np.asarray(x, dtype=f)
    one = np.ones_like(x)
    hs, cs = f(0.5) * f(s), f(0.3989422804014327) * f(s)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):       # (invalid: only for inf / nan inputs, outside FINITE)
        ax = np.abs(x) * f(0.70710678118654752)
        t = one / _fma32(np.full_like(x, f(0.3275911)), ax, one)
        poly = _fma32(np.full_like(x, f(1.061405429)), t, np.full_like(x, f(-1.453152027)))
        for coef in (1.421413741, -0.284496736, 0.254829592):
            poly = _fma32(poly, t, np.full_like(x, f(coef)))
        poly = poly * t
        e = np.exp((-ax * ax).astype(np.float64)).astype(f)
        erfv = np.copysign(_fma32(-poly, e, one), x)
        cdf = _fma32(np.full_like(x, hs), erfv, np.full_like(x, hs))
        y = x * cdf
        dy = _fma32(x * cs, e, cdf)
    return y, dy


def q8(x32):
    """the suite's e4m3 quantiser (tests/test_gpu_fp8.py, test_quantize_fp8_bit_exact): saturate at +-448, then torch's conversion"""
    return x32.clamp(-448.0, 448.0).to(FP8)


# ------------------------------------------------------------------------------------------------- the bar and its checker
def needed_c(got, want, u, s, rel=REL_BF16, extra=0.0, mask=None):
    """the smallest c at which |got - want| <= rel |want| + extra + c s max(|u|, 1) holds for every (masked-in) element; `want`
    already carries s.  inf where an element is not finite."""
    over = (got - want).abs() - rel * want.abs() - extra
    over = torch.where(torch.isfinite(over), over, torch.full_like(over, math.inf))
    c = over.clamp(min=0.0) / (s * u.abs().clamp(min=1.0))
    if mask is not None:
        c = c[mask]
    return float(c.max()) if c.numel() else 0.0


@functools.lru_cache(maxsize=None)
def c_ref():
    """the smallest c at which the float32 restatement, rounded to bf16, meets the bar for both outputs on all of FINITE (s = 1)"""
    idx = FINITE.long()
    y, dy = gelu_both_scaled_f32(VALUES[idx].float().numpy())
    g, d = reference()
    return max(needed_c(torch.from_numpy(y).to(BF16).double(), g[idx], VALUES[idx], 1.0),
               needed_c(torch.from_numpy(dy).to(BF16).double(), d[idx], VALUES[idx], 1.0))


def check_bar(got, want, u_bits, s, c, what, rel=REL_BF16, extra=0.0, mask=None, cap=6):
    """Every (masked-in) element of the float64 image `got` is within rel |want| + extra + c s max(|u|, 1) of `want` (= s ref,
    float64), u the value of the int32 pattern image `u_bits`.  No sampling, no allowed share of misses; a non-finite `got` is a
    miss.  The AssertionError names the count, the distinct patterns that miss, and pattern, u, got, want, (row, col) of the
    worst offenders."""
    assert got.shape == want.shape == u_bits.shape, (what, got.shape, want.shape, u_bits.shape)
    u = VALUES[u_bits.long()]
    err = (got - want).abs()
    lim = rel * want.abs() + extra + c * s * u.abs().clamp(min=1.0)
    bad = ~(err <= lim)
    if mask is not None:
        bad &= mask
    if not bool(bad.any()):
        return
    if got.dim() == 1:
        got, want, u_bits, u, err, lim, bad = (t.unsqueeze(0) for t in (got, want, u_bits, u, err, lim, bad))
    idx = bad.nonzero()
    excess = torch.nan_to_num(err / lim, nan=math.inf)[bad]
    order, shown = [], set()
    for j in excess.argsort(descending=True)[:65536].tolist():           # the worst offender of each of the first `cap` patterns
        pat = int(u_bits[idx[j, 0], idx[j, 1]])
        if pat not in shown:
            shown.add(pat)
            order.append(j)
            if len(order) == cap:
                break
    lines = []
    for r, col in idx[order].tolist():
        lines.append(f"pattern 0x{int(u_bits[r, col]):04x} u = {float(u[r, col]):.9g}: got {float(got[r, col]):.9g}, want {float(want[r, col]):.9g} "
                     f"(error {float(err[r, col]):.3e}, bar {float(lim[r, col]):.3e}) at (row {r}, col {col})")
    pats = torch.unique(u_bits[bad])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements ({len(pats)} distinct patterns, first 0x{int(pats[0]):04x}) "
                         f"miss the bar with c = {c:.3e}; worst: " + "; ".join(lines))


# ------------------------------------------------------------------------------------------------- one function of u
EMPTY_LO, EMPTY_HI = 1 << 40, -1


def per_pattern(u_bits, out_bits):
    """-> (lo, hi) int64[65536]: the smallest and largest value of `out_bits` (any non-negative integer image: here
    (out0 bits << 16) | out1 bits) over the occurrences of every pattern of `u_bits`; (EMPTY_LO, EMPTY_HI) where a pattern is absent"""
    idx, val = u_bits.reshape(-1).long(), out_bits.reshape(-1).long()
    lo = torch.full((65536,), EMPTY_LO, dtype=torch.int64).scatter_reduce_(0, idx, val, "amin")
    hi = torch.full((65536,), EMPTY_HI, dtype=torch.int64).scatter_reduce_(0, idx, val, "amax")
    return lo, hi


def check_one_function(tables, what, cap=6, fmt=lambda v: f"0x{v:08x}"):
    """`tables`: {launch name: per_pattern(...)}.  Every pattern has ONE output value over all its occurrences in all launches.  On a
    disagreement the AssertionError lists the first patterns and, for each, the values by the launch that produced them."""
    names = list(tables)
    lo = torch.stack([tables[k][0] for k in names]).min(0).values
    hi = torch.stack([tables[k][1] for k in names]).max(0).values
    present = hi >= 0
    bad = (present & (lo != hi)).nonzero().view(-1)
    if bad.numel() == 0:
        return int(present.sum())
    lines = []
    for pat in bad[:cap].tolist():
        seen = []
        for k in names:
            a, b = int(tables[k][0][pat]), int(tables[k][1][pat])
            if b >= 0:
                seen.append(f"{k}: {fmt(a)}" + ("" if a == b else f" and {fmt(b)}"))
        lines.append(f"pattern 0x{pat:04x} (u = {float(VALUES[pat]):.9g}) -> " + ", ".join(seen))
    raise AssertionError(f"{what}: {bad.numel()} of {int(present.sum())} patterns have more than one result; " + "; ".join(lines))
