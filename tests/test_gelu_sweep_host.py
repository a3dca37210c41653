"""tests/_gelu_sweep.py is exact, covers what it promises, and its bar comes from the arithmetic it restates (CPU only).

The planted operands give the planted pre-activation image under a float64 matmul; the three arrangements hold the patterns
their names promise; the float64 reference agrees with torch's own float64 GELU and its autograd derivative; the NumPy float32
restatement of common.h gelu_both_scaled meets the bar with c_ref (printed, asserted below C_REF_MAX), which is where the GPU
tests' c = 4 c_ref comes from; and the checkers fail, with the pattern in the message, on a table entry taken from a neighbouring
mantissa -- which the suite's whole-matrix bar accepts (asserted)."""
import math
import re

import pytest
import torch

import _gelu_sweep as S

SHAPES = [(2048, 2048), (64, 2048), (64, 2052)]        # the GPU file's ping-pong and two non-ping-pong launches


def test_pattern_sets():
    """2^-14 <= |u| < 16 is 18 binades x 128 mantissas x 2 signs; FINITE is everything but 2 x 128 inf / nan patterns and -0"""
    assert len(S.FINITE) == 65536 - 256 - 1 and 0x8000 not in S.FINITE.tolist()
    assert len(S.TABLE) == 18 * 128 * 2 == 4608 and len(S.OUTSIDE) == len(S.FINITE) - 4608
    v = S.VALUES[S.TABLE.long()].abs()
    assert float(v.min()) == 2.0 ** -14 and float(v.max()) == 16.0 - 2.0 ** -4
    out = S.VALUES[S.OUTSIDE.long()].abs()
    assert bool(((out < 2.0 ** -14) | (out >= 16.0)).all()) and bool(torch.isfinite(S.VALUES[S.FINITE.long()]).all())
    assert not bool(S.IN_TABLE[S.EDGES.long()].any()) and bool(torch.isin(S.EDGES, S.OUTSIDE).all())
    # the edges sit next to the range: one mantissa step inwards is a table entry
    assert bool(S.IN_TABLE[(S.E_LO << 7)]) and bool(S.IN_TABLE[(S.E_HI << 7) - 1])
    assert torch.equal(S.bits_of(S.to_bf16(S.ALL)), S.ALL)


@pytest.mark.parametrize("M,N", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", ["table", "arith", "mixed"])
def test_arrangements_are_exact_and_cover(kind, M, N):
    pats = S.arrange(kind, N * S.K_PLANT, seed=N)
    A, B, u_bits = S.plant(M, N, pats)
    assert A.shape == (M, 64) and B.shape == (N, 64) and u_bits.shape == (M, N)
    rows = min(M, 128)                                   # the image repeats every 64 rows: two periods are the whole of it
    acc = A[:rows].double() @ B.double().t()
    assert torch.equal(acc, S.VALUES[u_bits[:rows].long()]), "the float64 product is not the planted image"
    assert torch.equal(acc.to(S.BF16).double(), acc)
    assert M <= 128 or torch.equal(u_bits[128:], u_bits[128 - 64:M - 64])
    seen = torch.zeros(65536, dtype=torch.bool)
    seen[u_bits[:64].reshape(-1).long()] = True
    inside = S.IN_TABLE[u_bits.long()]
    if kind == "table":
        assert bool(seen[S.TABLE.long()].all()) and int(seen.sum()) == len(S.TABLE) and bool(inside.all())
    elif kind == "arith":
        assert bool(seen[S.FINITE.long()].all()) and int(seen.sum()) == len(S.FINITE)
        assert 0.92 < 1.0 - float(inside.double().mean()) < 0.94
    else:
        assert bool(inside.any()) and not bool(inside.all())
        assert bool(seen[S.EDGES.long()].all()), "an edge of the range test is missing from `mixed`"
        outsiders = u_bits[:64][~inside[:64]]
        assert outsiders.numel() == torch.unique(outsiders).numel(), "an outsider repeats: the sample is without repeats"
        assert 0.7 * S.DENSITY < float((~inside).double().mean()) < 1.3 * S.DENSITY
    if N % S.GROUP == 0:
        fast, groups = S.groups_in_range(u_bits)
        print(f"{kind} {M}x{N}: {fast} of {groups} groups of 16 x 16 are inside the table's range, {groups - fast} hold an outsider")
        if kind == "table":
            assert fast == groups
        elif kind == "arith":
            assert fast == 0
        else:
            assert 0.25 < fast / groups < 0.5, (fast, groups)         # (1 - 1/256)^256 = 0.367


def test_arrangement_along_columns():
    """the fp8 launch plants through the bias: one slot per column, N = 65536"""
    for kind in ("table", "arith", "mixed"):
        pats = S.arrange(kind, 65536, seed=3)
        assert bool(torch.isin(pats, S.FINITE).all())
        if kind == "arith":
            assert bool(torch.isin(S.FINITE, pats).all())
        if kind == "mixed":
            inside = S.IN_TABLE[pats.long()]
            assert bool(torch.isin(S.EDGES, pats).all()) and 128 < int((~inside).sum()) < 384
            fast = int(inside.view(-1, S.GROUP).all(1).sum())
            assert 0.9 < fast / (65536 // S.GROUP) < 0.97            # 16 columns per group here: (1 - 1/256)^16 = 0.94


def test_reference_agrees_with_torch_float64():
    u = S.VALUES[S.FINITE.long()].clone().requires_grad_(True)
    y = torch.nn.functional.gelu(u)
    y.sum().backward()
    g, d = S.reference()
    scale = u.detach().abs().clamp(min=1.0)
    eg = ((g[S.FINITE.long()] - y.detach()).abs() / scale).max()
    ed = ((d[S.FINITE.long()] - u.grad).abs() / scale).max()
    print(f"float64 reference against torch: gelu {float(eg):.3e}, gelu' {float(ed):.3e} (in units of max(|u|, 1))")
    assert float(eg) <= 1e-12 and float(ed) <= 1e-12
    # what 1 + erf loses and erfc keeps: the negative tail is not zero in the reference
    assert float(g[S.bits_of(torch.tensor([-8.0], dtype=S.BF16))[0]]) < -4e-15


def _restated_bf16(s=1.0):
    y, dy = S.gelu_both_scaled_f32(S.VALUES[S.FINITE.long()].float().numpy(), s)
    return torch.from_numpy(y), torch.from_numpy(dy)


def test_c_ref():
    y, dy = _restated_bf16()
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dy).all()), "the float32 restatement is not finite on FINITE"
    g, d = (r[S.FINITE.long()] for r in S.reference())
    u = S.VALUES[S.FINITE.long()]
    c_g = S.needed_c(y.to(S.BF16).double(), g, u, 1.0)
    c_d = S.needed_c(dy.to(S.BF16).double(), d, u, 1.0)
    c_ref = S.c_ref()
    print(f"c_ref = {c_ref:.4e} (gelu {c_g:.4e}, gelu' {c_d:.4e}); the GPU bar uses c = {S.C_GPU_FACTOR * c_ref:.4e}")
    assert c_ref == max(c_g, c_d)
    assert 0.0 < c_ref < S.C_REF_MAX
    S.check_bar(y.to(S.BF16).double(), g, S.FINITE, 1.0, c_ref, "restatement, gelu")
    S.check_bar(dy.to(S.BF16).double(), d, S.FINITE, 1.0, c_ref, "restatement, gelu'")
    with pytest.raises(AssertionError, match="miss the bar"):
        S.check_bar(y.to(S.BF16).double(), g, S.FINITE, 1.0, 0.0, "restatement, gelu, c = 0")


def test_doubling_is_exact_in_the_restatement():
    """s = 2 (p = 0.5) doubles both results bit for bit wherever nothing overflows or is subnormal: item 4 of the GPU file"""
    y1, d1 = _restated_bf16(1.0)
    y2, d2 = _restated_bf16(2.0)
    u = S.VALUES[S.FINITE.long()].abs()
    ok = u < 2.0 ** 126
    for a, b in ((y1, y2), (d1, d2)):
        normal = ok & (a.abs() >= 2.0 ** -126)
        assert torch.equal((2.0 * a)[normal], b[normal])


def test_checkers_catch_a_neighbouring_entry():
    """the table filled from the pattern two entries on (the next mantissa, same sign): both checkers fail and name the pattern,
    while the bar of test_gemm_nt_epilogues, 2^-7 |ref| + 2e-3 + 1.13 |u| 2^-7, accepts it almost everywhere"""
    g, d = S.reference()
    pats = S.arrange("table", 4096 * 4, seed=1).view(64, -1)
    y, dy = S.gelu_both_scaled_f32(S.VALUES.float().numpy())
    y, dy = torch.from_numpy(y).to(S.BF16), torch.from_numpy(dy).to(S.BF16)
    good_y, good_d = y[pats.long()], dy[pats.long()]
    c = S.C_GPU_FACTOR * S.c_ref()
    S.check_bar(good_y.double(), g[pats.long()], pats, 1.0, c, "good gelu")
    S.check_bar(good_d.double(), d[pats.long()], pats, 1.0, c, "good gelu'")
    shifted = torch.where(S.IN_TABLE[(pats + 1).long()], pats + 1, pats)        # the last mantissa of the top binade keeps its own
    bad_y = y[shifted.long()]
    with pytest.raises(AssertionError) as e:
        S.check_bar(bad_y.double(), g[pats.long()], pats, 1.0, c, "shifted gelu")
    assert re.search(r"pattern 0x[0-9a-f]{4} u = .* at \(row \d+, col \d+\)", str(e.value)), str(e.value)
    u = S.VALUES[pats.long()]
    loose = g[pats.long()].abs() * 2.0 ** -7 + 2e-3 + 1.13 * u.abs() * 2.0 ** -7
    missed = ((bad_y.double() - g[pats.long()]).abs() <= loose).double().mean()
    assert float(missed) > 0.9, float(missed)
    # one function of u: a launch that answers from the shifted table disagrees with one that does not
    pack = lambda a, b: (S.bits_of(b).long() << 16) | S.bits_of(a).long()
    tabs = {"good": S.per_pattern(pats, pack(good_y, good_d)), "again": S.per_pattern(pats.flip(0), pack(good_y.flip(0), good_d.flip(0)))}
    assert S.check_one_function(tabs, "two good launches") == len(S.TABLE)
    tabs["shifted"] = S.per_pattern(pats, pack(bad_y, good_d))
    with pytest.raises(AssertionError) as e:
        S.check_one_function(tabs, "with a shifted launch")
    assert re.search(r"pattern 0x[0-9a-f]{4} .*good: 0x[0-9a-f]{8}.*shifted: 0x[0-9a-f]{8}", str(e.value)), str(e.value)


def test_quantiser_saturates():
    x = torch.tensor([0.0, 447.0, 448.0, 470.0, 1e4, -1e4, math.inf, -math.inf, 2.0 ** -10, 2.0 ** -9])
    assert S.q8(x).float().tolist() == [0.0, 448.0, 448.0, 448.0, 448.0, -448.0, 448.0, -448.0, 0.0, 2.0 ** -9]
