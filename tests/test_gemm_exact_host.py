"""The bit-for-bit checker of tests/_gemm_exact.py is sharp (CPU only).

An fp32 emulation of the product passes it in every summation order a kernel may use (plain, K-chunks in reverse, split-K into a
zeroed output, a TN product cut into slabs over M), and ONE localised fault -- what a dropped product, K-tile, row, bias, slab or
a double rounding does in a kernel -- fails it with the right (row, col), block and tile in the message.  A row lost
from a column sum and a double rounding both stay inside the bars of the tolerance tests (asserted below): that is why this file
exists."""
import re

import pytest
import torch

import _gemm_exact as X
from _util import rel_l2

M, N, K = 300, 520, 512          # 2 x 3 tiles of 256 x 256, ragged in both directions; 8 K-chunks of 64


@pytest.fixture(scope="module")
def case():
    A, B, bias = X.operands(M, N, K, seed=1, colsum=True)
    acc = X.ref_nt(A, B)
    return A, B, bias, X.to_f32_exact(acc + bias.double())


def _chunks(A, B, order):
    out = torch.zeros(A.shape[0], B.shape[0])
    for c in order:
        out += A[:, 64 * c:64 * c + 64].float() @ B[:, 64 * c:64 * c + 64].float().t()
    return out


def _fails(got, want, what="mutant"):
    with pytest.raises(AssertionError) as e:
        X.check_exact(got, want, what)
    return str(e.value)


def test_fp32_and_fp64_references_agree_bit_for_bit(case):
    A, B, bias, want = case
    assert torch.equal(X.ref_nt(A, B, fp32=True), X.ref_nt(A, B))
    assert torch.equal(X.ref_nt(A, B), (A.long() @ B.long().t()).double())          # and both are the integer product
    At, Bt, _ = X.operands_tn(1000, 264, 8, seed=2)
    assert torch.equal(X.ref_tn(At, Bt, fp32=True), X.ref_tn(At, Bt))
    assert not bool((A == 0).any()) and not bool((B == 0).any())                    # no zeros: every product matters


def test_every_summation_order_passes(case):
    A, B, bias, want = case
    X.check_exact(A.float() @ B.float().t() + bias, want, "plain")
    X.check_exact(_chunks(A, B, reversed(range(K // 64))) + bias, want, "chunks of 64 in reverse order")
    out = torch.zeros(M, N)                                                         # split-K: slices added into a zeroed output,
    for s, ks in enumerate(((5, 6, 7), (0, 1), (2, 3, 4))):                         # slice 0 adds the bias
        out += _chunks(A, B, ks) + (bias if s == 0 else 0)
    X.check_exact(out, want, "split-K")
    X.check_exact((A.float() @ B.float().t() + bias).to(X.BF16), X.bf16_rne(want.double()), "one bf16 rounding")
    At, Bt, C0 = X.operands_tn(1000, 264, 8, seed=2)
    slabs = [At[r0:r1].float().t() @ Bt[r0:r1].float() for r0, r1 in ((0, 320), (320, 704), (704, 1000))]
    X.check_exact(C0 + (slabs[2] + slabs[0] + slabs[1]), X.to_f32_exact(C0.double() + X.ref_tn(At, Bt)), "TN in 3 slabs")
    zero = torch.zeros(4, 4)
    X.check_exact(-zero, zero, "+0 and -0 are equal")
    X.check_exact((-zero).to(X.BF16), zero.to(X.BF16), "+0 and -0 are equal (bf16)")


def test_one_dropped_product_changes_one_row(case):
    A, B, bias, want = case
    A2 = A.clone()
    A2[277, 130] = 0
    got = A2.float() @ B.float().t() + bias
    msg = _fails(got, want)
    assert f"{N} of {M * N} elements differ" in msg and "first at (row 277, col 0)" in msg
    assert "in 3 256x256 tile(s) (tile row, tile col): (1, 0), (1, 1), (1, 2)" in msg


def test_one_k_chunk_dropped_for_one_block(case):
    A, B, bias, want = case
    got = want.clone()
    got[272:288, 496:512] -= A[272:288, 192:256].float() @ B[496:512, 192:256].float().t()
    msg = _fails(got, want)
    assert "1 bad 16x16 block(s) (block row, block col): (17, 31)" in msg and "tile col): (1, 1)" in msg
    assert "a K-tile or an address?" in msg


def test_row_written_one_lower(case):
    *_, want = case
    got = want.clone()
    got[256] = want[255]
    got[255] = 7.0                                        # the sentinel the row leaves behind
    msg = _fails(got, want)
    assert "first at (row 255, col 0)" in msg and "tile col): (0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)" in msg


def test_column_shifted_by_four(case):
    *_, want = case
    got = want.clone()
    got[:, 260] = want[:, 256]
    msg = _fails(got, want)
    assert re.search(r"first at \(row \d+, col 260\)", msg) and "tile col): (0, 1), (1, 1)" in msg


def test_bias_left_off_one_tile(case):
    A, B, bias, want = case
    got = want.clone()
    got[256:, 512:] -= bias[512:]
    msg = _fails(got, want)
    assert "tile col): (1, 2)" in msg and "in 1 256x256 tile(s)" in msg
    nz = int((bias[512:] != 0).sum()) * (M - 256)
    assert f"{nz} of {M * N} elements differ" in msg
    got = want.clone()
    got[256:, 512:] -= 3.0                                # a constant offset over the tile is reported as constant
    assert "constant difference -3 over the bad region" in _fails(got, want)


def test_one_slab_added_twice():
    At, Bt, C0 = X.operands_tn(1000, 264, 8, seed=2)
    want = X.to_f32_exact(C0.double() + X.ref_tn(At, Bt))
    got = want + At[320:704].float().t() @ Bt[320:704].float()
    msg = _fails(got, want)
    assert "elements differ" in msg and "tile col): (0, 0), (1, 0)" in msg


def test_one_row_missing_from_a_column_sum():
    Mc = 50000
    A, B, bias = X.operands(Mc, 8, 64, seed=3, hi=1, colsum=True)
    out = X.to_f32_exact(X.ref_nt(A, B) + bias.double())
    want = X.to_f32_exact(out.double().sum(0))
    X.check_exact(out.sum(0), want, "column sums")
    X.check_exact(out.flip(0).view(50, 1000, 8).sum(1).sum(0), want, "column sums in partials")
    got = (out.double().sum(0) - out[49999].double()).float()
    msg = _fails(got, want, "column sums")
    assert "first at (row 0, col" in msg
    assert rel_l2(got, want) < 1e-3                       # the bar that judged the column sums so far passes this


def test_double_rounding_is_caught_in_the_round_regime():
    A, B, bias = X.operands(64, 512, 512, seed=4)         # hi = 3: |acc| passes 256
    A[:32], B[:256] = A[:32].abs(), B[:256].abs()         # one corner without cancellation: |acc| ~ 2048, 12 significant bits, where
    exact = X.ref_nt(A, B) + bias.double()                # an 11-bit intermediate rounds a value to a bf16 tie that RNE then resolves the other way
    assert float(exact.abs().max()) > 2048
    want = X.bf16_rne(exact)
    X.check_exact(X.to_f32_exact(exact).to(X.BF16), want, "one rounding")
    x = X.to_f32_exact(exact)
    bits = x.view(torch.int32)
    low = 1 << 13                                         # fp32 -> 11 significand bits (RNE) -> bf16
    mid = ((bits + (low >> 1) - 1 + ((bits >> 13) & 1)) & ~(low - 1)).view(torch.float32)
    twice = mid.to(X.BF16)
    assert not torch.equal(twice.view(torch.int16), want.view(torch.int16)), "the case has no value that rounds differently twice"
    msg = _fails(twice, want)
    assert "elements differ" in msg
    d = (twice.float() - want.float()).abs()
    assert bool((d <= want.float().abs() * 2.0 ** -7).all())           # inside the bf16 bar of the tolerance tests by construction


def test_stale_sentinel_element(case):
    *_, want = case
    got = want.clone()
    got[299, 519] = 7.0
    msg = _fails(got, want)
    assert "1 of" in msg and "first at (row 299, col 519): got 7" in msg and "(block row, block col): (18, 32)" in msg


def test_block_listing_is_capped(case):
    *_, want = case
    msg = _fails(want + 1, want)
    assert f"{M * N} of {M * N}" in msg and "more" in msg and "constant difference 1" in msg


def test_generators_assert_the_exactness_bound():
    with pytest.raises(AssertionError, match="2\\^24"):
        X.operands(8, 8, (1 << 24) // 9 + 64, seed=0, hi=3)
    with pytest.raises(AssertionError, match="column sums"):
        X.operands(50000, 8, 512, seed=0, hi=3, colsum=True)
    with pytest.raises(AssertionError, match="2\\^24"):
        X.operands_tn((1 << 24) // 9, 8, 8, seed=0, hi=3)
    with pytest.raises(AssertionError, match="K <= 128"):
        X.regime_hi("small", 192)
    with pytest.raises(AssertionError, match="not representable"):
        X.to_f32_exact(torch.tensor([float((1 << 24) + 1)], dtype=torch.float64))
    A, B, bias = X.operands(16, 16, 64, seed=0)
    assert X.to_fp8(A).dtype == X.FP8 and bool((bias.abs() <= 8).all()) and torch.equal(bias, bias.round())


def test_restated_plans_reach_the_paths_the_gpu_cases_name():
    # the helper-workgroup plans of tests/test_gpu_gemm_exact.py (one split + helpers, two splits + helpers) and a single-owner plan
    assert X.tn_batch_plan(1700, 13, 24) == (1, 22, 5)
    assert X.tn_batch_plan(3100, 11, 32) == (2, 22, 5)
    assert X.tn_batch_plan(1700, 13, 8) == (1, 27, 0) and X.tn_batch_workspace(1700, 13, 8) == 0
    assert X.tn_batch_plan(50176, 108, 256) == (2, 355, 74)            # the full-size ViT-B list (tests/test_gpu_round3.py)
    assert X.tn_plan(64, 264, 8, 256)[1] == 1 and X.tn_plan(65, 264, 8, 256)[1] == 2
    assert X.tn_plan(300, 520, 776, 8)[1] == 1                          # more tiles than CUs: direct
    assert X.nt_tile_rows(3330, 1160, 256) == ("big", 192) and X.nt_tile_rows(3330, 1160, 75) == ("big", 224)
    assert X.nt_tile_rows(3330, 1160, 8) == ("big", 256) and X.nt_tile_rows(1100, 772, 8) == ("small", 256)
