"""The binary cross-entropy kernel (include/vitssl_bce.h, vitssl_classify_bce) against its fp64 restatement (tests/_bce_ref.py),
with the bars of tests/test_gpu_classify.py: the loss within max(4 x the distance of torch's fp32 CPU
binary_cross_entropy_with_logits from the fp64 value, 1e-6) relative (both distances are printed; torch's is 7e-9 to 1.6e-7
at these shapes, so the floor decides); every gradient element within max(2^-8 |ref|, 2^-126) of the bf16-rounded fp64 value;
padding columns and ignored rows exactly zero; dbias within 1e-5 relative L2, accumulated onto a non-zero start
(tests/_bce_ref.py::dbias0); pred, counters and bad_labels exact.
Measured on MI355X over the 195 loss comparisons of this file: torch's fp32 CPU distance from the fp64 value is at most 1.5e-7, the
kernel's at most 5.1e-8 (the one rounding of its fp64 sum to the fp32 it returns, and the fp32 quotient)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bce_ref as Bc

DEV = torch.device("cuda:0")
BF16, F32, I64, I32 = torch.bfloat16, torch.float32, torch.int64, torch.int32
gpu = pytest.mark.gpu


def run_bce(z, y, C, eps, partner=None, lam=None, threshold=None, sum_classes=False, grad=True, ld_out=None, upstream=1.0):
    from vitssl_hip import ops
    B = z.shape[0]
    ld_out = ld_out or (C + 63) // 64 * 64
    out = dict(loss=torch.full((2,), 7.0, device=DEV), pred=torch.full((B,), -1, dtype=I64, device=DEV),
               counters=torch.tensor(Bc.COUNTERS0, dtype=I64, device=DEV), bad=torch.tensor([Bc.BAD0], dtype=I32, device=DEV))
    if grad:
        out["dlogits"] = torch.full((B, ld_out), float("nan"), dtype=BF16, device=DEV)
        out["dbias"] = torch.full((C,), Bc.dbias0(C, sum_classes), dtype=F32, device=DEV)
    tables = {} if partner is None else dict(partner=torch.from_numpy(np.asarray(partner, np.int32)).to(DEV),
                                             lam=torch.from_numpy(np.asarray(lam, np.float32)).to(DEV))
    ops.classify_bce(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), C, out["loss"], out["pred"], out["counters"], out["bad"],
                     dlogits=out.get("dlogits"), dbias=out.get("dbias"), smoothing=eps, target_threshold=threshold, sum_classes=sum_classes,
                     ignore_index=Bc.IGNORE, upstream=upstream, **tables)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def torch_fp32(z, ref, C, sum_classes):
    """torch's own fp32 CPU result on the valid rows, against the restatement's dense targets"""
    valid = ref["valid"]
    zt, t = torch.from_numpy(z[:, :C][valid].copy()), torch.from_numpy(ref["t"][valid].astype(np.float32))
    if sum_classes:
        return float(F.binary_cross_entropy_with_logits(zt, t, reduction="none").sum(-1).mean())
    return float(F.binary_cross_entropy_with_logits(zt, t))


def check(ref, got, z, C, sum_classes=False, grad=True, what=""):
    assert got["bad"].tolist() == [Bc.BAD0 + ref["n_bad"]]
    t32 = torch_fp32(z, ref, C, sum_classes) if ref["n_valid"] else float("nan")
    Bc.check_loss(ref, got["loss"].tolist(), t32, what)
    if ref["n_valid"] == 0:
        assert np.isnan(float(got["loss"][0] / got["loss"][1]))              # 0 / 0, formed as the models form it
    assert np.array_equal(got["pred"].numpy(), ref["pred"])                  # numpy.argmax: the first occurrence
    assert got["counters"].tolist() == [Bc.COUNTERS0[0] + ref["correct"], Bc.COUNTERS0[1] + ref["n_valid"]]
    if grad:
        Bc.check_grad(ref, got["dlogits"].double().numpy(), C)
        Bc.check_dbias(ref, got["dbias"].double().numpy(), Bc.dbias0(C, sum_classes))


def same_bits(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), f"{k}: bits differ"


@gpu
@pytest.mark.parametrize("two", [False, True], ids=["one-label", "two-label"])
@pytest.mark.parametrize("sum_classes", [False, True], ids=["mean", "sum"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C,ld", Bc.SHAPES, ids=str)
def test_kernel_against_fp64(B, C, ld, eps, sum_classes, two):
    for rot in range(6 if two and C < 65536 else 1):                         # two-label: every row meets each of the six lam values
        z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld, rot=rot)
        if not two:
            partner = lam = None
        ref = Bc.reference(z, y, C, eps, partner, lam, None, sum_classes)
        got = run_bce(z, y, C, eps, partner, lam, None, sum_classes)
        check(ref, got, z, C, sum_classes, what=f"(B,C)=({B},{C}) eps={eps} sum={sum_classes} two={two} rot={rot}")
        if rot == 0:
            same_bits(got, run_bce(z, y, C, eps, partner, lam, None, sum_classes))                       # two runs: the same bits
            ev = run_bce(z, y, C, eps, partner, lam, None, sum_classes, grad=False)                      # NULL dlogits: the evaluation case
            same_bits(got, ev, ("loss", "pred", "counters", "bad"))


@gpu
@pytest.mark.parametrize("threshold,shape", [(0.0, Bc.SHAPES[1]), (0.2, Bc.SHAPES[1]), (0.2, Bc.SHAPES[3])], ids=str)
def test_target_threshold_on_mixed_rows(threshold, shape):
    """eps = 0.1: the soft targets lie at eps / C, near lam and 1 - lam and at 1 - eps + eps / C, none within 1e-3 of the threshold;
    0.0 sets every target to 1 (sigmoid(z) - 1 as -sigmoid(-z) everywhere), 0.2 keeps the larger shares of a mixed row."""
    B, C, ld = shape
    for rot in range(6):
        z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld, rot=rot)
        for sum_classes in (False, True):
            ref = Bc.reference(z, y, C, 0.1, partner, lam, threshold, sum_classes)
            assert np.abs(ref["soft"][ref["valid"]] - threshold).min() >= 1e-3
            assert set(np.unique(ref["t"])) <= {0.0, 1.0} and (threshold > 0.0 or ref["t"][ref["valid"]].all())
            check(ref, run_bce(z, y, C, 0.1, partner, lam, threshold, sum_classes), z, C, sum_classes, what=f"threshold {threshold} (B,C)=({B},{C}) rot={rot}")
    ref = Bc.reference(z, y, C, 0.1, None, None, threshold)                  # and without tables
    check(ref, run_bce(z, y, C, 0.1, None, None, threshold), z, C, what=f"threshold {threshold} one-label")


@gpu
@pytest.mark.parametrize("two", [False, True], ids=["one-label", "two-label"])
@pytest.mark.parametrize("B,C,ld", Bc.SHAPES[:4], ids=str)
def test_all_rows_ignored(B, C, ld, two):
    z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld, all_ignored=True)
    if not two:
        partner = lam = None
    ref = Bc.reference(z, y, C, 0.1, partner, lam)
    assert ref["n_valid"] == 0 and ref["n_bad"] == 0
    check(ref, run_bce(z, y, C, 0.1, partner, lam), z, C)                    # 0 / 0 = nan


@gpu
@pytest.mark.parametrize("B,C,ld", [Bc.SHAPES[1], Bc.SHAPES[3]], ids=str)
def test_bad_rows_are_flagged_and_ignored(B, C, ld):
    """An out-of-range label (own or the partner's), an out-of-range partner, lam NaN or outside [0, 1]: the row is ignored,
    bad_labels advances by exactly that many, nothing is read through the bad index and nothing else is disturbed."""
    z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld)
    base = Bc.reference(z, y, C, 0.1, partner, lam)
    rows = np.flatnonzero(base["valid"])
    cases = [("label", lambda y, p, l, i: y.__setitem__(i, C)), ("label<0", lambda y, p, l, i: y.__setitem__(i, -5)),
             ("label=2^40", lambda y, p, l, i: y.__setitem__(i, 2 ** 40)),
             ("partner=-1", lambda y, p, l, i: p.__setitem__(i, -1)), ("partner=B", lambda y, p, l, i: p.__setitem__(i, B)),
             ("partner=2^31-1", lambda y, p, l, i: p.__setitem__(i, 2 ** 31 - 1)), ("lam=nan", lambda y, p, l, i: l.__setitem__(i, np.nan)),
             ("lam=1.5", lambda y, p, l, i: l.__setitem__(i, 1.5)), ("lam<0", lambda y, p, l, i: l.__setitem__(i, -2.0 ** -30))]
    everything = (y.copy(), partner.copy(), lam.copy())
    for n, (name, poke) in enumerate(cases):
        y2, p2, l2 = y.copy(), partner.copy(), lam.copy()
        poke(y2, p2, l2, rows[n % len(rows)])
        poke(*everything, rows[n % len(rows)])
        ref = Bc.reference(z, y2, C, 0.1, p2, l2)
        assert ref["n_bad"] >= 1 and ref["n_valid"] < base["n_valid"], name
        check(ref, run_bce(z, y2, C, 0.1, p2, l2), z, C, what=name)
    y3, p3, l3 = everything
    ref = Bc.reference(z, y3, C, 0.1, p3, l3)
    assert ref["n_bad"] >= 3
    check(ref, run_bce(z, y3, C, 0.1, p3, l3), z, C, what="all of them")
    bad = y.copy()                                                           # without tables: the labels alone
    bad[0], bad[2] = C, -5
    ref = Bc.reference(z, bad, C, 0.1)
    assert ref["n_bad"] == 2
    check(ref, run_bce(z, bad, C, 0.1), z, C, what="one-label bad labels")


@gpu
def test_nan_row_has_a_defined_prediction():
    z, y, _ = Bc.make_case(7, 1000, 1024)
    z[3, 700] = z[3, 12] = np.nan
    for tables in ((None, None), (np.arange(7, dtype=np.int32), np.ones(7, np.float32))):
        got = run_bce(z, y, 1000, 0.0, *tables)
        assert got["pred"][3] == 12 == int(np.argmax(z[3, :1000]))          # the first NaN, as numpy and torch answer
        ok = Bc.reference(z, y, 1000, 0.0)
        rest = np.arange(7) != 3
        assert np.array_equal(got["pred"].numpy()[rest], ok["pred"][rest])


@gpu
def test_wide_gradient_rows_and_upstream():
    """ld_out beyond the chunks that hold a class (the zero-fill loop) and an upstream gradient that is not 1"""
    for (B, C, ld), ld_out in ((Bc.SHAPES[1], 576), (Bc.SHAPES[3], 1344)):
        z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld, rot=2)
        for tables in ((None, None), (partner, lam)):
            got = run_bce(z, y, C, 0.1, *tables, ld_out=ld_out, upstream=0.5)
            assert got["dlogits"].shape == (B, ld_out)
            check(Bc.reference(z, y, C, 0.1, *tables, upstream=0.5), got, z, C, what=f"ld_out={ld_out} upstream=0.5")


@gpu
@pytest.mark.parametrize("case", [dict(eps=0.0), dict(eps=0.1, sum_classes=True), dict(eps=0.1, threshold=0.2)], ids=str)
@pytest.mark.parametrize("B,C,ld", Bc.SHAPES[:4], ids=str)
def test_degenerate_two_label_rows_give_the_bits_of_the_one_label_call(B, C, ld, case):
    """lam == 1, a == b and lam == 0: loss_out, dlogits, dbias, pred, counters and bad_labels of the call with tables equal
    those of the call with NULL tables bit for bit."""
    eps, thr, sc = case["eps"], case.get("threshold"), case.get("sum_classes", False)
    z, y, _ = Bc.make_case(B, C, ld)
    want = run_bce(z, y, C, eps, None, None, thr, sc)
    me = np.arange(B, dtype=np.int32)
    same_bits(want, run_bce(z, y, C, eps, me, np.ones(B, np.float32), thr, sc))
    same_bits(want, run_bce(z, y, C, eps, me, Bc.M.LAMS[np.arange(B) % 6], thr, sc))                     # a == b: lam does not matter
    ok = (B - 1) // 3 * 3                                                    # a row whose label is valid
    same_bits(want, run_bce(z, y, C, eps, np.full(B, ok, np.int32), np.ones(B, np.float32), thr, sc))   # lam == 1: the partner does not matter
    y0 = np.where(y == Bc.IGNORE, Bc.IGNORE, y[ok])                          # lam == 0: the partner's label alone
    swapped = run_bce(z, y, C, eps, np.full(B, ok, np.int32), np.zeros(B, np.float32), thr, sc)
    want0 = run_bce(z, y0, C, eps, None, None, thr, sc)
    same_bits(want0, swapped, ("loss", "dlogits", "dbias", "pred", "bad"))
    assert swapped["counters"][1] == want0["counters"][1]                    # (counters[0] compares with the row's own label)
    same_bits(run_bce(z, y, C, eps, None, None, thr, sc, grad=False), run_bce(z, y, C, eps, me, np.ones(B, np.float32), thr, sc, grad=False))
