"""The loss against two-label targets (include/vitssl_mixup.h, vitssl_classify_loss_mix) against its fp64 restatement
(tests/_mixup_ref.py), with the bars of tests/test_gpu_classify.py::check_against, which are the project's own: the loss within
max(4 x the distance of torch's fp32 CPU F.cross_entropy from the fp64 value, 1e-6) relative; every gradient element within
2^-8 |ref| of the bf16-rounded fp64 value; padding columns and ignored rows exactly zero; dbias within 1e-5 relative L2 and
counters exact, both accumulated onto a non-zero start."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _classify_ref as R
import _mixup_ref as M

DEV = torch.device("cuda:0")
BF16, F32, I64, I32 = torch.bfloat16, torch.float32, torch.int64, torch.int32
gpu = pytest.mark.gpu
DBIAS0 = 2.0 ** -6


def _outputs(B, C, grad, ld_out, dbias0):
    ld_out = ld_out or (C + 63) // 64 * 64
    out = dict(loss=torch.full((2,), 7.0, device=DEV), pred=torch.full((B,), -1, dtype=I64, device=DEV),
               counters=torch.tensor([5, 9], dtype=I64, device=DEV), bad=torch.tensor([3], dtype=I32, device=DEV))
    if grad:
        out["dlogits"] = torch.full((B, ld_out), float("nan"), dtype=BF16, device=DEV)
        out["dbias"] = torch.full((C,), dbias0, dtype=F32, device=DEV)
    return out


def run_mix(z, y, partner, lam, C, eps, grad=True, ld_out=None, upstream=1.0, dbias0=DBIAS0):
    from vitssl_hip import ops
    out = _outputs(z.shape[0], C, grad, ld_out, dbias0)
    ops.classify_loss_mix(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), torch.from_numpy(np.asarray(partner, np.int32)).to(DEV),
                          torch.from_numpy(np.asarray(lam, np.float32)).to(DEV), C, out["loss"], out["pred"], out["counters"], out["bad"],
                          dlogits=out.get("dlogits"), dbias=out.get("dbias"), label_smoothing=eps, ignore_index=M.IGNORE, upstream=upstream)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def run_one_label(z, y, C, eps, grad=True, dbias0=DBIAS0):
    from vitssl_hip import ops
    out = _outputs(z.shape[0], C, grad, None, dbias0)
    ops.classify_loss(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), C, out["loss"], out["pred"], out["counters"], out["bad"],
                      dlogits=out.get("dlogits"), dbias=out.get("dbias"), label_smoothing=eps, ignore_index=M.IGNORE)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_mix(ref, got, z, y, partner, lam, C, eps, grad=True, dbias0=DBIAS0, bad0=3):
    """tests/test_gpu_classify.py::check_against with probability targets where that has integer ones"""
    B = z.shape[0]
    valid = ref["valid"]
    assert float(got["loss"][1]) == ref["n_valid"] and got["bad"].tolist() == [bad0 + ref["n_bad"]]
    if ref["n_valid"] == 0:
        assert float(got["loss"][0]) == 0.0 and math.isnan(float(got["loss"][0] / got["loss"][1]))
    else:
        t, v2 = M.soft_targets(y, partner, lam, C)
        assert (v2 == valid).all()
        t32 = float(F.cross_entropy(torch.from_numpy(z[:, :C][valid].copy()), torch.from_numpy(t.astype(np.float32)), label_smoothing=eps))
        mine = float(got["loss"][0]) / float(got["loss"][1])
        d_torch, d_mine = abs(t32 - ref["loss"]) / abs(ref["loss"]), abs(mine - ref["loss"]) / abs(ref["loss"])
        print(f"mix loss (B,C)=({B},{C}) eps={eps}: fp64 {ref['loss']:.12g}  torch fp32 cpu rel {d_torch:.3g}  kernel rel {d_mine:.3g}")
        assert d_mine <= max(4 * d_torch, 1e-6)
    assert np.array_equal(got["pred"].numpy(), ref["pred"])
    assert got["counters"].tolist() == [5 + ref["correct"], 9 + ref["n_valid"]]
    if not grad:
        return
    g = got["dlogits"].double().numpy()
    want = torch.from_numpy(ref["grad"]).to(BF16).double().numpy()           # the bf16-rounded fp64 value
    assert not np.isnan(g).any()
    err, bar = np.abs(g[:, :C] - want), 2.0 ** -8 * np.abs(ref["grad"])
    assert (err <= bar).all(), f"gradient: {int((err > bar).sum())} elements over the bar, first at {np.argwhere(err > bar)[0]}"
    assert not g[:, C:].any()                                                # the padding is zeros ...
    assert not g[~valid].any()                                               # ... and so is every ignored row
    db = got["dbias"].double().numpy() - dbias0                              # accumulated onto what was there
    if ref["n_valid"]:
        assert np.linalg.norm(db - ref["dbias"]) <= 1e-5 * np.linalg.norm(ref["dbias"])
    else:
        assert not db.any()


def same_bits(a, b, keys=None):
    for k in keys or a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), f"{k}: bits differ"


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C,ld", M.LOSS_SHAPES, ids=str)
def test_mix_loss_against_fp64(B, C, ld, eps):
    for rot in range(6):                                                     # every row meets each of the six lam values
        z, y, partner, lam, _ = M.make_loss_case(B, C, ld, rot=rot)
        ref = M.loss_reference(z, y, partner, lam, C, eps)
        got = run_mix(z, y, partner, lam, C, eps)
        check_mix(ref, got, z, y, partner, lam, C, eps)
        if rot == 0:
            same_bits(got, run_mix(z, y, partner, lam, C, eps))              # two runs: the same bits
            ev = run_mix(z, y, partner, lam, C, eps, grad=False)             # NULL dlogits: the evaluation case
            same_bits(got, ev, ("loss", "pred", "counters", "bad"))


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C,ld", M.LOSS_SHAPES, ids=str)
def test_one_label_rows_give_the_bits_of_classify_loss(B, C, ld, eps):
    """lam == 1 with partner == self, and every other way of writing a one-label row: loss_out, dlogits, dbias, pred, counters
    (and bad_labels) equal those of vitssl_classify_loss on the same inputs bit for bit."""
    z, y, _ = R.make_case(B, C, ld)
    want = run_one_label(z, y, C, eps)
    me = np.arange(B, dtype=np.int32)
    same_bits(want, run_mix(z, y, me, np.ones(B, np.float32), C, eps))
    same_bits(want, run_mix(z, y, me, M.LAMS[np.arange(B) % 6], C, eps))     # a == b: lam does not matter
    ok = (B - 1) // 3 * 3                                                    # a row whose label is valid
    same_bits(want, run_mix(z, y, np.full(B, ok, np.int32), np.ones(B, np.float32), C, eps))             # lam == 1: the partner does not matter
    y0 = np.where(y == M.IGNORE, M.IGNORE, y[ok])                            # lam == 0: the partner's label alone
    swapped = run_mix(z, y, np.full(B, ok, np.int32), np.zeros(B, np.float32), C, eps)
    want0 = run_one_label(z, y0, C, eps)
    same_bits(want0, swapped, ("loss", "dlogits", "dbias", "pred", "bad"))
    assert swapped["counters"][1] == want0["counters"][1]                    # (counters[0] compares with the row's own label)
    ev, ev_want = run_mix(z, y, me, np.ones(B, np.float32), C, eps, grad=False), run_one_label(z, y, C, eps, grad=False)
    same_bits(ev_want, ev)


@gpu
@pytest.mark.parametrize("B,C,ld", M.LOSS_SHAPES, ids=str)
def test_mix_loss_all_rows_ignored(B, C, ld):
    z, y, partner, lam, _ = M.make_loss_case(B, C, ld, all_ignored=True)
    ref = M.loss_reference(z, y, partner, lam, C, 0.1)
    assert ref["n_valid"] == 0 and ref["n_bad"] == 0
    check_mix(ref, run_mix(z, y, partner, lam, C, 0.1), z, y, partner, lam, C, 0.1)      # 0 / 0


@gpu
@pytest.mark.parametrize("B,C,ld", [M.LOSS_SHAPES[1], M.LOSS_SHAPES[3]], ids=str)
def test_bad_rows_are_flagged_and_ignored(B, C, ld):
    """An out-of-range label (own or the partner's), an out-of-range partner, lam NaN or 1.5: the row is ignored, bad_labels
    advances by exactly that many, and nothing else is disturbed."""
    z, y, partner, lam, _ = M.make_loss_case(B, C, ld)
    base = M.loss_reference(z, y, partner, lam, C, 0.1)
    rows = np.flatnonzero(base["valid"])
    cases = [("label", lambda y, p, l, i: y.__setitem__(i, C)), ("label<0", lambda y, p, l, i: y.__setitem__(i, -5)),
             ("partner=-1", lambda y, p, l, i: p.__setitem__(i, -1)), ("partner=B", lambda y, p, l, i: p.__setitem__(i, B)),
             ("partner=2^31-1", lambda y, p, l, i: p.__setitem__(i, 2 ** 31 - 1)), ("lam=nan", lambda y, p, l, i: l.__setitem__(i, np.nan)),
             ("lam=1.5", lambda y, p, l, i: l.__setitem__(i, 1.5)), ("lam<0", lambda y, p, l, i: l.__setitem__(i, -2.0 ** -30))]
    everything = (y.copy(), partner.copy(), lam.copy())
    for n, (name, poke) in enumerate(cases):
        y2, p2, l2 = y.copy(), partner.copy(), lam.copy()
        poke(y2, p2, l2, rows[n % len(rows)])
        poke(*everything, rows[n % len(rows)])
        ref = M.loss_reference(z, y2, p2, l2, C, 0.1)
        assert ref["n_bad"] >= 1 and ref["n_valid"] < base["n_valid"], name
        check_mix(ref, run_mix(z, y2, p2, l2, C, 0.1), z, y2, p2, l2, C, 0.1)
    ref = M.loss_reference(z, *everything, C, 0.1)
    assert ref["n_bad"] >= 3
    check_mix(ref, run_mix(z, *everything, C, 0.1), z, *everything, C, 0.1)


@gpu
def test_mix_loss_wide_gradient_rows_and_upstream():
    for (B, C, ld), ld_out in ((M.LOSS_SHAPES[1], 576), (M.LOSS_SHAPES[3], 1344)):
        z, y, partner, lam, _ = M.make_loss_case(B, C, ld, rot=2)
        got = run_mix(z, y, partner, lam, C, 0.1, ld_out=ld_out, upstream=0.5)
        assert got["dlogits"].shape == (B, ld_out)
        check_mix(M.loss_reference(z, y, partner, lam, C, 0.1, upstream=0.5), got, z, y, partner, lam, C, 0.1)
