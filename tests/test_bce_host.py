"""No GPU needed: everything that hangs on include/vitssl_bce.h is exported and bound and every other header's ABI is what it
was, the argument checks come before any launch, the fp64 restatement the GPU tests use (tests/_bce_ref.py) is torch's own
binary_cross_entropy_with_logits on explicit dense targets, utils.losses.BinaryCrossEntropy is the same in value and gradient,
make_criterion builds it from a config, and the checker of the GPU tests refuses the wrong gradients it is there to catch."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bce_ref as Bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitssl_bce.h")
HOST_SHAPES = Bc.SHAPES[:4]


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vitssl_hip
    return vitssl_hip


def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|int64_t)\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


# ---------------------------------------------------------------------------------------------- header completeness
def test_bce_header_is_bound_and_exported(built):
    from vitssl_hip import _lib
    protos = _prototypes()
    sizing = {"vitssl_classify_bce_workspace_floats"}
    launching = {n: a for n, (r, a) in _lib.REGISTRY["bce"].items() if r is ctypes.c_int}
    assert set(_lib.header_symbols("bce")) == set(protos) == set(_lib.REGISTRY["bce"]) == set(launching) | sizing
    raw, lib = ctypes.CDLL(built.LIB_PATH), built.lib()
    for n in protos:
        assert hasattr(raw, n), f"{n} declared in include/vitssl_bce.h but not exported"
    for n, args in launching.items():
        assert len(args) == len([a for a in protos[n].split(",") if a.strip()]), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype is ctypes.c_int
    assert lib.vitssl_classify_bce_workspace_floats.restype is ctypes.c_int64
    others = {n for key in _lib.HEADERS if key != "bce" for n in _lib.header_symbols(key)}
    assert not set(protos) & others                                          # disjoint from every other header ...
    assert set(_lib.header_symbols("classify")) == {"vitssl_classify_loss", "vitssl_classify_loss_workspace_floats"}      # ... which are what they were
    assert set(_lib.header_symbols("mixup")) == {"vitssl_mix_batch", "vitssl_classify_loss_mix", "vitssl_classify_loss_mix_workspace_floats"}
    assert lib.vitssl_version() == _lib.ABI_VERSION == 3


def test_sizing_and_argument_errors(built):
    """Pointer, geometry, table and workspace checks come before any launch: they can be exercised without a GPU."""
    from vitssl_hip import _lib, ops
    lib = built.lib()
    wsf = lib.vitssl_classify_bce_workspace_floats
    for B, C in [(1, 2), (33, 10), (3, 65536), (0, 10), (4, 1), (4, 65537), ((1 << 22) + 1, 10)]:
        assert wsf(B, C) == lib.vitssl_classify_loss_workspace_floats(B, C)
    one = ctypes.c_void_p(256)                                               # never dereferenced: every call below is refused
    fn = lib.vitssl_classify_bce

    def loss(logits=one, labels=one, partner=one, lam=one, B=33, C=10, ld=64, eps=0.1, thr=-1.0, sumc=0, ign=-100, up=1.0, out=one, dl=one,
             ld_out=64, db=one, pred=one, cnt=one, bad=one, ws=one, wsn=1 << 20):
        return fn(logits, labels, partner, lam, B, C, ld, eps, thr, sumc, ign, up, out, dl, ld_out, db, pred, cnt, bad, ws, wsn, None)

    for kw, msg in [(dict(logits=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(partner=None), b"both NULL"),
                    (dict(lam=None), b"both NULL"), (dict(thr=float("nan")), b"target_threshold"),
                    (dict(B=0), b"1 <= B"), (dict(B=(1 << 22) + 1), b"1 <= B"), (dict(C=1), b"2 <= C <= 65536"), (dict(C=100), b"ld >= C"),
                    (dict(ld=62), b"multiple of 4"), (dict(ld_out=32), b"multiple of 64"), (dict(eps=1.5), b"0 <= eps <= 1"),
                    (dict(eps=-0.1), b"0 <= eps <= 1"), (dict(logits=ctypes.c_void_p(260)), b"16-byte aligned"),
                    (dict(partner=ctypes.c_void_p(258)), b"4-byte aligned"), (dict(ws=None), b"vitssl_classify_bce_workspace_floats"),
                    (dict(partner=None, lam=None, wsn=wsf(33, 10) - 1), b"vitssl_classify_bce_workspace_floats"),
                    (dict(wsn=wsf(33, 10) - 1), b"vitssl_classify_bce_workspace_floats")]:
        assert loss(**kw) == -1 and msg in lib.vitssl_last_error() and b"classify_bce" in lib.vitssl_last_error(), (kw, lib.vitssl_last_error())
    z, y = torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64)
    out = (torch.zeros(2), torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.VitsslError, match="CUDA"):                      # no CPU fallback in the wrapper either
        ops.classify_bce(z, y, 10, *out)
    with pytest.raises(_lib.VitsslError, match="2 <= C"):
        ops.classify_bce(z, y, 65, *out)
    with pytest.raises(_lib.VitsslError, match="both None"):
        ops.classify_bce(z, y, 10, *out, partner=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(_lib.VitsslError, match="target_threshold"):
        ops.classify_bce(z, y, 10, *out, target_threshold=-0.5)


# ---------------------------------------------------------------------------------------------- the restatement
def dense_targets(y, partner, lam, C, eps, threshold):
    """The targets as a user of torch would write them, independently of tests/_bce_ref.py: fp64 [n_kept, C] and the kept rows
    (own and partner label both not ignored)."""
    y = torch.from_numpy(np.asarray(y))
    yb = y if partner is None else y[torch.from_numpy(np.asarray(partner)).long()]
    l = torch.ones(len(y), dtype=torch.float64) if lam is None else torch.from_numpy(np.asarray(lam, np.float32)).double()
    keep = (y != Bc.IGNORE) & (yb != Bc.IGNORE)
    s = lambda lab: F.one_hot(lab[keep], C).double() * (1.0 - eps) + eps / C      # noqa: E731
    t = l[keep, None] * s(y) + (1.0 - l[keep, None]) * s(yb)
    if threshold is not None:
        t = (t > threshold).double()
    return t, keep


def torch_bce(z, t, sum_classes):
    if sum_classes:
        return F.binary_cross_entropy_with_logits(z, t, reduction="none").sum(-1).mean()
    return F.binary_cross_entropy_with_logits(z, t)


CASES = [dict(eps=0.0), dict(eps=0.1), dict(eps=0.1, sum_classes=True), dict(eps=0.1, threshold=0.2), dict(eps=0.1, threshold=0.0),
         dict(eps=0.0, threshold=0.2, sum_classes=True)]


@pytest.mark.parametrize("two", [False, True], ids=["one-label", "two-label"])
@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("B,C,ld", HOST_SHAPES, ids=str)
def test_restatement_is_torch_bce_with_logits_on_dense_targets(B, C, ld, case, two):
    eps, threshold, sum_classes = case["eps"], case.get("threshold"), case.get("sum_classes", False)
    z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld, rot=1)
    if not two:
        partner = lam = None
    ref = Bc.reference(z, y, C, eps, partner, lam, threshold, sum_classes)
    t, keep = dense_targets(y, partner, lam, C, eps, threshold)
    assert ref["n_valid"] == int(keep.sum()) >= 1 and ref["n_bad"] == 0 and (ref["valid"] == keep.numpy()).all()
    if B >= 3:
        assert not keep.all()                                                # an ignored row is left out of the mean
    if B == 1:
        assert 0.1 < ref["loss"] < 10.0 * (C if sum_classes else 1)          # logits of ordinary size: the loss is not about 0
    zt = torch.from_numpy(z[:, :C].astype(np.float64))[keep].requires_grad_(True)
    loss = torch_bce(zt, t, sum_classes)
    loss.backward()
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    g = ref["grad"][keep.numpy()]
    assert (np.abs(g - zt.grad.numpy()) <= 1e-12 * np.abs(g) + 1e-17).all()
    assert not ref["grad"][~keep.numpy()].any()
    assert np.abs(ref["t"][keep.numpy()] - t.numpy()).max() <= 1e-15
    assert ref["correct"] == int((z[:, :C].argmax(1)[keep.numpy()] == y[keep.numpy()]).sum())       # against the row's own label


def test_restatement_all_ignored_bad_rows_and_degenerate_tables():
    B, C, ld = Bc.SHAPES[1]
    z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld, all_ignored=True)
    ref = Bc.reference(z, y, C, 0.1, partner, lam)
    assert ref["n_valid"] == 0 and math.isnan(ref["loss"]) and ref["loss_sum"] == 0.0 and not ref["grad"].any()
    z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld)
    base = Bc.reference(z, y, C, 0.1, partner, lam)
    y2, p2, l2 = y.copy(), partner.copy(), lam.copy()
    rows = np.flatnonzero(base["valid"])
    y2[rows[0]], p2[rows[1]], l2[rows[2]] = C, B, np.nan
    ref = Bc.reference(z, y2, C, 0.1, p2, l2)
    assert ref["n_bad"] >= 3 and ref["n_valid"] <= base["n_valid"] - 3 and np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all()
    one = Bc.reference(z, y, C, 0.1)                                         # a == b, l == 1: the one-label values
    for p, l in ((np.arange(B, dtype=np.int32), lam), (partner, np.ones(B, np.float32))):
        two = Bc.reference(z, y, C, 0.1, p, l)
        keep = two["valid"]                                                  # (a partner's ignored label still ignores the row)
        assert np.allclose(two["grad"][keep] * two["n_valid"], one["grad"][keep] * one["n_valid"], rtol=1e-14, atol=0.0)


# ---------------------------------------------------------------------------------------------- the torch module
def test_module_is_torch_bce_in_value_and_gradient(built):
    from utils.losses import BinaryCrossEntropy
    B, C, ld = Bc.SHAPES[1]
    z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld, rot=1)
    for case in CASES:
        eps, threshold, sum_classes = case["eps"], case.get("threshold"), case.get("sum_classes", False)
        crit = BinaryCrossEntropy(smoothing=eps, target_threshold=threshold, sum_classes=sum_classes)
        ref = Bc.reference(z, y, C, eps, None, None, threshold, sum_classes)
        zt = torch.from_numpy(z[:, :C].astype(np.float64)).requires_grad_(True)
        loss = crit(zt, torch.from_numpy(y))                                 # integer labels, every third one ignored
        loss.backward()
        assert abs(float(loss.detach()) - ref["loss"]) <= 1e-12 * abs(ref["loss"]), case
        assert (np.abs(zt.grad.numpy() - ref["grad"]) <= 1e-12 * np.abs(ref["grad"]) + 1e-17).all(), case
        # dense targets (what Mixup hands a criterion): used as they are, every row counts
        t, keep = dense_targets(y, partner, lam, C, eps, None)
        zk = torch.from_numpy(z[:, :C].astype(np.float64))[keep]
        za, zb = zk.clone().requires_grad_(True), zk.clone().requires_grad_(True)
        mine = crit(za, t)
        want = torch_bce(zb, t if threshold is None else (t > threshold).double(), sum_classes)
        mine.backward()
        want.backward()
        assert float(mine.detach()) == float(want.detach()) and torch.equal(za.grad, zb.grad), case
        two = Bc.reference(z, y, C, eps, partner, lam, threshold, sum_classes)
        assert abs(float(mine.detach()) - two["loss"]) <= 1e-12 * abs(two["loss"])
    z32 = torch.from_numpy(z[:, :C].copy())
    keep = torch.from_numpy(y != Bc.IGNORE)
    crit = BinaryCrossEntropy(smoothing=0.1)
    t32 = dense_targets(y[y != Bc.IGNORE], None, None, C, 0.1, None)[0].float()
    want32 = float(torch_bce(z32[keep], t32, False))                         # fp32, no ignored label: timm's statement
    assert abs(float(crit(z32[keep], torch.from_numpy(y)[keep])) - want32) <= 1e-6 * want32
    assert abs(float(crit(z32, torch.from_numpy(y))) - want32) <= 1e-6 * want32          # ... and the same with the ignored rows in
    assert math.isnan(float(crit(z32, torch.full((B,), Bc.IGNORE))))         # 0 / 0, as nn.CrossEntropyLoss gives
    assert "smoothing=0.1" in repr(crit) and crit.ignore_index == -100 and crit.target_threshold is None and crit.sum_classes is False
    for bad in (dict(smoothing=1.5), dict(smoothing=-0.1), dict(target_threshold=-1.0), dict(target_threshold=float("nan"))):
        with pytest.raises(ValueError, match="BinaryCrossEntropy"):
            BinaryCrossEntropy(**bad)
    with pytest.raises(ValueError, match="dense targets"):
        crit(z32, torch.zeros(B, C + 1))


def test_make_criterion_builds_it_from_a_config(built):
    from torch import nn
    from utils import make_criterion
    from utils.losses import BinaryCrossEntropy
    c = make_criterion({"training": {"criterion": {"name": "BinaryCrossEntropy", "params": {"smoothing": 0.2, "target_threshold": 0.3,
                                                                                             "sum_classes": True}}}})
    assert type(c) is BinaryCrossEntropy and (c.smoothing, c.target_threshold, c.sum_classes, c.ignore_index) == (0.2, 0.3, True, -100)
    c = make_criterion({"training": {"criterion": {"name": "BinaryCrossEntropy", "params": {}}}})
    assert type(c) is BinaryCrossEntropy and c.smoothing == 0.1
    c = make_criterion({"training": {"criterion": {"name": "CrossEntropyLoss", "params": {"label_smoothing": 0.1}}}})
    assert type(c) is nn.CrossEntropyLoss and c.label_smoothing == 0.1       # torch.nn's names resolve as before


def test_step_keywords_are_checked_before_anything_runs(built):
    from vit_core.vit import loss_spec
    assert loss_spec("ce", None, False) is None
    assert loss_spec("bce", None, False) == (None, False) and loss_spec("bce", 0.2, 1) == (0.2, True)
    for args, msg in ((("focal", None, False), "neither"), (("BCE", None, False), "neither"), (("ce", 0.2, False), 'loss="bce"'),
                      (("ce", None, True), 'loss="bce"'), (("bce", -0.1, False), "target_threshold")):
        with pytest.raises(ValueError, match=msg):
            loss_spec(*args)


# ---------------------------------------------------------------------------------------------- negative controls of the checker
def _control():
    B, C, ld = Bc.SHAPES[1]
    z, y, partner, lam, _ = Bc.make_mix_case(B, C, ld, rot=1)
    return z, y, partner, lam, C


def _as_kernel_output(grad, C, ld_out=64):
    """an fp64 gradient as the checker receives the kernel's: rounded to bf16, zero-padded to ld_out"""
    g = np.zeros((grad.shape[0], ld_out))
    g[:, :C] = torch.from_numpy(grad).to(torch.bfloat16).double().numpy()
    return g


def test_checker_accepts_the_restatement_and_refuses_a_softmax_gradient():
    z, y, partner, lam, C = _control()
    ref = Bc.reference(z, y, C, 0.1, partner, lam)
    Bc.check_grad(ref, _as_kernel_output(ref["grad"], C), C)                 # the control of the controls
    zz = z[:, :C].astype(np.float64)
    p = np.exp(zz - zz.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    soft = (p - ref["soft"]) / ref["n_valid"]                                # what vitssl_classify_loss_mix writes
    soft[~ref["valid"]] = 0.0
    with pytest.raises(AssertionError, match="gradient"):
        Bc.check_grad(ref, _as_kernel_output(soft, C), C)


def test_checker_refuses_a_gradient_divided_by_n_valid_only():
    z, y, partner, lam, C = _control()
    ref = Bc.reference(z, y, C, 0.1, partner, lam, sum_classes=False)
    with pytest.raises(AssertionError, match="gradient"):
        Bc.check_grad(ref, _as_kernel_output(ref["grad"] * C, C), C)         # the 1 / C of the mean over the classes forgotten
    summed = Bc.reference(z, y, C, 0.1, partner, lam, sum_classes=True)
    Bc.check_grad(summed, _as_kernel_output(ref["grad"] * C, C), C)          # ... which is right exactly when sum_classes is on
    with pytest.raises(AssertionError):
        Bc.check_loss(ref, (summed["loss_sum"], summed["n_valid"]), ref["loss"])


def test_checker_refuses_an_unthresholded_target():
    z, y, partner, lam, C = _control()
    ref = Bc.reference(z, y, C, 0.1, partner, lam, threshold=0.2)
    soft = Bc.reference(z, y, C, 0.1, partner, lam)
    assert np.abs(ref["soft"][ref["valid"]] - 0.2).min() >= 1e-3             # no input near a tie with the threshold
    Bc.check_grad(ref, _as_kernel_output(ref["grad"], C), C)
    with pytest.raises(AssertionError, match="gradient"):
        Bc.check_grad(ref, _as_kernel_output(soft["grad"], C), C)
    with pytest.raises(AssertionError):
        Bc.check_loss(ref, (soft["loss_sum"], soft["n_valid"]), ref["loss"])
