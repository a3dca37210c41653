"""No GPU needed: everything that hangs on include/vitssl_classify.h is exported and bound, the ABI of vitssl_hip.h is what it
was, the argument checks of the entry point come before any launch, the fp64 restatement the GPU tests use
(tests/_classify_ref.py) is torch's own cross entropy, GradReducer's list of expected ranges, and the trainer's choice of
path and its un-freeze rule on a stub model."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _classify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitssl_classify.h")


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
def test_classify_header_is_bound_and_exported(built):
    from vitssl_hip import _lib
    protos = _prototypes()
    sizing = {"vitssl_classify_loss_workspace_floats"}
    launching = {n: a for n, (r, a) in _lib.REGISTRY["classify"].items() if r is ctypes.c_int}
    assert set(_lib.header_symbols("classify")) == set(protos) == set(_lib.REGISTRY["classify"]) == set(launching) | sizing
    assert {n for n, a in protos.items() if re.search(r"void\s*\*\s*stream", a)} == set(launching)
    raw = ctypes.CDLL(built.LIB_PATH)
    lib = built.lib()
    for n in protos:
        assert hasattr(raw, n), f"{n} declared in include/vitssl_classify.h but not exported"
    for n, args in launching.items():
        assert len(args) == len([a for a in protos[n].split(",") if a.strip()]), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype is ctypes.c_int
    assert lib.vitssl_classify_loss_workspace_floats.restype is ctypes.c_int64
    # the ABI of include/vitssl_hip.h is what it was, vitssl_cross_entropy included
    assert not set(protos) & set(_lib.header_symbols()) and not set(protos) & set(_lib.REGISTRY["hip"])
    assert "vitssl_cross_entropy" in _lib.REGISTRY["hip"] and lib.vitssl_version() == _lib.ABI_VERSION == 3
    import __graft_entry__ as ge
    assert "classify.hip" in ge.SOURCES


def test_sizing_and_argument_errors(built):
    """Pointer, geometry and workspace checks come before any launch: they can be exercised without a GPU."""
    from vitssl_hip import _lib, ops
    lib = built.lib()
    wsf = lib.vitssl_classify_loss_workspace_floats
    assert wsf(1, 2) == 4 + 4 and wsf(33, 10) == 68 + 33 * 12 and wsf(3, 65536) == 8 + 3 * 65536
    assert wsf(0, 10) == 0 and wsf(4, 1) == 0 and wsf(4, 65537) == 0
    one = ctypes.c_void_p(256)                                               # never dereferenced: every call below is refused
    fn = lib.vitssl_classify_loss

    def call(logits=one, labels=one, B=33, C=10, ld=64, eps=0.1, ign=-100, up=1.0, loss=one, dl=one, ld_out=64, db=one, pred=one,
             cnt=one, bad=one, ws=one, wsn=1 << 20):
        return fn(logits, labels, B, C, ld, eps, ign, up, loss, dl, ld_out, db, pred, cnt, bad, ws, wsn, None)

    for kw, msg in [(dict(logits=None), b"null pointer"), (dict(labels=None), b"null pointer"), (dict(loss=None), b"null pointer"),
                    (dict(pred=None), b"null pointer"), (dict(cnt=None), b"null pointer"), (dict(bad=None), b"null pointer"),
                    (dict(B=0), b"1 <= B"), (dict(C=1), b"2 <= C <= 65536"), (dict(C=65537, ld=65600, ld_out=65600), b"2 <= C <= 65536"),
                    (dict(C=100), b"ld >= C"), (dict(ld=62), b"multiple of 4"), (dict(ld_out=32), b"multiple of 64"),
                    (dict(C=100, ld=128, ld_out=64), b"ld_out >= C"), (dict(eps=1.5), b"label_smoothing"),
                    (dict(logits=ctypes.c_void_p(260)), b"16-byte aligned"), (dict(labels=ctypes.c_void_p(260)), b"8-byte aligned"),
                    (dict(ws=None), b"vitssl_classify_loss_workspace_floats"), (dict(wsn=wsf(33, 10) - 1), b"vitssl_classify_loss_workspace_floats")]:
        assert call(**kw) == -1 and msg in lib.vitssl_last_error(), (kw, lib.vitssl_last_error())
    z, y = torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64)
    out = (torch.zeros(2), torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.VitsslError, match="CUDA"):                      # no CPU fallback in the wrapper either
        ops.classify_loss(z, y, 10, *out)
    with pytest.raises(_lib.VitsslError, match="2 <= C"):
        ops.classify_loss(z, y, 65, *out)
    with pytest.raises(_lib.VitsslError, match="ld_out % 64"):
        ops.classify_loss(z, y, 10, *out, dlogits=torch.zeros(4, 32, dtype=torch.bfloat16))


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C,ld", R.SHAPES[:4], ids=str)
def test_restatement_is_torch_cross_entropy_in_fp64(B, C, ld, eps):
    z, y, (j1, j2) = R.make_case(B, C, ld)
    assert np.isnan(z[:, C:]).all() and z[0, j1] == z[0, j2] == z[0, :C].max() and j1 < j2
    if B >= 3:
        assert (y == R.IGNORE).any() and (y != R.IGNORE).any() and set(np.abs(z[B - 1, :C]).tolist()) == {80.0}
    ref = R.reference(z, y, C, eps)
    zt = torch.from_numpy(z[:, :C].astype(np.float64)).requires_grad_(True)
    loss = F.cross_entropy(zt, torch.from_numpy(y), label_smoothing=eps, ignore_index=R.IGNORE)
    loss.backward()
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert np.abs(ref["grad"] - zt.grad.numpy()).max() <= 1e-15             # torch's p - onehot carries the cancellation, not more
    assert ref["pred"][0] == j1 and (ref["pred"] == zt.detach().argmax(1).numpy()).all()
    assert ref["n_valid"] == int((y != R.IGNORE).sum())


def test_restatement_all_ignored_and_bad_labels():
    z, y, _ = R.make_case(33, 10, 64, all_ignored=True)
    ref = R.reference(z, y, 10, 0.1)
    zt = torch.from_numpy(z[:, :10].astype(np.float64)).requires_grad_(True)
    loss = F.cross_entropy(zt, torch.from_numpy(y), label_smoothing=0.1, ignore_index=R.IGNORE)
    loss.backward()
    assert math.isnan(ref["loss"]) and math.isnan(float(loss)) and ref["n_valid"] == 0 and ref["loss_sum"] == 0.0
    assert not ref["grad"].any() and not zt.grad.numpy().any()
    z, y, _ = R.make_case(33, 10, 64)
    bad = y.copy()
    bad[0], bad[2] = 10, -5                                                  # out of range: the rows count as ignored
    ign = y.copy()
    ign[0] = ign[2] = R.IGNORE
    a, b = R.reference(z, bad, 10, 0.1), R.reference(z, ign, 10, 0.1)
    assert a["loss_sum"] == b["loss_sum"] and a["n_valid"] == b["n_valid"] and (a["grad"] == b["grad"]).all()


# ---------------------------------------------------------------------------------------------- reducer ranges
def test_reducer_accepts_a_list_of_expected_ranges():
    from vitssl_hip._lib import VitsslError
    from vitssl_hip.engine import GradReducer
    g = torch.zeros(4096)
    r = GradReducer(g, expect=[(1024, 1500), (3072, 4096)])
    r.begin(); r.ready(3072, 4096); r.ready(1024, 1500); r.finish()
    assert r.stats() == (2, 4 * (1024 + 476))
    r.begin(); r.ready(3072, 3500); r.ready(3520, 4096); r.ready(1024, 1490); r.finish()     # alignment padding may be skipped
    r = GradReducer(g, bucket_mb=1e-4, expect=[(1024, 1500), (3072, 4096)])                  # every range a bucket of its own
    for ranges, msg in [([(3072, 4096)], "never handed"), ([(1024, 1500), (3072, 4096), (0, 512)], "outside the expected"),
                        ([(1024, 1500), (3072, 4096), (3072, 4096)], "reduced twice"), ([(1024, 1500), (2048, 2560), (3072, 4096)], "outside the expected"),
                        ([(1024, 1500), (3072, 3500)], r"\[3500, 4096\) was never handed")]:
        r.begin()
        for lo, hi in ranges:
            r.ready(lo, hi)
        with pytest.raises(VitsslError, match=msg):
            r.finish()
    r = GradReducer(g, expect=[(1024, 2048), (2048, 4096)])                  # adjacent ranges may arrive as one bucket
    r.begin(); r.ready(2048, 4096); r.ready(1024, 2048); r.finish()
    assert r.stats() == (1, 4 * 3072)
    for expect in (None, (0, 4096)):                                         # a single tuple and the default behave as before
        r = GradReducer(g, expect=expect)
        r.begin(); r.ready(0, 4096); r.finish()
        r.begin(); r.ready(0, 1024)
        with pytest.raises(VitsslError, match="never handed"):
            r.finish()


# ---------------------------------------------------------------------------------------------- trainer on a stub model
class _StubModel(nn.Module):
    """Records which path the trainer takes; parameters on the CPU, nothing is computed by the engine."""
    num_classes = 3

    def __init__(self):
        super().__init__()
        self.patch_embedding = nn.Linear(4, 4)
        self.encoder_blocks = nn.ModuleList([nn.Linear(4, 4)])
        self.classification_head = nn.Linear(4, 3)
        self.calls = []

    def forward(self, x):
        self.calls.append("forward")
        return self.classification_head(self.encoder_blocks[0](self.patch_embedding(x)))

    def train_step(self, x, labels, optimizer, reducer=None, label_smoothing=0.0, ignore_index=-100, counters=None):
        self.calls.append(("train_step", label_smoothing, ignore_index))
        self.last_pred = torch.zeros_like(labels)
        counters += torch.tensor([int((labels == 0).sum()), labels.numel()])
        return torch.tensor(1.5)

    def eval_step(self, x, labels, label_smoothing=0.0, ignore_index=-100, counters=None):
        self.calls.append(("eval_step", label_smoothing, ignore_index))
        self.last_pred = torch.zeros_like(labels)
        counters += torch.tensor([int((labels == 0).sum()), labels.numel()])
        return torch.tensor(2.5)

    def check_labels(self):
        self.calls.append("check_labels")

    def reduce_ranges(self):
        return None


def _cfg(fused=None, criterion=None, **training):
    t = {"type": "supervised", "num_epochs": 4, "warmup_epochs": 1, "warmup_initial_learning_rate": 1e-4,
         "warmup_final_learning_rate": 1e-2, "criterion": {"name": "CrossEntropyLoss", "params": criterion or {}},
         "optimizer": {"name": "SGD", "params": {"lr": 1e-2}},
         "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}}}
    if fused is not None:
        t["fused_step"] = fused
    t.update(training)
    return {"training": t, "eval": {}, "metrics": ["Accuracy", "F1Score"]}


def _trainer(cfg, model=None, fused_optimizer=True):
    from utils.trainers import SupervisedTrainer
    model = model or _StubModel()
    data = [(torch.rand(4, 4), torch.tensor([0, 1, 2, 0])), (torch.rand(4, 4), torch.tensor([0, 0, 2, 1]))]
    tr = SupervisedTrainer(model, "unused", cfg, data, data, "cpu")
    if fused_optimizer:
        tr._is_fused = lambda: True              # the stub has no flat store: stand in for "FusedAdamW over a model with train_step"
    return tr, model


def test_trainer_takes_the_fused_path_only_with_the_key_and_a_qualifying_criterion():
    tr, m = _trainer(_cfg(fused=True, criterion={"label_smoothing": 0.1, "ignore_index": -7}))
    out = tr.train_epoch(1)
    assert m.calls == [("train_step", 0.1, -7)] * 2 + ["check_labels"]
    assert set(out) == {"Loss", "Accuracy", "F1Score"} and out["Loss"] == 1.5 and out["Accuracy"] == 4 / 8
    del m.calls[:]
    out = tr.validate()
    assert m.calls == [("eval_step", 0.1, -7)] * 2 + ["check_labels"] and out["Loss"] == 2.5 and set(out) == {"Loss", "Accuracy", "F1Score"}
    for cfg, fused_opt in [(_cfg(), True), (_cfg(fused=False), True), (_cfg(fused=True, criterion={"reduction": "sum"}), True),
                           (_cfg(fused=True, criterion={"weight": torch.ones(3)}), True), (_cfg(fused=True), False)]:
        tr, m = _trainer(cfg, fused_optimizer=fused_opt)
        out = tr.train_epoch(1)
        tr.validate()
        assert m.calls == ["forward"] * 4 and set(out) == {"Loss", "Accuracy", "F1Score"}, cfg["training"]


@pytest.mark.parametrize("where", ["training", "top"])
def test_unfreeze_at_the_configured_epoch_carries_the_lr_and_the_schedulers(where):
    cfg = _cfg(freeze_backbone=True, **({"freeze_backbone_epochs": 3} if where == "training" else {}))
    if where == "top":
        cfg["freeze_backbone_epochs"] = 3                                    # the key the reference reads
    model = _StubModel()
    for part in (model.patch_embedding, model.encoder_blocks):
        for p in part.parameters():
            p.requires_grad = False
    tr, _ = _trainer(cfg, model, fused_optimizer=False)
    assert tr.freeze_backbone and tr.freeze_backbone_epochs == 3
    first = tr.optimizer
    assert len(first.param_groups[0]["params"]) == 2
    for epoch in (1, 2):
        tr.train_epoch(epoch)
        tr._update_schedulers(epoch)
    assert tr.optimizer is first and not model.patch_embedding.weight.requires_grad
    lr = first.param_groups[0]["lr"]
    assert 1e-6 < lr < 1e-2                                                  # warm-up done, one cosine step taken
    frozen_before = model.encoder_blocks[0].weight.clone()
    tr.train_epoch(3)
    assert tr.optimizer is not first and len(tr.optimizer.param_groups[0]["params"]) == 6 and not tr.optimizer.state_dict()["state"] is None
    assert all(p.requires_grad for p in model.parameters())
    assert tr.optimizer.param_groups[0]["lr"] == lr                          # carried over, not reset to the config's
    assert all(s.optimizer is tr.optimizer for s in tr.schedulers.values())
    assert not torch.equal(model.encoder_blocks[0].weight, frozen_before)    # the backbone trains again
    tr._update_schedulers(3)
    assert tr.optimizer.param_groups[0]["lr"] < lr and first.param_groups[0]["lr"] == lr     # the schedule drives the new optimizer
    tr.train_epoch(4)                                                        # only once
    assert len(tr.optimizer.param_groups[0]["params"]) == 6


def test_no_unfreeze_without_the_keys():
    model = _StubModel()
    for p in model.encoder_blocks.parameters():
        p.requires_grad = False
    tr, _ = _trainer(_cfg(freeze_backbone=True), model, fused_optimizer=False)
    assert tr.freeze_backbone_epochs == math.inf
    first = tr.optimizer
    tr.train_epoch(1)
    assert tr.optimizer is first and not model.encoder_blocks[0].weight.requires_grad
