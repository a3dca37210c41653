"""ViT.train_step / eval_step with loss="bce" against the autograd path with utils.losses.BinaryCrossEntropy on the tiny ViT of
tests/test_gpu_classify.py (2 blocks, 32 x 32, patch 8, D 128, 8 images, 10 classes): the loss within 1e-5 relative, every
parameter gradient within the model bar; with `mix` against the autograd path on the same mixed batch with dense targets; three
optimisation steps; a trainer epoch configured with the criterion; and what a step with loss="ce" launches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import rel_l2
from test_gpu_classify import MODEL_BAR, _cfg, autograd_grads, batch, fused_grads, tiny
from test_gpu_mixup_models import CLASSES, cases

DEV = torch.device("cuda:0")
I64 = torch.int64
gpu = pytest.mark.gpu
CASES = [dict(eps=0.0), dict(eps=0.1), dict(eps=0.1, sum_classes=True), dict(eps=0.1, target_threshold=0.2)]


def criterion(case):
    from utils.losses import BinaryCrossEntropy
    return BinaryCrossEntropy(smoothing=case["eps"], target_threshold=case.get("target_threshold"), sum_classes=case.get("sum_classes", False))


def step_keywords(case):
    return dict(label_smoothing=case["eps"], loss="bce", target_threshold=case.get("target_threshold"), sum_classes=case.get("sum_classes", False))


def compare(la, ga, lb, gb, what):
    assert abs(la - lb) <= 1e-5 * abs(la), (la, lb)
    worst = max((rel_l2(gb[n], ga[n]), n) for n in ga)
    print(f"{what}: loss {lb:.8g} (autograd {la:.8g}), largest relative L2 of a parameter gradient {worst[0]:.3g} ({worst[1]})")
    assert worst[0] < MODEL_BAR, worst


@gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_train_step_bce_equals_the_autograd_path(case):
    x, y = batch()
    y = y.clone()
    y[5] = -100                                                              # an ignored row is left out of the mean on both paths
    a, b = tiny(), tiny()
    la, ga = autograd_grads(a, x, y, criterion(case))
    lb, gb, _ = fused_grads(b, x, y, **step_keywords(case))
    assert set(ga) == set(gb)
    compare(la, ga, lb, gb, f"train_step(loss=bce, {case}) vs autograd")
    assert b.last_logits.shape == (8, 10) and torch.equal(b.last_pred, b.last_logits.argmax(1))
    ce, _, _ = fused_grads(tiny(), x, y, label_smoothing=case["eps"])
    assert abs(ce - lb) > 1e-3 * abs(ce)                                     # not the softmax loss
    b.check_labels()


@gpu
def test_head_only_schedule_with_bce_matches_autograd():
    from utils.model_builder import freeze_backbone
    x, y = batch()
    a, b = tiny(), tiny()
    for m in (a, b):
        freeze_backbone(m)
        m.patch_embedding.cls_token.requires_grad = False
    rt, st = b.runtime(), b.flat_store()
    assert rt.schedule() == "head"
    la, ga = autograd_grads(a, x, y, criterion(CASES[1]))
    lb, gb, rec = fused_grads(b, x, y, **step_keywords(CASES[1]))
    lo, hi = st.span("classification_head.norm.weight", "classification_head.linear.bias")
    assert not rec.gflat[:lo].any() and not rec.gflat[hi:].any() and "a" not in rt.bb.stack._saved
    assert set(ga) == {n for n in st.names if n.startswith("classification_head.")}
    compare(la, ga, lb, gb, "head schedule, bce")


@gpu
@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=str)
@pytest.mark.parametrize("kind", ["batch-blend", "elem"])
def test_train_step_bce_with_mix_equals_the_autograd_path(kind, case):
    """the autograd path on the same mixed batch, with the dense targets lam s(y) + (1 - lam) s(y[partner]) handed to the module"""
    from data import GPUMixup, MixSpec
    x, y = batch()
    mixer = GPUMixup(MixSpec())
    params = mixer.to_device(cases()[kind])
    eps = case["eps"]
    s = lambda lab: F.one_hot(lab, CLASSES).float() * (1.0 - eps) + eps / CLASSES      # noqa: E731
    lam = params.lam[:, None]
    dense = lam * s(y) + (1.0 - lam) * s(y[params.partner.long()])
    if case.get("target_threshold") is not None:
        assert float((dense - case["target_threshold"]).abs().min()) >= 1e-3          # no target near a tie with the threshold
    a, b = tiny(), tiny()
    for p in a.parameters():
        p.grad = None
    loss = criterion(case)(a(mixer.apply(x, params)), dense)
    loss.backward()
    la, ga = float(loss.detach()), {n: p.grad.clone() for n, p in a.named_parameters() if p.grad is not None}
    lb, gb, _ = fused_grads(b, x, y, mix=params, **step_keywords(case))
    assert set(ga) == set(gb)
    compare(la, ga, lb, gb, f"train_step(loss=bce, mix={kind}, {case}) vs autograd")
    plain, _, _ = fused_grads(tiny(), x, y, **step_keywords(case))
    assert abs(plain - lb) > 1e-4 * abs(plain)                               # the mix is not a no-op: 10 x the bar of the comparison above
    b.check_labels()


@gpu
def test_eval_step_bce_is_the_no_grad_forward():
    x, y = batch()
    m = tiny(dropout=0.1)
    counters = torch.zeros(2, dtype=I64, device=DEV)
    case = CASES[2]
    loss = m.eval_step(x, y, counters=counters, **step_keywords(case))
    m.eval()
    with torch.no_grad():
        logits = m(x)
        want = float(criterion(case)(logits, y))
    m.train()
    assert abs(float(loss) - want) <= 1e-5 * want
    assert float((m.last_logits - logits).abs().max()) <= 1e-5 and torch.equal(m.last_pred, logits.argmax(1))
    assert counters.tolist() == [int((logits.argmax(1) == y).sum()), 8]


@gpu
def test_three_bce_steps_equal_three_autograd_steps():
    from vitssl_hip.optim import FusedAdamW
    x, y = batch()
    a, b = tiny(), tiny()
    oa, ob = FusedAdamW(a.flat_store(), lr=1e-3, weight_decay=1e-2), FusedAdamW(b.flat_store(), lr=1e-3, weight_decay=1e-2)
    crit = criterion(CASES[1])
    counters = torch.zeros(2, dtype=I64, device=DEV)
    for _ in range(3):
        oa.zero_grad(set_to_none=True)
        crit(a(x), y).backward()
        oa.step()
        b.train_step(x, y, ob, counters=counters, **step_keywords(CASES[1]))
    torch.cuda.synchronize()
    sa, sb = a.flat_store(), b.flat_store()
    for n in sa.names:
        assert rel_l2(sb.view(n), sa.view(n)) < MODEL_BAR, n
    assert not torch.equal(sb.flat, tiny().flat_store().flat) and int(counters[1]) == 24 and 0 <= int(counters[0]) <= 24
    b.check_labels()


def _bce_cfg(fused, **params):
    cfg = _cfg(fused)
    cfg["training"]["criterion"] = {"name": "BinaryCrossEntropy", "params": dict(smoothing=0.1, **params)}
    return cfg


@gpu
@pytest.mark.parametrize("params", [{}, {"sum_classes": True, "target_threshold": 0.2}], ids=str)
def test_trainer_epoch_with_the_criterion_reports_what_the_default_path_reports(tmp_path, params):
    from utils.losses import BinaryCrossEntropy
    from utils.model_builder import build_model
    from utils.trainers import SupervisedTrainer
    g = torch.Generator().manual_seed(9)
    data = [(torch.rand(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(2)]
    trainers = []
    for fused in (False, True):
        torch.manual_seed(31)
        model = build_model(_bce_cfg(fused, **params)).to(DEV)
        trainers.append(SupervisedTrainer(model, str(tmp_path / ("f" if fused else "d")), _bce_cfg(fused, **params), data[:1], data, DEV))
    d, f = trainers
    assert f._fused_path() and not d._fused_path() and type(f.criterion) is BinaryCrossEntropy is type(d.criterion)
    seen = []
    step, ev = f.model.train_step, f.model.eval_step
    f.model.train_step = lambda *a, **k: (seen.append(k), step(*a, **k))[1]
    f.model.eval_step = lambda *a, **k: (seen.append(k), ev(*a, **k))[1]
    vd, vf = d.validate(), f.validate()
    assert set(vd) == set(vf) == {"Loss", "Accuracy", "F1Score"}
    assert vd["Accuracy"] == vf["Accuracy"] and vd["F1Score"] == vf["F1Score"] and abs(vd["Loss"] - vf["Loss"]) <= 1e-5 * vd["Loss"]
    td, tf = d.train_epoch(1), f.train_epoch(1)                              # one batch: predictions of the same weights
    assert td["Accuracy"] == tf["Accuracy"] and td["F1Score"] == tf["F1Score"] and abs(td["Loss"] - tf["Loss"]) <= 1e-5 * td["Loss"]
    assert len(seen) == 3 and all(k["loss"] == "bce" and k["label_smoothing"] == 0.1 and k["sum_classes"] == params.get("sum_classes", False)
                                  and k["target_threshold"] == params.get("target_threshold") and k["ignore_index"] == -100 for k in seen)


@gpu
def test_trainer_mixup_composes_with_the_criterion(tmp_path):
    from data import MixParams
    from utils.model_builder import build_model
    from utils.trainers import SupervisedTrainer
    g = torch.Generator().manual_seed(3)
    data = [(torch.rand(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(2)]
    cfg = _bce_cfg(True)
    cfg["training"]["mixup"] = {"mixup_alpha": 0.8, "cutmix_alpha": 1.0, "mode": "elem"}
    torch.manual_seed(31)
    tr = SupervisedTrainer(build_model(cfg).to(DEV), str(tmp_path / "m"), cfg, data, data[:1], DEV)
    tr.transform_generator = torch.Generator().manual_seed(99)
    seen = []
    step = tr.model.train_step
    tr.model.train_step = lambda *a, **k: (seen.append(k), step(*a, **k))[1]
    out = tr.train_epoch(1)
    assert len(seen) == 2 and all(isinstance(k["mix"], MixParams) and k["loss"] == "bce" for k in seen)
    assert np.isfinite(out["Loss"]) and 0.0 <= out["Accuracy"] <= 1.0


@gpu
def test_default_loss_launches_what_it_launched_and_gives_the_same_bits(monkeypatch):
    from vitssl_hip import ops
    x, y = batch()
    l0, _, r0 = fused_grads(tiny(), x, y, label_smoothing=0.1)
    l1, _, r1 = fused_grads(tiny(), x, y, label_smoothing=0.1, loss="ce")
    assert np.float32(l0).tobytes() == np.float32(l1).tobytes() and r0.gflat.any()
    assert torch.equal(r0.gflat.view(torch.int32), r1.gflat.view(torch.int32))
    m = tiny()
    fused_grads(m, x, y)                                                     # (the first step also builds the head's operands)
    launched = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a, **k: (launched.append(name), real_call(name, *a, **k))[1])
    fused_grads(m, x, y, loss="ce")
    e0 = m.eval_step(x, y, loss="ce")
    assert "vitssl_classify_loss" in launched and not [n for n in launched if "bce" in n]
    plain = [n for n in launched]
    assert np.float32(float(e0)).tobytes() == np.float32(float(m.eval_step(x, y))).tobytes()
    del launched[:]
    fused_grads(m, x, y, loss="bce")
    m.eval_step(x, y, loss="bce")
    assert launched.count("vitssl_classify_bce") == 2 and "vitssl_classify_loss" not in launched
    assert [n for n in launched if n != "vitssl_classify_bce"] == [n for n in plain if n != "vitssl_classify_loss"]
    for bad in ("focal", "BCE", None):
        with pytest.raises(ValueError, match="neither"):
            m.train_step(x, y, None, loss=bad)
        with pytest.raises(ValueError, match="neither"):
            m.eval_step(x, y, loss=bad)
