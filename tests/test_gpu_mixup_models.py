"""ViT.train_step(..., mix=params) against the autograd path on the same mixed batch and the same soft targets, on the tiny ViT
of tests/test_gpu_classify.py (2 blocks, 32 x 32, patch 8, D 128, 8 images, 10 classes); what a step without `mix` launches;
reproducibility; the frozen-backbone schedule; one trainer epoch with `training.mixup`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import rel_l2
from test_gpu_classify import MODEL_BAR, _cfg, batch, fused_grads, tiny

DEV = torch.device("cuda:0")
gpu = pytest.mark.gpu
B, H, W, CLASSES = 8, 32, 32, 10


def hand_params(kind, lam, box=(0, 0, 0, 0)):
    flip = (B - 1 - np.arange(B)).astype(np.int32)
    full = lambda v: np.full(B, v, np.int32)                                 # noqa: E731
    return dict(kind=full(kind), partner=flip, y0=full(box[0]), y1=full(box[1]), x0=full(box[2]), x1=full(box[3]),
                lam=np.full(B, lam, np.float32))


def cases():
    from data import MixSpec, sample_mix_params
    elem = sample_mix_params(MixSpec(mode="elem"), B, H, W, torch.Generator().manual_seed(6))
    assert {1, 2} <= set(elem["kind"].tolist())                              # the draw blends some rows and pastes into others
    return {"batch-blend": hand_params(1, 0.3), "batch-paste": hand_params(2, 1.0 - 16 * 12 / (H * W), (8, 24, 4, 16)), "elem": elem}


def soft_targets(y, params):
    lam = params.lam[:, None]
    return lam * F.one_hot(y, CLASSES).float() + (1.0 - lam) * F.one_hot(y[params.partner.long()], CLASSES).float()


def autograd_mixed(model, mixer, x, y, params, eps):
    for p in model.parameters():
        p.grad = None
    loss = F.cross_entropy(model(mixer.apply(x, params)), soft_targets(y, params), label_smoothing=eps)
    loss.backward()
    return float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("case", ["batch-blend", "batch-paste", "elem"])
def test_train_step_with_mix_equals_the_autograd_path(case, eps):
    from data import GPUMixup, MixSpec
    x, y = batch()
    mixer = GPUMixup(MixSpec())
    params = mixer.to_device(cases()[case])
    a, b = tiny(), tiny()
    la, ga = autograd_mixed(a, mixer, x, y, params, eps)
    lb, gb, _ = fused_grads(b, x, y, label_smoothing=eps, mix=params)
    assert abs(la - lb) <= 1e-5 * abs(la)
    worst = max((rel_l2(gb[n], ga[n]), n) for n in ga)
    print(f"train_step(mix={case}) vs autograd, eps={eps}: largest relative L2 of a parameter gradient {worst[0]:.3g} ({worst[1]})")
    assert set(ga) == set(gb) and worst[0] < MODEL_BAR, worst
    plain, _, _ = fused_grads(tiny(), x, y, label_smoothing=eps)
    assert abs(plain - lb) > 1e-3 * abs(plain)                               # the mix is not a no-op
    b.check_labels()


@gpu
def test_step_without_mix_launches_what_it_launched(monkeypatch):
    from data import GPUMixup, MixSpec
    from vitssl_hip import ops
    x, y = batch()
    m = tiny()
    fused_grads(m, x, y)                                                     # (the first step also builds the head's operands)
    launched = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a, **k: (launched.append(name), real_call(name, *a, **k))[1])
    fused_grads(m, x, y)
    assert "vitssl_classify_loss" in launched and "vitssl_classify_loss_mix" not in launched and "vitssl_mix_batch" not in launched
    plain = list(launched)
    del launched[:]
    m.eval_step(x, y)
    assert "vitssl_classify_loss" in launched and "vitssl_classify_loss_mix" not in launched and "vitssl_mix_batch" not in launched
    del launched[:]
    fused_grads(m, x, y, mix=GPUMixup(MixSpec()).to_device(cases()["elem"]))
    assert launched.count("vitssl_mix_batch") == 1 and launched.count("vitssl_classify_loss_mix") == 1 and "vitssl_classify_loss" not in launched
    assert launched.index("vitssl_mix_batch") < launched.index("vitssl_classify_loss_mix")
    rest = [n for n in launched if n not in ("vitssl_mix_batch", "vitssl_classify_loss_mix")]
    assert rest == [n for n in plain if n != "vitssl_classify_loss"]         # everything else is the unmixed step


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_all_copy_mix_gives_the_bits_of_no_mix(eps):
    from data import GPUMixup, MixSpec
    x, y = batch()
    params = GPUMixup(MixSpec()).to_device(hand_params(0, 1.0))
    l0, _, r0 = fused_grads(tiny(), x, y, label_smoothing=eps)
    l1, _, r1 = fused_grads(tiny(), x, y, label_smoothing=eps, mix=params)
    assert np.float32(l0).tobytes() == np.float32(l1).tobytes() and r0.gflat.any()
    assert torch.equal(r0.gflat.view(torch.int32), r1.gflat.view(torch.int32))


@gpu
def test_mixed_steps_with_dropout_are_reproducible():
    from data import GPUMixup, MixSpec
    from vitssl_hip.optim import FusedAdamW
    x, y = batch()
    runs = []
    for _ in range(2):
        m = tiny(dropout=0.1)
        opt = FusedAdamW(m.flat_store(), lr=1e-3, weight_decay=1e-2)
        mixer = GPUMixup(MixSpec(mode="elem"))
        gen = torch.Generator().manual_seed(5)
        torch.manual_seed(77)
        losses = torch.stack([m.train_step(x, y, opt, mix=mixer.draw(B, H, W, gen)) for _ in range(6)]).cpu()
        runs.append((losses, m.flat_store().flat.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][0]).all() and len(set(runs[0][0].tolist())) == 6


@gpu
def test_head_only_schedule_with_mix_matches_autograd():
    from data import GPUMixup, MixSpec
    from utils.model_builder import freeze_backbone
    x, y = batch()
    mixer = GPUMixup(MixSpec())
    params = mixer.to_device(cases()["elem"])
    a, b = tiny(), tiny()
    for m in (a, b):
        freeze_backbone(m)
        m.patch_embedding.cls_token.requires_grad = False
    rt, st = b.runtime(), b.flat_store()
    assert rt.schedule() == "head"
    la, ga = autograd_mixed(a, mixer, x, y, params, 0.1)
    lb, gb, rec = fused_grads(b, x, y, label_smoothing=0.1, mix=params)
    lo, hi = st.span("classification_head.norm.weight", "classification_head.linear.bias")
    assert not rec.gflat[:lo].any() and not rec.gflat[hi:].any() and "a" not in rt.bb.stack._saved
    assert abs(la - lb) <= 1e-5 * abs(la) and set(ga) == {n for n in st.names if n.startswith("classification_head.")}
    for n in ga:
        assert rel_l2(gb[n], ga[n]) < MODEL_BAR, n


@gpu
def test_trainer_epoch_with_mixup(tmp_path):
    """One epoch from a synthetic uint8 loader with `training.mixup`: every training step is handed a fresh draw, the loss is
    finite, and validation is the unmixed validation of a trainer without the key."""
    from data import MixParams
    from utils.model_builder import build_model
    from utils.trainers import SupervisedTrainer
    crop = [{"name": "RandomResizedCrop", "params": {"size": 32, "scale": [0.9, 1.0]}}, {"name": "RandomHorizontalFlip", "params": {}},
            {"name": "ToTensor"}]
    resize = [{"name": "Resize", "params": {"size": [32, 32]}}, {"name": "ToTensor"}]
    g = torch.Generator().manual_seed(3)
    data = [(torch.randint(0, 256, (8, 40, 48, 3), dtype=torch.uint8, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(3)]
    trainers = []
    for mixup in (None, {"mixup_alpha": 0.8, "cutmix_alpha": 1.0, "mode": "elem"}):
        cfg = dict(_cfg(True), transforms={"train": crop, "val": resize})
        if mixup:
            cfg["training"]["mixup"] = mixup
        torch.manual_seed(31)
        tr = SupervisedTrainer(build_model(cfg).to(DEV), str(tmp_path / ("m" if mixup else "p")), cfg, data, data[:2], DEV)
        tr.transform_generator = torch.Generator().manual_seed(99)
        trainers.append(tr)
    plain, mixed = trainers
    assert plain.mixup is None and mixed.mixup is not None and mixed.mixup.spec.mode == "elem" and mixed._fused_path()
    assert plain.validate() == mixed.validate()                              # same weights: validation never mixes
    seen = []
    for tr in trainers:
        step, ev = tr.model.train_step, tr.model.eval_step
        tr.model.train_step = lambda *a, _s=step, **k: (seen.append(("train", k.get("mix"))), _s(*a, **k))[1]
        tr.model.eval_step = lambda *a, _e=ev, **k: (seen.append(("eval", k.get("mix"))), _e(*a, **k))[1]
    tp, tm = plain.train_epoch(1), mixed.train_epoch(1)
    assert [m for k, m in seen[:3]] == [None] * 3 and all(isinstance(m, MixParams) for k, m in seen[3:6]) and len(seen) == 6
    assert len({tuple(m.lam.tolist()) for _, m in seen[3:6]}) == 3           # a fresh draw per batch
    assert np.isfinite(tm["Loss"]) and tm["Loss"] != tp["Loss"] and 0.0 <= tm["Accuracy"] <= 1.0
    del seen[:]
    vm = mixed.validate()
    assert [k for k, _ in seen] == ["eval"] * 2 and all(m is None for _, m in seen) and np.isfinite(vm["Loss"])
