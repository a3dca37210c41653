"""Fused train steps with FusedLamb on the three models.  After each fused step the flat gradient buffer still holds the
unclipped gradient of that step, so the float64 restatement of include/vitssl_lamb.h (tests/_lamb_ref.py), applied to that
gradient and the parameters before the step, must reproduce the parameters after it.  The bar is the op test's:
max(4 x the float32-vs-float64 distance of the restatement on the same gradients, 2e-6).  Then the frozen backbone, the
checkpoint round trip, make_optimizer / _is_fused and the refused configs."""
import copy

import pytest
import torch

import _lamb_ref as R

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
LR, WD, DECAY = 2e-3, 0.05, 0.75
VIT = dict(num_blocks=2, input_shape=(3, 32, 32), embed_dim=64, patch_size=8, num_heads=2, mlp_dim=128, dropout=0.0)


def _cfg(name="Lamb", params=None, **training):
    t = {"type": "supervised", "num_epochs": 4, "warmup_epochs": 1, "warmup_initial_learning_rate": LR, "warmup_final_learning_rate": LR,
         "criterion": {"name": "CrossEntropyLoss", "params": {}},
         "optimizer": {"name": name, "params": {"lr": LR, "weight_decay": WD} if params is None else params},
         "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}}, "fused_step": True}
    t.update(training)
    return {"training": t, "eval": {}, "data": {"img_size": 32},
            "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 64, "num_blocks": 2, "num_heads": 2, "mlp_dim": 128, "dropout": 0.0,
                      "num_classes": 10}}


def _batch(seed=6, n=4):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (n,), generator=g).to(DEV)


def trainable(store):
    return [n for n, p in zip(store.names, store.params) if p.requires_grad]


class Follower:
    """the restatement in float64 and float32 beside a FusedLamb: same rows, same hyper-parameters, moments of its own"""

    def __init__(self, store, opt):
        self.store, self.opt, self.names = store, opt, trainable(store)
        g = opt.param_groups[0]
        scale = opt.lr_scale or (lambda n: 1.0)
        decay = opt.weight_decay_of or (lambda n: g["weight_decay"])
        rows = [(scale(n), decay(n)) for n in self.names]
        zeros = [torch.zeros(store.offsets[n][1]) for n in self.names]
        # the betas as the C ABI receives them (float): 1 - 0.999f is 1.3e-5 (relative) away from 0.001, which cancels between v and
        # its bias correction only while both grew from zero under the same beta2 -- not when moments are loaded from a checkpoint
        betas = tuple(float(torch.tensor(b, dtype=torch.float32)) for b in g["betas"])
        kw = dict(lr=g["lr"], betas=betas, eps=g["eps"], always_adapt=g["always_adapt"], trust_clip=g["trust_clip"])
        self.refs = {dt: R.LambRef(zeros, rows, dt, **kw) for dt in (torch.float64, torch.float32)}
        self.rows = rows

    def slices(self, flat):
        flat = flat.detach().cpu()
        return [flat[o:o + n].clone() for o, n in (self.store.offsets[name] for name in self.names)]

    def check(self, do_step, what, gscale=1.0):
        """one fused step; the restatement applied to its gradient reproduces the new parameters and the trust ratios"""
        before = self.slices(self.store.flat)
        do_step(self.opt)
        torch.cuda.synchronize()
        grads, after = self.slices(self.store.gflat), self.slices(self.store.flat)
        out = {}
        for dt, ref in self.refs.items():
            ref.p = [x.to(dt) for x in before]
            coef, norm = R.clip_coef(grads, gscale, self.opt.max_grad_norm, dt)
            out[dt] = (ref.step(grads, gscale, coef), norm)
        p64, p32 = self.refs[torch.float64].p, self.refs[torch.float32].p
        bar = max(4.0 * max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64)), R.BAR_FLOOR)
        err = max(float((a.double() - b).abs().max()) for a, b in zip(after, p64))
        moved = max(float((a - b).abs().max()) for a, b in zip(after, before))
        trust64, norm64 = out[torch.float64]
        got = self.opt.trust_ratios()
        assert list(got) == self.names
        rel = max(abs(got[n] - t) / t for n, t in zip(self.names, trust64))
        print(f"{what}: max abs error {err:.3e} (bar {bar:.3e}), moved {moved:.3e}, trust error {rel:.3e}, "
              f"ratios {min(trust64):.4g} .. {max(trust64):.4g}, norm {norm64}")
        assert moved > 100 * bar, f"{what}: the step moved nothing"
        assert err < bar, f"{what}: parameters {err:.3e} from the float64 restatement, bar {bar:.3e}"
        assert rel < bar, f"{what}: trust ratios {rel:.3e} (relative) from the float64 restatement, bar {bar:.3e}"
        if norm64 is not None:
            assert abs(float(self.opt.grad_norm) - norm64) <= 2e-6 * norm64
        return trust64


# ---- the fused ViT step -----------------------------------------------------------------------------------------------------------
def test_vit_fused_step_with_every_key():
    from utils.model_builder import build_model
    from utils.train_utils import make_optimizer
    from vitssl_hip.optim import FusedLamb
    torch.manual_seed(5)
    cfg = _cfg(no_weight_decay=True, layer_decay=DECAY, clip_grad_norm=1.0)
    model = build_model(cfg).to(DEV).train()
    opt = make_optimizer(cfg, model)
    assert type(opt) is FusedLamb and opt.max_grad_norm == 1.0 and opt.lr_scale is not None and opt.weight_decay_of is not None
    x, y = _batch()
    follow = Follower(model.flat_store(), opt)
    assert {w for _, w in follow.rows} == {0.0, WD} and len({s for s, _ in follow.rows}) == 4
    for k in range(3):
        trust = follow.check(lambda o: model.train_step(x, y, o), f"vit step {k + 1}")
        assert all(t == 1.0 for t, (_, w) in zip(trust, follow.rows) if w == 0.0)
        assert all(t != 1.0 for t, (_, w) in zip(trust, follow.rows) if w != 0.0)
    assert opt.step_count == 3


# ---- the other models -------------------------------------------------------------------------------------------------------------
def test_simmim_fused_step():
    from vit_core.ssl.simmim.model import SimMIMViT
    from vitssl_hip.optim import FusedLamb
    torch.manual_seed(3)
    model = SimMIMViT(**VIT).to(DEV).train()
    x = _batch(1)[0]
    mask = torch.zeros(4, 16, dtype=torch.bool)
    mask[:, ::2] = True
    opt = FusedLamb(model.flat_store(), lr=LR, weight_decay=WD)
    Follower(model.flat_store(), opt).check(lambda o: model.train_step(x, o, mask_cpu=mask), "simmim")


def test_dino_fused_step_leaves_the_teacher_alone():
    from vit_core.ssl.dino import DINOViT
    from vit_core.ssl.dino.loss import DINOLoss
    from vitssl_hip.optim import FusedLamb
    torch.manual_seed(4)
    model = DINOViT(output_dim=128, center_momentum=0.9, **VIT).to(DEV).train()
    g = torch.Generator().manual_seed(2)
    views = [torch.rand(2, 3, 32, 32, generator=g).to(DEV) for _ in range(2)] + [torch.rand(2, 3, 16, 16, generator=g).to(DEV) for _ in range(2)]
    crit = DINOLoss(0.04, 0.1)
    store = model.trainable_store()
    opt = FusedLamb(store, lr=LR, weight_decay=WD, always_adapt=True)
    others = [s for s in model.all_stores() if s is not store]
    assert others and all(n.startswith("student_") for n in store.names)
    teacher = [s.flat.detach().clone() for s in others]
    # momentum 1: the EMA leaves the teacher what it is, so any change would be the optimizer's
    Follower(store, opt).check(lambda o: model.train_step(views, 2, crit, o, None, teacher_momentum=1.0), "dino")
    for s, t in zip(others, teacher):
        assert torch.equal(s.flat.view(torch.int32), t.view(torch.int32)), "the optimizer touched the teacher"


# ---- frozen backbone, make_optimizer and _is_fused through the trainer ----------------------------------------------------------------
def test_frozen_backbone_through_the_trainer(tmp_path):
    from utils.model_builder import build_model, freeze_backbone
    from utils.trainers import SupervisedTrainer
    from vitssl_hip.optim import FusedLamb
    torch.manual_seed(5)
    cfg = _cfg(freeze_backbone=True, freeze_backbone_epochs=2, no_weight_decay=True)
    model = build_model(cfg).to(DEV).train()
    freeze_backbone(model)
    x, y = _batch(n=8)
    data = [(x.cpu(), y.cpu())]
    tr = SupervisedTrainer(model, str(tmp_path / "t"), cfg, data, data, DEV)
    opt = tr.optimizer
    assert type(opt) is FusedLamb and tr._is_fused()
    store = model.flat_store()
    names = trainable(store)
    frozen = [n for n in store.names if n not in names]
    assert frozen and names and all(n.startswith("classification_head") or n.endswith("cls_token") for n in names)
    frozen_bits = {n: store.view(n).detach().cpu().view(torch.int32).clone() for n in frozen}
    follow = Follower(store, opt)
    for k in range(2):
        follow.check(lambda o: model.train_step(x, y, o), f"vit, frozen backbone, step {k + 1}")
        assert sorted(opt.trust_ratios()) == sorted(names)
        for n in frozen:
            o, cnt = store.offsets[n]
            assert torch.equal(store.view(n).detach().cpu().view(torch.int32), frozen_bits[n]), f"frozen {n} changed"
            assert not opt.exp_avg[o:o + cnt].any() and not opt.exp_avg_sq[o:o + cnt].any(), f"frozen {n} has moments"


@pytest.mark.parametrize("name", ["Lamb", "LAMB", "lamb"])
def test_make_optimizer_and_is_fused(tmp_path, name):
    from utils.model_builder import build_model
    from utils.trainers import SupervisedTrainer
    from vitssl_hip.optim import FusedLamb
    cfg = _cfg(name, {"lr": LR, "betas": (0.9, 0.99), "eps": 1e-7, "weight_decay": WD, "always_adapt": True, "trust_clip": True})
    model = build_model(cfg).to(DEV).train()
    x, y = _batch()
    data = [(x.cpu(), y.cpu())]
    tr = SupervisedTrainer(model, str(tmp_path / "t"), cfg, data, data, DEV)
    g = tr.optimizer.param_groups[0]
    assert type(tr.optimizer) is FusedLamb and tr._is_fused()
    assert g["betas"] == (0.9, 0.99) and g["eps"] == 1e-7 and g["always_adapt"] is True and g["trust_clip"] is True
    assert len(tr.optimizer.param_groups) == 1 and tr.optimizer.grad_norm is None


def test_refused_configs():
    from utils.model_builder import build_model
    from utils.train_utils import make_optimizer
    model = build_model(_cfg()).to(DEV)
    with pytest.raises(ValueError, match="amsgrad"):
        make_optimizer(_cfg(params={"lr": LR, "amsgrad": True}), model)
    with pytest.raises(ValueError, match="flat_store"):
        make_optimizer(_cfg(), torch.nn.Linear(2, 2))


# ---- checkpointing ----------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_gives_the_same_next_step():
    from vit_core.vit import ViT
    from vitssl_hip.optim import FusedLamb
    torch.manual_seed(7)
    a = ViT(num_classes=10, **VIT).to(DEV).train()
    b = copy.deepcopy(a)
    x, y = _batch()
    kw = dict(lr=LR, weight_decay=WD, max_grad_norm=0.5, trust_clip=True)
    oa = FusedLamb(a.flat_store(), **kw)
    for _ in range(2):
        a.train_step(x, y, oa)
    sd = oa.state_dict()
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 2.0 for s in sd["state"].values())
    ob = FusedLamb(b.flat_store(), lr=1.0, weight_decay=0.0)                    # every group value comes from the checkpoint
    ob.load_state_dict(sd)
    assert ob.step_count == 2 and ob.max_grad_norm == 0.5 and ob.param_groups[0]["trust_clip"] is True and ob.param_groups[0]["lr"] == LR
    with torch.no_grad():
        b.flat_store().flat.copy_(a.flat_store().flat)
    b.flat_store().mark_dirty()
    a.train_step(x, y, oa)
    b.train_step(x, y, ob)
    torch.cuda.synchronize()
    bits = lambda t: t.detach().view(torch.int32)          # noqa: E731
    assert torch.equal(bits(a.flat_store().flat), bits(b.flat_store().flat)), "the step after the round trip differs"
    assert torch.equal(bits(oa.exp_avg), bits(ob.exp_avg)) and torch.equal(bits(oa.exp_avg_sq), bits(ob.exp_avg_sq))
    assert oa.trust_ratios() == ob.trust_ratios()


def test_a_fused_adamw_state_dict_loads():
    from vit_core.vit import ViT
    from vitssl_hip.optim import FusedAdamW, FusedLamb
    torch.manual_seed(8)
    model = ViT(num_classes=10, **VIT).to(DEV).train()
    x, y = _batch()
    adamw = FusedAdamW(model.flat_store(), lr=LR, weight_decay=WD)
    model.train_step(x, y, adamw)
    lamb = FusedLamb(model.flat_store(), lr=LR, weight_decay=WD)
    lamb.load_state_dict(adamw.state_dict())
    assert lamb.step_count == 1 and torch.equal(lamb.exp_avg, adamw.exp_avg) and torch.equal(lamb.exp_avg_sq, adamw.exp_avg_sq)
    assert lamb.param_groups[0]["always_adapt"] is False and lamb.param_groups[0]["trust_clip"] is False
    follow = Follower(model.flat_store(), lamb)
    for ref in follow.refs.values():                          # the restatement continues from the loaded moments too
        ref.m, ref.v, ref.steps = [t.to(ref.dtype) for t in follow.slices(lamb.exp_avg)], [t.to(ref.dtype) for t in follow.slices(lamb.exp_avg_sq)], 1
    follow.check(lambda o: model.train_step(x, y, o), "vit after AdamW's state")
    assert lamb.step_count == 2
