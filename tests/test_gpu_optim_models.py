"""Fused train steps with FusedAdamW(max_grad_norm, lr_scale, weight_decay_of) on the three models.  A second copy of the
model runs the same fused step up to the gradient (its optimizer is a recorder); torch.optim.AdamW with one group per tensor
plus clip_grad_norm_, in float64 on the CPU, is applied to that gradient; the copy then takes over the first model's
parameters so that both see the same weights in the next step.  The bar is the op test's: 4 x the float32-vs-float64 distance
of the same torch recipe, never below 2e-6."""
import copy

import pytest
import torch

import _optim_cases as K

DEV = torch.device("cuda:0")
pytestmark = pytest.mark.gpu
LR, WD, DECAY = 1e-3, 0.05, 0.65


class Recorder:
    """optimizer stub: keeps the flat gradient the fused step hands to step_flat"""

    def __init__(self, store):
        self.store, self.gflat, self.gscale = store, None, None

    def step_flat(self, gscale=1.0):
        self.gflat, self.gscale = self.store.gflat.detach().cpu().clone(), gscale


class TorchRecipe:
    """torch.optim.AdamW, one param group per trainable tensor of the store, plus clip_grad_norm_, in `dtype` on the CPU"""

    def __init__(self, store, names, lr_scale, weight_decay_of, max_norm, dtype):
        flat = store.flat.detach().cpu()
        self.offsets = {n: store.offsets[n] for n in names}
        self.params = {n: flat[o:o + k].to(dtype).clone().requires_grad_(True) for n, (o, k) in self.offsets.items()}
        self.opt = torch.optim.AdamW([dict(params=[p], lr=LR * lr_scale(n), weight_decay=weight_decay_of(n)) for n, p in self.params.items()],
                                     lr=LR, betas=K.BETAS, eps=K.EPS)
        self.max_norm, self.dtype = max_norm, dtype

    def step(self, gflat, gscale):
        for n, (o, k) in self.offsets.items():
            self.params[n].grad = gflat[o:o + k].to(self.dtype) * gscale
        norm = torch.nn.utils.clip_grad_norm_(list(self.params.values()), self.max_norm)
        self.opt.step()
        return float(norm)

    def distance(self, other):
        return max(float((p.detach().double() - other.params[n].detach().double()).abs().max()) for n, p in self.params.items())


def settings(store):
    from vitssl_hip.engine import exempt_from_weight_decay, layer_id, num_layers
    layers = num_layers(store.names)
    ndim = {n: p.dim() for n, p in zip(store.names, store.params)}
    return (lambda n: DECAY ** (layers + 1 - layer_id(n, layers))), (lambda n: 0.0 if exempt_from_weight_decay(n, ndim[n]) else WD)


def trainable(store):
    return [n for n, p in zip(store.names, store.params) if p.requires_grad]


def run_steps(step_a, step_b, store_a, store_b, opt, rec, steps, what):
    """`steps` fused steps of both copies; returns after checking parameters and grad_norm of each against the float64 recipe"""
    names = trainable(store_a)
    assert names == trainable(store_b)
    max_norm = opt.param_groups[0]["max_grad_norm"]
    ref64 = TorchRecipe(store_a, names, opt.lr_scale, opt.weight_decay_of, max_norm, torch.float64)
    ref32 = TorchRecipe(store_a, names, opt.lr_scale, opt.weight_decay_of, max_norm, torch.float32)
    frozen = [n for n in store_a.names if n not in names]
    frozen_bits = {n: store_a.view(n).detach().cpu().view(torch.int32).clone() for n in frozen}
    clipped = 0
    for k in range(steps):
        step_b(rec)
        step_a(opt)
        norm = ref64.step(rec.gflat, rec.gscale)
        ref32.step(rec.gflat, rec.gscale)
        clipped += norm > max_norm
        bar = max(4.0 * ref32.distance(ref64), K.BAR_FLOOR)
        got = store_a.flat.detach().cpu()
        err = max(float((got[o:o + n].double() - ref64.params[name].detach()).abs().max()) for name, (o, n) in ref64.offsets.items())
        gn = float(opt.grad_norm)
        print(f"{what} step {k + 1}: max abs error {err:.3e} (bar {bar:.3e}), grad_norm {gn:.6e} against {norm:.6e}")
        assert err < bar, f"{what} step {k + 1}: parameters {err:.3e} from the torch float64 recipe, bar {bar:.3e}"
        assert abs(gn - norm) <= 2e-6 * norm, f"{what} step {k + 1}: grad_norm {gn} against clip_grad_norm_'s {norm}"
        for n in frozen:
            o, cnt = store_a.offsets[n]
            assert torch.equal(store_a.view(n).detach().cpu().view(torch.int32), frozen_bits[n]), f"{what}: frozen {n} changed"
            assert not opt.exp_avg[o:o + cnt].any() and not opt.exp_avg_sq[o:o + cnt].any(), f"{what}: frozen {n} has moments"
        with torch.no_grad():
            store_b.flat.copy_(store_a.flat)
        store_b.mark_dirty()
    assert clipped, f"{what}: the clip was never active"


def first_norm(step_b, rec):
    """global norm of the copy's first gradient (the copy's weights do not move: its optimizer is the recorder)"""
    step_b(rec)
    return float(rec.gflat.double().norm()) * rec.gscale


def test_simmim_fused_step():
    from vit_core.ssl.simmim.model import SimMIMViT
    from vitssl_hip.optim import FusedAdamW
    torch.manual_seed(3)
    a = SimMIMViT(num_blocks=2, input_shape=(3, 64, 64), embed_dim=128, patch_size=16, num_heads=2, mlp_dim=256, dropout=0.0).to(DEV).train()
    b = copy.deepcopy(a)
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    mask = torch.zeros(4, 16, dtype=torch.bool)
    mask[:, ::2] = True
    rec = Recorder(b.flat_store())
    step_b = lambda o: b.train_step(x, o, mask_cpu=mask)
    scale, decay = settings(a.flat_store())
    opt = FusedAdamW(a.flat_store(), lr=LR, weight_decay=WD, max_grad_norm=0.5 * first_norm(step_b, rec), lr_scale=scale, weight_decay_of=decay)
    run_steps(lambda o: a.train_step(x, o, mask_cpu=mask), step_b, a.flat_store(), b.flat_store(), opt, rec, 2, "simmim")


def test_dino_fused_step():
    from vit_core.ssl.dino import DINOViT
    from vit_core.ssl.dino.loss import DINOLoss
    from vitssl_hip.optim import FusedAdamW
    torch.manual_seed(4)
    a = DINOViT(num_blocks=2, input_shape=(3, 32, 32), embed_dim=128, patch_size=8, num_heads=2, mlp_dim=256, dropout=0.0, output_dim=256,
                center_momentum=0.9).to(DEV).train()
    b = copy.deepcopy(a)
    g = torch.Generator().manual_seed(2)
    views = [torch.rand(2, 3, 32, 32, generator=g).to(DEV) for _ in range(2)] + [torch.rand(2, 3, 16, 16, generator=g).to(DEV) for _ in range(2)]
    crit = DINOLoss(0.04, 0.1)
    rec = Recorder(b.trainable_store())
    # momentum 1: the teachers of both copies stay what they are, so both see the same targets in every step
    step_b = lambda o: b.train_step(views, 2, crit, o, None, teacher_momentum=1.0)
    scale, decay = settings(a.trainable_store())
    opt = FusedAdamW(a.trainable_store(), lr=LR, weight_decay=WD, max_grad_norm=0.5 * first_norm(step_b, rec), lr_scale=scale, weight_decay_of=decay)
    b.center.copy_(a.center)            # first_norm moved the copy's centre by one step: both start from the same one
    run_steps(lambda o: a.train_step(views, 2, crit, o, None, teacher_momentum=1.0), step_b, a.trainable_store(), b.trainable_store(),
              opt, rec, 2, "dino")


def _vit_cfg():
    t = {"type": "supervised", "num_epochs": 4, "warmup_epochs": 1, "warmup_initial_learning_rate": LR, "warmup_final_learning_rate": LR,
         "criterion": {"name": "CrossEntropyLoss", "params": {}}, "optimizer": {"name": "AdamW", "params": {"lr": LR, "weight_decay": WD}},
         "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}},
         "fused_step": True, "freeze_backbone": True, "freeze_backbone_epochs": 2,
         "clip_grad_norm": 1e-3, "no_weight_decay": True, "layer_decay": DECAY}
    return {"training": t, "eval": {}, "data": {"img_size": 32},
            "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 128, "num_blocks": 2, "num_heads": 2, "mlp_dim": 256, "dropout": 0.0,
                      "num_classes": 10}}


def test_vit_frozen_backbone_then_unfrozen_through_the_trainer(tmp_path):
    from utils.model_builder import build_model, freeze_backbone
    from utils.trainers import SupervisedTrainer
    torch.manual_seed(5)
    cfg = _vit_cfg()
    a = build_model(cfg).to(DEV).train()
    freeze_backbone(a)
    b = copy.deepcopy(a)
    g = torch.Generator().manual_seed(6)
    x, y = torch.rand(8, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (8,), generator=g).to(DEV)
    data = [(x.cpu(), y.cpu())]
    tr = SupervisedTrainer(a, str(tmp_path / "t"), cfg, data, data, DEV)
    opt = tr.optimizer
    assert opt.max_grad_norm == 1e-3 and opt.lr_scale is not None and opt.weight_decay_of is not None
    assert len(trainable(a.flat_store())) < len(a.flat_store().names)
    rec = Recorder(b.flat_store())
    step_a, step_b = (lambda o: a.train_step(x, y, o)), (lambda o: b.train_step(x, y, o))
    run_steps(step_a, step_b, a.flat_store(), b.flat_store(), opt, rec, 2, "vit, frozen backbone")

    tr._maybe_unfreeze(2)                                   # the trainer's rebuild: make_optimizer over the un-frozen model
    new = tr.optimizer
    assert new is not opt and len(new.param_groups[0]["params"]) == len(a.flat_store().names)
    assert new.max_grad_norm == 1e-3 and new.param_groups[0]["max_grad_norm"] == 1e-3
    layers = 2
    assert new.lr_scale("patch_embedding.conv.weight") == DECAY ** (layers + 1) and new.lr_scale("classification_head.linear.bias") == 1.0
    assert new.weight_decay_of("classification_head.linear.bias") == 0.0 and new.weight_decay_of("classification_head.linear.weight") == WD
    assert not new.exp_avg.any() and new.step_count == 0     # fresh moments
    for p in b.parameters():
        p.requires_grad = True
    run_steps(step_a, step_b, a.flat_store(), b.flat_store(), new, rec, 2, "vit, un-frozen")
