"""Host side of the per-parameter optimizer settings: the layer-id and no-weight-decay rules over the real parameter names of
the three models, the three config keys of make_optimizer, and FusedAdamW's state_dict with them set.  No kernel runs: the
stores are built on the CPU."""
import ctypes

import pytest
import torch

CPU = torch.device("cpu")
BACKBONE = dict(num_blocks=3, input_shape=(3, 32, 32), embed_dim=64, patch_size=16, num_heads=2, mlp_dim=128)


def _models():
    from vit_core.ssl.dino import DINOViT
    from vit_core.ssl.simmim.model import SimMIMViT
    from vit_core.vit import ViT
    return {"simmim": SimMIMViT(**BACKBONE), "vit": ViT(num_classes=5, **BACKBONE), "dino": DINOViT(output_dim=64, **BACKBONE)}


class _WithStore:
    """what make_optimizer needs of a model, with the store on the CPU"""

    def __init__(self, module, only=None):
        from vitssl_hip.engine import FlatStore
        self.module, self.store = module, FlatStore(module, CPU, only=only)

    def flat_store(self):
        return self.store

    def parameters(self):
        return self.module.parameters()


def _cfg(optimizer=None, **training):
    t = {"optimizer": optimizer or {"name": "AdamW", "params": {"lr": 1e-3, "weight_decay": 0.05}}}
    t.update(training)
    return {"training": t}


def _expected_layer(name, layers):
    """the issue's rule, restated on the literal names of the three models"""
    parts = name.split(".")
    if "encoder_blocks" in parts:
        return int(parts[parts.index("encoder_blocks") + 1]) + 1
    if name in ("mask_token", "positional_embedding", "projection.weight", "projection.bias"):           # SimMIMViT
        return 0
    if parts[0] == "patch_embedding" or parts[:2] == ["student_backbone", "patch_embedding"]:             # ViT, DINOViT (student)
        return 0
    assert parts[0] in ("simmim_head", "classification_head", "student_head"), name
    return layers + 1


def test_layer_id_of_every_parameter_name():
    from vitssl_hip.engine import layer_id, num_layers
    for kind, model in _models().items():
        names = [n for n, _ in model.named_parameters() if not n.startswith("teacher_")]
        L = num_layers(names)
        assert L == BACKBONE["num_blocks"], kind
        seen = set()
        for n in names:
            assert layer_id(n, L) == _expected_layer(n, L), (kind, n)
            seen.add(layer_id(n, L))
        assert seen == set(range(L + 2)), kind


def test_no_weight_decay_true_is_the_rule():
    from utils.train_utils import make_optimizer
    for kind, model in _models().items():
        wrapped = _WithStore(model, only=(lambda n: n.startswith("student_")) if kind == "dino" else None)
        opt = make_optimizer(_cfg(no_weight_decay=True), wrapped)
        assert opt.max_grad_norm is None and opt.lr_scale is None
        for n, p in zip(wrapped.store.names, wrapped.store.params):
            exempt = p.dim() <= 1 or n.endswith(("cls_token", "positional_embedding", "mask_token"))
            assert opt.weight_decay_of(n) == (0.0 if exempt else 0.05), (kind, n)
        decayed = [n for n in wrapped.store.names if opt.weight_decay_of(n) != 0.0]
        assert decayed and all(p.dim() >= 2 for n, p in zip(wrapped.store.names, wrapped.store.params) if n in decayed), kind


def test_no_weight_decay_patterns_and_layer_decay():
    from utils.train_utils import make_optimizer
    wrapped = _WithStore(_models()["vit"])
    opt = make_optimizer(_cfg(no_weight_decay=["*.bias", "patch_embedding.*"], layer_decay=0.75, clip_grad_norm=3.0), wrapped)
    assert opt.weight_decay_of("encoder_blocks.0.feed_forward.linear_in.bias") == 0.0
    assert opt.weight_decay_of("patch_embedding.conv.weight") == 0.0
    assert opt.weight_decay_of("encoder_blocks.0.layer_norm1.weight") == 0.05          # not matched: the list is all there is
    assert opt.max_grad_norm == 3.0 and opt.param_groups[0]["max_grad_norm"] == 3.0
    L = BACKBONE["num_blocks"]
    assert opt.lr_scale("patch_embedding.cls_token") == 0.75 ** (L + 1)
    assert opt.lr_scale("encoder_blocks.1.layer_norm1.bias") == 0.75 ** (L + 1 - 2)
    assert opt.lr_scale("classification_head.linear.weight") == 1.0
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 1e-3


def test_absent_keys_change_nothing():
    from utils.train_utils import make_optimizer
    from vitssl_hip.optim import FusedAdamW
    for cfg in (_cfg(), _cfg(no_weight_decay=False, clip_grad_norm=None)):
        opt = make_optimizer(cfg, _WithStore(_models()["simmim"]))
        assert type(opt) is FusedAdamW
        assert opt.max_grad_norm is None and opt.lr_scale is None and opt.weight_decay_of is None and opt.grad_norm is None
        assert set(opt.param_groups[0]) - {"params"} == {"lr", "betas", "eps", "weight_decay"}


@pytest.mark.parametrize("key,value", [("clip_grad_norm", 1.0), ("no_weight_decay", True), ("layer_decay", 0.75)])
def test_keys_without_the_fused_optimizer_raise(key, value):
    from utils.train_utils import make_optimizer
    wrapped = _WithStore(_models()["simmim"])
    for optimizer in ({"name": "SGD", "params": {"lr": 1e-2}}, {"name": "AdamW", "params": {"lr": 1e-3, "amsgrad": True}}):
        with pytest.raises(ValueError, match=f"training.{key}"):
            make_optimizer(_cfg(optimizer, **{key: value}), wrapped)
    with pytest.raises(ValueError, match=f"training.{key}"):
        make_optimizer(_cfg(**{key: value}), torch.nn.Linear(2, 2))              # no flat store


@pytest.mark.parametrize("key,value", [("clip_grad_norm", 0.0), ("clip_grad_norm", -1.0), ("layer_decay", 0.0), ("layer_decay", 1.5),
                                       ("no_weight_decay", "*.bias")])
def test_bad_values_raise(key, value):
    from utils.train_utils import make_optimizer
    with pytest.raises(ValueError, match=key):
        make_optimizer(_cfg(**{key: value}), _WithStore(_models()["simmim"]))


def test_state_dict_round_trip_with_the_keys_set():
    from utils.train_utils import make_optimizer
    cfg = _cfg(no_weight_decay=True, layer_decay=0.65, clip_grad_norm=5.0)
    a = make_optimizer(cfg, _WithStore(_models()["simmim"]))
    plain = make_optimizer(_cfg(), _WithStore(_models()["simmim"]))
    a.exp_avg.uniform_(-1, 1)
    a.exp_avg_sq.uniform_(0, 1)
    a.step_count = 7
    a.param_groups[0]["lr"] = 3e-4
    sd = a.state_dict()
    sd_plain = plain.state_dict()
    assert set(sd) == set(sd_plain) and set(sd["state"]) == set(sd_plain["state"])          # the layout is what it was
    assert set(sd["param_groups"][0]) == set(sd_plain["param_groups"][0]) | {"max_grad_norm"}
    assert sd["param_groups"][0]["max_grad_norm"] == 5.0 and len(sd["param_groups"]) == 1
    b = make_optimizer(cfg, _WithStore(_models()["simmim"]))
    b.load_state_dict(sd)
    assert b.step_count == 7 and b.param_groups[0]["lr"] == 3e-4 and b.param_groups[0]["max_grad_norm"] == 5.0
    mask = torch.zeros(a.store.numel, dtype=torch.bool)
    for o, n in a.store.offsets.values():
        mask[o:o + n] = True
    assert torch.equal(a.exp_avg[mask], b.exp_avg[mask]) and torch.equal(a.exp_avg_sq[mask], b.exp_avg_sq[mask])
    assert b.lr_scale("projection.weight") == 0.65 ** 4 and b.weight_decay_of("projection.bias") == 0.0


def test_header_symbols_are_the_bound_prototypes():
    from vitssl_hip import _lib
    sizing = {"vitssl_optim_table_bytes", "vitssl_grad_sumsq_workspace_bytes"}
    status = {n for n, (r, a) in _lib.REGISTRY["optim"].items() if r is ctypes.c_int}
    assert set(_lib.header_symbols("optim")) == set(_lib.REGISTRY["optim"]) == status | sizing and not status & sizing
    l = _lib.lib()
    for name in sizing:
        assert getattr(l, name).restype is not None and getattr(l, name)(0) == 0 and getattr(l, name)(3) > 0


def test_a_loaded_group_switches_the_clip_on():
    """max_grad_norm lives in the group dict: a checkpoint that carries it turns the clip on in an optimizer built without the key"""
    from utils.train_utils import make_optimizer
    clipped = make_optimizer(_cfg(clip_grad_norm=2.0), _WithStore(_models()["simmim"]))
    plain = make_optimizer(_cfg(), _WithStore(_models()["simmim"]))
    assert not plain._segmented and clipped._segmented
    plain.load_state_dict(clipped.state_dict())
    assert plain.max_grad_norm == 2.0 and plain._segmented
