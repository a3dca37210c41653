"""Host side of the fused LAMB: the CPU restatement of include/vitssl_lamb.h (tests/_lamb_ref.py) anchored to torch.optim.AdamW
and to a hand-computed step, its edge rules, the proof that the bar of the GPU tests tells LAMB from three wrong optimizers,
and the config plumbing of make_optimizer.  No kernel runs."""
import math

import pytest
import torch

import _lamb_ref as R

CPU = torch.device("cpu")
BACKBONE = dict(num_blocks=2, input_shape=(3, 32, 32), embed_dim=64, patch_size=16, num_heads=2, mlp_dim=128)


@pytest.fixture(scope="module")
def common():
    lay = R.Layout()
    params, grads = R.make_case(lay)
    return lay, params, grads


# ---- (i) anchor to torch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_without_decay_it_is_torch_adamw(common, gscale):
    """every wd == 0 and no always_adapt: the trust ratio is 1 and the denominators have torch's form"""
    lay, params, grads = common
    rows = [(s, 0.0) for s, _ in R.rows_of(lay)]
    got = R.run(params, grads, rows, torch.float64, gscale=gscale)
    ps = [p.double().clone().requires_grad_(True) for p in params]
    opt = torch.optim.AdamW([dict(params=[p], lr=R.LR * s) for p, (s, _) in zip(ps, rows)], lr=R.LR, betas=R.BETAS, eps=R.EPS, weight_decay=0.0)
    clipped = 0
    for k, g in enumerate(grads):
        for p, x in zip(ps, g):
            p.grad = x.double() * gscale
        norm = float(torch.nn.utils.clip_grad_norm_(ps, R.MAX_NORM))
        clipped += norm > R.MAX_NORM
        opt.step()
        assert got[k][3] == [1.0] * len(ps)
        assert abs(got[k][4] - norm) <= 1e-12 * norm
        for what, mine, theirs in (("p", got[k][0], [p.detach() for p in ps]), ("m", got[k][1], [opt.state[p]["exp_avg"] for p in ps]),
                                   ("v", got[k][2], [opt.state[p]["exp_avg_sq"] for p in ps])):
            for a, b in zip(mine, theirs):
                # relative to the tensor's magnitude: torch forms m as lerp(m, g, 1 - b1), and where 0.9 m and 0.1 g cancel,
                # two correct roundings differ by more than 1e-12 of the ELEMENT
                assert float((a - b).abs().max()) < 1e-12 * float(b.abs().max()), f"step {k + 1}: {what}"
    assert 0 < clipped < len(grads), "the case alternates an idle and an active clip"


# ---- (ii) one step by hand --------------------------------------------------------------------------------------------------------
def test_hand_computed_step():
    """p = (3, 4), g = (1, -1), step 1: m^ = g and sqrt(v^) = |g|, so the Adam part is +-a with a = 1 / (1 + eps);
    wd = 0.1 adds (0.3, 0.4): r = (a + 0.3, 0.4 - a), |p| = 5, trust = 5 / |r| ~ 5 / sqrt(1.69 + 0.36) ~ 3.4921"""
    lr, scale, wd, eps = 0.01, 0.5, 0.1, 1e-6
    ref = R.LambRef([torch.tensor([3.0, 4.0])], [(scale, wd)], torch.float64, lr=lr, betas=(0.9, 0.999), eps=eps)
    trust = ref.step([torch.tensor([1.0, -1.0])])
    a = 1.0 / (1.0 + eps)
    r = (a + 0.3, 0.4 - a)
    want = 5.0 / math.hypot(*r)
    assert abs(want - 3.4921) < 1e-3 and want > 1.0
    assert abs(trust[0] - want) < 1e-12
    for i, p0 in enumerate((3.0, 4.0)):
        assert abs(float(ref.p[0][i]) - (p0 - lr * scale * want * r[i])) < 1e-12
    assert abs(float(ref.m[0][0]) - 0.1) < 1e-15 and abs(float(ref.v[0][1]) - 0.001) < 1e-15
    # the Adam part alone would have stepped by lr * scale * a: the trust ratio and the decay term both show
    assert abs((3.0 - float(ref.p[0][0])) - lr * scale * a) > 1e-2


# ---- (iii) edge rules -------------------------------------------------------------------------------------------------------------
def test_zero_parameter_with_decay_gets_trust_one():
    ref = R.LambRef([torch.zeros(5)], [(1.0, 0.1)], torch.float64)
    assert ref.step([torch.ones(5)]) == [1.0]
    assert bool((ref.p[0] != 0).all())


def test_zero_update_gets_trust_one():
    ref = R.LambRef([torch.zeros(5), torch.ones(3)], [(1.0, 0.1), (1.0, 0.1)], torch.float64)
    trust = ref.step([torch.zeros(5), torch.ones(3)])
    assert trust[0] == 1.0 and trust[1] != 1.0
    assert not ref.p[0].any()
    # a nonzero parameter whose update vanishes: wd * p cancels the Adam part exactly
    ref = R.LambRef([torch.full((4,), -1.0)], [(1.0, 1.0)], torch.float64, eps=0.0)
    assert ref.step([torch.full((4,), 2.0)]) == [1.0]
    assert torch.equal(ref.p[0], torch.full((4,), -1.0, dtype=torch.float64))


def test_trust_clip_caps_at_one():
    big, grad = [torch.full((8,), 10.0)], [torch.ones(8)]
    free = R.LambRef(big, [(1.0, 0.01)], torch.float64).step(grad)
    capped = R.LambRef(big, [(1.0, 0.01)], torch.float64, trust_clip=True).step(grad)
    assert free[0] > 1.0 and capped == [1.0]
    small = [torch.full((8,), 0.01)]
    assert R.LambRef(small, [(1.0, 0.01)], torch.float64, trust_clip=True).step(grad)[0] < 1.0


def test_always_adapt_adapts_tensors_without_decay():
    p, grad = [torch.full((8,), 10.0)], [torch.ones(8)]
    assert R.LambRef(p, [(1.0, 0.0)], torch.float64).step(grad) == [1.0]
    t = R.LambRef(p, [(1.0, 0.0)], torch.float64, always_adapt=True).step(grad)[0]
    assert abs(t - 10.0 * (1.0 + R.EPS)) < 1e-9


# ---- (iv) the bar discriminates ---------------------------------------------------------------------------------------------------
def test_the_bar_tells_lamb_from_wrong_optimizers(common):
    lay, params, grads = common
    rows = R.rows_of(lay)
    run64 = R.run(params, grads, rows, torch.float64)
    bar, dist = R.bar_from(R.run(params, grads, rows, torch.float32), run64)
    print(f"float32-vs-float64 distance of the restatement {dist:.3e}, bar {bar:.3e}")
    assert any(w != 0.0 for _, w in rows) and any(w == 0.0 for _, w in rows)
    for variant in R.VARIANTS[1:]:
        wrong = R.distance(R.run(params, grads, rows, torch.float64, variant=variant), run64)
        print(f"{variant}: {wrong:.3e} from LAMB")
        assert wrong > bar, f"{variant} is {wrong:.3e} from LAMB, inside the bar {bar:.3e}"


# ---- config plumbing --------------------------------------------------------------------------------------------------------------
class _WithStore:
    """what make_optimizer needs of a model, with the store on the CPU"""

    def __init__(self, module):
        from vitssl_hip.engine import FlatStore
        self.module, self.store = module, FlatStore(module, CPU)

    def flat_store(self):
        return self.store

    def parameters(self):
        return self.module.parameters()


def _cfg(name="Lamb", params=None, **training):
    t = {"optimizer": {"name": name, "params": {"lr": 2e-3, "weight_decay": 0.05} if params is None else params}}
    t.update(training)
    return {"training": t}


def _vit():
    from vit_core.vit import ViT
    return ViT(num_classes=5, **BACKBONE)


@pytest.mark.parametrize("name", ["Lamb", "LAMB", "lamb"])
def test_make_optimizer_returns_fused_lamb(name):
    from utils.train_utils import make_optimizer
    from vitssl_hip.optim import FusedAdamW, FusedLamb, FusedOptimizer
    opt = make_optimizer(_cfg(name), _WithStore(_vit()))
    assert type(opt) is FusedLamb and isinstance(opt, FusedOptimizer) and not isinstance(opt, FusedAdamW)
    g = opt.param_groups[0]
    assert len(opt.param_groups) == 1 and g["lr"] == 2e-3 and g["weight_decay"] == 0.05 and g["eps"] == 1e-6
    assert g["always_adapt"] is False and g["trust_clip"] is False
    assert opt.max_grad_norm is None and opt.grad_norm is None and opt.trust_ratios() == {}


def test_group_options_compose_with_lamb():
    from utils.train_utils import make_optimizer
    params = {"lr": 1e-3, "betas": (0.9, 0.99), "eps": 1e-7, "weight_decay": 0.02, "always_adapt": True, "trust_clip": True}
    opt = make_optimizer(_cfg(params=params, clip_grad_norm=2.0, no_weight_decay=True, layer_decay=0.75), _WithStore(_vit()))
    g = opt.param_groups[0]
    assert g["always_adapt"] is True and g["trust_clip"] is True and g["betas"] == (0.9, 0.99) and g["eps"] == 1e-7
    assert opt.max_grad_norm == 2.0 and g["max_grad_norm"] == 2.0
    assert opt.weight_decay_of("classification_head.linear.bias") == 0.0 and opt.weight_decay_of("classification_head.linear.weight") == 0.02
    assert opt.lr_scale("patch_embedding.conv.weight") == 0.75 ** (BACKBONE["num_blocks"] + 1)


def test_refused_lamb_configs():
    from utils.train_utils import make_optimizer
    with pytest.raises(ValueError, match="amsgrad"):
        make_optimizer(_cfg(params={"lr": 1e-3, "amsgrad": True}), _WithStore(_vit()))
    with pytest.raises(ValueError, match="flat_store"):
        make_optimizer(_cfg(), torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="max_grad_norm"):
        make_optimizer(_cfg(params={"lr": 1e-3, "max_grad_norm": 1.0}), _WithStore(_vit()))      # the clip is training.clip_grad_norm


def test_group_keys_error_names_both_fused_optimizers():
    from utils.train_utils import make_optimizer
    with pytest.raises(ValueError, match="fused AdamW or the fused LAMB"):
        make_optimizer(_cfg("SGD", {"lr": 1e-2}, clip_grad_norm=1.0), _WithStore(_vit()))


def test_is_fused_accepts_both_classes():
    from utils.train_utils import make_optimizer
    from utils.trainers.base_trainer import BaseTrainer

    class Model(_WithStore):
        def train_step(self, *a, **k):
            raise AssertionError("not called")

    class Trainer(BaseTrainer):
        train_epoch = validate = None

    tr = Trainer.__new__(Trainer)
    tr.model = Model(_vit())
    for name in ("Lamb", "AdamW"):
        tr.optimizer = make_optimizer(_cfg(name), tr.model)
        assert tr._is_fused(), name
    tr.optimizer = torch.optim.SGD(tr.model.parameters(), lr=0.1)
    assert not tr._is_fused()


def test_state_dict_round_trip_and_adamw_state_loads():
    from utils.train_utils import make_optimizer
    a = make_optimizer(_cfg(clip_grad_norm=5.0, params={"lr": 1e-3, "always_adapt": True}), _WithStore(_vit()))
    adamw = make_optimizer(_cfg("AdamW"), _WithStore(_vit()))
    a.exp_avg.uniform_(-1, 1)
    a.exp_avg_sq.uniform_(0, 1)
    a.step_count = 7
    sd, sd_adamw = a.state_dict(), adamw.state_dict()
    assert set(sd["state"]) == set(sd_adamw["state"]) and all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    assert set(sd["param_groups"][0]) == set(sd_adamw["param_groups"][0]) | {"max_grad_norm", "always_adapt", "trust_clip"}
    b = make_optimizer(_cfg(), _WithStore(_vit()))
    b.load_state_dict(sd)
    assert b.step_count == 7 and b.max_grad_norm == 5.0 and b.param_groups[0]["always_adapt"] is True
    mask = torch.zeros(a.store.numel, dtype=torch.bool)
    for o, n in a.store.offsets.values():
        mask[o:o + n] = True
    assert torch.equal(a.exp_avg[mask], b.exp_avg[mask]) and torch.equal(a.exp_avg_sq[mask], b.exp_avg_sq[mask])
    adamw.exp_avg.uniform_(-1, 1)
    adamw.step_count = 3
    c = make_optimizer(_cfg(), _WithStore(_vit()))
    c.load_state_dict(adamw.state_dict())
    assert c.step_count == 3 and torch.equal(c.exp_avg[mask], adamw.exp_avg[mask])
    assert c.param_groups[0]["always_adapt"] is False and c.param_groups[0]["eps"] == 1e-8       # the group's values follow the checkpoint


def test_header_symbols_are_the_bound_prototypes():
    from vitssl_hip import _lib
    assert set(_lib.header_symbols("lamb")) == set(_lib.REGISTRY["lamb"]) == {"vitssl_lamb_workspace_bytes", "vitssl_lamb_segments"}
    assert _lib.LAMB_ALWAYS_ADAPT == 1 and _lib.LAMB_TRUST_CLIP == 2
