"""MAEViT on the GPU against tests/_mae_ref.py (the oracle's pieces with emu="bf16": the rounding points of the HIP path), with
tiny models.  Case a: 24 x 24 images, patch 8 (N = 9, K = 2), encoder head dim 64 and decoder head dim 32, so both attention
families run; B = 5.  Case b: 28 x 28, patch 14 (N = 4, K = 1): the padded patch geometry; B = 3.

Bars as tests/test_gpu_models.py: raw-pixel targets bit-equal, pred rel-L2 < 1e-2, loss within 1e-2 relative, every parameter
gradient by the rule of test_edge_batches_against_oracle (nearer of the oracle's two attention-backward forms < 2e-2, both
< 5e-2).  The fused step leaves in the flat gradient buffer what the autograd path leaves in .grad for the same d(loss)/d(pred)
(rel-L2 < 1e-6), and one fused AdamW step equals oracle.adamw_step on those gradients.  Two ranks: tests/test_gpu_mae_ddp.py."""
import contextlib
import functools

import pytest
import torch

import _mae_ref as Ref
from _util import max_abs, rel_l2
from oracle import vit_oracle as O
from vit_core.ssl.mae import masking as Mk

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
COMMON = dict(num_blocks=2, embed_dim=64, num_heads=1, mlp_dim=128, decoder_embed_dim=64, decoder_blocks=1, decoder_heads=2, mask_ratio=0.75)
CASES = {"a": (dict(input_shape=(3, 24, 24), patch_size=8, **COMMON), 5, 9, 2), "b": (dict(input_shape=(3, 28, 28), patch_size=14, **COMMON), 3, 4, 1)}
GRID = [(c, n) for c in CASES for n in (True, False)]


def build(case, norm_pix):
    """-> (model on the GPU in train mode, its initial state dict on the CPU, x, keep, restore); the same for every caller"""
    from vit_core.ssl.mae import MAEViT
    ctor, B, N, K = CASES[case]
    torch.manual_seed(17 + B)
    model = MAEViT(**ctor, norm_pix_loss=norm_pix)
    with torch.no_grad():                                     # norms and biases away from their 1 / 0 initial values
        for k, p in model.named_parameters():
            if "norm" in k or k.endswith(".bias"):
                p.add_(0.1 * torch.randn_like(p))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = torch.rand(B, *ctor["input_shape"])
    keep, restore = Mk.draw_keep(B, N, K, generator=torch.Generator().manual_seed(5))
    assert model.num_kept == K and model.num_patches == N
    return model.to(DEV).train(), sd, x, keep, restore


@functools.lru_cache(maxsize=None)
def reference(case, norm_pix):
    """The restatement's forward, loss and gradients, computed once per case: {mode: (pred, raw targets, loss, grads)} for the
    oracle's two attention-backward forms and the fp32 oracle."""
    ctor, B, N, K = CASES[case]
    _, sd, x, keep, restore = build(case, norm_pix)
    out = {}
    for mode in ("autograd", "flash", "fp32"):
        leaves = {k: v.clone().requires_grad_(v.is_floating_point() and "pos_embed" not in k) for k, v in sd.items()}
        with (O.flash_delta() if mode == "flash" else contextlib.nullcontext()):
            pe, te = Ref.forward(leaves, x, keep, restore, ctor["patch_size"], ctor["num_heads"], ctor["decoder_heads"],
                                 emu=None if mode == "fp32" else "bf16")
            t = Ref.normalise(te.double()).float() if norm_pix else te
            loss = ((pe - t) ** 2).mean()
            loss.backward()
        out[mode] = (pe.detach(), te, float(Ref.loss64(pe.detach(), te, norm_pix)[0]), {k: v.grad for k, v in leaves.items() if v.requires_grad})
    return out


@pytest.mark.parametrize("case,norm_pix", GRID, ids=str)
def test_forward_loss_and_gradients_against_the_restatement(case, norm_pix):
    ctor, B, N, K = CASES[case]
    model, sd, x, keep, restore = build(case, norm_pix)
    ref = reference(case, norm_pix)
    pred, tgt, mask = model(x.to(DEV), return_bool_mask=True, keep_cpu=keep)
    pe, te, loss_e, _ = ref["autograd"]
    assert mask.shape == (B, N, 1) and mask.dtype == torch.bool and torch.equal(mask[..., 0].cpu(), restore >= K)
    assert pred.shape == pe.shape == (B * (N - K), model.projection.in_features) and tgt.shape == te.shape
    if norm_pix:                                              # within 1 fp32 ulp of the rounded fp64 value
        t32 = Ref.normalise(te.double()).float()
        lo, hi = torch.nextafter(t32, torch.full_like(t32, -float("inf"))), torch.nextafter(t32, torch.full_like(t32, float("inf")))
        assert bool(((tgt.cpu() >= lo) & (tgt.cpu() <= hi)).all())
    else:
        assert torch.equal(tgt.cpu(), te)                     # raw pixels, (b, n) order: bit-equal
    assert rel_l2(pred, pe) < 1e-2, rel_l2(pred, pe)
    loss = torch.nn.MSELoss()(pred, tgt)
    assert abs(float(loss.detach()) - loss_e) < 1e-2 * loss_e, (float(loss.detach()), loss_e)
    loss.backward()
    report = {}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        report[k] = tuple(rel_l2(p.grad, ref[mode][3][k]) for mode in ("autograd", "flash", "fp32"))
    worst = max(report, key=lambda k: min(report[k][:2]))
    print(f"largest distance to the nearer oracle form: {worst} {tuple(round(v, 5) for v in report[worst])} (autograd, flash, fp32)")
    for k, (da, df, _) in report.items():
        assert min(da, df) < 2e-2 and max(da, df) < 5e-2, (k, report[k])
    assert model.pos_embed.grad is None and model.decoder_pos_embed.grad is None


def test_the_model_draws_its_noise_first():
    """without a keep table: torch.rand(B, N) from the default CPU generator is the step's first draw"""
    model, sd, x, _, _ = build("a", False)
    torch.manual_seed(123)
    _, _, mask = model(x.to(DEV), return_bool_mask=True)
    torch.manual_seed(123)
    _, restore = Mk.draw_keep(5, 9, 2)
    assert torch.equal(mask[..., 0].cpu(), restore >= 2) and int(mask.sum()) == 5 * 7


@pytest.mark.parametrize("case,norm_pix", GRID, ids=str)
def test_mae_fused_step_equals_autograd_path_and_oracle(case, norm_pix):
    from vitssl_hip.optim import FusedAdamW
    ctor, B, N, K = CASES[case]
    model, sd, x, keep, _ = build(case, norm_pix)
    ref = reference(case, norm_pix)
    st = model.flat_store()
    opt = FusedAdamW(st, lr=1e-3, weight_decay=1e-3)
    loss = model.train_step(x.to(DEV), opt, keep_cpu=keep)
    assert loss.shape == () and abs(float(loss) - ref["autograd"][2]) < 1e-2 * ref["autograd"][2]
    assert rel_l2(model.last_pred, ref["autograd"][0]) < 1e-2 and model.last_targets.shape == model.last_pred.shape
    grads = {k: st.gview(k).cpu().clone() for k in st.names}
    rt = model.runtime()
    Pd = rt.Pd
    dpred = rt.ws.get("dpred", (B * (N - K), rt.Pdp), torch.bfloat16, DEV).clone()
    assert not dpred[:, Pd:].any()
    # the gradient head: 2 (pred - t) / (Mm Pd) of the step's own prediction and targets, rounded to bf16
    want = (2.0 * (model.last_pred.double() - model.last_targets.double()) / model.last_pred.numel()).float()
    assert rel_l2(dpred[:, :Pd].float(), want) < 4e-3                       # bf16 rounding: relative 2^-9 per element at the most
    for k in st.names:                                                       # against the restatement
        da, df = rel_l2(grads[k], ref["autograd"][3][k].reshape(-1)), rel_l2(grads[k], ref["flash"][3][k].reshape(-1))
        assert min(da, df) < 2e-2 and max(da, df) < 5e-2, (k, da, df)
    # the autograd path of a second model with the same weights, from the same d(loss)/d(pred)
    twin, _, _, _, _ = build(case, norm_pix)
    pred2, _ = twin(x.to(DEV), keep_cpu=keep)
    pred2.backward(dpred[:, :Pd].float())
    for k, p in twin.named_parameters():
        assert rel_l2(p.grad.reshape(-1), grads[k]) < 1e-6, (k, rel_l2(p.grad.reshape(-1), grads[k]))
    # one fused AdamW step = oracle.adamw_step on those gradients (eps matters only for ~zero gradients)
    for k, p in model.named_parameters():
        got_g = grads[k].view(sd[k].shape)
        want_p, _, _ = O.adamw_step(sd[k], got_g, torch.zeros_like(sd[k]), torch.zeros_like(sd[k]), 1, 1e-3, wd=1e-3)
        nz = got_g.abs() > 1e-7
        assert max_abs(p.detach().cpu()[nz], want_p[nz]) < 2e-6, k
    assert torch.equal(model.pos_embed.cpu(), sd["pos_embed"])               # buffers: no step
    loss2 = model.train_step(x.to(DEV), opt)                                 # refreshed bf16 weights and a fresh draw
    assert torch.isfinite(loss2)


@pytest.mark.parametrize("case", list(CASES))
def test_inference_forward_equals_the_restatement_with_nothing_masked(case):
    ctor, B, N, K = CASES[case]
    model, sd, x, _, _ = build(case, True)
    want = Ref.inference(sd, x, ctor["patch_size"], ctor["num_heads"], emu="bf16")
    tokens = model.inference_forward(x.to(DEV), return_patch_features=True)
    assert not model.training and tokens.shape == (B, N, 64) and tokens.dtype == torch.float32
    assert rel_l2(tokens, want) < 1e-2
    feats = model.inference_forward(x.to(DEV))
    assert feats.shape == (B, 64) and rel_l2(feats, want.mean(dim=1)) < 1e-2


def test_two_steps_with_a_reducer_cover_the_gradient_buffer():
    from vitssl_hip.engine import GradReducer
    from vitssl_hip.optim import FusedAdamW
    model, _, x, keep, _ = build("a", True)
    st = model.flat_store()
    opt, red = FusedAdamW(st, lr=1e-3, weight_decay=1e-3), GradReducer(st.gflat, bucket_mb=0.01)
    assert red.check_coverage and red.world == 1
    for _ in range(2):
        assert torch.isfinite(model.train_step(x.to(DEV), opt, red, keep_cpu=keep))      # finish() runs _assert_covered
        got = sorted(red.launched)
        assert got[0][0] == 0 and st.numel - got[-1][1] < 64 and sum(hi - lo for lo, hi in got) <= st.numel


def test_fp8_operands_are_refused_naming_bf16():
    from vit_core.ssl.mae import MAEViT
    from vitssl_hip import _lib as L
    from vitssl_hip import engine
    before = engine.linear_operands()
    try:
        engine.set_linear_operands("fp8")
        with pytest.raises(L.VitsslError, match="bf16"):
            MAEViT(**CASES["a"][0]).to(DEV).runtime()
    finally:
        engine.set_linear_operands(before)


def test_trainer_takes_the_fused_path_for_mse_and_the_autograd_path_otherwise(tmp_path):
    from torch import nn
    from utils.model_builder import build_model
    from utils.trainers import MAETrainer

    def cfg(criterion):
        return {"training": {"type": "mae", "num_epochs": 1, "warmup_epochs": 1, "warmup_initial_learning_rate": 1e-6,
                             "warmup_final_learning_rate": 1e-3, "criterion": {"name": criterion, "params": {"reduction": "mean"}},
                             "optimizer": {"name": "AdamW", "params": {"lr": 1e-3, "weight_decay": 1e-3}},
                             "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}}},
                "eval": {}, "data": {"img_size": 24},
                "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 64, "num_blocks": 1, "num_heads": 1, "mlp_dim": 128, "dropout": 0.0,
                          "decoder_embed_dim": 64, "decoder_blocks": 1, "decoder_heads": 2}}

    torch.manual_seed(3)
    data = [torch.rand(4, 3, 24, 24) for _ in range(2)]
    for criterion, fused in (("MSELoss", True), ("L1Loss", False)):
        model = build_model(cfg(criterion)).to(DEV)
        tr = MAETrainer(model, str(tmp_path / criterion), cfg(criterion), data, data[:1], DEV)
        assert tr._fused_ok() is fused and isinstance(tr.criterion, getattr(nn, criterion))
        steps = []
        step = model.train_step
        model.train_step = lambda *a, **k: (steps.append(1), step(*a, **k))[1]
        before = model.decoder_pred.weight.detach().clone()
        train, val = tr.train_epoch(1), tr.validate()
        assert len(steps) == (2 if fused else 0)
        assert torch.isfinite(torch.tensor([train["Loss"], val["Loss"]])).all() and not torch.equal(before, model.decoder_pred.weight.detach())
