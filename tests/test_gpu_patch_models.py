"""The three models at patch sides and channel counts the GEMMs do not take as they are (tests/_patch_cases.py), against the CPU
oracle on the same inputs; tolerances are those of tests/test_gpu_models.py (bf16 GEMM operands against the oracle's emulation
of the same rounding points: outputs 1e-2, gradients 2e-2 of the nearer attention-backward mode and 5e-2 of both; against fp32:
outputs 2e-2, gradients 5e-2 / 6e-2 / 8e-2 as there).  Zero pad columns add exact zeros to fp32 accumulators: the padded
GEMMs bring no rounding of their own."""
import contextlib

import pytest
import torch

import _patch_cases as PC
from _util import rel_l2, max_abs, l1_backward_with_signs
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
RECON_BAR = 4 * __import__("_metrics_ref").fp32_formula_deviation()      # the bar of tests/test_gpu_metrics.py


def _simmim(C, P, img, D=64, H=1, F=64, seed=0, blocks=2):
    from vit_core.ssl.simmim import SimMIMViT
    torch.manual_seed(seed)
    model = SimMIMViT(num_blocks=blocks, input_shape=(C, img, img), embed_dim=D, patch_size=P, num_heads=H, mlp_dim=F,
                      dropout=0.0, mask_ratio=0.6)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.to(DEV).train(), sd


def _pads_are_zero(st, key, rows, cols):
    w = st.w(key)
    return float(w[rows:].float().abs().max() if w.shape[0] > rows else 0) == 0 and \
        float(w[:, cols:].float().abs().max() if w.shape[1] > cols else 0) == 0


@pytest.mark.parametrize("C,P,H_,W_", PC.SQUARE, ids=str)
@pytest.mark.parametrize("B", [1, 3])
def test_simmim_against_oracle(C, P, H_, W_, B):
    """tests/test_gpu_models.py::test_edge_batches_against_oracle at the new geometries: same mask draw, bit-exact targets,
    forward and every gradient against the bf16-emulating oracle in both attention-backward modes."""
    from vit_core.ssl.simmim.masking import draw_mask
    img, heads = H_, 1
    model, sd = _simmim(C, P, img, seed=B * 100 + img)
    x = torch.rand(B, C, img, img)
    N = (img // P) ** 2
    torch.manual_seed(77)
    mask = draw_mask(B, N, 0.6)
    torch.manual_seed(77)                                                    # the model draws the same mask
    pred, tgt, bm = model(x.to(DEV), return_bool_mask=True)
    assert torch.equal(bm[..., 0].cpu(), mask)
    assert pred.shape == tgt.shape == (int(mask.sum()), C * P * P) and tgt.is_contiguous()
    assert pred.is_contiguous() or (C * P * P) % 4 != 0, "pred is a view of a padded buffer only when Pd % 4 != 0"
    torch.nn.L1Loss()(pred, tgt).backward()
    dist = {}
    for mode in ("autograd", "flash"):
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        with (O.flash_delta() if mode == "flash" else contextlib.nullcontext()):
            pe, te = O.simmim_forward(leaves, x, mask, P, heads, emu="bf16")
        assert pred.shape == pe.shape and torch.equal(tgt.cpu(), te)
        print("pred", (C, P, B), mode, rel_l2(pred, pe))
        assert rel_l2(pred, pe) < 1e-2
        l1_backward_with_signs(pe, te, pred, tgt)
        dist[mode] = {k: rel_l2(p.grad, leaves[k].grad) for k, p in model.named_parameters()}
    for k in dist["flash"]:
        d = (dist["autograd"][k], dist["flash"][k])
        print("grad", (C, P, B), k, d)
        assert min(d) < 2e-2 and max(d) < 5e-2, (k, d)
    feat = model.inference_forward(x.to(DEV))
    assert rel_l2(feat, O.simmim_inference(sd, x, P, heads, emu="bf16")) < 1e-2


@pytest.mark.parametrize("C,P,img", [(3, 14, 42), (1, 7, 28)], ids=str)
def test_simmim_fused_step_equals_autograd_path_and_oracle(C, P, img):
    from vit_core.ssl.simmim.masking import draw_mask
    from vitssl_hip.optim import FusedAdamW
    B, heads, Pd = 3, 1, C * P * P
    model, sd = _simmim(C, P, img, seed=5)
    x = torch.rand(B, C, img, img)
    torch.manual_seed(11)
    mask = draw_mask(B, (img // P) ** 2, 0.6)
    # the autograd path on the same mask
    torch.manual_seed(11)
    pred, tgt = model(x.to(DEV))
    loss_a = torch.nn.L1Loss()(pred, tgt)
    loss_a.backward()
    grads_a = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pe, te = O.simmim_forward(leaves, x, mask, P, heads)                     # fp32: stands where the reference's golden stands
    loss_o = O.l1_loss_mean(pe, te)
    l1_backward_with_signs(pe, te, pred, tgt, strict=False)
    model.zero_grad(set_to_none=True)
    opt = FusedAdamW(model.flat_store(), lr=1e-3, weight_decay=1e-3)
    loss = model.train_step(x.to(DEV), opt, mask_cpu=mask)
    assert abs(float(loss) - float(loss_o)) < 1e-2 * float(loss_o)
    assert abs(float(loss) - float(loss_a)) < 1e-5 * float(loss_a)
    st = model.flat_store()
    for k in st.names:
        assert rel_l2(st.gview(k), grads_a[k].reshape(-1)) < 1e-5, (k, rel_l2(st.gview(k), grads_a[k].reshape(-1)))
        assert rel_l2(st.gview(k), leaves[k].grad.reshape(-1)) < 5e-2, (k, rel_l2(st.gview(k), leaves[k].grad.reshape(-1)))
    for k, p in model.named_parameters():
        got_g = st.gview(k).cpu().view(sd[k].shape)
        want, _, _ = O.adamw_step(sd[k], got_g, torch.zeros_like(sd[k]), torch.zeros_like(sd[k]), 1, 1e-3, wd=1e-3)
        nz = got_g.abs() > 1e-7
        assert max_abs(p.detach().cpu()[nz], want[nz]) < 2e-6, k
    assert model.last_pred.shape == model.last_targets.shape == (int(mask.sum()), Pd)
    # the second step refreshes the bf16 images from the updated weights: the pad stays zero, the body follows the weights
    loss2 = model.train_step(x.to(DEV), opt)
    assert torch.isfinite(loss2)
    rt = model.runtime()
    st.refresh_weights()                                                     # the images of the weights the second step left
    assert _pads_are_zero(st, "proj", rt.D, Pd) and _pads_are_zero(st, "head", Pd, rt.D) and _pads_are_zero(st, "head.T", rt.D, Pd)
    assert torch.equal(st.w("proj")[:, :Pd].cpu(), model.projection.weight.detach().cpu().to(BF16))
    assert torch.equal(st.w("head.T")[:, :Pd].cpu(), model.simmim_head.weight.detach().cpu().t().to(BF16))
    assert not torch.equal(model.projection.weight.detach().cpu(), sd["projection.weight"])


@pytest.mark.parametrize("C,P,img", [(1, 7, 28), (3, 14, 42)], ids=str)
def test_vit_supervised_against_oracle(C, P, img):
    from utils.model_builder import freeze_backbone
    from vit_core import ViT
    from vitssl_hip.optim import FusedAdamW
    B, D, heads, F, ncls = 3, 64, 1, 64, 5
    torch.manual_seed(P)
    model = ViT(num_classes=ncls, num_blocks=2, input_shape=(C, img, img), embed_dim=D, patch_size=P, num_heads=heads, mlp_dim=F,
                dropout=0.0)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x, labels = torch.rand(B, C, img, img), torch.tensor([1, 4, 0])
    logits, attn = model(x.to(DEV), return_attn=True)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    lo, ao = O.vit_forward(leaves, x, P, heads, return_attn=True)             # fp32, as the reference's golden
    assert logits.shape == (B, ncls)
    assert rel_l2(logits, lo) < 2e-2 and rel_l2(attn, ao) < 2e-2
    loss = torch.nn.CrossEntropyLoss()(logits, labels.to(DEV))
    loss_o = O.cross_entropy_mean(lo, labels)
    assert abs(float(loss) - float(loss_o)) < 1e-2 * abs(float(loss_o))
    loss.backward()
    loss_o.backward()
    grads = {}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        print("vit grad", (C, P), k, rel_l2(p.grad, leaves[k].grad))
        assert rel_l2(p.grad, leaves[k].grad) < 6e-2, (k, rel_l2(p.grad, leaves[k].grad))
        grads[k] = p.grad.detach().clone()
    model.zero_grad(set_to_none=True)
    # fused step: the same loss and gradients; eval_step; then a frozen backbone (no projection weight gradient)
    opt = FusedAdamW(model.flat_store(), lr=0.0, weight_decay=0.0)
    loss_f = model.train_step(x.to(DEV), labels.to(DEV), opt)
    assert abs(float(loss_f) - float(loss)) < 1e-5 * abs(float(loss))
    st = model.flat_store()
    for k in st.names:
        assert rel_l2(st.gview(k), grads[k].reshape(-1)) < 1e-5, k
    loss_e = model.eval_step(x.to(DEV), labels.to(DEV))
    assert abs(float(loss_e) - float(loss)) < 1e-5 * abs(float(loss))
    freeze_backbone(model)
    loss_z = model.train_step(x.to(DEV), labels.to(DEV), opt)
    assert abs(float(loss_z) - float(loss)) < 1e-5 * abs(float(loss))
    assert float(st.gview("patch_embedding.conv.weight").abs().max()) == 0.0, "proj_wgrad=False launches no weight-gradient GEMM"
    assert rel_l2(st.gview("patch_embedding.cls_token"), grads["patch_embedding.cls_token"].reshape(-1)) < 1e-5
    assert rel_l2(st.gview("classification_head.linear.weight"), grads["classification_head.linear.weight"].reshape(-1)) < 1e-5


def test_dino_patch14_with_a_resized_grid():
    """global 42 x 42 (3 x 3 grid) and local 28 x 28 (2 x 2, positional table resized) at patch 14 against O.dino_forward"""
    from vit_core.ssl.dino import DINOViT
    from vit_core.ssl.dino.loss import DINOLoss
    B, P, D, heads, F, K, G, Lv = 2, 14, 64, 1, 64, 128, 2, 2
    torch.manual_seed(3)
    model = DINOViT(num_blocks=2, input_shape=(3, 42, 42), embed_dim=D, patch_size=P, num_heads=heads, mlp_dim=F, dropout=0.0,
                    output_dim=K, center_momentum=0.9)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(4)
    views = [torch.rand(B, 3, 42, 42, generator=g) for _ in range(G)] + [torch.rand(B, 3, 28, 28, generator=g) for _ in range(Lv)]
    teacher, student = model([v.to(DEV) for v in views], G)
    leaves = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and k.startswith("student_") else v.clone()) for k, v in sd.items()}
    to, so, center1 = O.dino_forward(leaves, views, G, P, heads, (3, 3), sd["center"], 0.9)
    assert teacher.shape == (G * B, K) and student.shape == ((G + Lv) * B, K)
    print("dino", rel_l2(teacher, to), rel_l2(student, so))
    assert rel_l2(teacher, to) < 2e-2 and rel_l2(student, so) < 2e-2
    assert rel_l2(model.center, center1) < 2e-2
    crit = DINOLoss(teacher_temp=0.04, student_temp=0.1)
    loss = crit(teacher.view(G, B, K), student.view(G + Lv, B, K), model.center)
    loss_o = O.dino_loss_naive(to.view(G, B, K), so.view(G + Lv, B, K), center1, 0.04, 0.1)
    assert abs(float(loss) - float(loss_o)) < 1e-2 * abs(float(loss_o))
    loss.backward()
    loss_o.backward()
    for k, p in model.named_parameters():
        if k.startswith("teacher_"):
            assert p.grad is None, k
            continue
        print("dino grad", k, rel_l2(p.grad, leaves[k].grad))
        assert rel_l2(p.grad, leaves[k].grad) < 8e-2, (k, rel_l2(p.grad, leaves[k].grad))


@pytest.mark.parametrize("C,P,img", [(1, 7, 28), (3, 14, 42), (3, 5, 15)], ids=str)
def test_stand_alone_embedding_modules(C, P, img):
    from vit_core.patch_embedding import ConvolutionalPatchEmbedding, DynamicPatchEmbedding, ManualPatchEmbedding
    B, D = 2, 64
    x = torch.rand(B, C, img, img)
    for cls, wname in ((ConvolutionalPatchEmbedding, "conv"), (ManualPatchEmbedding, "linear"), (DynamicPatchEmbedding, "proj")):
        torch.manual_seed(1)
        m = cls((C, img, img), D, P)
        w, b = getattr(m, wname).weight.detach().clone(), getattr(m, wname).bias.detach().clone()
        cls_t, pos = m.cls_token.detach().clone(), m.positional_embedding.detach().clone()
        leaves = [v.requires_grad_(True) for v in (w, b, cls_t, pos)]
        want = O.conv_patch_embed(x, leaves[0].reshape(D, C, P, P), leaves[1], leaves[2], leaves[3], P, emu="bf16")
        m = m.to(DEV)
        got = m(x.to(DEV))
        assert got.shape == want.shape and rel_l2(got, want) < 1e-2, cls.__name__
        up = torch.randn(want.shape, generator=torch.Generator().manual_seed(2))
        (got * up.to(DEV)).sum().backward()
        (want * up).sum().backward()
        for p, l in zip((getattr(m, wname).weight, getattr(m, wname).bias, m.cls_token, m.positional_embedding), leaves):
            assert rel_l2(p.grad.reshape(-1), l.grad.reshape(-1)) < 2e-2, (cls.__name__, tuple(p.shape))


def test_load_weights_simmim_into_vit_at_patch14(tmp_path):
    from utils.model_builder import load_weights
    from vit_core import ViT
    sim, _ = _simmim(3, 14, 42, seed=8)
    path = str(tmp_path / "simmim_p14.pth")
    torch.save({"model_state_dict": {k: v.cpu() for k, v in sim.state_dict().items()}}, path)
    vit = ViT(5, 2, (3, 42, 42), 64, 14, 1, 64, 0.0).to(DEV)
    x = torch.rand(2, 3, 42, 42)
    vit(x.to(DEV))                                             # materialise the flat store and the bf16 images first
    load_weights(vit, path)
    sdv = {k: v.detach().cpu() for k, v in vit.state_dict().items()}
    assert torch.equal(sdv["encoder_blocks.1.feed_forward.linear_out.weight"], sim.state_dict()["encoder_blocks.1.feed_forward.linear_out.weight"].cpu())
    pe = sdv["patch_embedding.positional_embedding"]
    assert torch.equal(pe[:, 1:], sim.positional_embedding.detach().cpu()) and bool((pe[:, 0] == 0).all())
    with torch.no_grad():
        got = vit.eval()(x.to(DEV))
    assert rel_l2(got, O.vit_forward(sdv, x, 14, 1, emu="bf16")) < 1e-2      # the loaded weights are the ones the kernels use


def test_metrics_from_the_fused_step_at_patch14():
    """PSNR / SSIM from last_pred / last_targets whatever their strides, at the bar of tests/test_gpu_metrics.py"""
    from utils.gpu_metrics import GPUMetricHandler
    from vitssl_hip.optim import FusedAdamW
    import _metrics_ref as MR
    for C, P, img in ((3, 14, 42), (1, 7, 28)):           # pred contiguous at 588; a column-prefix view at 49
        model, _ = _simmim(C, P, img, seed=2)
        opt = FusedAdamW(model.flat_store(), lr=1e-3, weight_decay=0.0)
        model.train_step(torch.rand(3, C, img, img).to(DEV), opt)
        assert model.last_pred.is_contiguous() == (C * P * P % 4 == 0)
        h = GPUMetricHandler({"metrics": ["PSNR", "SSIM"]})
        h.update_recon(model.last_pred, model.last_targets, C, P)
        got = h.compute()
        want = MR.recon_metrics(model.last_pred.cpu().contiguous(), model.last_targets.cpu(), C, P)
        for k in ("PSNR", "SSIM"):
            print("metrics", (C, P), k, got[k], want[k])
            assert abs(got[k] - want[k]) <= RECON_BAR * max(abs(want[k]), 1e-300), (k, got[k], want[k])


def test_fp8_operands_at_patch14():
    from vitssl_hip import engine
    from vitssl_hip.optim import FusedAdamW
    engine.set_linear_operands("fp8")
    try:
        model, _ = _simmim(3, 14, 42, D=128, H=2, F=128, seed=4)
        opt = FusedAdamW(model.flat_store(), lr=1e-3, weight_decay=0.0)
        x = torch.rand(3, 3, 42, 42).to(DEV)
        l8 = [float(model.train_step(x, opt)) for _ in range(2)]
    finally:
        engine.set_linear_operands("bf16")
    assert all(v == v and v > 0 for v in l8)


def test_native_geometry_launches_nothing_of_the_patch_header(monkeypatch):
    from vitssl_hip import _lib, ops
    from vitssl_hip.optim import FusedAdamW
    launched = []
    real_call = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a, **k: (launched.append(name), real_call(name, *a, **k))[1])
    model, _ = _simmim(3, 16, 32, seed=6)
    opt = FusedAdamW(model.flat_store(), lr=1e-3, weight_decay=0.0)
    assert torch.isfinite(model.train_step(torch.rand(3, 3, 32, 32).to(DEV), opt))
    assert "vitssl_patchify_bf16" in launched and "vitssl_cast_transpose_batch" in launched and "vitssl_l1_loss" in launched
    assert not set(launched) & set(_lib.REGISTRY["patch"]), set(launched) & set(_lib.REGISTRY["patch"])
    pred = model.last_pred
    assert pred.is_contiguous() and model.last_targets.is_contiguous()


def test_simmim_matches_reference_golden_at_patch14():
    """tests/test_gpu_models.py::test_simmim_matches_reference_golden on the reference-written patch-14 fixture"""
    import numpy as np
    from _util import load_golden, split_prefix, t
    from vit_core.ssl.simmim import SimMIMViT
    g = load_golden("simmim_p14")
    B, img, patch, D, H, F, blocks = (int(v) for v in g["cfg"])
    model = SimMIMViT(num_blocks=blocks, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H, mlp_dim=F,
                      dropout=0.0, mask_ratio=float(g["ratio"]))
    sd = split_prefix(g, "sd/")
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    x = (t(g["x_u8"]).float() / 256.0).to(DEV)
    torch.manual_seed(int(g["mask_seed"]))
    pred, tgt, mask = model(x, return_bool_mask=True)
    assert np.array_equal(mask[..., 0].cpu().numpy(), g["mask"])             # bit-exact mask
    assert np.array_equal(tgt.cpu().numpy(), g["targets"])                   # bit-exact targets, (b,n) order
    assert rel_l2(pred, t(g["pred"])) < 2e-2
    loss = torch.nn.L1Loss(reduction="mean")(pred, tgt)
    assert abs(float(loss) - float(g["loss"])) < 1e-2 * float(g["loss"])
    loss.backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pe, te = O.simmim_forward(leaves, x.cpu(), t(g["mask"]), patch, H, emu="bf16")
    assert rel_l2(pred, pe) < 1e-2
    l1_backward_with_signs(pe, te, pred, tgt)
    ref = split_prefix(g, "grad/")
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        if k in ref:
            assert rel_l2(p.grad, ref[k]) < 5e-2, (k, rel_l2(p.grad, ref[k]))      # the reference's own gradients (its own signs)
        assert rel_l2(p.grad, leaves[k].grad) < 2e-2, (k, "emu", rel_l2(p.grad, leaves[k].grad))
    rows = [int(r) for r in g["head_rows"]]
    assert rel_l2(model.simmim_head.weight.grad[rows], t(g["gradrows/simmim_head.weight"])) < 5e-2
    feat = model.inference_forward(x)
    assert not model.training
    assert rel_l2(feat, t(g["feat"])) < 2e-2
    assert model.inference_forward(x, return_patch_features=True).shape == (B, (img // patch) ** 2, D)
