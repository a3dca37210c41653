"""Models with head dims other than 64 through the unchanged public API, against the CPU oracle and against the reference's
own vectors (tests/golden/vit_dh32.npz).  Bars of tests/test_gpu_models.py: against the oracle's bf16 emulation outputs 1e-2 and
gradients 2e-2 (for the engine's own d(loss)/d(pred) where SimMIM is concerned, _util.l1_backward_with_signs); against the fp32
golden vectors outputs 2e-2 and gradients 6e-2."""
import pytest
import torch

import _hd_golden as G
from _util import l1_backward_with_signs, max_abs, rel_l2, t
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _leaves(model):
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return sd, {k: v.clone().requires_grad_(True) for k, v in sd.items()}


def _flash_grads_close(model, leaves, tol=2e-2):
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        assert p.grad is not None, k
        assert rel_l2(p.grad, leaves[k].grad) < tol, (k, rel_l2(p.grad, leaves[k].grad))


def test_vit_dh32_against_oracle():
    """the reference's own tests/test_vit.py configuration: 128 / 4 heads"""
    from vit_core import ViT
    torch.manual_seed(41)
    model = ViT(num_classes=10, num_blocks=2, input_shape=(3, 32, 32), embed_dim=128, patch_size=8, num_heads=4, mlp_dim=256,
                dropout=0.0).to(DEV).train()
    sd, leaves = _leaves(model)
    x = torch.rand(4, 3, 32, 32)
    labels = torch.tensor([1, 9, 0, 4])
    logits, attn = model(x.to(DEV), return_attn=True)
    with O.flash_delta():
        le, ae = O.vit_forward(leaves, x, 8, 4, emu="bf16", return_attn=True)
        assert logits.shape == (4, 10) and attn.shape == ae.shape == (4, 4, 17, 17)
        assert rel_l2(logits, le) < 1e-2 and rel_l2(attn, ae) < 1e-2
        assert max_abs(attn.sum(-1), torch.ones(4, 4, 17)) < 1e-3
        torch.nn.CrossEntropyLoss()(logits, labels.to(DEV)).backward()
        O.cross_entropy_mean(le, labels).backward()
    _flash_grads_close(model, leaves)
    assert isinstance(model(x.to(DEV)), torch.Tensor)


def test_vit_dh32_matches_reference_golden():
    from vit_core import ViT
    g, sd, (B, img, patch, D, H, F, blocks, C) = G.load()
    model = ViT(num_classes=C, num_blocks=blocks, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H, mlp_dim=F,
                dropout=0.0)
    model.load_state_dict(sd)
    model = model.to(DEV).train()
    x = (t(g["x_u8"]).float() / 256.0).to(DEV)
    logits, attn = model(x, return_attn=True)
    assert rel_l2(logits, t(g["logits"])) < 2e-2 and rel_l2(attn, t(g["attn"])) < 2e-2
    loss = torch.nn.CrossEntropyLoss()(logits, t(g["labels"]).to(DEV))
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-2 * abs(float(g["loss"]))
    loss.backward()
    G.check_grads({k: p.grad for k, p in model.named_parameters()}, g, 6e-2)


def test_simmim_dh96_against_oracle():
    from vit_core.ssl.simmim import SimMIMViT
    from vit_core.ssl.simmim.masking import draw_mask
    torch.manual_seed(42)
    model = SimMIMViT(2, (3, 32, 32), 192, 8, 2, 256, 0.0, 0.6)
    sd, leaves = _leaves(model)
    model = model.to(DEV).train()
    x = torch.rand(3, 3, 32, 32)
    torch.manual_seed(77)
    mask = draw_mask(3, 16, 0.6)
    torch.manual_seed(77)
    pred, tgt, bm = model(x.to(DEV), return_bool_mask=True)
    assert torch.equal(bm[..., 0].cpu(), mask)
    torch.nn.L1Loss()(pred, tgt).backward()
    with O.flash_delta():
        pe, te = O.simmim_forward(leaves, x, mask, 8, 2, emu="bf16")
        assert torch.equal(tgt.cpu(), te) and rel_l2(pred, pe) < 1e-2
        l1_backward_with_signs(pe, te, pred, tgt)
    _flash_grads_close(model, leaves)
    # and a fused train step runs on the same model
    from vitssl_hip.optim import FusedAdamW
    loss = model.train_step(x.to(DEV), FusedAdamW(model.flat_store(), lr=1e-4, weight_decay=1e-3))
    assert torch.isfinite(loss)


def test_dino_dh8_against_oracle():
    from vit_core.ssl.dino import DINOViT
    torch.manual_seed(43)
    model = DINOViT(2, (3, 32, 32), 64, 8, 8, 128, 0.0, 256, 0.9)
    sd, leaves = _leaves(model)
    model = model.to(DEV).train()
    Bn, G_ = 2, 2
    views = [torch.rand(Bn, 3, 32, 32) for _ in range(G_)] + [torch.rand(Bn, 3, 16, 16) for _ in range(3)]
    center0 = model.center.detach().cpu().clone()
    teacher, student = model([v.to(DEV) for v in views], G_)
    with O.flash_delta():
        te, se, _ = O.dino_forward(leaves, views, G_, 8, 8, (4, 4), center0, 0.9, emu="bf16")
        assert teacher.shape == te.shape and student.shape == se.shape
        assert rel_l2(teacher, te) < 1e-2 and rel_l2(student, se) < 1e-2
        w = torch.randn(student.shape, generator=torch.Generator().manual_seed(5))
        (student * w.to(DEV)).sum().backward()
        (se * w).sum().backward()
    for k, p in model.named_parameters():
        if k.startswith("student_"):
            assert p.grad is not None and rel_l2(p.grad, leaves[k].grad) < 2e-2, (k, rel_l2(p.grad, leaves[k].grad))


def test_stand_alone_modules_dh8():
    from vit_core import EncoderBlock, MultiHeadedAttention
    torch.manual_seed(44)
    mha = MultiHeadedAttention(64, 8).to(DEV)
    _, leaves = _leaves(mha)
    x = torch.randn(3, 20, 64)
    xd, xr = x.to(DEV).requires_grad_(True), x.clone().requires_grad_(True)
    out, probs = mha(xd, xd, xd, return_attn=True)
    with O.flash_delta():
        ro, rp = O.mha(xr, leaves, "", 8, emu="bf16", return_attn=True)
        assert probs.shape == (3, 8, 20, 20) and rel_l2(out, ro) < 1e-2 and rel_l2(probs, rp) < 1e-2
        out.square().sum().backward()
        ro.square().sum().backward()
    assert rel_l2(xd.grad, xr.grad) < 2e-2
    _flash_grads_close(mha, leaves)

    blk = EncoderBlock(d_model=64, num_heads=8, mlp_dim=128, dropout=0.0).to(DEV).train()     # the reference's tests/test_encoder_block.py
    _, leaves = _leaves(blk)
    xd, xr = x.to(DEV).requires_grad_(True), x.clone().requires_grad_(True)
    y, probs = blk(xd, return_attn=True)
    with O.flash_delta():
        ry, rp = O.encoder_block(xr, leaves, "", 8, emu="bf16", return_attn=True)
        assert rel_l2(y, ry) < 1e-2 and rel_l2(probs, rp) < 1e-2
        y.square().sum().backward()
        ry.square().sum().backward()
    assert rel_l2(xd.grad, xr.grad) < 2e-2
    _flash_grads_close(blk, leaves)


def test_fp8_operands_refuse_dh32_before_any_launch():
    from vit_core import ViT
    from vitssl_hip import _lib as L
    from vitssl_hip.engine import set_linear_operands
    set_linear_operands("fp8")
    try:
        model = ViT(num_classes=10, num_blocks=2, input_shape=(3, 32, 32), embed_dim=128, patch_size=8, num_heads=4, mlp_dim=256,
                    dropout=0.0).to(DEV)
        with pytest.raises(L.VitsslError, match="bf16"):
            model(torch.rand(2, 3, 32, 32, device=DEV))
    finally:
        set_linear_operands("bf16")
