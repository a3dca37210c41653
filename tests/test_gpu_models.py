"""Model-level parity of the HIP engine against (a) golden vectors produced by the
reference itself and (b) the CPU oracle on the same seeded inputs.

Tolerances (bf16 GEMM operands, fp32 accumulate / residual / LN / softmax, vs an fp32
reference): outputs rel-L2 <= 2e-2, loss rel <= 1e-2, gradients rel-L2 <= 5e-2 per
tensor; against the oracle's bf16-rounding emulation (same rounding points) outputs 1e-2 and
gradients 2e-2 for the same d(loss)/d(pred) (_util.l1_backward_with_signs).
Masks, gather order and targets: bit-exact."""
import contextlib

import numpy as np
import pytest
import torch

from _util import load_golden, split_prefix, t, rel_l2, max_abs, l1_backward_with_signs
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _simmim_from_golden(name, dropout=0.0):
    from vit_core.ssl.simmim import SimMIMViT
    g = load_golden(name)
    B, img, patch, D, H, F, blocks = (int(v) for v in g["cfg"])
    model = SimMIMViT(num_blocks=blocks, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H,
                      mlp_dim=F, dropout=dropout, mask_ratio=float(g["ratio"]))
    sd = split_prefix(g, "sd/")
    model.load_state_dict(sd)
    return g, model.to(DEV), sd, (B, img, patch, D, H, F, blocks)


@pytest.mark.parametrize("name", ["simmim_tiny", "simmim_n196"])
def test_simmim_matches_reference_golden(name):
    g, model, sd, (B, img, patch, D, H, F, blocks) = _simmim_from_golden(name)
    x = (t(g["x_u8"]).float() / 256.0).to(DEV)
    model.train()
    torch.manual_seed(int(g["mask_seed"]))
    pred, tgt, mask = model(x, return_bool_mask=True)
    assert mask.shape == (B, (img // patch) ** 2, 1) and mask.dtype == torch.bool
    assert np.array_equal(mask[..., 0].cpu().numpy(), g["mask"])             # bit-exact mask
    assert np.array_equal(tgt.cpu().numpy(), g["targets"])                   # bit-exact targets, (b,n) order
    assert rel_l2(pred, t(g["pred"])) < 2e-2
    loss = torch.nn.L1Loss(reduction="mean")(pred, tgt)
    assert abs(float(loss) - float(g["loss"])) < 1e-2 * float(g["loss"])
    loss.backward()
    # tight check against the oracle with the same rounding points
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pe, te = O.simmim_forward(leaves, x.cpu(), t(g["mask"]), patch, H, emu="bf16")
    assert rel_l2(pred, pe) < 1e-2
    l1_backward_with_signs(pe, te, pred, tgt)             # the oracle's backward starts from the signs this path saw (_util.py)
    ref = split_prefix(g, "grad/")
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        assert rel_l2(p.grad, ref[k]) < 5e-2, (k, rel_l2(p.grad, ref[k]))      # the reference's own gradients (its own signs)
        assert rel_l2(p.grad, leaves[k].grad) < 2e-2, (k, "emu", rel_l2(p.grad, leaves[k].grad))
    feat = model.inference_forward(x)
    assert not model.training
    assert rel_l2(feat, t(g["feat"])) < 2e-2
    tokens = model.inference_forward(x, return_patch_features=True)
    assert tokens.shape == (B, (img // patch) ** 2, D)


def test_simmim_fused_step_equals_autograd_path_and_oracle():
    from vitssl_hip.optim import FusedAdamW
    g, model, sd, (B, img, patch, D, H, F, blocks) = _simmim_from_golden("simmim_tiny")
    x = (t(g["x_u8"]).float() / 256.0).to(DEV)
    mask = t(g["mask"])
    opt = FusedAdamW(model.flat_store(), lr=1e-3, weight_decay=1e-3)
    loss = model.train_step(x, opt, mask_cpu=mask)
    assert abs(float(loss) - float(g["loss"])) < 1e-2 * float(g["loss"])
    # gradients of the fused path live in the flat buffer
    st = model.flat_store()
    ref = split_prefix(g, "grad/")
    for k in st.names:
        assert rel_l2(st.gview(k), ref[k].reshape(-1)) < 5e-2, k
    # the flat AdamW kernel applied exactly one torch.optim.AdamW step to every parameter,
    # from the gradients the engine produced (gradient parity is asserted above; Adam's
    # first step is lr*sign(g), so it is checked against the engine's own gradients)
    for k, p in model.named_parameters():
        got_g = st.gview(k).cpu().view(sd[k].shape)
        want, _, _ = O.adamw_step(sd[k], got_g, torch.zeros_like(sd[k]), torch.zeros_like(sd[k]), 1, 1e-3, wd=1e-3)
        nz = got_g.abs() > 1e-7          # eps matters only for ~zero gradients
        assert max_abs(p.detach().cpu()[nz], want[nz]) < 2e-6, k
    # second step runs on the refreshed bf16 weights and a fresh mask
    loss2 = model.train_step(x, opt)
    assert torch.isfinite(loss2)


def test_simmim_dropout_matches_oracle_with_exported_masks():
    """p > 0: the engine's counter-based masks are exported and fed to the oracle."""
    from vitssl_hip import ops
    from vit_core import _runtime as R
    from vit_core.ssl.simmim.masking import draw_mask
    p = 0.1
    g, model, sd, (B, img, patch, D, H, F, blocks) = _simmim_from_golden("simmim_tiny", dropout=p)
    x = (t(g["x_u8"]).float() / 256.0).to(DEV)
    N = (img // patch) ** 2
    model.train()
    torch.manual_seed(77)
    pred, tgt = model(x)
    torch.manual_seed(77)
    pred_again, _ = model(x)
    assert torch.equal(pred, pred_again)                                      # reproducible under torch.manual_seed
    torch.manual_seed(77)
    mask = draw_mask(B, N, float(g["ratio"]))
    seed = R.next_seed()
    keeps = []
    for i in range(blocks):
        ks = []
        for which, cols in ((0, D), (1, F), (2, D)):
            k = ops.dropout_mask(B * N, cols, ops.make_dropout(p, seed, 3 * i + which), DEV)
            ks.append(k.float().cpu().view(B, N, cols))
        keeps.append(ks)
    p_eff = round(p * 65536) / 65536
    pe, te = O.simmim_forward(sd, x.cpu(), mask, patch, H, emu="bf16", keeps=keeps, p_drop=p_eff)
    assert torch.equal(tgt.cpu(), te)
    assert rel_l2(pred, pe) < 1e-2
    model.eval()
    torch.manual_seed(77)
    pred_eval, _ = model(x)
    assert not torch.equal(pred_eval, pred)                                   # dropout differs train vs eval


def _export_keeps(p, seed, blocks, rows, D, F, shape):
    """The engine's three dropout masks per block (drop1, FFN inner, drop2), as float 0/1 tensors for the oracle."""
    from vitssl_hip import ops
    return [[ops.dropout_mask(rows, cols, ops.make_dropout(p, seed, 3 * i + which), DEV).float().cpu().view(*shape, cols)
             for which, cols in ((0, D), (1, F), (2, D))] for i in range(blocks)]


@pytest.mark.parametrize("path", ["autograd", "train_step"])
def test_simmim_dropout_backward_matches_oracle_with_exported_masks(path):
    """bf16 schedule, dropout ON (the headline bench configuration): every parameter gradient of
    EncoderStack.backward against the oracle run with the exported masks -- i.e. the SITE wiring of the backward
    (_drop(i, 0) in the LN2 backward, _drop(i - 1, 2) in the LN1 backward of block i, _drop(last, 2) in grad_mask_cast,
    g' carrying site 1) is compared with the reference's placement (encoder_block.py:45-46,51-52, feed_forward.py:27).
    Three blocks, so that first / middle / last block each take their own branch of the schedule."""
    from vit_core import _runtime as R
    from vit_core.ssl.simmim import SimMIMViT
    from vit_core.ssl.simmim.masking import draw_mask
    from vitssl_hip.optim import FusedAdamW
    p, B, D, H, F, blocks, img, patch = 0.1, 4, 128, 2, 256, 3, 64, 16
    N = (img // patch) ** 2
    torch.manual_seed(5)
    model = SimMIMViT(num_blocks=blocks, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H, mlp_dim=F,
                      dropout=p, mask_ratio=0.6)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x = torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(6))
    torch.manual_seed(91)
    mask = draw_mask(B, N, 0.6)
    if path == "autograd":
        torch.manual_seed(91)
        pred, tgt = model(x.to(DEV))
        loss = torch.nn.functional.l1_loss(pred, tgt)
        loss.backward()
        grads = {k: prm.grad for k, prm in model.named_parameters()}
        torch.manual_seed(91)
        draw_mask(B, N, 0.6)
        seed = R.next_seed()
    else:
        opt = FusedAdamW(model.flat_store(), lr=1e-4, weight_decay=0.0)
        torch.manual_seed(92)
        loss = model.train_step(x.to(DEV), opt, mask_cpu=mask)
        st = model.flat_store()
        grads = {k: st.gview(k).view(sd[k].shape) for k in st.names}
        pred, tgt = model.last_pred, model.last_targets
        torch.manual_seed(92)
        seed = R.next_seed()
    keeps = _export_keeps(p, seed, blocks, B * N, D, F, (B, N))
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pe, te = O.simmim_forward(leaves, x, mask, patch, H, emu="bf16", keeps=keeps, p_drop=round(p * 65536) / 65536)
    assert torch.equal(tgt.cpu(), te) and rel_l2(pred, pe) < 1e-2
    wl = O.l1_loss_mean(pe, te)
    l1_backward_with_signs(pe, te, pred, tgt)             # same d(loss)/d(pred) on both sides (_util.py)
    assert abs(float(loss) - float(wl.detach())) < 1e-2 * float(wl.detach())
    for k in leaves:
        assert rel_l2(grads[k], leaves[k].grad) < 2e-2, (path, k, rel_l2(grads[k], leaves[k].grad))


def test_encoder_block_dropout_backward_matches_oracle_with_exported_masks():
    """Stand-alone EncoderBlock, p = 0.25: output, input gradient and every parameter gradient with the masks exported."""
    from vit_core import EncoderBlock
    from vit_core import _runtime as R
    p, B, T, D, H, F = 0.25, 3, 20, 128, 2, 256
    torch.manual_seed(8)
    blk = EncoderBlock(D, H, F, p)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    blk = blk.to(DEV).train()
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(9))
    w = torch.randn(B, T, D, generator=torch.Generator().manual_seed(10))
    xg = x.to(DEV).requires_grad_(True)
    torch.manual_seed(55)
    y, _ = blk(xg)
    (y * w.to(DEV)).sum().backward()
    torch.manual_seed(55)
    seed = R.next_seed()
    keep = _export_keeps(p, seed, 1, B * T, D, F, (B, T))[0]
    for k in keep:
        assert abs(float(k.mean()) - 0.75) < 0.03
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    ye, _ = O.encoder_block(xo, leaves, "", H, emu="bf16", keep=keep, p_drop=round(p * 65536) / 65536)
    assert rel_l2(y, ye) < 1e-2
    (ye * w).sum().backward()
    assert rel_l2(xg.grad, xo.grad) < 5e-2, rel_l2(xg.grad, xo.grad)
    for k, prm in blk.named_parameters():
        assert rel_l2(prm.grad, leaves[k].grad) < 5e-2, (k, rel_l2(prm.grad, leaves[k].grad))


@pytest.mark.parametrize("which", [0, 2])
def test_dropout_backward_check_detects_a_swapped_site(which):
    """Negative control of the test above: with ONE dropout site of the backward schedule pointed at another block's
    stream (what a swapped index in engine.EncoderStack.backward would do) the gradient comparison must fail."""
    from vit_core import _runtime as R
    from vit_core.ssl.simmim import SimMIMViT
    from vit_core.ssl.simmim.masking import draw_mask
    p, B, D, H, F, blocks, img, patch = 0.1, 4, 128, 2, 256, 3, 64, 16
    N = (img // patch) ** 2
    torch.manual_seed(5)
    model = SimMIMViT(num_blocks=blocks, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H, mlp_dim=F,
                      dropout=p, mask_ratio=0.6)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x = torch.rand(B, 3, img, img, generator=torch.Generator().manual_seed(6))
    torch.manual_seed(91)
    mask = draw_mask(B, N, 0.6)
    torch.manual_seed(91)
    pred, tgt = model(x.to(DEV))
    stack = model.runtime().stack
    orig = stack._drop
    stack._drop = lambda i, w, seed, training: orig((i + 1) % blocks if (w == which and i == 1) else i, w, seed, training)
    try:
        torch.nn.functional.l1_loss(pred, tgt).backward()
    finally:
        stack._drop = orig
    torch.manual_seed(91)
    draw_mask(B, N, 0.6)
    keeps = _export_keeps(p, R.next_seed(), blocks, B * N, D, F, (B, N))
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pe, te = O.simmim_forward(leaves, x, mask, patch, H, emu="bf16", keeps=keeps, p_drop=round(p * 65536) / 65536)
    O.l1_loss_mean(pe, te).backward()
    worst = max(rel_l2(prm.grad, leaves[k].grad) for k, prm in model.named_parameters())
    assert worst > 5e-2, worst


def test_vit_supervised_matches_reference_golden():
    from vit_core import ViT
    g = load_golden("vit_tiny")
    B, img, patch, D, H, F, blocks, C = (int(v) for v in g["cfg"])
    model = ViT(num_classes=C, num_blocks=blocks, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H,
                mlp_dim=F, dropout=0.0)
    model.load_state_dict(split_prefix(g, "sd/"))
    model = model.to(DEV).train()
    x = (t(g["x_u8"]).float() / 256.0).to(DEV)
    logits, attn = model(x, return_attn=True)
    assert logits.shape == (B, C)
    assert rel_l2(logits, t(g["logits"])) < 2e-2
    assert rel_l2(attn, t(g["attn"])) < 2e-2
    loss = torch.nn.CrossEntropyLoss()(logits, t(g["labels"]).to(DEV))
    assert abs(float(loss) - float(g["loss"])) < 1e-2 * abs(float(g["loss"]))
    loss.backward()
    ref = split_prefix(g, "grad/")
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        assert rel_l2(p.grad, ref[k]) < 6e-2, (k, rel_l2(p.grad, ref[k]))
    # batch independence (the reference's own test property, tests/test_vit.py:76-114)
    model.eval()
    with torch.no_grad():
        full = model(x)
        single = torch.cat([model(x[i:i + 1]) for i in range(B)])
    assert max_abs(full, single) < 1e-5
    # plain tensor return when return_attn is False
    assert isinstance(full, torch.Tensor)


# ----------------------------------------------------------------------------- DINO
def _dino_from_golden():
    from synth import dino_big_weights
    from vit_core.ssl.dino import DINOViT
    g = load_golden("dino_tiny")
    B, gi, li, patch, D, H, F, blocks, K, G, Lv = (int(v) for v in g["cfg"])
    model = DINOViT(num_blocks=blocks, input_shape=(3, gi, gi), embed_dim=D, patch_size=patch, num_heads=H, mlp_dim=F,
                    dropout=0.0, output_dim=K, center_momentum=0.9)
    sd = split_prefix(g, "sd/")
    for k, a in dino_big_weights(D).items():
        sd[k] = t(a)
    model.load_state_dict(sd)
    return g, model.to(DEV), sd, (B, gi, li, patch, D, H, F, blocks, K, G, Lv)


def test_dino_matches_reference_golden():
    from synth import summarize, BIG_KEYS
    from vit_core.ssl.dino.loss import DINOLoss
    g, model, sd, (B, gi, li, patch, D, H, F, blocks, K, G, Lv) = _dino_from_golden()
    assert not any(p.requires_grad for n, p in model.named_parameters() if n.startswith("teacher_"))
    views = [(t(g[f"view{i}_u8"]).float() / 256.0).to(DEV) for i in range(G + Lv)]
    model.train()
    assert max_abs(model.center, t(g["center0"])) == 0
    teacher, student = model(views, G)
    assert teacher.shape == (G * B, K) and student.shape == ((G + Lv) * B, K)
    assert not teacher.requires_grad
    assert rel_l2(teacher, t(g["teacher"])) < 2e-2
    assert rel_l2(student, t(g["student"])) < 2e-2
    assert rel_l2(model.center, t(g["center1"])) < 2e-2          # centre updated inside forward
    crit = DINOLoss(teacher_temp=0.04, student_temp=0.1)
    loss = crit(teacher.view(G, B, K), student.view(G + Lv, B, K), model.center)
    assert abs(float(loss) - float(g["loss"])) < 1e-2 * abs(float(g["loss"]))
    # the loss kernel itself, on the reference's exact logits: tight
    lt, ls, c1 = t(g["teacher"]).to(DEV), t(g["student"]).to(DEV).requires_grad_(True), t(g["center1"]).to(DEV)
    loss_exact = crit(lt.view(G, B, K), ls.view(G + Lv, B, K), c1)
    assert abs(float(loss_exact) - float(g["loss"])) < 1e-5 * abs(float(g["loss"]))
    loss_exact.backward()
    ls_cpu = t(g["student"]).clone().requires_grad_(True)
    O.dino_loss_naive(t(g["teacher"]).view(G, B, K), ls_cpu.view(G + Lv, B, K), t(g["center1"]), 0.04, 0.1).backward()
    assert rel_l2(ls.grad, ls_cpu.grad) < 1e-2                   # bf16-stored gradient
    loss.backward()
    ref = split_prefix(g, "grad/")
    for k, p in model.named_parameters():
        if k.startswith("teacher_"):
            assert p.grad is None, k
            continue
        assert p.grad is not None, k
        if any(k.endswith(b) for b in BIG_KEYS) and "_head." in k:
            s = summarize(p.grad.cpu().numpy())
            assert rel_l2(t(s["rows"]), t(g[f"gradsum/{k}/rows"])) < 8e-2, k
            assert rel_l2(t(s["cols"]), t(g[f"gradsum/{k}/cols"])) < 8e-2, k
        else:
            assert rel_l2(p.grad, ref[k]) < 8e-2, (k, rel_l2(p.grad, ref[k]))
    # EMA over the flat stores == per-tensor reference update
    model.momentum_update_teacher(0.996)
    for k, want in split_prefix(g, "ema/").items():
        assert max_abs(dict(model.state_dict())[k], want) < 1e-6, k
    feats = model.inference_forward(views[0], return_features=True)
    assert rel_l2(feats, t(g["feats"])) < 2e-2 and not model.training
    out = model.inference_forward(views[0])
    assert out.shape == (B, K)


def test_dino_fused_step_runs_and_matches_autograd_loss():
    from vit_core.ssl.dino.loss import DINOLoss
    from vitssl_hip.optim import FusedAdamW
    g, model, sd, (B, gi, li, patch, D, H, F, blocks, K, G, Lv) = _dino_from_golden()
    views = [(t(g[f"view{i}_u8"]).float() / 256.0).to(DEV) for i in range(G + Lv)]
    model.train()
    crit = DINOLoss(0.04, 0.1)
    opt = FusedAdamW(model.trainable_store(), lr=1e-4, weight_decay=1e-3)
    teacher_before = model.teacher_head.mlp[0].bias.detach().clone()
    student_before = model.student_head.mlp[0].bias.detach().clone()
    loss = model.train_step(views, G, crit, opt, None, teacher_momentum=0.9)
    assert abs(float(loss) - float(g["loss"])) < 1e-2 * abs(float(g["loss"]))
    st = model.trainable_store()
    ref = split_prefix(g, "grad/")
    for k in ("student_backbone.patch_embedding.positional_embedding", "student_head.mlp.4.bias",
              "student_head.fully_connected.parametrizations.weight.original0",
              "student_backbone.encoder_blocks.0.self_attention.w_key.weight"):
        assert rel_l2(st.gview(k), ref[k].reshape(-1)) < 8e-2, k
    student_after = model.student_head.mlp[0].bias.detach()
    assert not torch.equal(student_after, student_before)                     # AdamW moved the student
    want = 0.9 * teacher_before + 0.1 * student_after                        # EMA uses the UPDATED student
    assert max_abs(model.teacher_head.mlp[0].bias, want) < 1e-6
    loss2 = model.train_step(views, G, crit, opt, None, teacher_momentum=0.9)
    assert torch.isfinite(loss2)


@pytest.mark.parametrize("B,img,patch,D,H,F,tol", [(1, 16, 8, 64, 1, 64, 5e-2), (1, 32, 8, 128, 2, 192, 2e-2), (5, 24, 8, 64, 1, 128, 2e-2)])
def test_edge_batches_against_oracle(B, img, patch, D, H, F, tol):
    """Smallest shapes the path accepts: a single image, 4 / 9 / 16 tokens (all GEMMs ragged
    in M, attention with one partial key tile), odd batch: forward, loss and every gradient
    against the CPU oracle on the same mask."""
    from vit_core.ssl.simmim import SimMIMViT
    from vit_core.ssl.simmim.masking import draw_mask
    torch.manual_seed(B * 100 + img)
    model = SimMIMViT(num_blocks=2, input_shape=(3, img, img), embed_dim=D, patch_size=patch, num_heads=H, mlp_dim=F,
                      dropout=0.0, mask_ratio=0.6)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x = torch.rand(B, 3, img, img)
    N = (img // patch) ** 2
    torch.manual_seed(77)
    mask = draw_mask(B, N, 0.6)
    torch.manual_seed(77)                                                    # the model draws the same mask
    pred, tgt, bm = model(x.to(DEV), return_bool_mask=True)
    assert torch.equal(bm[..., 0].cpu(), mask)
    torch.nn.L1Loss()(pred, tgt).backward()
    # the bf16-emulating oracle with autograd's attention backward, and with the flash-style one of csrc/attention.hip
    # (oracle sdpa(): delta from the bf16 output): within 2e-2 of the nearer, 5e-2 of both, for the same d(loss)/d(pred) (_util.py).
    # The single 4-token image keeps the 5e-2 bar: its smallest gradient (query weights of block 0, |g| 30x below the others)
    # sits 2-3 % away (measured while the column sums were float atomics; they are slot-row reduces added in a fixed order now,
    # DESIGN §5, and tests/test_gpu_step_streams.py asserts that fused steps give the same bits run to run).
    dist = {}
    for mode in ("autograd", "flash"):
        leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        with (O.flash_delta() if mode == "flash" else contextlib.nullcontext()):
            pe, te = O.simmim_forward(leaves, x, mask, patch, H, emu="bf16")
        assert pred.shape == pe.shape and torch.equal(tgt.cpu(), te)
        assert rel_l2(pred, pe) < 1e-2
        l1_backward_with_signs(pe, te, pred, tgt)
        dist[mode] = {k: rel_l2(p.grad, leaves[k].grad) for k, p in model.named_parameters()}
    for k in dist["flash"]:
        d = (dist["autograd"][k], dist["flash"][k])
        assert min(d) < tol and max(d) < 2.5 * tol, (k, d)


def test_single_token_image_has_nothing_masked():
    """int(N * mask_ratio) == 0 (one token per image): the reference indexes with an all-false mask and returns EMPTY pred /
    targets (vit_core/ssl/simmim/model.py:56-62 there); L1Loss(mean) of them is nan and every gradient zero.  Same here, on
    the autograd path and in the fused step (which still applies the optimizer: weight decay only)."""
    from vit_core.ssl.simmim import SimMIMViT
    from vitssl_hip.optim import FusedAdamW
    torch.manual_seed(5)
    model = SimMIMViT(num_blocks=2, input_shape=(3, 8, 8), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=64,
                      dropout=0.1, mask_ratio=0.6).to(DEV).train()
    x = torch.rand(3, 3, 8, 8, device=DEV)
    pred, tgt, bm = model(x, return_bool_mask=True)
    assert tuple(pred.shape) == (0, 192) and tuple(tgt.shape) == (0, 192) and tuple(bm.shape) == (3, 1, 1) and not bool(bm.any())
    loss = torch.nn.L1Loss()(pred, tgt)
    assert torch.isnan(loss)
    loss.backward()
    for k, p in model.named_parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = FusedAdamW(model.flat_store(), lr=1e-2, weight_decay=0.5)
    out = model.train_step(x, opt)
    assert torch.isnan(out)
    after = model.state_dict()
    for k, v in before.items():
        assert torch.allclose(after[k], v * (1.0 - 1e-2 * 0.5), rtol=0, atol=1e-7), k      # zero gradients: decay only
