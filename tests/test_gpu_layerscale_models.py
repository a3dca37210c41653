"""LayerScale (layer_scale_init) in the models against the CPU oracle.

The unchanged oracle expresses LayerScale through its keep triples (tests/_layerscale_ref.py): keep[0] = g1 * k1, keep[2] = g2 * k2
with g1 / g2 leaves, so every gamma gradient comes from autograd.  The gammas are set to per-channel random values in +-[0.5, 1.5],
different for the two branches of every block: with init-sized gammas the branches vanish and a broken kernel would pass.

Tiny shapes as in tests/test_gpu_droppath_models.py: 5 images of 64 x 64, patch 16, D = 128, 2 heads, 3 blocks (first / middle /
last block each take their own branch of EncoderStack.backward).  Bars as there, against the oracle's bf16-rounding emulation:
outputs 1e-2, loss 1e-2 relative, every gradient 2e-2 rel-L2, the gamma gradients included."""
import copy

import numpy as np
import pytest
import torch

import _droppath_ref as DP
import _layerscale_ref as LS
from _util import l1_backward_with_signs, rel_l2
from oracle import vit_oracle as O
from test_gpu_droppath_models import (B, BLOCKS, CLASSES, D, DEV, F, GRAD_BAR, H, IMG, LOSS_BAR, OUT_BAR, PATCH, Recorder, _gen_state, dino_views,
                                      find_seed, vit_batch, worst_grad)

pytestmark = pytest.mark.gpu
INIT = 1e-5
T = (IMG // PATCH) ** 2 + 1
GAMMA_KEYS = [f"encoder_blocks.{i}.layer_scale{k}.gamma" for i in range(BLOCKS) for k in (1, 2)]


def with_gammas(m, ones=False, seed=21):
    """load per-channel random gammas (or ones) into a freshly built model -> (model on the GPU in training mode, its state)"""
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    new = LS.random_gammas(sd, D, seed)
    assert new, "the model holds no gammas"
    sd.update({k: torch.ones(D) for k in new} if ones else new)
    m.load_state_dict(sd)
    return m.to(DEV).train(), sd


def make_vit(p=0.0, init=INIT, rate=None, ones=False, seed=5):
    from vit_core import ViT
    torch.manual_seed(seed)
    extra = ({} if init is None else {"layer_scale_init": init}) | ({} if rate is None else {"drop_path_rate": rate})
    m = ViT(num_classes=CLASSES, num_blocks=BLOCKS, input_shape=(3, IMG, IMG), embed_dim=D, patch_size=PATCH, num_heads=H, mlp_dim=F,
            dropout=p, **extra)
    if init is None:
        return m.to(DEV).train(), {k: v.detach().clone() for k, v in m.state_dict().items()}
    return with_gammas(m, ones)


def dropout_keeps(p, seed, nb, tokens, tab=None):
    """the oracle's base keep triples: exported dropout masks (p > 0) times a drop-path table (or ones)"""
    from vitssl_hip import ops
    dk = None
    if p > 0:
        dk = [[ops.dropout_mask(nb * tokens, cols, ops.make_dropout(p, seed, 3 * i + which), DEV).float().cpu().view(nb, tokens, cols)
               for which, cols in ((0, D), (1, F), (2, D))] for i in range(BLOCKS)]
    if tab is None:
        tab = np.ones((2 * BLOCKS, nb), np.float32)
    return DP.oracle_keeps(tab, tokens, D, F, dk)


def vit_reference(sd, x, y, p, seed, tab=None, swap=None, training=True):
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    base = dropout_keeps(p if training else 0.0, seed, x.shape[0], T, tab)
    logits = LS.vit_forward(leaves, x, PATCH, H, D, F, base=base, p_drop=round(p * 65536) / 65536 if training else 0.0, swap=swap)
    loss = O.cross_entropy_mean(logits, y)
    loss.backward()
    return logits.detach(), float(loss.detach()), leaves


def vit_run(model, path, x, y, ms):
    torch.manual_seed(ms)
    if path == "autograd":
        logits = model(x.to(DEV))
        loss = torch.nn.functional.cross_entropy(logits, y.to(DEV))
        loss.backward()
        return logits.detach(), float(loss.detach()), {k: prm.grad for k, prm in model.named_parameters() if prm.grad is not None}
    rec = Recorder(model.flat_store())
    loss = model.train_step(x.to(DEV), y.to(DEV), rec)
    torch.cuda.synchronize()
    return model.last_logits.detach().clone(), float(loss), rec.grads()


def step_seed(ms):
    from vit_core import _runtime as R
    torch.manual_seed(ms)
    return R.next_seed()


# ------------------------------------------------------------------------------------------------ supervised ViT
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("path", ["autograd", "train_step"])
def test_vit_matches_the_oracle(path, p):
    model, sd = make_vit(p)
    assert model.runtime().bb.stack.layer_scale
    x, y = vit_batch()
    ms = 31
    logits, loss, grads = vit_run(model, path, x, y, ms)
    le, we, leaves = vit_reference(sd, x, y, p, step_seed(ms) if p else 0)
    fig = (rel_l2(logits, le), abs(loss - we) / abs(we), worst_grad(grads, leaves), worst_grad(grads, leaves, GAMMA_KEYS))
    print(f"ViT {path} p={p}: logits {fig[0]:.3g}, loss {fig[1]:.3g}, worst gradient {fig[2][0]:.3g} ({fig[2][1]}), "
          f"worst gamma gradient {fig[3][0]:.3g} ({fig[3][1]})")
    assert fig[0] < OUT_BAR and fig[1] < LOSS_BAR
    assert set(grads) == set(leaves) and set(GAMMA_KEYS) <= set(grads) and fig[2][0] < GRAD_BAR, fig[2]
    assert all(float(leaves[k].grad.abs().max()) > 0 for k in GAMMA_KEYS)


@pytest.mark.parametrize("path", ["autograd", "train_step"])
def test_vit_composes_with_drop_path(path):
    """drop_path_rate 0.2 (block rates 0, 0.1, 0.2) with dropout 0.1: the reference takes the table the engine exported"""
    rates = DP.rates(0.2, BLOCKS)
    model, sd = make_vit(0.1, rate=0.2)
    x, y = vit_batch()
    ms, seed = find_seed([B], rates=rates)
    logits, loss, grads = vit_run(model, path, x, y, ms)
    stack = model.runtime().bb.stack
    want = DP.table(rates, B, seed, stack.site_base)
    got = stack.drop_path_table("a")
    assert DP.mixed(want, rates) and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    le, we, leaves = vit_reference(sd, x, y, 0.1, seed, tab=want)
    fig = (rel_l2(logits, le), abs(loss - we) / abs(we), worst_grad(grads, leaves))
    print(f"ViT {path} with drop path: logits {fig[0]:.3g}, loss {fig[1]:.3g}, worst gradient {fig[2][0]:.3g} ({fig[2][1]})")
    assert fig[0] < OUT_BAR and fig[1] < LOSS_BAR and fig[2][0] < GRAD_BAR, fig


@pytest.mark.parametrize("block", [0, 2])
def test_reference_with_swapped_gammas_exceeds_the_gradient_bar(block):
    """negative control: the same comparison with g1 / g2 of one block exchanged in the REFERENCE must fail"""
    model, sd = make_vit(0.0)
    x, y = vit_batch()
    _, _, grads = vit_run(model, "autograd", x, y, 31)
    _, _, leaves = vit_reference(sd, x, y, 0.0, 0)
    assert worst_grad(grads, leaves)[0] < GRAD_BAR
    _, _, swapped = vit_reference(sd, x, y, 0.0, 0, swap=block)
    assert worst_grad(grads, swapped)[0] > GRAD_BAR


def test_eval_and_validation_apply_gamma():
    model, sd = make_vit(0.1)
    ones, _ = make_vit(0.1, ones=True)
    x, y = vit_batch()
    xd, yd = x.to(DEV), y.to(DEV)
    le, we, _ = vit_reference(sd, x, y, 0.1, 0, training=False)
    for m in (model, ones):
        m.eval()
    with torch.no_grad():
        a, b = model(xd), ones(xd)
    assert rel_l2(a, le) < OUT_BAR and rel_l2(b, le) > OUT_BAR and not torch.equal(a, b)
    loss = model.eval_step(xd, yd)
    assert rel_l2(model.last_logits, le) < OUT_BAR and abs(float(loss) - we) < LOSS_BAR * abs(we)
    assert torch.equal(model.last_logits, a)                                 # validation and the eval forward: the same launches
    model.train()
    with torch.no_grad():                                                    # a non-saving training forward applies it too
        torch.manual_seed(31)
        c = model(xd)
    le_t, _, _ = vit_reference(sd, x, y, 0.1, step_seed(31))
    assert rel_l2(c, le_t) < OUT_BAR


@pytest.mark.parametrize("sched", ["input_grad", "head"])
def test_frozen_backbone_schedules(sched):
    from utils.model_builder import freeze_backbone
    model, sd = make_vit(0.0)
    freeze_backbone(model)
    if sched == "head":
        model.patch_embedding.cls_token.requires_grad = False
    assert model.runtime().schedule() == sched
    x, y = vit_batch()
    logits, loss, grads = vit_run(model, "train_step", x, y, 31)
    le, we, leaves = vit_reference(sd, x, y, 0.0, 0)
    trained = [k for k, prm in model.named_parameters() if prm.requires_grad]
    assert trained and not any("layer_scale" in k for k in trained)
    assert rel_l2(logits, le) < OUT_BAR and abs(loss - we) < LOSS_BAR * abs(we)
    w = worst_grad(grads, leaves, trained)
    print(f"frozen backbone, {sched}: worst trained gradient {w[0]:.3g} ({w[1]})")
    assert w[0] < GRAD_BAR, w


def test_fused_adamw_step_moves_the_gammas_by_the_oracles_rule():
    """one fused step with the recipes' rules (no weight decay on 1-D parameters, layer-wise lr decay): every gamma moves to
    oracle.adamw_step(gamma, gradient, step 1, lr * decay^(L + 1 - (i + 1)), wd 0).  Bar: the update is computed in fp32 and added to
    a gamma of magnitude [0.5, 1.5]: half an ulp of the result (2^-24 .. 2^-23) plus the fp32 error of an update of size lr = 1e-3,
    orders below; 2 ulp of 1.5 = 2.4e-7."""
    from vitssl_hip.engine import exempt_from_weight_decay, layer_id, num_layers
    from vitssl_hip.optim import FusedAdamW
    lr, wd, decay = 1e-3, 0.05, 0.65
    a, _ = make_vit(0.0)
    b = copy.deepcopy(a)
    x, y = vit_batch()
    st = a.flat_store()
    layers = num_layers(st.names)
    ndim = {n: p.dim() for n, p in zip(st.names, st.params)}
    scale = lambda n: decay ** (layers + 1 - layer_id(n, layers))            # noqa: E731
    wdof = lambda n: 0.0 if exempt_from_weight_decay(n, ndim[n]) else wd     # noqa: E731
    assert all(wdof(k) == 0.0 and scale(k) == decay ** (layers - int(k.split(".")[1])) for k in GAMMA_KEYS)
    opt = FusedAdamW(st, lr=lr, weight_decay=wd, lr_scale=scale, weight_decay_of=wdof)
    rec = Recorder(b.flat_store())
    b.train_step(x.to(DEV), y.to(DEV), rec)
    before = {k: st.view(k).detach().cpu().double().clone() for k in GAMMA_KEYS}
    a.train_step(x.to(DEV), y.to(DEV), opt)
    torch.cuda.synchronize()
    grads = rec.grads()
    for k in GAMMA_KEYS:
        g = grads[k].detach().cpu().double()
        want, _, _ = O.adamw_step(before[k], g, torch.zeros_like(g), torch.zeros_like(g), 1, lr * scale(k), wd=0.0)
        got = st.view(k).detach().cpu().double()
        assert float((got - before[k]).abs().min()) > 0.5 * lr * scale(k), k    # the first Adam step moves every element by ~lr
        assert float((got - want).abs().max()) <= 2.4e-7, k
        assert torch.equal(a.state_dict()[k].cpu().double(), got)            # the gammas are in the state_dict


def test_without_the_key_everything_is_bit_identical():
    """logits, loss, every gradient and the torch generator state of a model built with layer_scale_init=None against one built
    without the keyword, dropout on; neither holds a gamma nor launches the LayerScale entries"""
    x, y = vit_batch()
    xd, yd = x.to(DEV), y.to(DEV)
    plain, _ = make_vit(0.1, init=None)
    torch.manual_seed(5)
    from vit_core import ViT
    none = ViT(num_classes=CLASSES, num_blocks=BLOCKS, input_shape=(3, IMG, IMG), embed_dim=D, patch_size=PATCH, num_heads=H, mlp_dim=F,
               dropout=0.1, layer_scale_init=None).to(DEV).train()
    assert list(none.state_dict()) == list(plain.state_dict()) and not none.runtime().bb.stack.layer_scale
    from vitssl_hip import ops
    calls = []
    orig = ops.call
    ops.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        outs = []
        for m in (plain, none):
            torch.manual_seed(11)
            out = m(xd)
            loss = torch.nn.functional.cross_entropy(out, yd)
            loss.backward()
            rec = Recorder(m.flat_store())
            torch.manual_seed(12)
            l2 = m.train_step(xd, yd, rec)
            outs.append((out.detach(), loss.detach(), {k: prm.grad.clone() for k, prm in m.named_parameters()}, l2, rec.gflat, _gen_state()))
    finally:
        ops.call = orig
    (o1, l1, g1, t1, f1, s1), (o2, l2, g2, t2, f2, s2) = outs
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and all(torch.equal(g1[k], g2[k]) for k in g1) and set(g1) == set(g2)
    assert torch.equal(t1, t2) and torch.equal(f1, f2) and torch.equal(s1, s2)
    assert calls and not any(n.endswith("_ls") for n in calls)


def test_fp8_operands_with_the_key_are_refused():
    from vitssl_hip import VitsslError
    from vitssl_hip import engine as E
    model, _ = make_vit(0.0)
    plain, _ = make_vit(0.0, init=None)
    E.set_linear_operands("fp8")
    try:
        with pytest.raises(VitsslError, match="bf16"):
            model.runtime(DEV)
        assert plain.runtime(DEV).bb.stack.fp8
    finally:
        E.set_linear_operands("bf16")


# ------------------------------------------------------------------------------------------------ SimMIM
def make_simmim(p, ones=False):
    from vit_core.ssl.simmim import SimMIMViT
    torch.manual_seed(5)
    m = SimMIMViT(num_blocks=BLOCKS, input_shape=(3, IMG, IMG), embed_dim=D, patch_size=PATCH, num_heads=H, mlp_dim=F, dropout=p,
                  mask_ratio=0.6, layer_scale_init=INIT)
    return with_gammas(m, ones)


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("path", ["autograd", "train_step"])
def test_simmim_matches_the_oracle(path, p):
    from vit_core import _runtime as R
    from vit_core.ssl.simmim.masking import draw_mask
    N = (IMG // PATCH) ** 2
    model, sd = make_simmim(p)
    x = torch.rand(B, 3, IMG, IMG, generator=torch.Generator().manual_seed(6))
    if path == "autograd":                                                   # the model draws its mask, then the step seed
        torch.manual_seed(41)
        mask = draw_mask(B, N, 0.6)
        seed = R.next_seed() if p else 0
        torch.manual_seed(41)
        pred, tgt = model(x.to(DEV))
        loss = torch.nn.functional.l1_loss(pred, tgt)
        loss.backward()
        grads = {k: prm.grad for k, prm in model.named_parameters()}
    else:
        torch.manual_seed(91)
        mask = draw_mask(B, N, 0.6)
        seed = step_seed(42) if p else 0
        torch.manual_seed(42)
        rec = Recorder(model.flat_store())
        loss = model.train_step(x.to(DEV), rec, mask_cpu=mask)
        torch.cuda.synchronize()
        grads, pred, tgt = rec.grads(), model.last_pred, model.last_targets
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pe, te = LS.simmim_forward(leaves, x, mask, PATCH, H, D, F, base=dropout_keeps(p, seed, B, N), p_drop=round(p * 65536) / 65536)
    assert torch.equal(tgt.cpu(), te)
    wl = float(O.l1_loss_mean(pe, te).detach())
    l1_backward_with_signs(pe, te, pred, tgt)
    fig = (rel_l2(pred, pe), abs(float(loss.detach()) - wl) / wl, worst_grad(grads, leaves), worst_grad(grads, leaves, GAMMA_KEYS))
    print(f"SimMIM {path} p={p}: pred {fig[0]:.3g}, loss {fig[1]:.3g}, worst gradient {fig[2][0]:.3g} ({fig[2][1]}), gamma {fig[3][0]:.3g}")
    assert fig[0] < OUT_BAR and fig[1] < LOSS_BAR and fig[2][0] < GRAD_BAR, fig


def test_simmim_inference_forward_applies_gamma():
    model, sd = make_simmim(0.1)
    ones, _ = make_simmim(0.1, ones=True)
    x = torch.rand(B, 3, IMG, IMG, generator=torch.Generator().manual_seed(6))
    for feats in (False, True):
        want = LS.simmim_inference(sd, x, PATCH, H, D, F, return_patch_features=feats)
        got, other = model.inference_forward(x.to(DEV), return_patch_features=feats), ones.inference_forward(x.to(DEV), return_patch_features=feats)
        assert rel_l2(got, want) < OUT_BAR and rel_l2(other, want) > OUT_BAR


# ------------------------------------------------------------------------------------------------ DINO
def make_dino(ones=False):
    from vit_core.ssl.dino import DINOViT
    torch.manual_seed(5)
    m = DINOViT(num_blocks=BLOCKS, input_shape=(3, IMG, IMG), embed_dim=D, patch_size=PATCH, num_heads=H, mlp_dim=F, dropout=0.0,
                output_dim=256, center_momentum=0.9, layer_scale_init=INIT)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    new = LS.random_gammas(sd, D, 21, "student_backbone.") | LS.random_gammas(sd, D, 22, "teacher_backbone.")      # the two stacks differ
    assert len(new) == 4 * BLOCKS
    sd.update({k: torch.ones(D) for k in new} if ones else new)
    m.load_state_dict(sd)
    return m.to(DEV).train(), sd


def test_dino_student_and_teacher_match_the_oracle_and_the_ema_moves_the_teacher_gammas():
    nb, G = 2, 2
    model, sd = make_dino()
    views = dino_views(nb)
    rt = model.runtime()
    assert rt.bb["student"].stack.layer_scale and rt.bb["teacher"].stack.layer_scale
    w = torch.randn(4 * nb, 256, generator=torch.Generator().manual_seed(9))
    teacher, student = model([v.to(DEV) for v in views], G)
    (student * w.to(DEV)).sum().backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    grid = (IMG // PATCH, IMG // PATCH)
    se = torch.cat([LS.dino_branch(leaves, "student", torch.cat(views[:G]), PATCH, H, grid, D, F),
                    LS.dino_branch(leaves, "student", torch.cat(views[G:]), PATCH, H, grid, D, F)])
    with torch.no_grad():
        te = LS.dino_branch(sd, "teacher", torch.cat(views[:G]), PATCH, H, grid, D, F)
    (se * w).sum().backward()
    grads = {k: prm.grad for k, prm in model.named_parameters() if k.startswith("student_")}
    names = list(grads)
    gam = [k for k in names if "layer_scale" in k]
    assert len(gam) == 2 * BLOCKS and all(grads[k] is not None for k in names)
    assert all(prm.grad is None for k, prm in model.named_parameters() if k.startswith("teacher_"))
    fig = (rel_l2(student, se), rel_l2(teacher, te), worst_grad(grads, leaves, names), worst_grad(grads, leaves, gam))
    print(f"DINO: student {fig[0]:.3g}, teacher {fig[1]:.3g}, worst gradient {fig[2][0]:.3g} ({fig[2][1]}), gamma {fig[3][0]:.3g}")
    assert fig[0] < OUT_BAR and fig[1] < OUT_BAR and fig[2][0] < GRAD_BAR, fig
    # the teacher applies ITS gammas: with the student's it misses the bar
    swapped = dict(sd)
    for k in sd:
        if k.startswith("teacher_backbone.") and "layer_scale" in k:
            swapped[k] = sd[k.replace("teacher_", "student_")]
    with torch.no_grad():
        assert rel_l2(teacher, LS.dino_branch(swapped, "teacher", torch.cat(views[:G]), PATCH, H, grid, D, F)) > OUT_BAR
    # inference_forward runs the teacher with its gammas
    with torch.no_grad():
        got = model.inference_forward(views[0].to(DEV))
        want = LS.dino_branch(sd, "teacher", views[0], PATCH, H, grid, D, F)
    assert rel_l2(got, want) < OUT_BAR
    # EMA: theta_t <- m theta_t + (1 - m) theta_s, the gammas like every parameter
    model.momentum_update_teacher(0.9)
    new = model.state_dict()
    for i in range(BLOCKS):
        for k in (1, 2):
            t, s = (f"{who}_backbone.encoder_blocks.{i}.layer_scale{k}.gamma" for who in ("teacher", "student"))
            want = O.ema_update(sd[t].double(), sd[s].double(), 0.9)
            assert float((new[t].cpu().double() - want).abs().max()) < 1e-6 and not torch.equal(new[t].cpu(), sd[t])


# ------------------------------------------------------------------------------------------------ a lone block
def test_encoder_block_on_its_own_matches_the_oracle():
    from vit_core import EncoderBlock
    Tn = 20
    torch.manual_seed(8)
    blk = EncoderBlock(D, H, F, 0.0, layer_scale_init=INIT)
    blk, sd = with_gammas(blk)
    x = torch.randn(B, Tn, D, generator=torch.Generator().manual_seed(9))
    w = torch.randn(B, Tn, D, generator=torch.Generator().manual_seed(10))
    xg = x.to(DEV).requires_grad_(True)
    yb, _ = blk(xg)
    (yb * w.to(DEV)).sum().backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    ye = LS.block_forward(leaves, xo, H, D, F)
    (ye * w).sum().backward()
    assert rel_l2(yb, ye) < OUT_BAR and rel_l2(xg.grad, xo.grad) < GRAD_BAR
    got = {k: prm.grad for k, prm in blk.named_parameters()}
    assert {"layer_scale1.gamma", "layer_scale2.gamma"} <= set(got)
    assert worst_grad(got, leaves)[0] < GRAD_BAR
