"""ViT(global_pool="avg") through every path that ends in the classification head, against tests/_pool_ref.py's restatement of
the oracle (emu="bf16", cross_entropy_mean) at the project's ViT bars (tests/test_gpu_round2.py, README round 4): logits
rel_l2 < 1e-2, every parameter gradient 2e-2, the loss 1e-2 relative.

Models: D = 64, two blocks, one head, at T = 10 (3 images) and T = 257 (2 images, the streaming attention); D = 192, three heads,
at T = 197.  The reference of a model (logits, loss, gradients; the `cls` logits for the negative control) is computed once and
only read afterwards.  fp8 operands: logits of a D = 128 model against the restatement's emu="fp8" at the band
tests/test_gpu_fp8.py holds model outputs to (rel_l2 < 1e-2, test_simmim_fp8_matches_oracle_and_trains)."""
import functools

import pytest
import torch

import _pool_ref as PR
from _util import rel_l2
from oracle import vit_oracle as O
from test_gpu_classify import Recorder, fused_grads

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOGITS_BAR, GRAD_BAR, LOSS_BAR = 1e-2, 2e-2, 1e-2
CLASSES = 10
# name -> (constructor keywords, images)
MODELS = {
    "T10": (dict(num_blocks=2, input_shape=(3, 24, 24), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=128), 3),
    "T257": (dict(num_blocks=2, input_shape=(3, 128, 128), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=128), 2),
    "T197-D192": (dict(num_blocks=2, input_shape=(3, 112, 112), embed_dim=192, patch_size=8, num_heads=3, mlp_dim=384), 2),
}
NAMES = list(MODELS)


def build(name, dropout=0.0, global_pool="avg", seed=17, **kw):
    from vit_core.vit import ViT
    torch.manual_seed(seed)
    return ViT(num_classes=CLASSES, dropout=dropout, global_pool=global_pool, **{**MODELS[name][0], **kw})


@functools.lru_cache(maxsize=None)
def fixed(name):
    """-> (state dict, x, labels, reference): built once, only read afterwards"""
    kw, B = MODELS[name]
    sd = {k: v.detach().clone() for k, v in build(name).state_dict().items()}
    g = torch.Generator().manual_seed(23)
    x, y = torch.rand(B, *kw["input_shape"], generator=g), torch.randint(0, CLASSES, (B,), generator=g)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logits = PR.vit_forward(leaves, x, kw["patch_size"], kw["num_heads"], "avg", "bf16")
    loss = O.cross_entropy_mean(logits, y)
    loss.backward()
    with torch.no_grad():
        cls = PR.vit_forward(sd, x, kw["patch_size"], kw["num_heads"], "cls", "bf16")
    ref = dict(logits=logits.detach(), loss=float(loss.detach()), grads={k: v.grad.clone() for k, v in leaves.items()}, cls_logits=cls)
    return sd, x, y, ref


def on_gpu(name, **kw):
    sd, x, y, ref = fixed(name)
    m = build(name, **kw)
    m.load_state_dict(sd, strict="layer_scale_init" not in kw)                  # (LayerScale adds its gammas: they keep their initial value)
    return m.to(DEV).train(), x.to(DEV), y.to(DEV), ref


def worst_grad(got, ref, names):
    """(largest relative L2 distance, the parameter it belongs to)"""
    return max((rel_l2(got[n], ref[n]), n) for n in names)


@pytest.mark.parametrize("name", NAMES)
def test_autograd_path_against_the_restatement_and_the_negative_control(name):
    m, x, y, ref = on_gpu(name)
    logits, probs = m(x, return_attn=True)
    T = (MODELS[name][0]["input_shape"][1] // 8) ** 2 + 1
    assert logits.shape == (x.shape[0], CLASSES) and probs.shape[-2:] == (T, T)
    d_avg, d_cls = rel_l2(logits, ref["logits"]), rel_l2(logits, ref["cls_logits"])
    loss = torch.nn.functional.cross_entropy(logits, y)
    loss.backward()
    loss = loss.detach()
    got = {n: p.grad for n, p in m.named_parameters()}
    assert set(got) == set(ref["grads"]) and all(g is not None for g in got.values())
    worst = worst_grad(got, ref["grads"], got)
    print(f"{name}: logits {d_avg:.3g} from the avg restatement, {d_cls:.3g} from the cls one; loss {float(loss):.6g} (ref {ref['loss']:.6g}); "
          f"largest relative L2 of a parameter gradient {worst[0]:.3g} ({worst[1]})")
    assert d_avg < LOGITS_BAR, d_avg
    assert d_cls > LOGITS_BAR, f"the test cannot tell avg from cls: {d_cls}"
    assert abs(float(loss) - ref["loss"]) < LOSS_BAR * abs(ref["loss"])
    assert worst[0] < GRAD_BAR, worst
    # the CLS token still trains: it is a key and a value of every patch token's attention
    assert float(got["patch_embedding.cls_token"].abs().max()) > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_the_default_mode_is_the_cls_model(name):
    m, x, y, ref = on_gpu(name, global_pool="cls")
    with torch.no_grad():
        logits = m(x)
    assert rel_l2(logits, ref["cls_logits"]) < LOGITS_BAR and rel_l2(logits, ref["logits"]) > LOGITS_BAR


@pytest.mark.parametrize("name", NAMES)
def test_fused_train_step_and_eval_step(name):
    m, x, y, ref = on_gpu(name)
    loss, got, rec = fused_grads(m, x, y)
    st = m.flat_store()
    assert set(got) == set(ref["grads"]) == set(st.names)
    worst = worst_grad(got, ref["grads"], got)
    d = rel_l2(m.last_logits, ref["logits"])
    print(f"{name}: train_step loss {loss:.6g} (ref {ref['loss']:.6g}), logits {d:.3g}, largest relative L2 of a gflat slice {worst[0]:.3g} ({worst[1]})")
    assert abs(loss - ref["loss"]) < LOSS_BAR * abs(ref["loss"]) and d < LOGITS_BAR
    assert worst[0] < GRAD_BAR, worst
    ev = m.eval_step(x, y)
    step_logits = m.last_logits.clone()
    m.eval()
    with torch.no_grad():
        logits = m(x)
    m.train()
    assert torch.equal(step_logits.view(torch.int32), logits.view(torch.int32)), "eval_step and the eval-mode forward give other bits"
    assert abs(float(ev) - float(torch.nn.functional.cross_entropy(logits, y))) <= 1e-5 * abs(float(ev))


@pytest.mark.parametrize("name", ["T10", "T197-D192"])
def test_two_identical_steps_with_dropout_give_the_same_bits(name):
    runs = []
    for _ in range(2):
        m, x, y, _ = on_gpu(name, dropout=0.1, drop_path_rate=0.1, layer_scale_init=0.1)
        torch.manual_seed(5)                                                    # the source of the dropout and drop-path keys
        loss, _, rec = fused_grads(m, x, y, label_smoothing=0.1, loss="bce")
        runs.append((loss, rec.gflat.cpu().view(torch.int32).clone(), m.last_logits.cpu().contiguous().view(torch.int32).clone()))
    (la, ga, za), (lb, gb, zb) = runs
    assert la == lb and torch.equal(ga, gb) and torch.equal(za, zb) and ga.any()
    m, x, y, _ = on_gpu(name, dropout=0.1, drop_path_rate=0.1, layer_scale_init=0.1)
    torch.manual_seed(6)
    _, _, rec = fused_grads(m, x, y, label_smoothing=0.1, loss="bce")
    assert not torch.equal(rec.gflat.cpu().view(torch.int32), ga)               # and another seed is another step


def test_mixup_composes_with_the_pooled_head():
    """the autograd path on the same mixed batch with dense targets, as tests/test_gpu_mixup_models.py compares the cls model"""
    from data import GPUMixup, MixSpec
    m, x, y, _ = on_gpu("T10")
    a, _, _, _ = on_gpu("T10")
    mixer = GPUMixup(MixSpec(mode="elem"))
    params = mixer.draw(x.shape[0], x.shape[-2], x.shape[-1], torch.Generator().manual_seed(3))
    lam = params.lam[:, None]
    onehot = lambda lab: torch.nn.functional.one_hot(lab, CLASSES).float()      # noqa: E731
    dense = lam * onehot(y) + (1.0 - lam) * onehot(y[params.partner.long()])
    logp = torch.log_softmax(a(mixer.apply(x, params)), dim=1)
    la = -(dense * logp).sum(1).mean()
    la.backward()
    la = la.detach()
    ga = {n: p.grad for n, p in a.named_parameters()}
    lb, gb, _ = fused_grads(m, x, y, mix=params)
    assert abs(float(la) - lb) <= 1e-5 * abs(float(la))
    worst = worst_grad(gb, ga, ga)
    assert worst[0] < GRAD_BAR, worst


@pytest.mark.parametrize("sched", ["input_grad", "head"])
@pytest.mark.parametrize("name", ["T10", "T257"])
def test_frozen_backbone_schedules(name, sched):
    from utils.model_builder import freeze_backbone
    m, x, y, ref = on_gpu(name)
    freeze_backbone(m)
    if sched == "head":
        m.patch_embedding.cls_token.requires_grad = False
    rt, st = m.runtime(), m.flat_store()
    assert rt.schedule() == sched
    loss, got, rec = fused_grads(m, x, y)
    trainable = [n for n, p in m.named_parameters() if p.requires_grad]
    assert set(trainable) == {n for n in st.names if n.startswith("classification_head.")} | ({"patch_embedding.cls_token"} if sched == "input_grad" else set())
    worst = worst_grad(got, ref["grads"], trainable)
    print(f"{name}, {sched}: loss {loss:.6g} (ref {ref['loss']:.6g}), largest relative L2 of a trainable gradient {worst[0]:.3g} ({worst[1]})")
    assert abs(loss - ref["loss"]) < LOSS_BAR * abs(ref["loss"])
    assert worst[0] < GRAD_BAR, worst
    # the frozen slices of gflat: "head" writes nothing outside the head; "input_grad" launches no weight-gradient GEMM, so every
    # frozen matrix stays zero (the frozen bias / LayerNorm / position-table slices there are by-products of the fused
    # input-gradient kernels, as with the CLS head: tests/test_gpu_classify.py; the optimizer step below shows that they move nothing)
    for n, p in m.named_parameters():
        if not p.requires_grad and (sched == "head" or n == "patch_embedding.conv.weight" or (n.startswith("encoder_blocks.") and p.dim() == 2)):
            assert not got[n].any(), f"the frozen slice {n} of gflat is not zero"
    if sched == "head":
        assert "a" not in rt.bb.stack._saved and "a" not in rt.bb.rec
    # the autograd path of the frozen model: the same trainable gradients
    for p in m.parameters():
        p.grad = None
    torch.nn.functional.cross_entropy(m(x), y).backward()
    auto = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
    assert set(auto) == set(trainable)
    worst = worst_grad(auto, ref["grads"], trainable)
    assert worst[0] < GRAD_BAR, worst
    # and an optimizer step moves what trains, nothing else
    from vitssl_hip.optim import FusedAdamW
    before = st.flat.clone()
    m.train_step(x, y, FusedAdamW(st, lr=1e-3, weight_decay=1e-2))
    torch.cuda.synchronize()
    for n, p in zip(st.names, st.params):
        o, cnt = st.offsets[n]
        assert torch.equal(st.flat[o:o + cnt], before[o:o + cnt]) != p.requires_grad, n      # frozen: bit-unchanged; trainable: moved


def test_an_mae_checkpoint_lands_in_the_pooled_vit(tmp_path):
    from utils.model_builder import load_weights
    from vit_core.ssl.mae.model import MAEViT
    torch.manual_seed(41)
    mae = MAEViT(num_blocks=2, input_shape=(3, 24, 24), embed_dim=64, patch_size=8, num_heads=1, mlp_dim=128, decoder_embed_dim=64,
                 decoder_blocks=1, decoder_heads=2)
    path = tmp_path / "mae.pth"
    torch.save({"model_state_dict": mae.state_dict()}, path)
    vit = build("T10", seed=43)
    fresh = {k: v.detach().clone() for k, v in vit.state_dict().items()}
    load_weights(vit, str(path))
    sd = {k: v.detach().clone() for k, v in vit.state_dict().items()}
    assert torch.equal(sd["patch_embedding.conv.weight"].reshape(64, -1), mae.projection.weight.detach())
    assert torch.equal(sd["encoder_blocks.1.feed_forward.linear_out.weight"], mae.encoder_blocks[1].feed_forward.linear_out.weight.detach())
    assert not torch.equal(sd["encoder_blocks.0.feed_forward.linear_in.weight"], fresh["encoder_blocks.0.feed_forward.linear_in.weight"])
    for k in sd:                                                                # the head, its norm (MAE's fc_norm) included, is untouched
        if k.startswith("classification_head."):
            assert torch.equal(sd[k], fresh[k]), k
    assert torch.equal(sd["classification_head.norm.weight"], torch.ones(64)) and not sd["classification_head.norm.bias"].any()
    x = torch.rand(3, 3, 24, 24, generator=torch.Generator().manual_seed(2))
    vit = vit.to(DEV).eval()
    with torch.no_grad():
        logits = vit(x.to(DEV))
        want, other = PR.vit_forward(sd, x, 8, 1, "avg", "bf16"), PR.vit_forward(sd, x, 8, 1, "cls", "bf16")
    assert rel_l2(logits, want) < LOGITS_BAR and rel_l2(logits, other) > LOGITS_BAR


def test_fp8_operands_against_the_fp8_restatement():
    from vitssl_hip import engine
    kw = dict(num_blocks=2, input_shape=(3, 64, 64), embed_dim=128, patch_size=16, num_heads=2, mlp_dim=256)
    from vit_core.vit import ViT
    torch.manual_seed(11)
    m = ViT(num_classes=CLASSES, dropout=0.0, global_pool="avg", **kw)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    x = torch.rand(4, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    y = torch.randint(0, CLASSES, (4,), generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        want = PR.vit_forward(sd, x, 16, 2, "avg", "fp8")
        other = PR.vit_forward(sd, x, 16, 2, "cls", "fp8")
    engine.set_linear_operands("fp8")
    try:
        m = m.to(DEV).train()
        logits = m(x.to(DEV))
        d, dc = rel_l2(logits, want), rel_l2(logits, other)
        print(f"fp8 operands: logits {d:.3g} from the avg restatement (emu=fp8), {dc:.3g} from the cls one")
        assert d < 1e-2 and dc > 1e-2                                           # the band of tests/test_gpu_fp8.py for a model's output
        torch.nn.functional.cross_entropy(logits, y.to(DEV)).backward()        # and the backward runs: every gradient arrives, finite
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()) for p in m.parameters())
        rec = Recorder(m.flat_store())
        assert bool(torch.isfinite(m.train_step(x.to(DEV), y.to(DEV), rec)))
    finally:
        engine.set_linear_operands("bf16")
