"""Stochastic depth (drop_path_rate) in the three models against the CPU oracle.

The unchanged oracle expresses drop path: oracle.vit_oracle.encoder_block multiplies the two residual branches by arbitrary float
tensors keep[0] / keep[2], so the reference is the oracle called with keep1 * s_att[b] and keep2 * s_mlp[b] broadcast over
[B, T, 1] (tests/_droppath_ref.py), s from the table of branch scales the engine exported, which is also compared with the NumPy
restatement of the stream.

Tiny shapes: 5 images of 64 x 64, patch 16, D = 128, 2 heads, 3 blocks (first / middle / last block each take their own branch of
EncoderStack.backward), rate 0.5 (block rates 0, 0.25, 0.5).  The step seed is chosen on the CPU so that every block with a
nonzero rate has a dropped and a kept sample in each branch (asserted).  Bars as in tests/test_gpu_models.py against the oracle's
bf16-rounding emulation: outputs 1e-2, loss 1e-2 relative, every gradient 2e-2 rel-L2."""
import numpy as np
import pytest
import torch

import _droppath_ref as DP
from _util import l1_backward_with_signs, rel_l2
from oracle import vit_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, IMG, PATCH, D, H, F, BLOCKS, RATE, CLASSES = 5, 64, 16, 128, 2, 256, 3, 0.5, 10
RATES = DP.rates(RATE, BLOCKS)
OUT_BAR, LOSS_BAR, GRAD_BAR = 1e-2, 1e-2, 2e-2


class Recorder:
    """optimizer stub: keeps the flat gradient buffer the fused step hands to step_flat"""

    def __init__(self, store):
        self.store, self.gflat = store, None

    def step_flat(self, gscale=1.0):
        self.gflat = self.store.gflat.clone()

    def grads(self):
        st = self.store
        return {n: self.gflat[st.offsets[n][0]:st.offsets[n][0] + st.offsets[n][1]].view(p.shape) for n, p in zip(st.names, st.params)}


def find_seed(nb, prelude=lambda: None, offsets=(0,), start=1, rates=RATES):
    """(manual seed, step seed): after torch.manual_seed(ms) and `prelude()` (what the model draws first), next_seed() gives a step seed
    whose tables (one per seed offset) hold a kept and a dropped sample in every branch of every block with a nonzero rate"""
    from vit_core import _runtime as R
    for ms in range(start, start + 100000):
        torch.manual_seed(ms)
        prelude()
        seed = R.next_seed()
        if all(DP.mixed(DP.table(rates, n, seed + o), rates) for n, o in zip(nb, offsets)):
            return ms, seed
    raise AssertionError("no seed found")


def keeps_for(tab, T, p, seed, nb):
    """oracle keeps of one pass: exported dropout masks (p > 0) times the table's branch scales"""
    from vitssl_hip import ops
    dk = None
    if p > 0:
        dk = [[ops.dropout_mask(nb * T, cols, ops.make_dropout(p, seed, 3 * i + which), DEV).float().cpu().view(nb, T, cols)
               for which, cols in ((0, D), (1, F), (2, D))] for i in range(BLOCKS)]
    return DP.oracle_keeps(tab, T, D, F, dk)


def check_table(stack, slot, seed, nb):
    """the table the forward applied == the restatement for the step seed, and it is mixed"""
    want = DP.table(RATES, nb, seed, stack.site_base)
    assert DP.mixed(want, RATES)
    got = stack.drop_path_table(slot)
    assert got is not None and np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    return want


def worst_grad(got, want, names=None):
    return max((rel_l2(got[k], want[k].grad), k) for k in (names if names is not None else want))


# ------------------------------------------------------------------------------------------------ supervised ViT
def make_vit(p=0.0, rate=RATE, seed=5, **kw):
    from vit_core import ViT
    torch.manual_seed(seed)
    m = ViT(num_classes=CLASSES, num_blocks=BLOCKS, input_shape=(3, IMG, IMG), embed_dim=D, patch_size=PATCH, num_heads=H, mlp_dim=F,
            dropout=p, **({} if rate is None else {"drop_path_rate": rate}), **kw)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).train(), sd


def vit_batch():
    g = torch.Generator().manual_seed(6)
    return torch.rand(B, 3, IMG, IMG, generator=g), torch.randint(0, CLASSES, (B,), generator=g)


def vit_reference(sd, x, y, tab, p, seed, swap=None):
    T = (IMG // PATCH) ** 2 + 1
    tab = np.array(tab)
    if swap is not None:                                                     # negative control: one block's two rows exchanged
        tab[[2 * swap, 2 * swap + 1]] = tab[[2 * swap + 1, 2 * swap]]
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    logits = DP.vit_forward(leaves, x, PATCH, H, keeps_for(tab, T, p, seed, B), p_drop=round(p * 65536) / 65536)
    loss = O.cross_entropy_mean(logits, y)
    loss.backward()
    return logits.detach(), float(loss.detach()), leaves


def vit_run(model, path, x, y, ms):
    """one training forward + backward under torch.manual_seed(ms) -> (logits, loss, gradients by name)"""
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


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("path", ["autograd", "train_step"])
def test_vit_matches_the_oracle_with_the_exported_table(path, p):
    model, sd = make_vit(p)
    x, y = vit_batch()
    ms, seed = find_seed([B])
    logits, loss, grads = vit_run(model, path, x, y, ms)
    stack = model.runtime().bb.stack
    assert stack.drop_path == RATES
    tab = check_table(stack, "a", seed, B)
    le, we, leaves = vit_reference(sd, x, y, tab, p, seed)
    fig = (rel_l2(logits, le), abs(loss - we) / abs(we), worst_grad(grads, leaves))
    print(f"ViT {path} p={p}: logits {fig[0]:.3g}, loss {fig[1]:.3g}, worst gradient {fig[2][0]:.3g} ({fig[2][1]})")
    assert fig[0] < OUT_BAR and fig[1] < LOSS_BAR
    assert set(grads) == set(leaves) and fig[2][0] < GRAD_BAR, fig[2]


def test_vit_dropped_samples_leave_exact_zeros_in_the_branch_gradients():
    """a block whose every sample is dropped from both branches: exact zeros in every gradient of that block, none elsewhere"""
    from vitssl_hip import ops
    model, _ = make_vit(0.0)
    x, y = vit_batch()
    stack = model.runtime().bb.stack
    orig = ops.droppath_table

    def all_dropped_in_block_1(pairs, nb, seed, out):
        orig(pairs, nb, seed, out)
        out[2:4].zero_()
        return out
    ops.droppath_table = all_dropped_in_block_1
    try:
        torch.manual_seed(3)
        torch.nn.functional.cross_entropy(model(x.to(DEV)), y.to(DEV)).backward()
    finally:
        ops.droppath_table = orig
    assert not stack.drop_path_table("a")[2:4].any()
    for k, prm in model.named_parameters():
        if k.startswith("encoder_blocks.1."):                                 # (its LayerNorm parameters too: their branch gradient is zero)
            assert not prm.grad.any(), k
        elif k.startswith("encoder_blocks."):
            assert prm.grad.any(), k


@pytest.mark.parametrize("block", [1, 2])
def test_reference_with_swapped_tables_exceeds_the_gradient_bar(block):
    """negative control: the same comparison with the attention and MLP rows of one block exchanged in the REFERENCE must fail"""
    model, sd = make_vit(0.0)
    x, y = vit_batch()
    ms, seed = find_seed([B])
    for ms in range(ms, ms + 1000):                                          # ... and the two rows of that block must differ
        torch.manual_seed(ms)
        from vit_core import _runtime as R
        seed = R.next_seed()
        tab = DP.table(RATES, B, seed)
        if DP.mixed(tab, RATES) and not np.array_equal(tab[2 * block], tab[2 * block + 1]):
            break
    _, _, grads = vit_run(model, "autograd", x, y, ms)
    tab = check_table(model.runtime().bb.stack, "a", seed, B)
    _, _, leaves = vit_reference(sd, x, y, tab, 0.0, seed)
    assert worst_grad(grads, leaves)[0] < GRAD_BAR
    _, _, swapped = vit_reference(sd, x, y, tab, 0.0, seed, swap=block)
    assert worst_grad(grads, swapped)[0] > GRAD_BAR


@pytest.mark.parametrize("sched", ["input_grad", "head"])
def test_frozen_backbone_schedules(sched):
    """frozen backbone (CLS token trainable: the input-gradient chain without weight-gradient GEMMs) and head only (no backbone
    activations kept): the step runs and the trained parameters' gradients meet the bar"""
    from utils.model_builder import freeze_backbone
    model, sd = make_vit(0.0)
    freeze_backbone(model)
    if sched == "head":
        model.patch_embedding.cls_token.requires_grad = False
    assert model.runtime().schedule() == sched
    x, y = vit_batch()
    ms, seed = find_seed([B])
    logits, loss, grads = vit_run(model, "train_step", x, y, ms)
    tab = DP.table(RATES, B, seed)
    if sched == "input_grad":
        check_table(model.runtime().bb.stack, "a", seed, B)
    le, we, leaves = vit_reference(sd, x, y, tab, 0.0, seed)
    trained = [k for k, prm in model.named_parameters() if prm.requires_grad]
    assert trained and all(k.startswith("classification_head.") or k == "patch_embedding.cls_token" for k in trained)
    assert rel_l2(logits, le) < OUT_BAR and abs(loss - we) < LOSS_BAR * abs(we)
    w = worst_grad(grads, leaves, trained)
    print(f"frozen backbone, {sched}: worst trained gradient {w[0]:.3g} ({w[1]})")
    assert w[0] < GRAD_BAR, w


# ------------------------------------------------------------------------------------------------ SimMIM
@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
@pytest.mark.parametrize("path", ["autograd", "train_step"])
def test_simmim_matches_the_oracle_with_the_exported_table(path, p):
    from vit_core.ssl.simmim import SimMIMViT
    from vit_core.ssl.simmim.masking import draw_mask
    N = (IMG // PATCH) ** 2
    torch.manual_seed(5)
    model = SimMIMViT(num_blocks=BLOCKS, input_shape=(3, IMG, IMG), embed_dim=D, patch_size=PATCH, num_heads=H, mlp_dim=F, dropout=p,
                      mask_ratio=0.6, drop_path_rate=RATE)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.to(DEV).train()
    x = torch.rand(B, 3, IMG, IMG, generator=torch.Generator().manual_seed(6))
    if path == "autograd":                                                   # the model draws its mask, then the step seed
        ms, seed = find_seed([B], prelude=lambda: draw_mask(B, N, 0.6))
        torch.manual_seed(ms)
        mask = draw_mask(B, N, 0.6)
        torch.manual_seed(ms)
        pred, tgt = model(x.to(DEV))
        loss = torch.nn.functional.l1_loss(pred, tgt)
        loss.backward()
        grads = {k: prm.grad for k, prm in model.named_parameters()}
    else:
        torch.manual_seed(91)
        mask = draw_mask(B, N, 0.6)
        ms, seed = find_seed([B])
        torch.manual_seed(ms)
        rec = Recorder(model.flat_store())
        loss = model.train_step(x.to(DEV), rec, mask_cpu=mask)
        torch.cuda.synchronize()
        grads, pred, tgt = rec.grads(), model.last_pred, model.last_targets
    stack = model.runtime().stack
    tab = check_table(stack, "a", seed, B)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    pe, te = O.simmim_forward(leaves, x, mask, PATCH, H, emu="bf16", keeps=keeps_for(tab, N, p, seed, B), p_drop=round(p * 65536) / 65536)
    assert torch.equal(tgt.cpu(), te)
    wl = float(O.l1_loss_mean(pe, te).detach())
    l1_backward_with_signs(pe, te, pred, tgt)             # the engine's own d(loss)/d(pred) on both sides (_util.py)
    fig = (rel_l2(pred, pe), abs(float(loss.detach()) - wl) / wl, worst_grad(grads, leaves))
    print(f"SimMIM {path} p={p}: pred {fig[0]:.3g}, loss {fig[1]:.3g}, worst gradient {fig[2][0]:.3g} ({fig[2][1]})")
    assert fig[0] < OUT_BAR and fig[1] < LOSS_BAR and fig[2][0] < GRAD_BAR, fig


# ------------------------------------------------------------------------------------------------ DINO
def make_dino(rate, seed=5):
    from vit_core.ssl.dino import DINOViT
    torch.manual_seed(seed)
    m = DINOViT(num_blocks=BLOCKS, input_shape=(3, IMG, IMG), embed_dim=D, patch_size=PATCH, num_heads=H, mlp_dim=F, dropout=0.0,
                output_dim=256, center_momentum=0.9, **({} if rate is None else {"drop_path_rate": rate}))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m.to(DEV).train(), sd


def dino_views(nb=2):
    g = torch.Generator().manual_seed(8)
    return [torch.rand(nb, 3, IMG, IMG, generator=g) for _ in range(2)] + [torch.rand(nb, 3, 32, 32, generator=g) for _ in range(2)]


def test_dino_student_matches_the_oracle_with_per_pass_tables_and_the_teacher_never_drops():
    """2 global + 2 local views of 2 images: the two student passes run 4 samples each with the step seed and the step seed + 1;
    the teacher's outputs are the bits of a model built without the key"""
    nb, G = 2, 2
    model, sd = make_dino(RATE)
    plain, _ = make_dino(None)
    views = dino_views(nb)
    rt = model.runtime()
    assert rt.bb["student"].stack.drop_path == RATES and rt.bb["teacher"].stack.drop_path is None
    ms, seed = find_seed([G * nb, 2 * nb], offsets=(0, 1))
    w = torch.randn(4 * nb, 256, generator=torch.Generator().manual_seed(9))
    torch.manual_seed(ms)
    teacher, student = model([v.to(DEV) for v in views], G)
    (student * w.to(DEV)).sum().backward()
    stack = rt.bb["student"].stack
    tab_g, tab_l = check_table(stack, "g", seed, G * nb), check_table(stack, "l", seed + 1, 2 * nb)
    assert not np.array_equal(tab_g, tab_l)
    t_plain, _ = plain([v.to(DEV) for v in views], G)
    assert torch.equal(teacher.view(torch.int32), t_plain.view(torch.int32)), "the teacher must never drop a path"
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    grid = (IMG // PATCH, IMG // PATCH)
    s_g = DP.dino_student(leaves, torch.cat(views[:G]), PATCH, H, grid, keeps_for(tab_g, 17, 0.0, seed, G * nb))
    s_l = DP.dino_student(leaves, torch.cat(views[G:]), PATCH, H, grid, keeps_for(tab_l, 5, 0.0, seed + 1, 2 * nb))
    se = torch.cat([s_g, s_l])
    (se * w).sum().backward()
    grads = {k: prm.grad for k, prm in model.named_parameters() if k.startswith("student_")}
    names = [k for k in grads]
    assert all(grads[k] is not None for k in names) and all(prm.grad is None for k, prm in model.named_parameters() if k.startswith("teacher_"))
    fig = (rel_l2(student, se), worst_grad(grads, leaves, names))
    print(f"DINO student: outputs {fig[0]:.3g}, worst gradient {fig[1][0]:.3g} ({fig[1][1]})")
    assert fig[0] < OUT_BAR and fig[1][0] < GRAD_BAR, fig


# ------------------------------------------------------------------------------------------------ where drop path never runs
def _gen_state():
    return torch.get_rng_state().clone()


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["nodrop", "drop0.1"])
def test_vit_without_the_key_rate_zero_eval_and_validation_are_bit_identical(p):
    x, y = vit_batch()
    xd, yd = x.to(DEV), y.to(DEV)
    plain, _ = make_vit(p, rate=None)
    zero, _ = make_vit(p, rate=0.0)
    dp, _ = make_vit(p, rate=RATE)
    assert zero.runtime().bb.stack.drop_path is None and plain.runtime().bb.stack.drop_path is None

    def train_fwd_bwd(m):
        torch.manual_seed(11)
        out = m(xd)
        torch.nn.functional.cross_entropy(out, yd).backward()
        return out.detach(), {k: prm.grad.clone() for k, prm in m.named_parameters()}, _gen_state()

    # drop_path_rate = 0.0: today's model, bit for bit, gradients and generator state included
    (o1, g1, s1), (o2, g2, s2) = train_fwd_bwd(plain), train_fwd_bwd(zero)
    assert torch.equal(o1, o2) and torch.equal(s1, s2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    rec1, rec2 = Recorder(plain.flat_store()), Recorder(zero.flat_store())
    torch.manual_seed(12)
    l1 = plain.train_step(xd, yd, rec1)
    st1 = _gen_state()
    torch.manual_seed(12)
    l2 = zero.train_step(xd, yd, rec2)
    assert torch.equal(l1, l2) and torch.equal(rec1.gflat, rec2.gflat) and torch.equal(st1, _gen_state())
    # a model WITH a rate: eval mode, no-grad eval forwards, return_attn of an eval model and eval_step draw nothing and drop nothing
    for m in (plain, dp):
        m.eval()
    with torch.no_grad():
        torch.manual_seed(13)
        a, pa = plain(xd, return_attn=True)
        sa = _gen_state()
        torch.manual_seed(13)
        b, pb = dp(xd, return_attn=True)
        assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(sa, _gen_state())
    torch.manual_seed(14)
    la = plain.eval_step(xd, yd)
    sa = _gen_state()
    torch.manual_seed(14)
    lb = dp.eval_step(xd, yd)
    assert torch.equal(la, lb) and torch.equal(plain.last_logits, dp.last_logits) and torch.equal(sa, _gen_state())
    # ... and in training mode it differs from the model without the key
    dp.train()
    plain.train()
    torch.manual_seed(find_seed([B])[0])
    with torch.no_grad():
        assert not torch.equal(dp(xd), plain(xd))


def test_simmim_and_dino_inference_forward_ignore_the_rate():
    from vit_core.ssl.simmim import SimMIMViT
    x = torch.rand(B, 3, IMG, IMG, generator=torch.Generator().manual_seed(6)).to(DEV)
    outs = []
    for extra in ({}, {"drop_path_rate": RATE}):
        torch.manual_seed(5)
        m = SimMIMViT(num_blocks=BLOCKS, input_shape=(3, IMG, IMG), embed_dim=D, patch_size=PATCH, num_heads=H, mlp_dim=F, dropout=0.0,
                      mask_ratio=0.6, **extra).to(DEV).train()
        torch.manual_seed(15)
        outs.append((m.inference_forward(x), m.inference_forward(x, return_patch_features=True), _gen_state()))
    assert all(torch.equal(u, v) for u, v in zip(*outs))
    outs = []
    for rate in (None, RATE):
        m, _ = make_dino(rate)
        torch.manual_seed(16)
        outs.append((m.inference_forward(x), m.inference_forward(x, return_features=True), _gen_state()))
    assert all(torch.equal(u, v) for u, v in zip(*outs))


def test_training_forwards_follow_the_torch_seed():
    model, _ = make_vit(0.0)
    x, _ = vit_batch()
    xd = x.to(DEV)
    ms, _ = find_seed([B])
    ms2, _ = find_seed([B], start=ms + 1)
    outs = []
    with torch.no_grad():
        for s in (ms, ms, ms2):
            torch.manual_seed(s)
            outs.append(model(xd).clone())
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


def test_encoder_block_on_its_own_takes_drop_path():
    """the stand-alone block reaches the engine through _functions.StackRunner: output, input gradient and parameter gradients"""
    from vit_core import EncoderBlock
    T = 20
    torch.manual_seed(8)
    blk = EncoderBlock(D, H, F, 0.0, drop_path=0.5)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    blk = blk.to(DEV).train()
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(9))
    w = torch.randn(B, T, D, generator=torch.Generator().manual_seed(10))
    ms, seed = find_seed([B], rates=[0.5])
    xg = x.to(DEV).requires_grad_(True)
    torch.manual_seed(ms)
    yb, _ = blk(xg)
    (yb * w.to(DEV)).sum().backward()
    tab = DP.table([0.5], B, seed)
    assert DP.mixed(tab, [0.5])
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    xo = x.clone().requires_grad_(True)
    ye, _ = O.encoder_block(xo, leaves, "", H, emu="bf16", keep=DP.oracle_keeps(tab, T, D, F)[0], p_drop=0.0)
    (ye * w).sum().backward()
    dropped = torch.from_numpy(tab[1] == 0)
    assert rel_l2(yb, ye) < OUT_BAR and rel_l2(xg.grad, xo.grad) < GRAD_BAR
    assert worst_grad({k: prm.grad for k, prm in blk.named_parameters()}, leaves)[0] < GRAD_BAR
    both = torch.from_numpy((tab[0] == 0) & (tab[1] == 0))
    if bool(both.any()):                                                     # dropped from both branches: the block is the identity
        assert torch.equal(yb.detach().cpu()[both], x[both])
    assert bool(dropped.any())


def test_fp8_operands_with_a_rate_are_refused():
    from vitssl_hip import VitsslError
    from vitssl_hip import engine as E
    model, _ = make_vit(0.0)
    zero, _ = make_vit(0.0, rate=0.0)
    E.set_linear_operands("fp8")
    try:
        with pytest.raises(VitsslError, match="bf16"):
            model.runtime(DEV)
        assert zero.runtime(DEV).bb.stack.fp8                               # rate 0: fp8 stacks build as before
    finally:
        E.set_linear_operands("bf16")
