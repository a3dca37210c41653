"""The classification loss kernel (include/vitssl_classify.h) against its fp64 restatement, ViT.train_step / eval_step against
the autograd path on the same weights, the three backward schedules of a frozen model, and the trainer's fused path.

Loss bar: 4 x the distance of torch's own fp32 CPU F.cross_entropy from the fp64 value on the same inputs, floor 1e-6
relative.  Measured on MI355X, relative distance from the fp64 value of torch fp32 on the CPU / of the kernel, at eps = 0 and 0.1:
(1,2,64) 2.8e-9 / 2.8e-9 and the same; (33,10,64) 2.0e-7 / 3.1e-8 and 2.4e-7 / 3.1e-8; (7,1000,1024) 5.1e-8 / 1.0e-8 and 6.8e-8 / 3.3e-8;
(5,1027,1088) 4.8e-8 / 1.5e-8 and 6.3e-8 / 2.9e-8; (3,65536,65536) 4.5e-8 / 3.4e-8 and 7.9e-8 / 4.0e-8.  The floor decides everywhere
(4 x torch's distance is at most 9.5e-7); the kernel's distance is the one rounding of its fp64 sum to the fp32 it returns."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _classify_ref as R
from _util import rel_l2

DEV = torch.device("cuda:0")
BF16, F32, I64, I32 = torch.bfloat16, torch.float32, torch.int64, torch.int32
gpu = pytest.mark.gpu
MODEL_BAR = 2e-2          # the project's model bar (tests/test_gpu_models.py): relative L2 of a parameter gradient


# ---------------------------------------------------------------------------------------------- kernel
def run_kernel(z, y, C, eps, grad=True, ld_out=None, upstream=1.0, dbias0=0.0):
    from vitssl_hip import ops
    B, ld = z.shape
    ld_out = ld_out or (C + 63) // 64 * 64
    zd, yd = torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV)
    out = dict(loss=torch.full((2,), 7.0, device=DEV), pred=torch.full((B,), -1, dtype=I64, device=DEV),
               counters=torch.tensor([5, 9], dtype=I64, device=DEV), bad=torch.tensor([3], dtype=I32, device=DEV))
    if grad:
        out["dlogits"] = torch.full((B, ld_out), float("nan"), dtype=BF16, device=DEV)
        out["dbias"] = torch.full((C,), dbias0, dtype=F32, device=DEV)
    ops.classify_loss(zd, yd, C, out["loss"], out["pred"], out["counters"], out["bad"], dlogits=out.get("dlogits"), dbias=out.get("dbias"),
                      label_smoothing=eps, ignore_index=R.IGNORE, upstream=upstream)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_against(ref, got, z, y, C, eps, grad=True, dbias0=0.0):
    B = z.shape[0]
    assert float(got["loss"][1]) == ref["n_valid"]
    if ref["n_valid"] == 0:
        assert float(got["loss"][0]) == 0.0 and math.isnan(float(got["loss"][0] / got["loss"][1]))
    else:
        yt = torch.from_numpy(np.where((y >= 0) & (y < C), y, R.IGNORE))     # (torch refuses an out-of-range target: the kernel ignores the row)
        t32 = float(F.cross_entropy(torch.from_numpy(z[:, :C].copy()), yt, label_smoothing=eps, ignore_index=R.IGNORE))
        mine = float(got["loss"][0]) / float(got["loss"][1])
        d_torch, d_mine = abs(t32 - ref["loss"]) / abs(ref["loss"]), abs(mine - ref["loss"]) / abs(ref["loss"])
        print(f"loss (B,C)=({B},{C}) eps={eps}: fp64 {ref['loss']:.12g}  torch fp32 cpu rel {d_torch:.3g}  kernel rel {d_mine:.3g}")
        assert d_mine <= max(4 * d_torch, 1e-6)
    assert np.array_equal(got["pred"].numpy(), ref["pred"])                  # numpy.argmax: the first occurrence
    assert got["counters"].tolist() == [5 + ref["correct"], 9 + ref["n_valid"]]
    if not grad:
        return
    g = got["dlogits"].double().numpy()
    want = torch.from_numpy(ref["grad"]).to(BF16).double().numpy()           # the bf16-rounded fp64 value
    assert not np.isnan(g).any()
    assert (np.abs(g[:, :C] - want) <= 2.0 ** -8 * np.abs(ref["grad"])).all()
    assert not g[:, C:].any()                                                # the padding is zeros ...
    valid = (y != R.IGNORE) & (y >= 0) & (y < C)
    assert not g[~valid].any()                                               # ... and so is every ignored row
    db = got["dbias"].double().numpy() - dbias0                              # accumulated onto what was there
    if ref["n_valid"]:
        assert np.linalg.norm(db - ref["dbias"]) <= 1e-5 * np.linalg.norm(ref["dbias"])
    else:
        assert not db.any()


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C,ld", R.SHAPES, ids=str)
def test_kernel_against_fp64(B, C, ld, eps):
    z, y, _ = R.make_case(B, C, ld)
    got = run_kernel(z, y, C, eps)
    assert got["bad"].tolist() == [3]
    check_against(R.reference(z, y, C, eps), got, z, y, C, eps)
    again = run_kernel(z, y, C, eps)
    for k in got:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), f"{k}: two runs differ"
    ev = run_kernel(z, y, C, eps, grad=False)                                # NULL dlogits: the evaluation case
    assert torch.equal(ev["loss"], got["loss"]) and torch.equal(ev["pred"], got["pred"]) and torch.equal(ev["counters"], got["counters"])


@gpu
@pytest.mark.parametrize("B,C,ld", R.SHAPES[:4], ids=str)
def test_kernel_all_rows_ignored(B, C, ld):
    z, y, _ = R.make_case(B, C, ld, all_ignored=True)
    check_against(R.reference(z, y, C, 0.1), run_kernel(z, y, C, 0.1), z, y, C, 0.1)


@gpu
def test_kernel_wide_gradient_rows_and_upstream():
    """ld_out beyond the chunks that hold a class (the zero-fill loop), an upstream gradient that is not 1, and a bias gradient
    that is added to what the buffer held (2^-6: the sum's own rounding stays far below the bar)."""
    for (B, C, ld), ld_out in ((R.SHAPES[1], 576), (R.SHAPES[3], 1344)):
        z, y, _ = R.make_case(B, C, ld)
        got = run_kernel(z, y, C, 0.1, ld_out=ld_out, upstream=0.5, dbias0=2.0 ** -6)
        assert got["dlogits"].shape == (B, ld_out)
        check_against(R.reference(z, y, C, 0.1, upstream=0.5), got, z, y, C, 0.1, dbias0=2.0 ** -6)


@gpu
@pytest.mark.parametrize("B,C,ld", [R.SHAPES[1], R.SHAPES[3]], ids=str)
def test_kernel_out_of_range_labels_are_flagged_and_ignored(B, C, ld):
    z, y, _ = R.make_case(B, C, ld)
    bad = y.copy()
    bad[0], bad[2] = C, -5
    got = run_kernel(z, bad, C, 0.1)
    assert got["bad"].tolist() == [3 + 2]
    check_against(R.reference(z, bad, C, 0.1), got, z, bad, C, 0.1)          # nothing else is disturbed


@gpu
def test_kernel_nan_row_has_a_defined_prediction():
    z, y, _ = R.make_case(7, 1000, 1024)
    z[3, 700] = z[3, 12] = np.nan
    got = run_kernel(z, y, 1000, 0.0)
    assert got["pred"][3] == 12 == int(np.argmax(z[3, :1000]))              # the first NaN, as numpy and torch answer


# ---------------------------------------------------------------------------------------------- fused step against autograd
def tiny(dropout=0.0, seed=21, classes=10):
    from vit_core.vit import ViT
    torch.manual_seed(seed)
    return ViT(num_classes=classes, num_blocks=2, input_shape=(3, 32, 32), embed_dim=128, patch_size=8, num_heads=2, mlp_dim=256,
               dropout=dropout).to(DEV).train()


def batch():
    g = torch.Generator().manual_seed(5)
    return torch.rand(8, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (8,), generator=g).to(DEV)


class Recorder:
    """optimizer stub: keeps the flat gradient buffer the fused step hands to step_flat"""

    def __init__(self, store):
        self.store, self.gflat, self.gscale = store, None, None

    def step_flat(self, gscale=1.0):
        self.gflat, self.gscale = self.store.gflat.clone(), gscale


def autograd_grads(model, x, y, criterion):
    for p in model.parameters():
        p.grad = None
    loss = criterion(model(x), y)
    loss.backward()
    return float(loss), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def fused_grads(model, x, y, **kw):
    rec = Recorder(model.flat_store())
    loss = model.train_step(x, y, rec, **kw)
    torch.cuda.synchronize()
    st = model.flat_store()
    return float(loss), {n: rec.gflat[st.offsets[n][0]:st.offsets[n][0] + st.offsets[n][1]].view(p.shape) for n, p in zip(st.names, st.params)}, rec


@gpu
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_train_step_gradients_equal_the_autograd_path(eps):
    x, y = batch()
    a, b = tiny(), tiny()
    la, ga = autograd_grads(a, x, y, nn.CrossEntropyLoss(label_smoothing=eps))
    lb, gb, _ = fused_grads(b, x, y, label_smoothing=eps)
    assert abs(la - lb) <= 1e-5 * abs(la)
    worst = max((rel_l2(gb[n], ga[n]), n) for n in ga)
    print(f"train_step vs autograd, eps={eps}: largest relative L2 of a parameter gradient {worst[0]:.3g} ({worst[1]})")
    assert set(ga) == set(gb) and worst[0] < MODEL_BAR, worst
    assert b.last_logits.shape == (8, 10) and torch.equal(b.last_pred, b.last_logits.argmax(1))
    with torch.no_grad():
        assert float((b.last_logits - a(x)).abs().max()) <= 1e-5


@gpu
def test_three_train_steps_equal_three_autograd_steps():
    from vitssl_hip.optim import FusedAdamW
    x, y = batch()
    a, b = tiny(), tiny()
    oa, ob = FusedAdamW(a.flat_store(), lr=1e-3, weight_decay=1e-2), FusedAdamW(b.flat_store(), lr=1e-3, weight_decay=1e-2)
    crit = nn.CrossEntropyLoss()
    counters = torch.zeros(2, dtype=I64, device=DEV)
    for _ in range(3):
        oa.zero_grad(set_to_none=True)
        crit(a(x), y).backward()
        oa.step()
        b.train_step(x, y, ob, counters=counters)
    torch.cuda.synchronize()
    sa, sb = a.flat_store(), b.flat_store()
    for n in sa.names:
        assert rel_l2(sb.view(n), sa.view(n)) < MODEL_BAR, n
    assert not torch.equal(sb.flat, tiny().flat_store().flat) and int(counters[1]) == 24 and 0 <= int(counters[0]) <= 24
    b.check_labels()


@gpu
def test_train_step_with_dropout_is_reproducible_and_learns():
    from vitssl_hip.optim import FusedAdamW
    x, y = batch()
    runs = []
    for _ in range(2):
        m = tiny(dropout=0.1)
        opt = FusedAdamW(m.flat_store(), lr=1e-3, weight_decay=1e-2)
        torch.manual_seed(77)
        losses = torch.stack([m.train_step(x, y, opt) for _ in range(10)]).cpu()
        runs.append((losses, m.flat_store().flat.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert float(runs[0][0][9]) < float(runs[0][0][0])


@gpu
def test_eval_step_is_the_no_grad_forward():
    x, y = batch()
    m = tiny(dropout=0.1)
    _, _, _ = fused_grads(m, x, y)                                           # leaves a pending record behind
    saved = {k: v.clone() for k, v in m.runtime().bb.stack._saved["a"]["blocks"][0].items() if torch.is_tensor(v)}
    counters = torch.zeros(2, dtype=I64, device=DEV)
    loss = m.eval_step(x, y, counters=counters)
    m.eval()
    with torch.no_grad():
        logits = m(x)
    m.train()
    assert abs(float(loss) - float(F.cross_entropy(logits, y))) <= 1e-5 * float(loss)
    assert float((m.last_logits - logits).abs().max()) <= 1e-5 and torch.equal(m.last_pred, logits.argmax(1))
    assert counters.tolist() == [int((logits.argmax(1) == y).sum()), 8]
    for k, v in saved.items():                                               # the buffers of the pending backward are untouched
        assert torch.equal(m.runtime().bb.stack._saved["a"]["blocks"][0][k], v), k


# ---------------------------------------------------------------------------------------------- the autograd adapter
@gpu
@pytest.mark.parametrize("classes", [10, 64])
def test_autograd_logits_do_not_alias_engine_storage(classes):
    """The head writes its padded logits into a workspace buffer that the next forward overwrites; with 64 classes the [:, :C]
    slice of that buffer is already contiguous, so only a copy keeps the first result."""
    m = tiny(classes=classes)
    x1, _ = batch()
    y1 = m(x1)
    kept = y1.detach().clone()
    y2 = m(1.0 - x1)
    torch.cuda.synchronize()
    assert y1.shape == (8, classes) and y1.requires_grad and not torch.equal(y2, kept)
    assert torch.equal(y1, kept)


@gpu
@pytest.mark.parametrize("sched", ["full", "head"])
def test_stale_graph_is_refused_after_a_fused_step(sched):
    """A fused step replaces the activations the engine keeps for the one pending backward, as a second grad forward does."""
    from utils.model_builder import freeze_backbone
    from vitssl_hip import VitsslError
    x, y = batch()
    m = tiny()
    if sched == "head":
        freeze_backbone(m)
        m.patch_embedding.cls_token.requires_grad = False
    assert m.runtime().schedule() == sched
    out = m(x)
    m.train_step(x, y, Recorder(m.flat_store()))
    with pytest.raises(VitsslError, match=r"backward of forward #1, but a later grad-enabled forward \(#2\)"):
        out.sum().backward()


@gpu
def test_no_grad_forward_between_forward_and_backward_changes_no_gradient():
    """no_grad forwards (train or eval mode) and eval_step write the head's "head.tmp." buffers (and the backbone's ".tmp" ones), never those a pending
    backward reads: its gradients are bit-identical to a run without the interloper."""
    x, y = batch()
    grads = []
    for interloper in (False, True):
        m = tiny(dropout=0.1)
        torch.manual_seed(3)
        loss = F.cross_entropy(m(x), y)
        if interloper:
            with torch.no_grad():
                m(1.0 - x)
            m.eval()
            with torch.no_grad():
                m(1.0 - x)
            m.train()
            m.eval_step(1.0 - x, y)
        loss.backward()
        grads.append({n: p.grad.clone() for n, p in m.named_parameters()})
    assert len(grads[0]) == len(m.flat_store().names)
    for n, g in grads[0].items():
        assert g.any() and torch.equal(g, grads[1][n]), n


# ---------------------------------------------------------------------------------------------- frozen schedules
def block_matrices(store):
    return [n for n, p in zip(store.names, store.params) if n.startswith("encoder_blocks.") and p.dim() == 2]


@gpu
def test_frozen_backbone_runs_the_input_gradient_schedule():
    from utils.model_builder import freeze_backbone
    from vitssl_hip.optim import FusedAdamW
    x, y = batch()
    a, b, full = tiny(), tiny(), tiny()
    freeze_backbone(a)
    freeze_backbone(b)
    st = b.flat_store()
    assert b.runtime().schedule() == "input_grad" and full.runtime().schedule() == "full"
    assert b.reduce_ranges() == [st.span("patch_embedding.cls_token", "patch_embedding.conv.bias"),
                                 st.span("classification_head.norm.weight", "classification_head.linear.bias")]
    _, gfull, _ = fused_grads(full, x, y)
    la, ga = autograd_grads(a, x, y, nn.CrossEntropyLoss())
    lb, gb, _ = fused_grads(b, x, y)
    mats = block_matrices(st)
    assert len(mats) == 2 * 6
    for n in mats + ["patch_embedding.conv.weight"]:
        assert not gb[n].any(), n                                            # no weight-gradient GEMM ran ...
        assert gfull[n].any(), n                                             # ... where the full schedule runs one
    assert set(ga) == {"patch_embedding.cls_token"} | {n for n in st.names if n.startswith("classification_head.")}
    assert abs(la - lb) <= 1e-5 * abs(la)
    for n in ga:
        assert rel_l2(gb[n], ga[n]) < MODEL_BAR, n
    before = st.flat.clone()
    opt = FusedAdamW(st, lr=1e-3, weight_decay=1e-2)
    for _ in range(3):
        b.train_step(x, y, opt)
    torch.cuda.synchronize()
    for n, p in zip(st.names, st.params):
        o, cnt = st.offsets[n]
        assert torch.equal(st.flat[o:o + cnt], before[o:o + cnt]) != p.requires_grad, n      # frozen: bit-unchanged; trainable: moved


@gpu
def test_head_only_schedule_keeps_nothing_of_the_backbone():
    from utils.model_builder import freeze_backbone
    x, y = batch()
    a, b = tiny(), tiny()
    for m in (a, b):
        freeze_backbone(m)
        m.patch_embedding.cls_token.requires_grad = False
    rt, st = b.runtime(), b.flat_store()
    assert rt.schedule() == "head" and b.reduce_ranges() == [st.span("classification_head.norm.weight", "classification_head.linear.bias")]
    la, ga = autograd_grads(a, x, y, nn.CrossEntropyLoss())
    lb, gb, rec = fused_grads(b, x, y)
    assert "a" not in rt.bb.rec and "a" not in rt.bb.stack._saved            # no saved record for the slot
    lo, hi = st.span("classification_head.norm.weight", "classification_head.linear.bias")
    assert not rec.gflat[:lo].any() and not rec.gflat[hi:].any()
    assert abs(la - lb) <= 1e-5 * abs(la) and set(ga) == {n for n in st.names if n.startswith("classification_head.")}
    for n in ga:
        assert rel_l2(gb[n], ga[n]) < MODEL_BAR, n


@gpu
def test_unfreezing_between_two_steps_switches_to_the_full_schedule():
    from utils.model_builder import freeze_backbone
    x, y = batch()
    a, b = tiny(), tiny()
    freeze_backbone(b)
    fused_grads(b, x, y)
    for p in b.parameters():
        p.requires_grad = True
    assert b.runtime().schedule() == "full" and b.reduce_ranges() is None
    la, ga = autograd_grads(a, x, y, nn.CrossEntropyLoss())
    lb, gb, _ = fused_grads(b, x, y)
    assert abs(la - lb) <= 1e-5 * abs(la) and len(ga) == len(b.flat_store().names)
    for n in ga:
        assert rel_l2(gb[n], ga[n]) < MODEL_BAR, n


# ---------------------------------------------------------------------------------------------- trainer
def _cfg(fused):
    t = {"type": "supervised", "num_epochs": 1, "warmup_epochs": 1, "warmup_initial_learning_rate": 1e-6, "warmup_final_learning_rate": 1e-3,
         "criterion": {"name": "CrossEntropyLoss", "params": {"label_smoothing": 0.1}},
         "optimizer": {"name": "AdamW", "params": {"lr": 1e-3, "weight_decay": 1e-3}},
         "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}}}
    if fused:
        t["fused_step"] = True
    return {"training": t, "eval": {}, "data": {"img_size": 32}, "metrics": ["Accuracy", "F1Score"],
            "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 128, "num_blocks": 2, "num_heads": 2, "mlp_dim": 256, "dropout": 0.0,
                      "num_classes": 10}}


@gpu
def test_trainer_fused_path_reports_what_the_default_path_reports(tmp_path):
    from utils.model_builder import build_model
    from utils.trainers import SupervisedTrainer
    g = torch.Generator().manual_seed(9)
    data = [(torch.rand(8, 3, 32, 32, generator=g), torch.randint(0, 10, (8,), generator=g)) for _ in range(2)]
    trainers = []
    for fused in (False, True):
        torch.manual_seed(31)
        model = build_model(_cfg(fused)).to(DEV)
        trainers.append(SupervisedTrainer(model, str(tmp_path / ("f" if fused else "d")), _cfg(fused), data[:1], data, DEV))
    d, f = trainers
    assert f._fused_path() and not d._fused_path()
    xd, yd = data[0][0].to(DEV), data[0][1].to(DEV)
    d.model.eval()
    with torch.no_grad():
        logits = d.model(xd)
    f.model.eval_step(xd, yd)
    assert float((f.model.last_logits - logits).abs().max()) <= 1e-5       # the predictions come from the same logits
    vd, vf = d.validate(), f.validate()
    assert set(vd) == set(vf) == {"Loss", "Accuracy", "F1Score"}
    assert vd["Accuracy"] == vf["Accuracy"] and vd["F1Score"] == vf["F1Score"] and abs(vd["Loss"] - vf["Loss"]) <= 1e-5 * vd["Loss"]
    td, tf = d.train_epoch(1), f.train_epoch(1)                              # one batch: predictions of the same weights
    assert set(td) == set(tf) == {"Loss", "Accuracy", "F1Score"}
    assert td["Accuracy"] == tf["Accuracy"] and td["F1Score"] == tf["F1Score"] and abs(td["Loss"] - tf["Loss"]) <= 1e-5 * td["Loss"]
    f.fit(1)
    ck = torch.load(tmp_path / "f" / "best_model.pth", weights_only=False)
    assert "best_val_acc" in ck and "best_val_loss" not in ck
