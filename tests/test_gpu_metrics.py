"""The metric kernels of include/vitssl_metrics.h (reconstruction PSNR / SSIM sums, DINO output statistics) against the fp64
restatements of tests/_metrics_ref.py, their determinism and refusals, and the trainers' `metrics` plumbing on tiny models.

Tolerance of the reconstruction sums.  The bar is not chosen: it is 4x what the SAME formula loses when torch evaluates it
in fp32 instead of fp64 on the CPU, on the very inputs of these tests (_metrics_ref.fp32_formula_deviation(): the largest
relative deviation of the squared-error sum or the SSIM sum over RECON_GRID and RECON_SPECIAL).  Measured: 2.5184743790392845e-03,
at P = 6, C = 3, n = 1000, where the SSIM indices of unrelated random patches nearly cancel in the sum (the squared-error sums
deviate by at most 1.4e-07).  The factor 4 allows for a filter order and an FMA use that differ from torch's.  The kernel
accumulates in fp64, so it sits many orders below the bar; the bar is still the one the definition above gives.

DINO statistics: Mean and CenterNorm 1e-6, Var / STD / CosineSim 1e-5 relative against fp64 -- with fp64 partial sums only the
rounding of the fp32 inputs is left, which the fp64 restatement shares."""
import ctypes as C

import pytest
import torch

import _metrics_ref as R
from _util import load_golden

DEV = torch.device("cuda:0")
gpu = pytest.mark.gpu
F64 = torch.float64

FP32_FORMULA_DEVIATION = 2.5184743790392845e-03        # measured as the docstring says
RECON_BAR = 4 * FP32_FORMULA_DEVIATION                 # = 1.0073897516157138e-02 relative

DINO_TOL = {"CenterNorm": 1e-6, "TeacherMean": 1e-6, "StudentMean": 1e-6, "TeacherVar": 1e-5, "StudentVar": 1e-5, "TeacherSTD": 1e-5,
            "StudentSTD": 1e-5, "CosineSim": 1e-5}


def _L():
    from vitssl_hip import _lib
    return _lib


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def close(got, want, bar):
    return abs(got - want) <= bar * abs(want)


# ---------------------------------------------------------------------------------------------- reconstruction metrics
def recon_run(pred, target, Cc, Pp, acc=None):
    from vitssl_hip import ops
    acc = torch.zeros(4, dtype=F64, device=DEV) if acc is None else acc
    ops.recon_metrics(pred.to(DEV), target.to(DEV), acc, Cc, Pp)
    return acc


RECON_CASES = [(Pp, Cc, n, "random") for Pp, Cc, n in R.RECON_GRID] + R.RECON_SPECIAL


@gpu
@pytest.mark.parametrize("Pp,Cc,n,kind", RECON_CASES, ids=lambda v: str(v))
def test_recon_sums_equal_fp64(Pp, Cc, n, kind):
    pred, target = R.recon_inputs(Pp, Cc, n, kind)
    want_sse, want_ssim = R.recon_sums(pred, target, Cc, Pp)
    acc = recon_run(pred, target, Cc, Pp)
    got = acc.cpu().tolist()
    print(f"P={Pp} C={Cc} n={n} {kind}: sse {got[0]!r} vs {want_sse!r}, ssim sum {got[1]!r} vs {want_ssim!r}, bar {RECON_BAR:.3e}")
    assert close(got[0], want_sse, RECON_BAR) and close(got[1], want_ssim, RECON_BAR)
    assert got[2] == n * Cc * Pp * Pp and got[3] == n
    assert torch.equal(recon_run(pred, target, Cc, Pp), acc), "two runs differ in their bits"
    if kind == "equal":
        assert got[0] == 0.0
    if kind == "constant":
        a, b = pred[:, 0].double(), target[:, 0].double()
        assert close(got[1], float(((2 * a * b + 1e-4) / (a * a + b * b + 1e-4)).sum()), RECON_BAR)
    from utils.gpu_metrics import recon_values
    want = R.recon_metrics(pred, target, Cc, Pp)
    have = recon_values(acc.cpu())
    assert have["PSNR"] == want["PSNR"] or close(have["PSNR"], want["PSNR"], RECON_BAR)
    assert close(have["SSIM"], want["SSIM"], RECON_BAR)


@gpu
def test_recon_calls_add_up_and_empty_call_is_a_no_op():
    pred, target = R.recon_inputs(16, 3, 67)
    whole = recon_run(pred, target, 3, 16)
    acc = recon_run(pred[:30], target[:30], 3, 16)
    before = acc.clone()
    recon_run(pred[:0], target[:0], 3, 16, acc)                              # n == 0: untouched
    assert torch.equal(acc, before)
    recon_run(pred[30:].contiguous(), target[30:].contiguous(), 3, 16, acc)
    a, w = acc.cpu().tolist(), whole.cpu().tolist()
    print(f"split {a} vs whole {w}")
    assert close(a[0], w[0], RECON_BAR) and close(a[1], w[1], RECON_BAR) and a[2:] == w[2:] == [67.0 * 768, 67.0]
    # an odd patch side takes the unvectorised loads
    pred, target = R.recon_inputs(8, 3, 67)
    p7, t7 = pred[:, :147].contiguous(), target[:, :147].contiguous()
    got = recon_run(p7, t7, 3, 7).cpu().tolist()
    want = R.recon_sums(p7, t7, 3, 7)
    assert close(got[0], want[0], RECON_BAR) and close(got[1], want[1], RECON_BAR)


@gpu
def test_recon_refusals_leave_the_accumulator_untouched():
    L = _L()
    lib = L.lib()
    pred, target = (t.to(DEV) for t in R.recon_inputs(8, 3, 5))
    acc = torch.full((4,), 7.25, dtype=F64, device=DEV)
    need = int(lib.vitssl_recon_metrics_workspace_floats(5, 3, 8))
    ws = torch.zeros(max(need, 4096), device=DEV)
    fn = lib.vitssl_recon_metrics
    for args, msg in [((5, 3, 4, P(ws), ws.numel()), b"6 <= P <= 32"), ((5, 3, 33, P(ws), ws.numel()), b"6 <= P <= 32"),
                      ((5, 5, 8, P(ws), ws.numel()), b"1 <= C <= 4"), ((5, 3, 8, P(ws), need - 1), b"vitssl_recon_metrics_workspace_floats"),
                      ((5, 3, 8, P(None), ws.numel()), b"vitssl_recon_metrics_workspace_floats")]:
        assert fn(P(pred), P(target), P(acc), *args, S()) == -1 and msg in lib.vitssl_last_error(), (args, lib.vitssl_last_error())
    with pytest.raises(L.VitsslError, match="6 <= P <= 32"):
        L.call("vitssl_recon_metrics", P(pred), P(target), P(acc), 5, 3, 4, P(ws), ws.numel(), S())
    torch.cuda.synchronize()
    assert bool((acc == 7.25).all()) and bool((ws == 0).all())


# ---------------------------------------------------------------------------------------------- DINO statistics
def dino_inputs(G, V, B, K, kind):
    if kind == "golden":
        g = load_golden("metrics")
        return torch.from_numpy(g["teacher"]), torch.from_numpy(g["student"]), torch.from_numpy(g["center"]).reshape(-1)
    gen = torch.Generator().manual_seed(7919 * G + 104729 * V + 31 * B + K)
    if kind == "offset":                                                     # logits 50 + 0.1 N(0, 1)
        teacher, student = 50 + 0.1 * torch.randn(G, B, K, generator=gen), 50 + 0.1 * torch.randn(V, B, K, generator=gen)
    else:
        teacher, student = 0.3 + 1.5 * torch.randn(G, B, K, generator=gen), 0.7 * torch.randn(V, B, K, generator=gen) - 0.2
        student[:G] += 0.5 * teacher
    return teacher, student, 0.05 + 0.1 * torch.randn(K, generator=gen)


def dino_run(teacher, student, center):
    from vitssl_hip import ops
    out = torch.empty(8, dtype=F64, device=DEV)
    ops.dino_stats(teacher.to(DEV), student.to(DEV), None if center is None else center.to(DEV), out)
    return out


DINO_SHAPES = [(2, 4, 3, 256), (2, 2, 1, 4), (2, 10, 2, 4096), (2, 10, 2, 65536), (1, 3, 5, 1000), (3, 16, 2, 8200)]
DINO_CASES = [(2, 4, 3, 256, "golden")] + [s + (k,) for s in DINO_SHAPES for k in ("random", "offset")]


@gpu
@pytest.mark.parametrize("G,V,B,K,kind", DINO_CASES, ids=lambda v: str(v))
def test_dino_stats_equal_fp64(G, V, B, K, kind):
    from utils.gpu_metrics import dino_values
    teacher, student, center = dino_inputs(G, V, B, K, kind)
    want = R.dino_metrics(teacher, student, center)
    out = dino_run(teacher, student, center)
    got = dino_values(out.cpu(), G * V * B)
    for name, tol in DINO_TOL.items():
        print(f"{name}: {got[name]!r} vs {want[name]!r} (rel {abs(got[name] - want[name]) / abs(want[name]):.2e}, bar {tol:.0e})")
    for name, tol in DINO_TOL.items():
        assert close(got[name], want[name], tol), name
    assert out[0].item() == G * B * K and out[3].item() == V * B * K
    assert torch.equal(dino_run(teacher, student, center), out), "two runs differ in their bits"
    if kind == "golden":
        g = load_golden("metrics")
        for name in DINO_TOL:
            assert close(got[name], float(g[f"dino_{name}"]), 1e-6), name    # the reference's own (fp32) results
    if kind == "offset" and K >= 256:
        assert abs(R.naive_fp32_var(teacher) - want["TeacherVar"]) > 1e-5 * want["TeacherVar"]     # the formula the kernel must not use
    no_center = dino_run(teacher, student, None).cpu()
    assert no_center[7] == 0.0 and torch.equal(no_center[:7], out.cpu()[:7])


@gpu
def test_dino_refusals_leave_the_output_untouched():
    L = _L()
    lib = L.lib()
    teacher, student, center = (t.to(DEV) for t in dino_inputs(2, 4, 3, 1004, "random"))
    out = torch.full((8,), 7.25, dtype=F64, device=DEV)
    need = int(lib.vitssl_dino_stats_workspace_floats(2, 4, 3, 1004))
    ws = torch.zeros(max(need, 4096), device=DEV)
    fn = lib.vitssl_dino_stats
    for args, msg in [((2, 4, 3, 1002, P(ws), ws.numel()), b"multiple of 4"), ((4, 2, 3, 1004, P(ws), ws.numel()), b"G <= V"),
                      ((2, 4, 3, 1004, P(ws), need - 1), b"vitssl_dino_stats_workspace_floats"),
                      ((2, 4, 3, 1004, P(None), ws.numel()), b"vitssl_dino_stats_workspace_floats")]:
        assert fn(P(teacher), P(student), P(center), P(out), *args, S()) == -1 and msg in lib.vitssl_last_error(), (args, lib.vitssl_last_error())
    with pytest.raises(L.VitsslError, match="multiple of 4"):
        L.call("vitssl_dino_stats", P(teacher), P(student), P(center), P(out), 2, 4, 3, 1002, P(ws), ws.numel(), S())
    torch.cuda.synchronize()
    assert bool((out == 7.25).all()) and bool((ws == 0).all())


# ---------------------------------------------------------------------------------------------- trainers, tiny
def _cfg(mode, metrics=None):
    cfg = {"training": {"type": mode, "num_epochs": 1, "warmup_epochs": 1, "warmup_initial_learning_rate": 1e-6,
                        "warmup_final_learning_rate": 1e-3, "criterion": {"name": "L1Loss", "params": {"reduction": "mean"}},
                        "optimizer": {"name": "AdamW", "params": {"lr": 1e-3, "weight_decay": 1e-3}},
                        "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}}},
           "eval": {}, "data": {"img_size": 32},
           "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 128, "num_blocks": 1, "num_heads": 2, "mlp_dim": 192,
                     "dropout": 0.1, "mask_ratio": 0.6, "num_classes": 5, "output_dim": 256, "center_momentum": 0.9}}
    if mode != "simmim" and mode != "dino":
        cfg["training"]["criterion"] = {"name": "CrossEntropyLoss", "params": {}}
    if metrics is not None:
        cfg["metrics"] = metrics
    return cfg


def _record_outputs(model):
    """every (pred, targets) the model hands out from now on: through train_step (last_pred / last_targets) or forward"""
    seen = []
    step, fwd = model.train_step, model.forward

    def train_step(*a, **k):
        loss = step(*a, **k)
        seen.append((model.last_pred.detach().float().clone(), model.last_targets.detach().float().clone()))
        return loss

    def forward(*a, **k):
        pred, targets = fwd(*a, **k)
        seen.append((pred.detach().float().clone(), targets.detach().float().clone()))
        return pred, targets
    model.train_step, model.forward = train_step, forward
    return seen


@gpu
def test_simmim_trainer_reports_psnr_ssim_and_selects_by_them(tmp_path):
    from utils.model_builder import build_model
    from utils.trainers import SimMIMTrainer
    torch.manual_seed(11)
    data = [torch.rand(4, 3, 32, 32) for _ in range(2)]
    cfg = _cfg("simmim", ["PSNR", "SSIM"])
    model = build_model(cfg).to(DEV)
    tr = SimMIMTrainer(model, str(tmp_path / "m"), cfg, data, data, DEV)
    assert tr._fused_ok() and tr.metric_handler.metric_names == ["PSNR", "SSIM"]
    seen = _record_outputs(model)
    for split in ("train", "val"):
        del seen[:]
        m = tr.train_epoch(1) if split == "train" else tr.validate()
        assert set(m) == {"Loss", "PSNR", "SSIM"} and len(seen) == 2
        pred, targets = torch.cat([p for p, _ in seen]), torch.cat([t for _, t in seen])
        want = R.recon_metrics(pred, targets, 3, 8)
        print(split, m, want)
        assert close(m["PSNR"], want["PSNR"], RECON_BAR) and close(m["SSIM"], want["SSIM"], RECON_BAR)
    tr.fit(1)
    ck = torch.load(tmp_path / "m" / "best_model.pth", weights_only=False)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "config", "best_val_score"}
    assert ck["best_val_score"] == tr.best_val_score > -float("inf")
    # the same run without `metrics`: today's dicts and keys
    cfg0 = _cfg("simmim")
    tr0 = SimMIMTrainer(build_model(cfg0).to(DEV), str(tmp_path / "plain"), cfg0, data, data, DEV)
    assert tr0.metric_handler is None
    assert set(tr0.train_epoch(1)) == {"Loss"} and set(tr0.validate()) == {"Loss"}
    tr0.fit(1)
    ck = torch.load(tmp_path / "plain" / "best_model.pth", weights_only=False)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "config", "best_val_loss"}
    # the autograd path feeds the handler too
    cfg2 = _cfg("simmim", ["SSIM", "PSNR"])
    cfg2["training"]["optimizer"] = {"name": "SGD", "params": {"lr": 0.05}}
    model2 = build_model(cfg2).to(DEV)
    tr2 = SimMIMTrainer(model2, str(tmp_path / "sgd"), cfg2, data, data, DEV)
    assert not tr2._fused_ok()
    seen = _record_outputs(model2)
    m = tr2.train_epoch(1)
    want = R.recon_metrics(torch.cat([p for p, _ in seen]), torch.cat([t for _, t in seen]), 3, 8)
    assert list(m)[:2] == ["SSIM", "PSNR"] and close(m["PSNR"], want["PSNR"], RECON_BAR) and close(m["SSIM"], want["SSIM"], RECON_BAR)


@gpu
def test_dino_trainer_reports_the_eight_statistics(tmp_path):
    from utils.model_builder import build_model
    from utils.trainers import DINOTrainer
    torch.manual_seed(12)
    names = list(DINO_TOL)
    cfg = _cfg("dino", names)
    views = [[torch.rand(4, 3, 32, 32), torch.rand(4, 3, 32, 32), torch.rand(4, 3, 16, 16), torch.rand(4, 3, 16, 16)] for _ in range(2)]
    model = build_model(cfg).to(DEV)
    tr = DINOTrainer(model, str(tmp_path / "d"), cfg, views, views, DEV)
    assert tr._is_fused()
    m = tr.train_epoch(1)
    assert set(m) == set(names) | {"Loss", "TeacherTemp", "Momentum"}
    want = R.dino_metrics(model.last_teacher.view(2, 4, 256), model.last_student.view(4, 4, 256), model.center)
    for name, tol in DINO_TOL.items():
        assert close(m[name], want[name], tol), (name, m[name], want[name])
    v = tr.validate()
    assert set(v) == set(names) | {"Loss"}
    teacher, student = tr._last_outputs
    want = R.dino_metrics(teacher.view(2, 4, 256), student.view(4, 4, 256), model.center)
    for name, tol in DINO_TOL.items():
        assert close(v[name], want[name], tol), (name, v[name], want[name])
    tr.fit(1)
    ck = torch.load(tmp_path / "d" / "best_model.pth", weights_only=False)
    assert "best_val_score" in ck and "best_val_loss" not in ck
    cfg0 = _cfg("dino")
    tr0 = DINOTrainer(build_model(cfg0).to(DEV), str(tmp_path / "d0"), cfg0, views[:1], views[:1], DEV)
    assert set(tr0.train_epoch(1)) == {"Loss", "TeacherTemp", "Momentum"} and set(tr0.validate()) == {"Loss"}


@gpu
def test_supervised_trainer_reports_the_label_metrics(tmp_path):
    from utils.model_builder import build_model
    from utils.trainers import SupervisedTrainer
    torch.manual_seed(13)
    names = ["Accuracy", "F1Score", "Recall", "Precision"]
    cfg = _cfg("supervised", names)
    data = [(torch.rand(4, 3, 32, 32), torch.tensor([0, 1, 3, 3])), (torch.rand(4, 3, 32, 32), torch.tensor([1, 0, 0, 3]))]
    model = build_model(cfg).to(DEV)
    tr = SupervisedTrainer(model, str(tmp_path / "s"), cfg, data, data, DEV)
    logits, fwd = [], model.forward

    def forward(x):
        out = fwd(x)
        logits.append(out.detach().argmax(1).cpu())
        return out
    model.forward = forward
    y_true = torch.cat([y for _, y in data])
    for split in ("train", "val"):
        del logits[:]
        m = tr.train_epoch(1) if split == "train" else tr.validate()
        assert set(m) == set(names) | {"Loss"}
        want = R.label_metrics(torch.cat(logits), y_true)                   # classes 0 .. 3: class 2 never occurs, class 4 is beyond max(y_true)
        for name in names:
            assert abs(m[name] - want[name]) < 1e-12, (split, name, m[name], want[name])
    tr.fit(1)
    ck = torch.load(tmp_path / "s" / "best_model.pth", weights_only=False)
    assert "best_val_acc" in ck and "best_val_loss" not in ck
    cfg0 = _cfg("supervised")
    tr0 = SupervisedTrainer(build_model(cfg0).to(DEV), str(tmp_path / "s0"), cfg0, data, data, DEV)
    assert set(tr0.train_epoch(1)) == {"Loss", "Accuracy"} and set(tr0.validate()) == {"Loss", "Accuracy"}
