"""No GPU needed: the fp64 restatements of the training metrics (tests/_metrics_ref.py) against the reference's own results
(tests/golden/metrics.npz), sanity of the SSIM restatement, the GPUMetricHandler registry and its confusion-matrix metrics,
the completeness of everything that hangs on include/vitssl_metrics.h, the argument checks of the two entry points (they run
before anything is launched), and the trainers' best-checkpoint rules on a stub model."""
import ctypes
import math
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _metrics_ref as R
from _util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitssl_metrics.h")
DINO_NAMES = ["CenterNorm", "TeacherMean", "TeacherSTD", "TeacherVar", "StudentMean", "StudentSTD", "StudentVar", "CosineSim"]
C1 = 0.01 ** 2


def rel(a, b):
    return abs(a - b) / abs(b)


# ---------------------------------------------------------------------------------------------- restatements
def test_restatements_reproduce_the_reference():
    g = load_golden("metrics")
    assert g["teacher"].shape == (2, 3, 256) and g["student"].shape == (4, 3, 256)
    got = R.dino_metrics(torch.from_numpy(g["teacher"]), torch.from_numpy(g["student"]), torch.from_numpy(g["center"]))
    for name in DINO_NAMES:
        assert rel(got[name], float(g[f"dino_{name}"])) < 1e-6, name
    y_pred, y_true = torch.from_numpy(g["y_pred"]), torch.from_numpy(g["y_true"])
    assert len(y_true) == 200 and int(y_true.max()) == 5 and not (y_pred == 5).any() and (y_pred == 6).any()
    got = R.label_metrics(y_pred, y_true)
    for name in ("Accuracy", "F1Score", "Recall"):
        assert rel(got[name], float(g[f"sup_{name}"])) < 1e-6, name
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "metrics.npz")) < 64 << 10


def test_ssim_restatement_sanity():
    pred, target = R.recon_inputs(16, 3, 5, "equal")
    sse, s = R.recon_sums(pred, target, 3, 16)
    assert sse == 0.0 and abs(s - 5) < 1e-12
    assert R.recon_metrics(pred, target, 3, 16)["PSNR"] == float("inf")
    pred, target = R.recon_inputs(8, 3, 67, "constant")
    a, b = pred[:, 0].double(), target[:, 0].double()
    want = float(((2 * a * b + C1) / (a * a + b * b + C1)).sum())
    assert rel(R.recon_sums(pred, target, 3, 8)[1], want) < 1e-9
    pred, target = R.recon_inputs(8, 3, 67)
    perm = torch.randperm(67, generator=torch.Generator().manual_seed(1))
    s0, s1 = R.recon_sums(pred, target, 3, 8), R.recon_sums(pred[perm], target[perm], 3, 8)
    assert rel(s1[0], s0[0]) < 1e-12 and abs(s1[1] - s0[1]) < 1e-10
    assert (pred < 0).any() and (pred > 1).any()                             # the clamp acts on both sides
    m = R.recon_metrics(pred, target, 3, 8)
    assert rel(m["PSNR"], 10 * math.log10(pred.numel() / s0[0])) < 1e-12 and rel(m["SSIM"], s0[1] / 67) < 1e-12


def test_naive_fp32_variance_misses_the_bar_on_the_offset_input():
    """The control of the variance requirement: logits 50 + 0.1 N(0, 1).  sum(x^2) - n mean^2 in fp32 misses the 1e-5 bar
    the statistics kernel is held to (tests/test_gpu_metrics.py), by orders of magnitude: the case bites."""
    for shape in ((2, 3, 256), (2, 2, 65536)):
        x = 50 + 0.1 * torch.randn(*shape, generator=torch.Generator().manual_seed(5))
        assert rel(R.naive_fp32_var(x), float(x.double().var())) > 1e-3, shape


# ---------------------------------------------------------------------------------------------- handler
def test_handler_registry():
    from utils.gpu_metrics import REGISTRY, GPUMetricHandler
    assert set(REGISTRY) == set(DINO_NAMES) | {"PSNR", "SSIM", "Accuracy", "F1Score", "Recall", "Precision"}
    with pytest.raises(ValueError, match="Unknown metric 'Sharpness'"):
        GPUMetricHandler({"metrics": ["PSNR", "Sharpness"]})
    for cfg in ({}, {"metrics": None}, {"metrics": []}, SimpleNamespace(training={})):
        assert GPUMetricHandler.from_config(cfg) is None
    h = GPUMetricHandler.from_config({"metrics": ["SSIM", "PSNR"]})
    assert h.metric_names == ["SSIM", "PSNR"] and h.compute() == {}
    import utils
    assert not os.path.exists(os.path.join(os.path.dirname(utils.__file__), "metrics.py"))    # utils.metrics stays the reference's


def test_handler_confusion_matrix_metrics():
    from utils.gpu_metrics import GPUMetricHandler
    g = load_golden("metrics")
    y_pred, y_true = torch.from_numpy(g["y_pred"]), torch.from_numpy(g["y_true"])
    h = GPUMetricHandler({"metrics": ["Accuracy", "F1Score", "Recall", "Precision"]})
    for lo in range(0, 200, 64):                                             # several batches add up
        h.update_classification(y_pred[lo:lo + 64], y_true[lo:lo + 64], 7)
    got = h.compute()
    for name in ("Accuracy", "F1Score", "Recall"):
        assert rel(got[name], float(g[f"sup_{name}"])) < 1e-6, name
    assert rel(got["Precision"], R.label_metrics(y_pred, y_true)["Precision"]) < 1e-12
    h.reset()
    assert h.compute() == {}
    h.update_classification(y_pred[:10], y_true[:10], 7)
    assert rel(h.compute()["Accuracy"], float((y_pred[:10] == y_true[:10]).sum()) / 10) < 1e-12     # nothing survives a reset
    only = GPUMetricHandler({"metrics": ["Recall"]})
    only.update_classification(y_pred, y_true, 7)
    assert list(only.compute()) == ["Recall"]


def test_values_from_sums():
    from utils.gpu_metrics import dino_values, recon_values
    v = recon_values(torch.tensor([2.0, 3.0, 800.0, 4.0], dtype=torch.float64))
    assert rel(v["PSNR"], 10 * math.log10(400.0)) < 1e-12 and v["SSIM"] == 0.75
    assert recon_values(torch.tensor([0.0, 4.0, 800.0, 4.0]))["PSNR"] == float("inf")
    d = dino_values(torch.tensor([10.0, 0.5, 18.0, 20.0, -1.0, 76.0, 6.0, 9.0], dtype=torch.float64), 12)
    assert d == {"CenterNorm": 3.0, "TeacherMean": 0.5, "TeacherSTD": math.sqrt(2.0), "TeacherVar": 2.0, "StudentMean": -1.0,
                 "StudentSTD": 2.0, "StudentVar": 4.0, "CosineSim": 0.5}


# ---------------------------------------------------------------------------------------------- header completeness
@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vitssl_hip
    return vitssl_hip


def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|int64_t)\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def test_metrics_header_is_bound_and_exported(built):
    from vitssl_hip import _lib
    protos = _prototypes()
    sizing = {"vitssl_recon_metrics_workspace_floats", "vitssl_dino_stats_workspace_floats"}
    launching = {n: a for n, (r, a) in _lib.REGISTRY["metrics"].items() if r is ctypes.c_int}
    assert set(_lib.header_symbols("metrics")) == set(protos) == set(_lib.REGISTRY["metrics"]) == set(launching) | sizing
    assert {n for n, a in protos.items() if re.search(r"void\s*\*\s*stream", a)} == set(launching)
    raw = ctypes.CDLL(built.LIB_PATH)
    lib = built.lib()
    for n in protos:
        assert hasattr(raw, n), f"{n} declared in include/vitssl_metrics.h but not exported"
    for n, args in launching.items():
        assert len(args) == len([a for a in protos[n].split(",") if a.strip()]), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype is ctypes.c_int
    for n in sizing:
        assert getattr(lib, n).restype is ctypes.c_int64
    # the ABI of include/vitssl_hip.h is what it was
    assert not set(protos) & set(_lib.header_symbols()) and not set(protos) & set(_lib.REGISTRY["hip"])
    assert lib.vitssl_version() == _lib.ABI_VERSION == 3
    # the header cites what it replaces
    txt = open(HEADER).read()
    for cite in ("simmim_trainer.py:79-96", "utils/metrics.py:159-187", "utils/metrics.py:58-156", "dino_trainer.py:114-118"):
        assert cite in txt, cite


def test_sizing_and_argument_errors(built):
    """Geometry, pointer and workspace checks come before any launch: they can be exercised without a GPU."""
    from vitssl_hip import _lib, ops
    lib = built.lib()
    rws, dws = lib.vitssl_recon_metrics_workspace_floats, lib.vitssl_dino_stats_workspace_floats
    assert rws(29952, 3, 16) > 0 and rws(1, 1, 6) == 4 and rws(0, 3, 16) == 0 and rws(5, 3, 4) == 0 and rws(5, 5, 8) == 0
    assert rws(2000, 3, 16) >= rws(1000, 3, 16) > rws(1, 3, 16)
    assert dws(2, 10, 64, 65536) == 2 * 64 * 8 * 56 and dws(2, 2, 1, 4) == 2 * 56 and dws(3, 4, 1, 4) == 2 * 2 * 56
    assert dws(2, 10, 2, 1002) == 0 and dws(3, 2, 2, 256) == 0 and dws(2, 17, 2, 256) == 0
    one = ctypes.c_void_p(256)                                               # never dereferenced: every call below is refused
    rm = lib.vitssl_recon_metrics
    for args, msg in [((one, one, one, 5, 3, 4, one, 1 << 20), b"6 <= P <= 32"), ((one, one, one, 5, 3, 33, one, 1 << 20), b"6 <= P <= 32"),
                      ((one, one, one, 5, 5, 8, one, 1 << 20), b"1 <= C <= 4"), ((one, one, one, -1, 3, 8, one, 1 << 20), b"n = -1"),
                      ((None, one, one, 5, 3, 8, one, 1 << 20), b"null pointer"), ((one, one, None, 5, 3, 8, one, 1 << 20), b"null pointer"),
                      ((one, one, one, 5, 3, 8, None, 1 << 20), b"vitssl_recon_metrics_workspace_floats"),
                      ((one, one, one, 5, 3, 8, one, rws(5, 3, 8) - 1), b"vitssl_recon_metrics_workspace_floats")]:
        assert rm(*args, None) == -1 and msg in lib.vitssl_last_error(), (args, lib.vitssl_last_error())
    assert rm(None, None, None, 0, 3, 8, None, 0, None) == 0                 # n == 0: nothing to do, nothing touched
    ds = lib.vitssl_dino_stats
    for args, msg in [((one, one, one, one, 2, 4, 3, 1002, one, 1 << 20), b"multiple of 4"), ((one, one, one, one, 4, 2, 3, 256, one, 1 << 20), b"G <= V"),
                      ((one, one, one, one, 2, 17, 3, 256, one, 1 << 20), b"G <= V <= 16"), ((one, one, one, one, 0, 4, 3, 256, one, 1 << 20), b"1 <= G"),
                      ((one, one, one, one, 2, 4, 0, 256, one, 1 << 20), b"B = 0"), ((None, one, one, one, 2, 4, 3, 256, one, 1 << 20), b"null pointer"),
                      ((one, one, one, None, 2, 4, 3, 256, one, 1 << 20), b"null pointer"),
                      ((ctypes.c_void_p(260), one, one, one, 2, 4, 3, 256, one, 1 << 20), b"16-byte aligned"),
                      ((one, one, one, one, 2, 4, 3, 256, None, 1 << 20), b"vitssl_dino_stats_workspace_floats"),
                      ((one, one, one, one, 2, 4, 3, 256, one, dws(2, 4, 3, 256) - 1), b"vitssl_dino_stats_workspace_floats")]:
        assert ds(*args, None) == -1 and msg in lib.vitssl_last_error(), (args, lib.vitssl_last_error())
    with pytest.raises(_lib.VitsslError, match="CUDA"):                      # no CPU fallback in the wrappers either
        ops.recon_metrics(torch.zeros(2, 192), torch.zeros(2, 192), torch.zeros(4, dtype=torch.float64), 3, 8)
    with pytest.raises(_lib.VitsslError, match="CUDA"):
        ops.dino_stats(torch.zeros(2, 1, 8), torch.zeros(2, 1, 8), None, torch.zeros(8, dtype=torch.float64))
    with pytest.raises(_lib.VitsslError, match="expected pred"):
        ops.recon_metrics(torch.zeros(2, 100), torch.zeros(2, 100), torch.zeros(4, dtype=torch.float64), 3, 8)


# ---------------------------------------------------------------------------------------------- best-checkpoint rules
class _Stub:
    def state_dict(self):
        return {"w": torch.zeros(1)}


def _trainer(cls, tmp_path, metrics):
    from utils.gpu_metrics import GPUMetricHandler
    t = cls.__new__(cls)
    t.model, t.optimizer, t.rank, t.save_path = _Stub(), _Stub(), 0, str(tmp_path)
    t.config = {"metrics": metrics} if metrics is not None else {}
    t.metric_handler = GPUMetricHandler.from_config(t.config)
    t.best_val_loss, t.best_val_score, t.best_val_acc = math.inf, -math.inf, -math.inf
    return t


def _saved(tmp_path):
    path = os.path.join(tmp_path, "best_model.pth")
    if not os.path.exists(path):
        return None
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    os.remove(path)
    return ckpt


BASE_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "config"}


def test_save_if_best_rules(tmp_path):
    from utils.trainers import DINOTrainer, SimMIMTrainer, SupervisedTrainer
    # SimMIM: SSIM + 0.01 PSNR, strict improvement, from -inf
    t = _trainer(SimMIMTrainer, tmp_path, ["PSNR", "SSIM"])
    t._save_if_best(1, {"Loss": 9.0, "SSIM": -0.5, "PSNR": 10.0})
    ck = _saved(tmp_path)
    assert set(ck) == BASE_KEYS | {"best_val_score"} and abs(ck["best_val_score"] - (-0.4)) < 1e-12 and ck["epoch"] == 1
    t._save_if_best(2, {"Loss": 1.0, "SSIM": -0.5, "PSNR": 10.0})           # equal score, better loss: not saved
    assert _saved(tmp_path) is None
    t._save_if_best(3, {"Loss": 99.0, "SSIM": 0.2, "PSNR": 12.0})
    assert abs(_saved(tmp_path)["best_val_score"] - 0.32) < 1e-12 and t.best_val_loss == math.inf
    # DINO: CosineSim - |CenterNorm - 1| - |StudentSTD - TeacherSTD|
    t = _trainer(DINOTrainer, tmp_path, DINO_NAMES)
    m = {"Loss": 5.0, "CosineSim": 0.5, "CenterNorm": 1.5, "StudentSTD": 2.0, "TeacherSTD": 2.25}
    t._save_if_best(1, m)
    ck = _saved(tmp_path)
    assert set(ck) == BASE_KEYS | {"best_val_score"} and abs(ck["best_val_score"] - (-0.25)) < 1e-12
    t._save_if_best(2, dict(m, Loss=0.1))
    assert _saved(tmp_path) is None
    t._save_if_best(3, dict(m, CenterNorm=0.75, Loss=50.0))
    assert abs(_saved(tmp_path)["best_val_score"] - 0.0) < 1e-12
    # supervised: accuracy
    t = _trainer(SupervisedTrainer, tmp_path, ["Accuracy", "F1Score"])
    t._save_if_best(1, {"Loss": 2.0, "Accuracy": 0.0})
    assert set(_saved(tmp_path)) == BASE_KEYS | {"best_val_acc"}
    t._save_if_best(2, {"Loss": 1.0, "Accuracy": 0.0})
    assert _saved(tmp_path) is None
    t._save_if_best(3, {"Loss": 3.0, "Accuracy": 0.25})
    assert _saved(tmp_path)["best_val_acc"] == 0.25
    # a partial list does not switch the rule; other ranks save nothing
    for cls, names in ((SimMIMTrainer, ["PSNR"]), (DINOTrainer, ["CosineSim", "CenterNorm"]), (SupervisedTrainer, ["F1Score"])):
        t = _trainer(cls, tmp_path, names)
        t._save_if_best(1, {"Loss": 2.0, "PSNR": 1.0, "CosineSim": 1.0, "CenterNorm": 1.0, "F1Score": 1.0})
        assert set(_saved(tmp_path)) == BASE_KEYS | {"best_val_loss"}
    t = _trainer(SimMIMTrainer, tmp_path, ["PSNR", "SSIM"])
    t.rank = 1
    t._save_if_best(1, {"Loss": 9.0, "SSIM": 0.5, "PSNR": 10.0})
    assert _saved(tmp_path) is None


def test_save_if_best_without_metrics_is_todays(tmp_path):
    from utils.trainers import DINOTrainer, SimMIMTrainer, SupervisedTrainer
    for cls in (SimMIMTrainer, DINOTrainer, SupervisedTrainer):
        t = _trainer(cls, tmp_path, None)
        assert t.metric_handler is None and t._metric_values() == {}
        t._save_if_best(1, {"Loss": 2.0, "Accuracy": 0.5})
        ck = _saved(tmp_path)
        assert set(ck) == BASE_KEYS | {"best_val_loss"} and ck["best_val_loss"] == 2.0
        t._save_if_best(2, {"Loss": 2.0, "Accuracy": 0.1})                   # `>=`: an equal loss saves again, as before
        assert _saved(tmp_path)["epoch"] == 2
        t._save_if_best(3, {"Loss": 2.5, "Accuracy": 0.9})
        assert _saved(tmp_path) is None and t.best_val_loss == 2.0
