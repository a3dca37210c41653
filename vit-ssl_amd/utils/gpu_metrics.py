"""Per-epoch training metrics computed where the tensors lie (reference: utils/metrics.py, MetricHandler :8-45 and the
metric classes behind it, which need ignite and torcheval).  Same registry names, same `metrics` config key, same
`ValueError` for an unknown name; not the same mechanics:

  * PSNR / SSIM: every batch's predictions and targets are reduced by `ops.recon_metrics` into a 4-double device
    accumulator (the reference keeps all of them alive and concatenates: simmim_trainer.py:79-96); one host read per epoch.
    `reset()` clears SSIM too -- the reference's SSIMMetric never resets its ignite metric between epochs.
  * CenterNorm, Teacher/Student Mean/STD/Var, CosineSim: one `ops.dino_stats` launch over the tensors of the epoch's last
    batch (dino_trainer.py:114-118), without the [G, V, B, K] product of CosineSimMetric.
  * Accuracy, F1Score, Recall, Precision: a [C, C] confusion matrix accumulated on the labels' device with torch.bincount
    (not hot, no kernel).  Semantics of utils/metrics.py:198-256: macro average over max(y_true) + 1 classes, a class with
    a zero denominator counts as 0.  Precision returns the macro precision the reference computes and then drops (its
    compute() ends without `return`).

This module is deliberately not named `metrics`: `utils.metrics` must keep resolving to the reference's module when this
package sits in front of it (utils/__init__.py)."""
import math

import torch

from ._config import cfg_get

RECON_METRICS = ("PSNR", "SSIM")
DINO_METRICS = ("CenterNorm", "TeacherMean", "TeacherSTD", "TeacherVar", "StudentMean", "StudentSTD", "StudentVar", "CosineSim")
CLASSIFICATION_METRICS = ("Accuracy", "F1Score", "Recall", "Precision")
REGISTRY = DINO_METRICS + RECON_METRICS + CLASSIFICATION_METRICS


def metric_list(config):
    """The config's `metrics` list ([] when the key is absent or empty)."""
    names = cfg_get(config, "metrics")
    return [str(n) for n in names] if names else []


def recon_values(acc):
    """{"PSNR", "SSIM"} from the four sums of ops.recon_metrics (torcheval PeakSignalNoiseRatio(data_range=1.0), ignite SSIM)."""
    sse, ssim_sum, elements, patches = (float(v) for v in acc)
    if patches == 0:
        return {"PSNR": float("nan"), "SSIM": float("nan")}
    return {"PSNR": 10.0 * math.log10(elements / sse) if sse > 0 else float("inf"), "SSIM": ssim_sum / patches}


def dino_values(stats, pairs):
    """The eight DINO metrics from the eight sums of ops.dino_stats; `pairs` = G * V * B.  Var / STD: torch's unbiased default."""
    nt, mt, m2t, ns, ms, m2s, cos, csq = (float(v) for v in stats)
    var_t = m2t / (nt - 1) if nt > 1 else float("nan")
    var_s = m2s / (ns - 1) if ns > 1 else float("nan")
    return {"CenterNorm": math.sqrt(csq), "TeacherMean": mt, "TeacherSTD": math.sqrt(var_t), "TeacherVar": var_t,
            "StudentMean": ms, "StudentSTD": math.sqrt(var_s), "StudentVar": var_s, "CosineSim": cos / pairs}


def classification_values(cm):
    """Accuracy and the macro F1Score / Recall / Precision of a confusion matrix cm[true, predicted] (any integer tensor)."""
    cm = cm.detach().to("cpu", torch.float64)
    total = float(cm.sum())
    if total == 0:
        return {n: float("nan") for n in CLASSIFICATION_METRICS}
    support = cm.sum(1)
    nc = int(support.nonzero().max()) + 1                       # max(y_true) + 1
    tp = cm.diagonal()[:nc]
    pred_n, true_n = cm.sum(0)[:nc], support[:nc]               # tp + fp, tp + fn
    zero = torch.zeros(nc, dtype=torch.float64)
    precision = torch.where(pred_n > 0, tp / pred_n.clamp(min=1), zero)
    recall = torch.where(true_n > 0, tp / true_n.clamp(min=1), zero)
    pr = precision + recall
    f1 = torch.where(pr > 0, 2 * precision * recall / pr.clamp(min=1e-300), zero)
    return {"Accuracy": float(cm.diagonal().sum()) / total, "F1Score": float(f1.mean()), "Recall": float(recall.mean()),
            "Precision": float(precision.mean())}


class GPUMetricHandler:
    """Built from a config whose `metrics` lists registry names; `reset()` per epoch, `update_*()` per batch, `compute()`
    once per epoch -> {name: float} of the listed names whose inputs were seen."""

    def __init__(self, config):
        self._names = []
        for name in metric_list(config):
            if name not in REGISTRY:
                raise ValueError(f"Unknown metric '{name}'")
            if name not in self._names:
                self._names.append(name)
        self.reset()

    @classmethod
    def from_config(cls, config):
        """The handler of a config that lists metrics, None for one that lists none."""
        return cls(config) if metric_list(config) else None

    @property
    def metric_names(self):
        return list(self._names)

    def wants(self, group):
        return any(n in group for n in self._names)

    def reset(self):
        self._recon = None      # f64 [4] on the device
        self._dino = None       # (f64 [8] on the device, G * V * B)
        self._cm = None         # int64 [C, C] confusion matrix, cm[true, predicted]

    # ---- per batch
    def update_recon(self, pred, target, channels, patch):
        """pred / target [n, C*P*P] of one step (bf16 or fp32 on the device)"""
        if not self.wants(RECON_METRICS):
            return
        from vitssl_hip import ops
        if self._recon is None:
            self._recon = torch.zeros(ops.RECON_ACC, dtype=torch.float64, device=pred.device)
        ops.recon_metrics(pred.detach().float().contiguous(), target.detach().float().contiguous(), self._recon, channels, patch)

    def update_dino(self, teacher, student, center):
        """teacher [G, B, K], student [V, B, K], center [K] or [1, K]: the statistics REPLACE those of an earlier call"""
        if not self.wants(DINO_METRICS):
            return
        from vitssl_hip import ops
        teacher, student = teacher.detach().float().contiguous(), student.detach().float().contiguous()
        out = torch.empty(ops.DINO_STATS, dtype=torch.float64, device=teacher.device)
        ops.dino_stats(teacher, student, center.detach().float().reshape(-1).contiguous(), out)
        self._dino = (out, teacher.shape[0] * student.shape[0] * teacher.shape[1])

    def update_classification(self, predicted, labels, num_classes):
        """predicted / labels: integer class tensors of one batch (any device)"""
        if not self.wants(CLASSIFICATION_METRICS):
            return
        if self._cm is None:
            self._cm = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=labels.device)
        idx = labels.reshape(-1).long() * num_classes + predicted.reshape(-1).long()
        self._cm += torch.bincount(idx, minlength=num_classes * num_classes).view(num_classes, num_classes)

    # ---- per epoch
    def compute(self):
        values = {}
        if self._recon is not None:
            values.update(recon_values(self._recon.cpu()))
        if self._dino is not None:
            values.update(dino_values(self._dino[0].cpu(), self._dino[1]))
        if self._cm is not None:
            values.update(classification_values(self._cm))
        return {n: values[n] for n in self._names if n in values}
