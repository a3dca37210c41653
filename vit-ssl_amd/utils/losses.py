"""Criteria that torch.nn does not have; `make_criterion` resolves these names before it looks in torch.nn.

BinaryCrossEntropy: the DeiT III loss, timm's `BinaryCrossEntropy` restated (nothing here imports timm): a sigmoid per class
against label-smoothed one-hot targets, or against dense targets as they come, with an optional target threshold.  It is a
plain torch module -- the criterion of the autograd path, and usable on the CPU; with `training.fused_step` the supervised
trainer hands its fields to `ViT.train_step(loss="bce")`, whose kernel (csrc/classify.hip, include/vitssl_bce.h) computes the
same loss.  One extension over timm: rows whose integer label equals `ignore_index` are left out of the mean, as
nn.CrossEntropyLoss leaves them out; without such labels the value is timm's."""
import torch
import torch.nn.functional as F
from torch import nn


class BinaryCrossEntropy(nn.Module):
    """loss(logits [B, C], target): target is integer labels [B] -> (1 - smoothing) onehot + smoothing / C, or dense [B, C]
    (used as it is: Mixup's targets carry their own smoothing).  `target_threshold`: targets become (t > threshold) as 0 / 1.
    `sum_classes`: a row's loss is the sum over its classes instead of their mean.  The result is the mean over the rows whose
    label is not `ignore_index` (nan when there is none, as nn.CrossEntropyLoss gives)."""

    def __init__(self, smoothing: float = 0.1, target_threshold=None, sum_classes: bool = False, ignore_index: int = -100):
        super().__init__()
        if not 0.0 <= float(smoothing) <= 1.0:
            raise ValueError(f"BinaryCrossEntropy: smoothing = {smoothing!r} is outside 0 <= smoothing <= 1")
        if target_threshold is not None and not float(target_threshold) >= 0.0:
            raise ValueError(f"BinaryCrossEntropy: target_threshold = {target_threshold!r} must be None or a number >= 0")
        self.smoothing = float(smoothing)
        self.target_threshold = None if target_threshold is None else float(target_threshold)
        self.sum_classes = bool(sum_classes)
        self.ignore_index = int(ignore_index)

    def extra_repr(self):
        return (f"smoothing={self.smoothing}, target_threshold={self.target_threshold}, sum_classes={self.sum_classes}, "
                f"ignore_index={self.ignore_index}")

    def targets(self, logits, target):
        """-> (dense targets [B, C] in the logits' dtype, keep [B] bool or None when every row counts)"""
        B, C = logits.shape
        keep = None
        if target.dim() == 1:
            if target.shape[0] != B or target.dtype.is_floating_point:
                raise ValueError(f"BinaryCrossEntropy: expected {B} integer labels, got {tuple(target.shape)} of {target.dtype}")
            keep = target != self.ignore_index
            off = self.smoothing / C
            on = 1.0 - self.smoothing + off
            index = torch.where(keep, target, torch.zeros_like(target)).long().view(B, 1)
            t = torch.full((B, C), off, dtype=logits.dtype, device=logits.device).scatter_(1, index, on)
        elif tuple(target.shape) == (B, C):
            t = target.to(logits.dtype)
        else:
            raise ValueError(f"BinaryCrossEntropy: expected labels [{B}] or dense targets [{B}, {C}], got {tuple(target.shape)}")
        if self.target_threshold is not None:
            t = (t > self.target_threshold).to(logits.dtype)
        return t, keep

    def forward(self, logits, target):
        if logits.dim() != 2:
            raise ValueError(f"BinaryCrossEntropy: expected logits [B, C], got {tuple(logits.shape)}")
        t, keep = self.targets(logits, target)
        if keep is None:                                         # timm's two statements
            if self.sum_classes:
                return F.binary_cross_entropy_with_logits(logits, t, reduction="none").sum(-1).mean()
            return F.binary_cross_entropy_with_logits(logits, t, reduction="mean")
        e = F.binary_cross_entropy_with_logits(logits, t, reduction="none")
        rows = e.sum(-1) if self.sum_classes else e.mean(-1)
        rows = torch.where(keep, rows, torch.zeros_like(rows))
        return rows.sum() / keep.sum()                           # 0 / 0 = nan when every row is ignored


CRITERIA = {"BinaryCrossEntropy": BinaryCrossEntropy}          # the names make_criterion resolves before torch.nn
