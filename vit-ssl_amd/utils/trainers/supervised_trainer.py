"""Supervised / fine-tune trainer (reference: utils/trainers/supervised_trainer.py:30-48):
logits = model(x); CrossEntropy; backward; step.  By default it runs the reference-style autograd path
through the HIP engine; with `training.fused_step: true` (and the fused AdamW, a model with `train_step`, and
nn.CrossEntropyLoss(weight=None, reduction="mean") or utils.losses.BinaryCrossEntropy) every step is `ViT.train_step` /
`ViT.eval_step`: loss, backward, all-reduce and AdamW as one engine schedule that does only the work the model's frozen state needs, with one host read
per epoch.  Anything else falls back to the autograd path and says so once.
`training.mixup: {mixup_alpha, cutmix_alpha, prob, switch_prob, mode}` (fused path only, else a ValueError at construction): the
training batches are mixed on the GPU (data.GPUMixup, timm's Mixup semantics) and the loss is taken against the two-label targets.
Batches are (images, labels); uint8 [B,H,W,3] images are rendered on the GPU (`BaseTrainer._batch`).
The names of the config's `metrics` (Accuracy, F1Score, Recall, Precision) come from a confusion matrix accumulated on the
device per batch (utils/gpu_metrics.py); with `Accuracy` listed the best checkpoint is the one with the highest validation
accuracy, stored as `best_val_acc` (reference :126-138).
`training.freeze_backbone` with `freeze_backbone_epochs` (under `training`, else the top-level key the reference reads,
:16-19): at the start of that epoch the patch embedding and the encoder blocks train again and the optimizer is rebuilt
with fresh moments (reference :88-90, :120-124).  Deviation, on purpose: the new optimizer takes over the old one's
current learning rate and the existing schedulers are re-pointed at it; the reference leaves its schedulers driving the
discarded optimizer, which freezes the learning rate at its initial value."""
import logging
import math

import torch
from torch import nn

from .._config import cfg_get, to_plain
from ..losses import BinaryCrossEntropy
from ..train_utils import make_optimizer
from .base_trainer import BaseTrainer

logger = logging.getLogger(__name__)


class SupervisedTrainer(BaseTrainer):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._read_schedule_keys()
        self._read_mixup()
        if self.reducer is not None and self._fused_path():
            self._rebuild_reducer()

    def _read_schedule_keys(self):
        self.freeze_backbone = bool(cfg_get(self.config, "training", "freeze_backbone", default=False))
        epochs = cfg_get(self.config, "training", "freeze_backbone_epochs")
        if epochs is None:
            epochs = cfg_get(self.config, "freeze_backbone_epochs")
        self.freeze_backbone_epochs = math.inf if epochs is None else epochs
        self.fused_step = bool(cfg_get(self.config, "training", "fused_step", default=False))
        self._fallback_logged = False
        self._step_counters = None

    def _read_mixup(self):
        """`training.mixup: {mixup_alpha, cutmix_alpha, prob, switch_prob, mode}` (timm's Mixup; data.MixSpec): the training
        batches of the fused step are mixed on the GPU and the loss is taken against the two-label targets.  Validation
        never mixes."""
        node = cfg_get(self.config, "training", "mixup")
        self.mixup = None
        if node is None or node is False:
            return
        from data import GPUMixup, MixSpec
        spec = MixSpec.from_config({} if node is True else to_plain(node))
        if not self._fused_path():
            c = self.criterion
            raise ValueError("training.mixup needs the fused supervised step (training.fused_step: true, with the fused AdamW over a "
                             "model with train_step and nn.CrossEntropyLoss(weight=None, reduction='mean') or "
                             "utils.losses.BinaryCrossEntropy): only its loss kernels take two-label targets; configured here are "
                             f"training.fused_step = {getattr(self, 'fused_step', False)!r}, "
                             f"optimizer {type(self.optimizer).__name__}, criterion {type(c).__name__}")
        self.mixup = GPUMixup(spec)

    # ---- fused path --------------------------------------------------------------
    def _fused_path(self) -> bool:
        """training.fused_step, the fused optimizer over a model with train_step, and a criterion the loss kernel implements."""
        if not getattr(self, "fused_step", False):
            return False
        c = self.criterion
        known = (type(c) is nn.CrossEntropyLoss and c.weight is None and c.reduction == "mean") or type(c) is BinaryCrossEntropy
        ok = self._is_fused() and known
        if not ok and not self._fallback_logged:
            logger.warning("training.fused_step is set, but the fused step needs the fused AdamW, a model with train_step and "
                           "nn.CrossEntropyLoss(weight=None, reduction='mean') or utils.losses.BinaryCrossEntropy: using the autograd path")
            self._fallback_logged = True
        return ok

    def _loss_keywords(self):
        """What train_step / eval_step are told about the criterion (one of the two `_fused_path` accepts)."""
        c = self.criterion
        if type(c) is BinaryCrossEntropy:
            return dict(label_smoothing=c.smoothing, ignore_index=c.ignore_index, loss="bce", target_threshold=c.target_threshold,
                        sum_classes=c.sum_classes)
        return dict(label_smoothing=c.label_smoothing, ignore_index=c.ignore_index)

    def _rebuild_reducer(self):
        """Data parallel: the reducer expects the gradient ranges of the model's current frozen state."""
        from vitssl_hip.engine import GradReducer
        self.reducer = GradReducer(self._dp_store().gflat, expect=self.model.reduce_ranges())

    def _counters(self):
        """(correct, valid) of the epoch on the device: one host read at its end."""
        if self._step_counters is None:
            self._step_counters = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._step_counters.zero_()
        return self._step_counters

    def _epoch_values(self, running, total, counters):
        self.model.check_labels()
        correct, valid = counters.tolist()
        loss = float(running) / total if total else float("nan")
        return {**self._metric_values(), "Loss": loss, "Accuracy": correct / max(valid, 1)}

    def _fused_update_metrics(self, labels):
        if self.metric_handler is not None:
            self.metric_handler.update_classification(self.model.last_pred, labels, self.model.num_classes)

    def _train_epoch_fused(self, epoch):
        total, running, counters = 0, None, self._counters()
        for batch in self.train_loader:
            inputs, labels = self._labelled(batch, "train")
            kw = self._loss_keywords()
            if getattr(self, "mixup", None) is not None:
                kw["mix"] = self.mixup.draw(inputs.shape[0], inputs.shape[2], inputs.shape[3], self.transform_generator, inputs.device)
            loss = self.model.train_step(inputs, labels, self.optimizer, self.reducer, counters=counters, **kw)
            self._warmup_step(epoch)
            running = loss if running is None else running + loss
            self._fused_update_metrics(labels)
            total += 1
        return self._log_grad_norm(epoch, self._epoch_values(running, total, counters))

    def _validate_fused(self):
        total, running, counters = 0, None, self._counters()
        kw = self._loss_keywords()
        for batch in self.val_loader:
            inputs, labels = self._labelled(batch, "val")
            loss = self.model.eval_step(inputs, labels, counters=counters, **kw)
            running = loss if running is None else running + loss
            self._fused_update_metrics(labels)
            total += 1
        return self._epoch_values(running, total, counters)

    # ---- un-freeze -----------------------------------------------------------------
    def _maybe_unfreeze(self, epoch):
        if not getattr(self, "freeze_backbone", False) or epoch != self.freeze_backbone_epochs:
            return
        for part in (self.model.patch_embedding, self.model.encoder_blocks):
            for p in part.parameters():
                p.requires_grad = True
        old = self.optimizer
        self.optimizer = make_optimizer(self.config, self.model)             # fresh moments, as in the reference
        for new_group, old_group in zip(self.optimizer.param_groups, old.param_groups):
            new_group["lr"] = old_group["lr"]
            if "initial_lr" in old_group:
                new_group["initial_lr"] = old_group["initial_lr"]
        for scheduler in self.schedulers.values():
            if scheduler is not None:
                scheduler.optimizer = self.optimizer
        if self.reducer is not None and self._fused_path():
            self._rebuild_reducer()
        logger.info("epoch %d: backbone un-frozen, optimizer rebuilt at lr %g", epoch, self.optimizer.param_groups[0]["lr"])

    # ---- reference-style path ----------------------------------------------------
    def _labelled(self, batch, split):
        inputs, labels = self._batch(batch, split, non_blocking=False)
        if labels is None:
            raise ValueError("SupervisedTrainer: the loader yielded images without labels; it must yield (images, labels)")
        return inputs, labels

    def _update_metrics(self, logits, labels):
        if self.metric_handler is not None:
            self.metric_handler.update_classification(logits.argmax(1), labels, logits.shape[1])

    def _best_score(self, val_metrics):
        if self._listed("Accuracy"):
            return "best_val_acc", val_metrics["Accuracy"]
        return None

    def train_epoch(self, epoch: int):
        self.model.train()
        self._maybe_unfreeze(epoch)
        if self._fused_path():
            return self._train_epoch_fused(epoch)
        total, correct, seen, running = 0, 0, 0, None
        for idx, batch in enumerate(self.train_loader):
            inputs, labels = self._labelled(batch, "train")
            self.optimizer.zero_grad(set_to_none=True)
            logits = self.model(inputs)
            loss = self.criterion(logits, labels)
            loss.backward()
            self._generic_reduce()
            self.optimizer.step()
            self._warmup_step(epoch)
            running = loss.detach() if running is None else running + loss.detach()
            self._update_metrics(logits.detach(), labels)
            correct += int((logits.argmax(1) == labels).sum())
            seen += labels.numel()
            total += 1
        return self._log_grad_norm(epoch, {**self._metric_values(), "Loss": float(running) / max(total, 1),
                                           "Accuracy": correct / max(seen, 1)})

    def validate(self):
        self.model.eval()
        if self._fused_path():
            return self._validate_fused()
        total, correct, seen, running = 0, 0, 0, None
        with torch.no_grad():
            for idx, batch in enumerate(self.val_loader):
                inputs, labels = self._labelled(batch, "val")
                logits = self.model(inputs)
                loss = self.criterion(logits, labels)
                running = loss if running is None else running + loss
                self._update_metrics(logits, labels)
                correct += int((logits.argmax(1) == labels).sum())
                seen += labels.numel()
                total += 1
        return {**self._metric_values(), "Loss": float(running) / max(total, 1) if total else float("nan"),
                "Accuracy": correct / max(seen, 1)}
