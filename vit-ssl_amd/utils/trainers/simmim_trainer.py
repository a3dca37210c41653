"""SimMIM trainer (reference: utils/trainers/simmim_trainer.py:53-135).

Step body = the reference's zero_grad -> forward -> criterion -> backward -> step
(-> warm-up).  With nn.L1Loss(mean) + AdamW (the reference's configs/simmim/training.yaml)
the whole step runs fused in the HIP engine (SimMIMViT.train_step); any other criterion /
optimizer takes the reference-style autograd path through the same kernels.  The loss is
accumulated on the device and read once per epoch (the reference syncs every step).
A loader may yield float batches (as the reference's) or decoded uint8 [B,H,W,3] images, alone
or with labels, which `BaseTrainer._batch` renders on the GPU (transforms.train / transforms.val).
With `metrics: [PSNR, SSIM]` in the config every step's predictions and targets are reduced on the GPU where they lie
(utils/gpu_metrics.py; the reference keeps them all for the epoch, :79-96) and the best checkpoint is the one with the
largest SSIM + 0.01 PSNR (reference :137-153)."""
import logging

import torch
from torch import nn

from .base_trainer import BaseTrainer

logger = logging.getLogger(__name__)


class SimMIMTrainer(BaseTrainer):
    def _fused_ok(self):
        return self._is_fused() and isinstance(self.criterion, nn.L1Loss) and self.criterion.reduction == "mean"

    def _update_metrics(self, preds, targets):
        if self.metric_handler is not None:
            self.metric_handler.update_recon(preds, targets, self.model.input_shape[0], self.model.patch_size)

    def _best_score(self, val_metrics):
        if self._listed("SSIM", "PSNR"):
            return "best_val_score", val_metrics["SSIM"] + 0.01 * val_metrics["PSNR"]
        return None

    def train_epoch(self, epoch: int):
        self.model.train()
        total = 0
        running = None
        fused = self._fused_ok()
        for idx, inputs in enumerate(self.train_loader):
            inputs, _ = self._batch(inputs, "train")
            if fused:
                loss = self.model.train_step(inputs, self.optimizer, self.reducer)
                self._update_metrics(self.model.last_pred, self.model.last_targets)
            else:
                self.optimizer.zero_grad(set_to_none=True)
                preds, targets = self.model(inputs)
                loss = self.criterion(preds, targets)
                loss.backward()
                self._generic_reduce()
                self.optimizer.step()
                loss = loss.detach()
                self._update_metrics(preds, targets)
            self._warmup_step(epoch)
            running = loss if running is None else running + loss
            total += 1
        return self._log_grad_norm(epoch, {**self._metric_values(), "Loss": float(running) / max(total, 1)})

    def validate(self):
        self.model.eval()
        total, running = 0, None
        with torch.no_grad():
            for idx, inputs in enumerate(self.val_loader):
                inputs, _ = self._batch(inputs, "val")
                preds, targets = self.model(inputs)
                loss = self.criterion(preds, targets)
                self._update_metrics(preds, targets)
                running = loss if running is None else running + loss
                total += 1
        return {**self._metric_values(), "Loss": float(running) / max(total, 1) if total else float("nan")}
