"""Supervised / fine-tune trainer (reference: utils/trainers/supervised_trainer.py:30-48):
logits = model(x); CrossEntropy; backward; step.  Runs the reference-style autograd path
through the HIP engine (the supervised config is the reference's small plumbing case).
Batches are (images, labels); uint8 [B,H,W,3] images are rendered on the GPU (`BaseTrainer._batch`).
The names of the config's `metrics` (Accuracy, F1Score, Recall, Precision) come from a confusion matrix accumulated on the
device per batch (utils/gpu_metrics.py); with `Accuracy` listed the best checkpoint is the one with the highest validation
accuracy, stored as `best_val_acc` (reference :126-138)."""
import logging

import torch

from .base_trainer import BaseTrainer

logger = logging.getLogger(__name__)


class SupervisedTrainer(BaseTrainer):
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
        return {**self._metric_values(), "Loss": float(running) / max(total, 1), "Accuracy": correct / max(seen, 1)}

    def validate(self):
        self.model.eval()
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
