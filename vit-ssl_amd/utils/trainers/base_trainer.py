"""Common trainer scaffolding (reference: utils/trainers/base_trainer.py:16-123):
criterion / optimizer / scheduler factories, epoch loop, checkpoint dict layout
{epoch, model_state_dict, optimizer_state_dict, best_val_loss, config}.  The reference's
rich Logger and TrainingHistory are out of scope; stdlib logging reports the loss.  Its MetricHandler is
`utils.gpu_metrics.GPUMetricHandler`, built only when the config lists `metrics`; the listed names then decide which
checkpoint is best (`_best_score`: the reference trainers' per-mode `_save_if_best` rules), otherwise the validation loss does.  New: data-parallel gradient reduction when torch.distributed is initialised; uint8 [B,H,W,3] batches are
rendered on the GPU by the config's `transforms.train` / `transforms.val` list (`_batch`, data.GPUTransform)."""
import logging
import math
import os
from abc import ABC, abstractmethod

import torch
import torch.distributed as dist

from vit_core._runtime import limit_host_threads

from .._config import cfg_get, to_plain
from ..gpu_metrics import GPUMetricHandler
from ..train_utils import make_criterion, make_optimizer, make_schedulers

logger = logging.getLogger(__name__)


class BaseTrainer(ABC):
    def __init__(self, model, save_path: str, config, train_loader, val_loader, device):
        self.model = model
        self.config = config
        self.train_loader = train_loader
        self.val_loader = val_loader
        self.device = device
        self.save_path = save_path
        self.warmup_epochs = cfg_get(config, "training", "warmup_epochs")
        self.num_epochs = cfg_get(config, "training", "num_epochs")
        self.eval_interval = cfg_get(config, "eval", "interval", default=0)

        if torch.device(device).type == "cuda":
            limit_host_threads()
        self.criterion = self.create_criterion()
        self.optimizer = make_optimizer(config, model)
        self.schedulers = make_schedulers(config, self.optimizer, self.num_epochs, self.warmup_epochs * len(train_loader))
        self.best_val_loss = math.inf
        self.metric_handler = GPUMetricHandler.from_config(config)      # None unless the config lists `metrics`
        self.best_val_score = -math.inf                                 # the reference's best_score (SimMIM, DINO)
        self.best_val_acc = -math.inf                                   # (supervised, finetune)
        self.current_epoch = 0
        self.start_epoch = 0

        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        self.reducer = None
        if self.world > 1:
            self._setup_data_parallel()
        self._gpu_transforms = {}           # split -> data.GPUTransform, built on the first uint8 batch
        self.transform_generator = None     # torch.Generator of the crop / flip draws (None: the global CPU generator)

    # ---- data parallel -----------------------------------------------------------
    def _dp_store(self):
        return self.model.trainable_store() if hasattr(self.model, "trainable_store") else self.model.flat_store()

    def _setup_data_parallel(self):
        from vitssl_hip.engine import GradReducer
        for store in self.model.all_stores() if hasattr(self.model, "all_stores") else [self.model.flat_store()]:
            dist.broadcast(store.flat, 0)                      # identical weights on every rank
            store.mark_dirty()
        self.reducer = GradReducer(self._dp_store().gflat)

    def _is_fused(self) -> bool:
        from vitssl_hip.optim import FusedAdamW, FusedLamb
        return isinstance(self.optimizer, (FusedAdamW, FusedLamb)) and hasattr(self.model, "train_step")

    def _log_grad_norm(self, epoch, values):
        """With `training.clip_grad_norm`: log the pre-clip gradient norm of the epoch's last step.  Called once per epoch where
        the epoch's loss has just been read, so the one-float read adds no wait of its own.  Returns `values` unchanged."""
        norm = getattr(self.optimizer, "grad_norm", None)
        if norm is not None:
            logger.info("epoch %d: grad_norm %.4g before clipping at %g", epoch, float(norm),
                        self.optimizer.param_groups[0]["max_grad_norm"])
        return values

    def _generic_reduce(self):
        """Reference-style path (loss.backward through autograd): average p.grad across ranks."""
        if self.world == 1:
            return
        for p in self.model.parameters():
            if p.grad is not None:
                dist.all_reduce(p.grad)
                p.grad.div_(self.world)

    # ---- input ---------------------------------------------------------------------
    def _batch(self, batch, split, non_blocking=True):
        """What a loader yields -> (float32 images on the device, labels on the device or None).  A uint8 [B,H,W,3] tensor
        of decoded images, alone or as the first element of (images, labels), is rendered on the GPU by the
        `transforms.<split>` list of the config (the list the reference's datasets run per image on the CPU:
        utils/train_utils.py:54-68); float batches pass through untouched.  `non_blocking`: how the batch is copied to the
        device (each trainer keeps the copy it always made)."""
        labels = None
        if isinstance(batch, (tuple, list)):
            batch, labels = batch[0], batch[1]
            labels = labels.to(self.device, non_blocking=non_blocking)
        images = batch.to(self.device, non_blocking=non_blocking)
        if images.dtype == torch.uint8 and images.dim() == 4:
            tf = self._gpu_transforms.get(split)
            if tf is None:
                from data import GPUTransform, TransformSpec
                sequence = cfg_get(self.config, "transforms", split)
                if sequence is None:
                    raise ValueError(f"{type(self).__name__}: the loader yielded a uint8 batch {tuple(images.shape)} but the config has no "
                                     f"`transforms.{split}` list to render it with")
                tf = self._gpu_transforms[split] = GPUTransform(TransformSpec.from_config(sequence))
            images = tf(images, self.transform_generator)
        return images, labels

    # ---- abstract ------------------------------------------------------------------
    @abstractmethod
    def train_epoch(self, epoch):
        pass

    @abstractmethod
    def validate(self):
        pass

    def create_criterion(self):
        return make_criterion(self.config)

    # ---- loop ----------------------------------------------------------------------
    def fit(self, num_epochs: int):
        end_epoch = self.start_epoch + num_epochs
        for epoch in range(self.start_epoch + 1, end_epoch + 1):
            self.current_epoch = epoch
            train_metrics = self.train_epoch(epoch)
            val_metrics = self.validate()
            self._update_schedulers(epoch)
            self._log_metrics(epoch, train_metrics, val_metrics)
            self._save_if_best(epoch, val_metrics)
            self._save_last(epoch)

    def _update_schedulers(self, epoch):
        if epoch > self.warmup_epochs:
            self.schedulers["main"].step()

    def _warmup_step(self, epoch):
        if self.schedulers["warmup"] is not None and epoch <= self.warmup_epochs:
            self.schedulers["warmup"].step()

    def _log_metrics(self, epoch, train_metrics, val_metrics):
        if self.rank == 0:
            logger.info(f"epoch {epoch}: train {train_metrics} | val {val_metrics}")

    def _checkpoint(self, epoch, **extra):
        ckpt = {"epoch": epoch, "model_state_dict": self.model.state_dict(),
                "optimizer_state_dict": self.optimizer.state_dict(), "config": to_plain(self.config)}
        ckpt.update(extra)
        return ckpt

    def _listed(self, *names):
        """True when the config's `metrics` lists every one of `names`."""
        have = self.metric_handler.metric_names if self.metric_handler is not None else ()
        return all(n in have for n in names)

    def _metric_values(self):
        """The epoch's listed metrics ({} without a handler); the handler is reset for the next epoch or split."""
        if self.metric_handler is None:
            return {}
        values = self.metric_handler.compute()
        self.metric_handler.reset()
        return values

    def _best_score(self, val_metrics):
        """(checkpoint key = trainer attribute, score) of the mode's metric rule -- larger is better, compared with `>` from
        -inf as the reference trainers do -- or None: the validation loss decides (every trainer without listed metrics)."""
        return None

    def _save_if_best(self, epoch, val_metrics):
        """Rank 0 decides from the metrics of its own shard, as it does for the loss."""
        if self.rank != 0:
            return
        rule = self._best_score(val_metrics)
        if rule is None:
            val_loss = val_metrics["Loss"]
            if not self.best_val_loss >= val_loss:
                return
            self.best_val_loss = val_loss
            logger.info(f"New best validation loss: {self.best_val_loss:.4f}. Saving model...")
            extra = {"best_val_loss": self.best_val_loss}
        else:
            key, score = rule
            if not score > getattr(self, key):
                return
            setattr(self, key, score)
            logger.info(f"New best validation {'accuracy' if key == 'best_val_acc' else 'score'}: {score:.4f}. Saving model...")
            extra = {key: score}
        os.makedirs(self.save_path, exist_ok=True)
        torch.save(self._checkpoint(epoch, **extra), os.path.join(self.save_path, "best_model.pth"))

    def _save_last(self, epoch):
        if self.rank == 0:
            os.makedirs(self.save_path, exist_ok=True)
            torch.save(self._checkpoint(epoch), os.path.join(self.save_path, "last_model.pth"))
